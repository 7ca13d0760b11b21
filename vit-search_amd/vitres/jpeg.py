"""The host half of JPEG decoding: ctypes calls on libvitres_jpeg.so (include/vitres_jpeg.h), which parse the markers and
Huffman-decode a baseline stream into its quantised coefficients.  The calls release the GIL.  This module needs numpy only: it
imports neither torch nor the HIP library, so a DataLoader worker that decodes with it holds nothing of the GPU.  The device half is
vitres.kernels.jpeg_reconstruct_u8; vitres.data.jpeg_collate / DeviceJpegLoader put the two together.
"""
import ctypes

import numpy as np

from . import _lib


class JpegError(ValueError):
    """vr_jpeg_entropy_decode refused the stream: `.code` is VR_EUNSUPPORTED (-3) for a stream the fast path does not take,
    VR_EINVAL (-1) for a damaged one."""

    def __init__(self, code):
        ValueError.__init__(self, "vr_jpeg_entropy_decode failed: %s" % _lib._ERR.get(code, code))
        self.code = code


def _buffer(data):
    """the stream as (keep-alive object, address, length) without copying bytes / bytearray / uint8 arrays"""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1 or not data.flags.c_contiguous:
            raise TypeError("a JPEG stream is bytes or a contiguous 1-D uint8 array")
        return data, data.ctypes.data, data.size
    if isinstance(data, bytes):
        return data, ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, len(data)
    arr = np.frombuffer(data, dtype=np.uint8)
    return arr, arr.ctypes.data, arr.size


def _info(I):
    return dict(supported=bool(I.supported), width=I.width, height=I.height, ncomp=I.ncomp, hs=I.hs, vs=I.vs,
                restart_interval=I.restart_interval, blocks=tuple(I.blocks), bw=tuple(I.bw), bh=tuple(I.bh))


def probe(data):
    """vr_jpeg_probe: the frame's geometry as a dict (supported, width, height, ncomp, hs, vs, restart_interval, blocks, bw, bh);
    supported = False -- and zeros -- for everything the fast path does not take, files that are not JPEG included."""
    keep, addr, n = _buffer(data)
    I = _lib.JpegInfo()
    rc = _lib.jpeg_lib().vr_jpeg_probe(addr, n, ctypes.byref(I))
    del keep
    _lib.check(rc, "vr_jpeg_probe")
    return _info(I)


def entropy_decode(data, coef=None, qtab=None, info=None):
    """vr_jpeg_entropy_decode -> (info dict, [per component: int16 view [bh, bw, 64] of its blocks, natural order], qtab uint16 [3, 64]).
    coef: a ZEROED contiguous int16 array to decode into (at least 64 * sum(blocks) elements; allocated when None) -- the component
    views are views of it; qtab: a uint16 [3, 64] array to fill.  info: the dict probe() returned for this stream, to skip the second
    probe when coef is None.  Raises JpegError for an unsupported or a damaged stream."""
    keep, addr, n = _buffer(data)
    L = _lib.jpeg_lib()
    I = _lib.JpegInfo()
    if coef is None:
        if info is None:
            _lib.check(L.vr_jpeg_probe(addr, n, ctypes.byref(I)), "vr_jpeg_probe")
            total = 64 * sum(I.blocks) if I.supported else 0
        else:
            total = 64 * sum(info["blocks"])
        coef = np.zeros(total, dtype=np.int16)
    elif coef.dtype != np.int16 or not coef.flags.c_contiguous or not coef.flags.writeable:
        raise TypeError("entropy_decode: coef must be a writable contiguous int16 array")
    if qtab is None:
        qtab = np.empty((3, 64), dtype=np.uint16)
    elif qtab.dtype != np.uint16 or qtab.shape != (3, 64) or not qtab.flags.c_contiguous:
        raise TypeError("entropy_decode: qtab must be a contiguous uint16 [3, 64] array")
    rc = L.vr_jpeg_entropy_decode(addr, n, ctypes.byref(I), coef.ctypes.data, coef.size, qtab.ctypes.data)
    del keep
    if rc != 0:
        raise JpegError(rc)
    flat, views, lo = coef.reshape(-1), [], 0
    for c in range(I.ncomp):
        views.append(flat[lo:lo + 64 * I.blocks[c]].reshape(I.bh[c], I.bw[c], 64))
        lo += 64 * I.blocks[c]
    return _info(I), views, qtab
