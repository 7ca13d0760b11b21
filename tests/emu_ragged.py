"""Numpy emulation of the ragged entries (include/vitres_hip.h: vr_ragged_plane, vr_jpeg_reconstruct_ragged_u8,
vr_resample_ragged_u8), built on emu_resample and emu_jpeg -- which have no scale limit -- and restating the layout and the device's
record checks on its own: nothing here is shared with the product code.

A plane table is a structured array (PLANE: off, pitch, rows, ws_off), or the int32 [B, 8] form the device reads.
`install(monkeypatch)` puts the emulations -- and the padded ones of emu_resample / emu_jpeg -- in the place of the four entries of
vitres.kernels that the loaders of vitres.data call: the only function here that touches the product.
"""
import os

import numpy as np

import emu_jpeg as EJ
import emu_resample as ER

PLANE = np.dtype([("off", "<i8"), ("pitch", "<i4"), ("rows", "<i4"), ("ws_off", "<i8"), ("reserved", "<i4", (2,))])
MAX_SIDE = 8192
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f23_ragged_pil.npz")


def table(planes):
    planes = np.asarray(planes)
    if planes.dtype != PLANE:
        planes = np.ascontiguousarray(planes, dtype=np.int32).view(PLANE).reshape(-1)
    return planes


def pack(images, extra_pitch=None, gap=0, fill=0, lead=0):
    """images: [C,h,w] uint8 arrays -> (flat uint8 [n], planes PLANE [B]).  Sample b has pitch = its width rounded up to 4 plus
    extra_pitch[b] (a multiple of 4), rows = its height; it starts on the first multiple of 16 at least `gap` bytes after the
    previous sample's end (`lead` bytes before the first).  Everything that is not a pixel -- pad columns and gaps -- is `fill`."""
    B = len(images)
    extra_pitch = [0] * B if extra_pitch is None else extra_pitch
    planes = np.zeros(B, dtype=PLANE)
    pos = lead
    for b, img in enumerate(images):
        C, h, w = img.shape
        pos = (pos + 15) // 16 * 16
        planes[b]["off"], planes[b]["pitch"], planes[b]["rows"] = pos, (w + 3) // 4 * 4 + extra_pitch[b], h
        pos += C * h * int(planes[b]["pitch"]) + gap
    flat = np.full((pos + 15) // 16 * 16, fill, dtype=np.uint8)
    for img, p in zip(images, planes):
        C, h, w = img.shape
        off, pitch = int(p["off"]), int(p["pitch"])
        flat[off:off + C * h * pitch].reshape(C, h, pitch)[:, :, :w] = img
    return flat, planes


def pixel_mask(planes, shapes, nbytes):
    """bool [nbytes]: True on the bytes that are image pixels (shapes: (C, h, w) per sample)"""
    mask = np.zeros(nbytes, dtype=bool)
    for p, (C, h, w) in zip(table(planes), shapes):
        off, pitch, rows = int(p["off"]), int(p["pitch"]), int(p["rows"])
        mask[off:off + C * rows * pitch].reshape(C, rows, pitch)[:, :h, :w] = True
    return mask


def plane_ok(p, C, nbytes, Hs, Ws):
    """the device's own test of one record"""
    off, pitch, rows = int(p["off"]), int(p["pitch"]), int(p["rows"])
    if off < 0 or off % 16:
        return False
    if pitch < 4 or pitch % 4 or pitch > Ws or rows < 1 or rows > Hs:
        return False
    return off + C * rows * pitch <= nbytes


def view(flat, p, C):
    off, pitch, rows = int(p["off"]), int(p["pitch"]), int(p["rows"])
    return flat[off:off + C * rows * pitch].reshape(C, rows, pitch)


def ws_offsets(planes, C, So_w, heights):
    """fills ws_off (the intermediates packed over `heights`); returns the bytes they need, rounded up to 16"""
    planes = table(planes)
    pos = 0
    for p, h in zip(planes, heights):
        p["ws_off"] = pos
        pos += C * int(h) * So_w
    return (pos + 15) // 16 * 16


def resample_plane(plane, box, So_h, So_w, filt):
    """emu_resample.resample_plane with PIL's pass order: Image.resize runs the VERTICAL pass first on an image more than 100 times
    as tall as wide that shrinks vertically (`if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`: resize to (w, oh),
    then to (ow, oh), an 8-bit image between) -- the image being the crop here.  Every other crop goes horizontal first."""
    x0, y0, w, h, ow, oh, wx, wy, flip = (int(v) for v in box)
    if not (h > 100 * w and oh < h):
        return ER.resample_plane(plane, box, So_h, So_w, filt)
    crop = plane[y0:y0 + h, x0:x0 + w].astype(np.int64)
    half = 1 << (ER.PRECISION_BITS - 1)
    tmp = np.empty((So_h, w), dtype=np.int64)
    for r, (ymin, ks) in enumerate(ER.axis_coeffs(h, oh, filt, wy, So_h)):
        acc = np.full(w, half, dtype=np.int64)
        for t, k in enumerate(ks):
            acc += crop[ymin + t] * k
        tmp[r] = ER._clip8(acc)
    out = np.empty((So_h, So_w), dtype=np.uint8)
    for c, (xmin, ks) in enumerate(ER.axis_coeffs(w, ow, filt, wx, So_w)):
        acc = np.full(So_h, half, dtype=np.int64)
        for t, k in enumerate(ks):
            acc += tmp[:, xmin + t] * k
        out[:, c] = ER._clip8(acc)
    return out[:, ::-1] if flip else out


def resample_ragged_u8(flat, planes, boxes, C, So_h, So_w, filt, nbytes=None, bounds=None, ws_bytes=None):
    """The device entry on the CPU -> uint8 [B,C,So_h,So_w].  A sample whose plane record fails the device's check (or, with ws_bytes
    given, whose intermediate does not lie inside the workspace) is zeros; a box is clamped into its own plane as the kernel clamps."""
    flat, planes = np.asarray(flat), table(planes)
    nbytes = flat.size if nbytes is None else nbytes
    Hs, Ws = (MAX_SIDE, MAX_SIDE) if bounds is None else bounds
    out = np.zeros((len(planes), C, So_h, So_w), dtype=np.uint8)
    for b, p in enumerate(planes):
        if not plane_ok(p, C, nbytes, Hs, Ws):
            continue
        x0, y0, w, h, ow, oh, wx, wy, flip = (int(v) for v in boxes[b][:9])
        pitch, rows = int(p["pitch"]), int(p["rows"])
        w, h = min(max(w, 1), pitch, MAX_SIDE), min(max(h, 1), rows, MAX_SIDE)
        x0, y0 = min(max(x0, 0), pitch - w), min(max(y0, 0), rows - h)
        ow, oh = max(ow, So_w), max(oh, So_h)
        wx, wy = min(max(wx, 0), ow - So_w), min(max(wy, 0), oh - So_h)
        if ws_bytes is not None:
            ws_off = int(p["ws_off"])
            if ws_off < 0 or ws_off % 4 or ws_off + C * h * So_w > ws_bytes:
                continue
        src = view(flat, p, C)
        for c in range(C):
            out[b, c] = resample_plane(src[c], (x0, y0, w, h, ow, oh, wx, wy, 1 if flip else 0), So_h, So_w, filt)
    return out


def reconstruct_ragged_u8(blob, descs, qtabs, dst, planes, nbytes=None, bounds=None):
    """The device entry on the CPU: writes into a copy of dst (uint8 [n]) and returns it.  Every byte of the three planes of a sample
    whose plane record passes and holds its image; nothing for the others; an invalid JPEG record leaves its planes zero."""
    dst, planes = np.array(dst, dtype=np.uint8), table(planes)
    descs = np.asarray(descs, dtype=np.int32)
    nbytes = dst.size if nbytes is None else nbytes
    if bounds is None:
        bounds = (min(int(planes["rows"].max()), MAX_SIDE), min(int(planes["pitch"].max()), MAX_SIDE))
    Hs, Ws = bounds
    for b, p in enumerate(planes):
        if not plane_ok(p, 3, nbytes, Hs, Ws):
            continue
        pitch, rows = int(p["pitch"]), int(p["rows"])
        if EJ.record_ok(descs[b], np.asarray(blob).size, Hs, Ws) and (int(descs[b][1]) > pitch or int(descs[b][2]) > rows):
            continue
        if EJ.record_ok(descs[b], np.asarray(blob).size, Hs, Ws):
            view(dst, p, 3)[...] = EJ.reconstruct_u8(blob, descs[b:b + 1], np.asarray(qtabs)[b:b + 1], rows, pitch)[0]
        else:
            view(dst, p, 3)[...] = 0
    return dst


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(GOLDEN)
    return _G


def golden_case(name):
    """(images [C,h,w] per SAMPLE, boxes int32 [B,9], (So_h, So_w), filter, PIL's output) of a resample case of the fixture"""
    g = golden()
    index = g[name + ".map"]
    images = [g["%s.img%d" % (name, int(i))] for i in index]
    So_h, So_w, filt = (int(v) for v in g[name + ".meta"])
    return images, g[name + ".boxes"], (So_h, So_w), filt, g[name + ".out"]


def golden_jpeg_big():
    """(streams as bytes, PIL's RGB pixels [h,w,3], boxes, (So_h, So_w), filter, PIL's crops) of the fixture's encoded files"""
    g = golden()
    streams = [g["jpeg_big.stream%d" % k].tobytes() for k in range(4)]
    pixels = [g["jpeg_big.pixels%d" % k] for k in range(4)]
    So_h, So_w, filt = (int(v) for v in g["jpeg_big.meta"])
    return streams, pixels, g["jpeg_big.boxes"], (So_h, So_w), filt, g["jpeg_big.out"]


def repack_padded(src, fill=255):
    """a padded canvas batch [B,C,Hs,Ws] as ragged planes: every sample's whole canvas plane is its image (pitch = Ws)"""
    return pack([s for s in np.asarray(src)], gap=48, fill=fill)


def install(monkeypatch):
    """Swap the four entries the loaders of vitres.data call -- resample_u8, resample_ragged_u8, jpeg_reconstruct_u8 and
    jpeg_reconstruct_ragged_u8 of vitres.kernels -- for the emulations (torch CPU tensors in and out)."""
    import torch
    import vitres.kernels as K

    def padded_resample(src, boxes, out_size, filter, out=None):
        So_h, So_w = K._out_size(out_size)
        B, _, Hs, Ws = src.shape
        if K.resample_band_rows(src.shape[1], Hs, Ws, (So_h, So_w), filter) < 1:     # (raises VR_EUNSUPPORTED as the entry does)
            raise AssertionError
        return torch.from_numpy(ER.resample_u8(src.numpy(), boxes.numpy(), So_h, So_w, K._resample_filter(filter)))

    def ragged_resample(src, planes, boxes, C, out_size, filter, out=None, workspace=None, src_bytes=None, bounds=None):
        So_h, So_w = K._out_size(out_size)
        assert workspace is not None and bounds is not None
        return torch.from_numpy(resample_ragged_u8(src.numpy(), planes.numpy(), boxes.numpy(), C, So_h, So_w,
                                                   K._resample_filter(filter), bounds=bounds, ws_bytes=workspace.numel()))

    def padded_reconstruct(blob, descs, qtabs, Hs, Ws, out=None, workspace=None):
        out.copy_(torch.from_numpy(EJ.reconstruct_u8(blob.numpy(), descs.numpy(), qtabs.numpy(), Hs, Ws)))
        return out

    def ragged_reconstruct(blob, descs, qtabs, planes, dst=None, dst_bytes=None, workspace=None, bounds=None):
        dst.copy_(torch.from_numpy(reconstruct_ragged_u8(blob.numpy(), descs.numpy(), qtabs.numpy(), dst.numpy(), planes.numpy(),
                                                         bounds=bounds)))
        return dst

    for name, f in (("resample_u8", padded_resample), ("resample_ragged_u8", ragged_resample),
                    ("jpeg_reconstruct_u8", padded_reconstruct), ("jpeg_reconstruct_ragged_u8", ragged_reconstruct)):
        monkeypatch.setattr(K, name, f)
