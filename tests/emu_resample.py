"""Integer / float64 numpy emulation of vr_resample_u8 (include/vitres_hip.h): PIL's 8-bit two-pass resample of a crop, restated
on its own -- nothing here is shared with the product code.  Python floats are IEEE doubles and every statement below is one
rounded operation per operator, which is how PIL's C evaluates on x86-64 (no fused multiply-add).

    out = crop((x0, y0, x0 + w, y0 + h)).resize((ow, oh), filter).crop((wx, wy, wx + So_w, wy + So_h)) [mirrored if flip]

PIL 12's ImagingResample: coefficients per axis in double (precompute_coeffs), turned into 22-bit fixed point
(normalize_coeffs_8bpc), a horizontal pass over the source rows the vertical pass touches with an 8-bit intermediate, then the
vertical pass.  A pass whose axis keeps its size is skipped by PIL; its coefficients are then exactly (1 << 22) on one tap, so
running it changes no byte and the emulation does not special-case it.
"""
import numpy as np

BILINEAR, BICUBIC = 2, 3                 # PIL's numbers
SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}
PRECISION_BITS = 32 - 8 - 2


def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {BILINEAR: _bilinear, BICUBIC: _bicubic}


def _trunc(v):
    return int(v)                        # C's (int) of a double: towards zero


def axis_coeffs(in_size, out_size, filt, first, count):
    """[(xmin, [int coefficient, ...]), ...] for the output indices first .. first + count - 1 of an axis resampled from in_size
    to out_size."""
    f = _FILTER[filt]
    scale = float(in_size) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = SUPPORT[filt] * filterscale
    ss = 1.0 / filterscale
    rows = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(_trunc(center - support + 0.5), 0)
        xmax = min(_trunc(center + support + 0.5), in_size)
        ws = [f((x - center + 0.5) * ss) for x in range(xmin, xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        ks = []
        for w in ws:
            if ww != 0.0:
                w = w / ww
            ks.append(_trunc(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else _trunc(0.5 + w * (1 << PRECISION_BITS)))
        rows.append((xmin, ks))
    return rows


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_plane(plane, box, So_h, So_w, filt):
    """One channel [Hs, Ws] uint8 and one box (x0, y0, w, h, ow, oh, wx, wy, flip) -> [So_h, So_w] uint8."""
    x0, y0, w, h, ow, oh, wx, wy, flip = (int(v) for v in box)
    Hs, Ws = plane.shape
    assert w >= 1 and h >= 1 and 0 <= x0 and x0 + w <= Ws and 0 <= y0 and y0 + h <= Hs, "box outside the canvas"
    assert 0 <= wx and wx + So_w <= ow and 0 <= wy and wy + So_h <= oh, "window outside the resized image"
    crop = plane[y0:y0 + h, x0:x0 + w].astype(np.int64)
    horiz = axis_coeffs(w, ow, filt, wx, So_w)
    vert = axis_coeffs(h, oh, filt, wy, So_h)
    ylo = min(ymin for ymin, _ in vert)
    yhi = max(ymin + len(ks) for ymin, ks in vert)
    tmp = np.empty((yhi - ylo, So_w), dtype=np.uint8)
    for c, (xmin, ks) in enumerate(horiz):
        acc = np.full(yhi - ylo, 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t, k in enumerate(ks):
            acc += crop[ylo:yhi, xmin + t] * k
        acc = ((acc + 2 ** 31) % 2 ** 32) - 2 ** 31          # (PIL accumulates in int32; it never wraps with these weights)
        tmp[:, c] = _clip8(acc)
    out = np.empty((So_h, So_w), dtype=np.uint8)
    tmp64 = tmp.astype(np.int64)
    for r, (ymin, ks) in enumerate(vert):
        acc = np.full(So_w, 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t, k in enumerate(ks):
            acc += tmp64[ymin - ylo + t] * k
        out[r] = _clip8(acc)
    return out[:, ::-1] if flip else out


def resample_u8(src, boxes, So_h, So_w, filt):
    """src uint8 [B,C,Hs,Ws], boxes int [B, >=9] (x0, y0, w, h, ow, oh, wx, wy, flip, ...) -> uint8 [B,C,So_h,So_w]."""
    src = np.asarray(src)
    B, C = src.shape[:2]
    out = np.empty((B, C, So_h, So_w), dtype=np.uint8)
    for b in range(B):
        for c in range(C):
            out[b, c] = resample_plane(src[b, c], boxes[b][:9], So_h, So_w, filt)
    return out


def pil_resample_u8(src, boxes, So_h, So_w, filt):
    """The same through PIL itself (the authority); only where PIL is importable."""
    from PIL import Image
    src = np.asarray(src)
    B, C = src.shape[:2]
    out = np.empty((B, C, So_h, So_w), dtype=np.uint8)
    for b in range(B):
        x0, y0, w, h, ow, oh, wx, wy, flip = (int(v) for v in boxes[b][:9])
        for c in range(C):
            im = Image.fromarray(np.ascontiguousarray(src[b, c]))
            im = im.crop((x0, y0, x0 + w, y0 + h)).resize((ow, oh), filt).crop((wx, wy, wx + So_w, wy + So_h))
            if flip:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            out[b, c] = np.asarray(im)
    return out
