"""Numpy restatement of vr_rand_augment_u8 (include/vitres_hip.h): the eleven op kinds that cover timm's fifteen RandAugment ops, each
bit for bit what PIL 12 makes of the HWC RGB image, applied layer after layer to a uint8 [B,3,H,W] batch.  Portable: numpy only.
tests/golden/f21_randaugment_pil.npz (PIL's own outputs) pins it; the GPU tests compare the kernel with both.

A table is anything indexable by field name that gives arrays of shape [B, layers] ("op", "filter", "iarg", "factor") and
[B, layers, 6] ("m"): vitres.kernels.ra_table's structured array, or a dict of arrays.
"""
import numpy as np

(IDENTITY, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, AUTOCONTRAST, EQUALIZE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS,
 AFFINE) = range(12)
BILINEAR, BICUBIC = 2, 3
_I = np.arange(256, dtype=np.int64)


def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def point_lut(op, iarg):
    """the [256] table of a per-value op, or None where the record is out of range (the kernel treats it as identity)"""
    if op == INVERT:
        return _clip8(255 - _I)
    if op == POSTERIZE and 0 <= iarg <= 8:
        return _clip8(_I & ~(2 ** (8 - iarg) - 1))
    if op == SOLARIZE and 0 <= iarg <= 256:
        return _clip8(np.where(_I < iarg, _I, 255 - _I))
    if op == SOLARIZE_ADD and 0 <= iarg <= 255:
        return _clip8(np.where(_I < 128, np.minimum(255, _I + iarg), _I))
    return None


def autocontrast_lut(h):
    """ImageOps.autocontrast(cutoff=0) of one channel's histogram h [256]"""
    nz = np.flatnonzero(h)
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return _I.astype(np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return _clip8((_I.astype(np.float64) * scale + offset).astype(np.int64))      # int() truncates towards zero; so does astype


def equalize_step(h):
    """ImageOps.equalize's step of one channel's histogram; 0 where the channel is left as it is"""
    nz = h[h != 0]
    return 0 if len(nz) <= 1 else int((int(nz.sum()) - int(nz[-1])) // 255)


def equalize_lut(h):
    step = equalize_step(h)
    if step == 0:
        return _I.astype(np.uint8)
    n = step // 2 + np.concatenate([[0], np.cumsum(h.astype(np.int64))[:-1]])
    return _clip8(n // step)


def grey(img):
    """PIL's RGB -> L"""
    r, g, b = (img[c].astype(np.int64) for c in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def contrast_mean(img):
    """ImageEnhance.Contrast's constant: int(mean(L) + 0.5), the mean an exact integer sum divided by the count in double"""
    L = grey(img)
    return int(float(int(L.sum(dtype=np.int64))) / float(L.size) + 0.5)


def smooth(img):
    """ImageFilter.SMOOTH per channel: the 3x3 kernel (1,1,1,1,5,1,1,1,1)/13 plus 0.5, truncated; the one-pixel border is the
    source's.  PIL sums in float32; a sum s of integers has s/13 + 0.5 at least 1/26 away from every integer, far beyond float32's
    error at 255, so the exact floor((2s + 13) / 26) is the same byte."""
    out = img.copy()
    H, W = img.shape[1:]
    if H < 3 or W < 3:
        return out
    x = img.astype(np.int64)
    s = 4 * x[:, 1:-1, 1:-1]
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            s = s + x[:, dy:H - 2 + dy, dx:W - 2 + dx]
    out[:, 1:-1, 1:-1] = ((2 * s + 13) // 26).astype(np.uint8)
    return out


def blend(deg, img, factor):
    """Image.blend(deg, img, factor): float32, one rounding per operator"""
    alpha = np.float32(factor)
    d, x = deg.astype(np.float32), img.astype(np.float32)
    with np.errstate(invalid="ignore"):
        t = d + alpha * (x - d)
        assert t.dtype == np.float32
        if 0 <= alpha <= 1:
            return t.astype(np.uint8)
        return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def affine(img, m, filt, fill):
    """Image.transform(size, AFFINE, m, resample=filt, fillcolor=fill) of [3,H,W]: double, one rounding per operator"""
    _, H, W = img.shape
    m = [float(v) for v in m]
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    xin = m[0] * xs + m[1] * ys + m[2]
    yin = m[3] * xs + m[4] * ys + m[5]
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin = np.where(inside, xin, 0.5) - 0.5
    yin = np.where(inside, yin, 0.5) - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = xin - x0, yin - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    cx = lambda v: np.clip(v, 0, W - 1)                                          # noqa: E731
    cy = lambda v: np.clip(v, 0, H - 1)                                          # noqa: E731
    out = np.empty_like(img)
    for c in range(3):
        p = img[c].astype(np.float64)
        if filt == BILINEAR:
            rows = []
            for j in (0, 1):
                a, b = p[cy(y0 + j), cx(x0)], p[cy(y0 + j), cx(x0 + 1)]
                rows.append(a + (b - a) * dx)
            v = rows[0] + (rows[1] - rows[0]) * dy
            res = v.astype(np.int64)                                             # (uint8)v: v lies inside [0, 255]
        else:
            def cubic(v1, v2, v3, v4, d):
                p1 = v2
                p2 = -v1 + v3
                p3 = 2 * (v1 - v2) + v3 - v4
                p4 = -v1 + v2 - v3 + v4
                return p1 + d * (p2 + d * (p3 + d * p4))
            rows = [cubic(*(p[cy(y0 + j), cx(x0 + i)] for i in (-1, 0, 1, 2)), dx) for j in (-1, 0, 1, 2)]
            v = cubic(*rows, dy)
            res = np.where(v <= 0, 0, np.where(v >= 255, 255, v)).astype(np.int64)
        out[c] = np.where(inside, res, fill[c]).astype(np.uint8)
    return out


def apply_op(img, op, filt, iarg, factor, m, fill):
    """one record on one sample [3,H,W]; an unknown or out-of-range record is identity"""
    op, filt, iarg = int(op), int(filt), int(iarg)
    lut = point_lut(op, iarg)
    if lut is not None:
        return lut[img]
    if op in (AUTOCONTRAST, EQUALIZE):
        make = autocontrast_lut if op == AUTOCONTRAST else equalize_lut
        return np.stack([make(np.bincount(img[c].ravel(), minlength=256))[img[c]] for c in range(3)])
    if op == BRIGHTNESS:
        return blend(np.zeros_like(img), img, factor)
    if op == COLOR:
        return blend(np.broadcast_to(grey(img), img.shape), img, factor)
    if op == CONTRAST:
        return blend(np.full_like(img, contrast_mean(img)), img, factor)
    if op == SHARPNESS:
        return blend(smooth(img), img, factor)
    if op == AFFINE and filt in (BILINEAR, BICUBIC):
        return affine(img, m, filt, fill)
    return img


def fill_rgb(fill):
    """(r, g, b) of the packed fill word r | g << 8 | b << 16, or of a triple"""
    if isinstance(fill, (int, np.integer)):
        return (int(fill) & 255, (int(fill) >> 8) & 255, (int(fill) >> 16) & 255)
    return tuple(int(v) for v in fill)


def rand_augment_u8(src, table, fill):
    """src uint8 [B,3,H,W]; every sample's layers in order"""
    fill = fill_rgb(fill)
    out = np.array(src, dtype=np.uint8, copy=True)
    B, layers = np.asarray(table["op"]).shape
    for b in range(B):
        img = out[b]
        for k in range(layers):
            img = apply_op(img, table["op"][b][k], table["filter"][b][k], table["iarg"][b][k], table["factor"][b][k],
                           table["m"][b][k], fill)
        out[b] = img
    return out


FIELDS = ("op", "filter", "iarg", "factor", "m")


def golden_case(g, name):
    """(src, table as a dict of arrays, fill (r, g, b), PIL's output) of a case of tests/golden/f21_randaugment_pil.npz (g: the
    loaded file)"""
    ops = g[name + ".ops"]
    table = dict(op=ops[..., 0], filter=ops[..., 1], iarg=ops[..., 2], factor=g[name + ".factor"], m=g[name + ".m"])
    return g[name + ".src"], table, tuple(int(v) for v in g[name + ".fill"]), g[name + ".out"]


def golden_names(g):
    return sorted({k.rsplit(".", 1)[0] for k in g.files} - {"sweep"})


def fill_records(records, table):
    """copies a table's fields into `records`, a zeroed structured array of the same shape (vitres.kernels.ra_table); returns it"""
    for f in FIELDS:
        records[f] = table[f]
    return records
