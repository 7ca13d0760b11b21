"""Writes tests/golden/f21_randaugment_pil.npz: seeded uint8 RGB batches, op tables and what PIL itself makes of them -- every
sample's records applied in order with the PIL calls timm's RandAugment ops make (ImageOps.*, ImageEnhance.*, Image.point,
Image.transform, Image.rotate) -- for the cases tests/test_randaugment_host.py and tests/test_gpu_randaugment.py pin.  Needs PIL
(written with 12.2.0); the tests read only the .npz.  Run from the repository root:  python tests/golden/make_randaugment_golden.py

Nothing of the project is imported: the op codes below restate include/vitres_hip.h's VR_RA_* enum, the records are written by
hand, and the rotation matrix is Image.rotate's own arithmetic (checked against Image.rotate for every rotation stored).

Every case <name> stores <name>.src uint8 [B,3,H,W], <name>.ops int32 [B,L,3] (op, filter, iarg), <name>.factor float64 [B,L],
<name>.m float64 [B,L,6], <name>.fill int32 [3] and <name>.out uint8 [B,3,H,W].  The factor sweep is stored apart, to keep the file
small: sweep.src [1,3,16,16], sweep.factors [64], sweep.fill and sweep.out [4,64,3,16,16] (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS).
"""
import math
import os

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

(IDENTITY, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, AUTOCONTRAST, EQUALIZE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS,
 AFFINE) = range(12)
BILINEAR, BICUBIC = 2, 3
FILL = (124, 116, 104)
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
_ENHANCE = {BRIGHTNESS: ImageEnhance.Brightness, COLOR: ImageEnhance.Color, CONTRAST: ImageEnhance.Contrast,
            SHARPNESS: ImageEnhance.Sharpness}


def rec(op, iarg=0, factor=0.0, m=EYE, filt=0, angle=None):
    return dict(op=op, iarg=iarg, factor=factor, m=tuple(float(v) for v in m), filt=filt, angle=angle)


def rotation(angle, W, H, filt):
    """Image.rotate's matrix for an image of that size"""
    a = angle % 360.0
    assert a not in (0, 90, 180, 270)
    cx, cy = W / 2, H / 2
    a = -math.radians(a)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return rec(AFFINE, m=m, filt=filt, angle=angle)


def shear_x(f, filt):
    return rec(AFFINE, m=(1, f, 0, 0, 1, 0), filt=filt)


def shear_y(f, filt):
    return rec(AFFINE, m=(1, 0, 0, f, 1, 0), filt=filt)


def translate_x(pct, W, filt):
    return rec(AFFINE, m=(1, 0, pct * W, 0, 1, 0), filt=filt)


def translate_y(pct, H, filt):
    return rec(AFFINE, m=(1, 0, 0, 0, 1, pct * H), filt=filt)


def pil_apply(img, r, fill):
    op = r["op"]
    if op == IDENTITY:
        return img
    if op == INVERT:
        return ImageOps.invert(img)
    if op == POSTERIZE:
        return ImageOps.posterize(img, r["iarg"])
    if op == SOLARIZE:
        return ImageOps.solarize(img, r["iarg"])
    if op == SOLARIZE_ADD:
        lut = [min(255, i + r["iarg"]) if i < 128 else i for i in range(256)]
        return img.point(lut + lut + lut)
    if op == AUTOCONTRAST:
        return ImageOps.autocontrast(img)
    if op == EQUALIZE:
        return ImageOps.equalize(img)
    if op in _ENHANCE:
        return _ENHANCE[op](img).enhance(r["factor"])
    assert op == AFFINE
    out = img.transform(img.size, Image.AFFINE, r["m"], resample=r["filt"], fillcolor=fill)
    if r["angle"] is not None:
        assert np.array_equal(np.asarray(out), np.asarray(img.rotate(r["angle"], resample=r["filt"], fillcolor=fill)))
    return out


def pil_case(src, table, fill):
    out = np.empty_like(src)
    for b in range(src.shape[0]):
        img = Image.fromarray(np.ascontiguousarray(src[b].transpose(1, 2, 0)), "RGB")
        for r in table[b]:
            img = pil_apply(img, r, fill)
        out[b] = np.asarray(img).transpose(2, 0, 1)
    return out


def noise(seed, B, H, W, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, (B, 3, H, W)).astype(np.uint8)


def smooth_noise(seed, B, H, W):
    """low-frequency content plus noise: interpolation and the 3x3 filter have something to work on"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((B, 3, H, W), dtype=np.uint8)
    for b in range(B):
        for c in range(3):
            f = rs.uniform(0.05, 0.4, 2)
            v = 128 + 150 * np.sin(f[0] * x + rs.uniform(0, 6)) * np.cos(f[1] * y + rs.uniform(0, 6)) + rs.normal(0, 12, (H, W))
            out[b, c] = np.clip(v, 0, 255).astype(np.uint8)
    return out


def grey_with_sum(seed, S, total):
    """an S x S image with R = G = B (so L is that value) whose pixels sum to `total`"""
    n = S * S
    base, extra = divmod(total, n)
    v = np.full(n, base, dtype=np.int64)
    v[:extra] += 1
    rs = np.random.RandomState(seed)
    for _ in range(200):                                    # spread the values, keeping the sum
        i, j = rs.randint(0, n, 2)
        d = int(rs.randint(1, 40))
        if v[i] + d <= 255 and v[j] - d >= 0:
            v[i] += d
            v[j] -= d
    assert v.sum() == total
    rs.shuffle(v)
    return np.broadcast_to(v.reshape(1, S, S), (3, S, S)).astype(np.uint8)


def cases():
    one = lambda *recs: [[r] for r in recs]                                                          # noqa: E731
    yield "lut_a", noise(1, 4, 16, 16), one(rec(INVERT), rec(POSTERIZE, 0), rec(POSTERIZE, 7), rec(POSTERIZE, 3))
    yield "lut_b", noise(2, 4, 16, 16), one(rec(SOLARIZE, 0), rec(SOLARIZE, 256), rec(SOLARIZE, 100), rec(SOLARIZE_ADD, 110))
    yield "lut_c", noise(3, 3, 16, 16), one(rec(POSTERIZE, 8), rec(SOLARIZE_ADD, 0), rec(SOLARIZE_ADD, 37))
    # autocontrast: a stretched sample, one whose green channel is constant, one with four values per channel, a full-range one
    ac = noise(4, 4, 16, 16)
    ac[0] = noise(5, 1, 16, 16, 40, 201)[0]
    ac[1, 1] = 77
    ac[1, 0] = noise(6, 1, 16, 16, 3, 250)[0, 0]
    ac[2] = noise(7, 1, 16, 16, 100, 104)[0]
    yield "autocontrast", ac, one(*[rec(AUTOCONTRAST)] * 4)
    # equalize: 256 pixels whose last non-empty bin holds two -> step == 0 (identity), holds one -> step == 1; 1024 and 2304 pixels
    # -> step > 0; a skewed sample that ends in bin 255; a channel with one value
    e16 = noise(8, 3, 16, 16, 0, 255)
    e16[:2, :, 0, :2] = 255
    e16[2, :, 0, 0] = 255
    yield "equalize16", e16, one(*[rec(EQUALIZE)] * 3)
    eq = noise(9, 3, 32, 32)
    eq[1] = np.minimum(255, (noise(10, 1, 32, 32)[0].astype(np.int64) ** 2) // 200).astype(np.uint8)
    eq[1, :, 0, :5] = 255
    eq[2, 2] = 9
    yield "equalize32", eq, one(*[rec(EQUALIZE)] * 3)
    yield "equalize48", smooth_noise(11, 2, 48, 48), one(*[rec(EQUALIZE)] * 2)
    # the blend ops at the ends and the middle of timm's range
    for f in (0.1, 1.0, 1.9):
        yield "blend_%s" % f, smooth_noise(12, 4, 16, 16), one(*[rec(op, factor=f) for op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS)])
    # factor 0: the degenerate images themselves (sharpness: the smoothed image with the source's border)
    yield "degenerate", smooth_noise(13, 4, 16, 16), one(*[rec(op, factor=0.0) for op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS)])
    # contrast where mean(L) is k + 0.5 exactly, and 1/1024 below and above it
    k = 117
    half = np.stack([grey_with_sum(14 + i, 32, 1024 * k + 512 + d) for i, d in enumerate((0, -1, 1))])
    yield "contrast_half", half, one(*[rec(CONTRAST, factor=1.6)] * 3)
    # affine, both filters in every launch
    S = 16
    yield "affine_shear", smooth_noise(20, 4, S, S), one(shear_x(0.3, BICUBIC), shear_x(-0.3, BILINEAR), shear_y(0.3, BILINEAR),
                                                         shear_y(-0.3, BICUBIC))
    yield "affine_translate", smooth_noise(21, 4, S, S), one(translate_x(0.45, S, BILINEAR), translate_x(-0.45, S, BICUBIC),
                                                             translate_y(0.45, S, BICUBIC), translate_y(-0.45, S, BILINEAR))
    yield "affine_rotate", smooth_noise(22, 4, S, S), one(rotation(30.0, S, S, BICUBIC), rotation(-30.0, S, S, BILINEAR),
                                                          rotation(1.5, S, S, BICUBIC), rotation(-0.7, S, S, BILINEAR))
    inside = (0.5, 0.0, S / 4, 0.0, 0.5, S / 4)                              # a zoom about the centre: no pixel maps outside
    yield "affine_fill", smooth_noise(23, 4, S, S), one(rec(AFFINE, m=(1, 0, 2 * S, 0, 1, 0), filt=BICUBIC),
                                                        rec(AFFINE, m=(1, 0, 0, 0, 1, -3 * S), filt=BILINEAR),
                                                        rec(AFFINE, m=inside, filt=BICUBIC), rec(AFFINE, m=inside, filt=BILINEAR))
    yield "affine_noise", noise(24, 4, S, S), one(rotation(17.0, S, S, BICUBIC), shear_x(0.21, BICUBIC), rotation(-9.0, S, S, BILINEAR),
                                                  translate_y(0.33, S, BICUBIC))
    yield "affine_wide", smooth_noise(25, 3, 16, 32), one(rotation(30.0, 32, 16, BICUBIC), shear_y(-0.3, BILINEAR),
                                                          translate_x(-0.45, 32, BICUBIC))
    yield "affine_tall", smooth_noise(26, 2, 48, 32), one(rotation(-30.0, 32, 48, BILINEAR), shear_x(0.3, BICUBIC))
    # two layers: a statistics op after an affine one, so that the fill enters the histogram / the mean
    S = 32
    yield "chain_stats", smooth_noise(30, 4, S, S), [
        [rotation(30.0, S, S, BICUBIC), rec(AUTOCONTRAST)], [translate_x(0.45, S, BILINEAR), rec(EQUALIZE)],
        [shear_y(0.3, BICUBIC), rec(CONTRAST, factor=1.7)], [rotation(-30.0, S, S, BILINEAR), rec(SHARPNESS, factor=1.9)]]
    yield "identity2", noise(31, 2, 16, 16), [[rec(IDENTITY), rec(IDENTITY)]] * 2
    # different ops per sample, an identity in either layer, 48 x 48
    S = 48
    yield "mixed", smooth_noise(32, 4, S, S), [
        [rec(IDENTITY), rec(COLOR, factor=1.8)], [rec(EQUALIZE), rec(IDENTITY)],
        [rec(SOLARIZE, 26), rotation(-27.0, S, S, BICUBIC)], [rec(SHARPNESS, factor=0.19), rec(POSTERIZE, 1)]]
    # three and four layers
    S = 32
    yield "layers3", smooth_noise(33, 2, S, S), [
        [shear_x(-0.3, BICUBIC), rec(IDENTITY), rec(EQUALIZE)], [rec(CONTRAST, factor=0.2), rec(AUTOCONTRAST), rec(INVERT)]]
    yield "layers4", smooth_noise(34, 2, S, S), [
        [rec(BRIGHTNESS, factor=1.5), translate_y(-0.2, S, BILINEAR), rec(COLOR, factor=0.3), rec(SOLARIZE_ADD, 60)],
        [rec(IDENTITY), rec(IDENTITY), rec(IDENTITY), rec(SHARPNESS, factor=1.4)]]
    # 68 x 64: more pixel quads (1088) than a workgroup has lanes, so the per-quad loops of the blends and the affine map go round twice
    yield "trips", smooth_noise(36, 2, 68, 64), [[rotation(-21.0, 64, 68, BICUBIC), rec(SHARPNESS, factor=1.8)],
                                                 [rec(CONTRAST, factor=0.4), shear_x(0.3, BILINEAR)]]
    # graph replay: one source, two tables
    g = smooth_noise(35, 2, 16, 16)
    yield "graph_a", g, [[rec(INVERT), rec(BRIGHTNESS, factor=0.6)], [rotation(12.0, 16, 16, BICUBIC), rec(IDENTITY)]]
    yield "graph_b", g, [[rec(IDENTITY), shear_x(0.25, BILINEAR)], [rec(EQUALIZE), rec(COLOR, factor=1.9)]]


def main():
    out = {}
    count = 0
    for name, src, table in cases():
        B, L = len(table), len(table[0])
        assert src.shape[0] == B and all(len(t) == L for t in table)
        out[name + ".src"] = src
        out[name + ".ops"] = np.array([[(r["op"], r["filt"], r["iarg"]) for r in t] for t in table], dtype=np.int32)
        out[name + ".factor"] = np.array([[r["factor"] for r in t] for t in table], dtype=np.float64)
        out[name + ".m"] = np.array([[r["m"] for r in t] for t in table], dtype=np.float64)
        out[name + ".fill"] = np.array(FILL, dtype=np.int32)
        out[name + ".out"] = pil_case(src, table, FILL)
        count += 1
    src = smooth_noise(40, 1, 16, 16)
    src[0, :, :2, :] = np.array([0, 255] * 8, dtype=np.uint8)                      # both clip ends, next to each other
    factors = np.linspace(0.1, 1.9, 64)
    out["sweep.src"], out["sweep.factors"], out["sweep.fill"] = src, factors, np.array(FILL, dtype=np.int32)
    out["sweep.out"] = np.stack([np.concatenate([pil_case(src, [[rec(op, factor=float(f))]], FILL) for f in factors])
                                 for op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS)])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f21_randaugment_pil.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases and the sweep, %d bytes" % (path, count, os.path.getsize(path)))


if __name__ == "__main__":
    main()
