"""float64 statement of the random-erasing noise contract (include/vitres_hip.h: vr_random_erase and the *_erase forms of the uint8
entries) with a derived per-element bound on what the device's fp32 arithmetic may differ by.  numpy only, CPU only; never imported by
the product.

The contract
------------
    (r0, r1, r2, r3) = Philox4x32-10(counter = (w, b + (domain << 24), call_lo, call_hi), key = (seed_lo, seed_hi))
    domain 0 ('pixel'): w = ((c H + y) W + x) // 4, the aligned quad; the four values are pixels 4 (x // 4) .. + 3 of row y, channel c
    domain 1 ('rand'):  w = the rectangle's index; the four values are the colours of channels 0..3
    u1 = ((r >> 8) + 1) 2^-24 in (0, 1],  u2 = (r' >> 8) 2^-24 in [0, 1)   for (r, r') = (r0, r1) and (r2, r3)
    rad = sqrt(-2 ln u1),  ang = 2 pi u2,  z = rad cos(ang),  z' = rad sin(ang)
    'const' fills +0.0.  Rectangles [y0, y1) x [x0, x1) over all channels, the later one winning where they overlap.

Philox is integer arithmetic and is restated in uint64 (products of two 32-bit words fit).  u1 and u2 are exact in fp32 and in float64.
Everything after them is evaluated here in float64; the device evaluates it in fp32 as

    rad = sqrtf(-2 * logf(u1)),  ang = fl(TWO_PI_F32 * u2),  z = fl(rad * cosf(ang)),  z' = fl(rad * sinf(ang)).

The bound
---------
u = 2^-24 is the unit roundoff of an fp32 operation; an error of k ulp of a result v is at most 2 k u |v| (ulp(v) <= 2^-23 |v|).
ULP figures of the device functions: the ROCm device library builds its float functions to the OpenCL single-precision conformance
limits -- log <= 3 ulp, sqrt <= 3 ulp, sin and cos <= 4 ulp (OpenCL C specification, "Relative error as ULPs").  The ROCm installation
ships no document that states the figures for its release, so they are ASSUMED here (HIP's own sqrtf is correctly rounded by default,
0.5 ulp: 3 is the conservative figure).  First order, per element:

    L = -2 ln u1: the multiplication by -2 is exact, so |dL| <= 6 u L.  (u1 = 1: logf(1) = 0 exactly, rad = 0, z = 0.)
    rad = sqrt(L): half the relative error of L plus the root's own 3 ulp:            |drad| <= (3 u + 6 u) rad = 9 u rad
    ang: the fp32 constant is off 2 pi by d2pi = |TWO_PI_F32 - 2 pi| / (2 pi) (2.8e-8), the product rounds once:
                                                                                        |dang| <= (d2pi + u) ang
    cos / sin: the argument's error passes through with slope <= 1, the function adds 4 ulp of a value <= 1 (ulp(1) = 2^-23):
                                                                                        |dtrig| <= |dang| + 8 u
    z = fl(rad trig):                                          |dz| <= rad |dtrig| + |z| (9 u + u)

and, as in tests/rowstat_ref64.py and attn_ref64.py, the first-order bound is multiplied by 2 -- the one margin -- and by nothing else:

    bound = 2 (rad ((d2pi + u) ang + 8 u) + 10 u |z|)            <= 1.9e-5 at the extremes rad = 5.77, ang = 2 pi.

|z| <= rad <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.768..., the largest value the contract can produce.
"""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
MODES = {"const": 0, "rand": 1, "pixel": 2}
U32 = 2.0 ** -24
TWO_PI_F32 = float(np.float32(2 * math.pi))
D2PI = abs(TWO_PI_F32 - 2 * math.pi) / (2 * math.pi)
Z_MAX = math.sqrt(48 * math.log(2))


def philox4x32_10(counter, key):
    """counter: integer array [..., 4]; key: (k0, k1).  Returns the uint32 words [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def box_muller(words):
    """uint32 words [..., 4] -> (z float64 [..., 4], bound [..., 4]): the contract's four normal values and how far an fp32
    evaluation may be from each."""
    w = words.astype(np.uint64)
    z, bound = np.empty(words.shape, dtype=np.float64), np.empty(words.shape, dtype=np.float64)
    for h in (0, 1):
        u1 = ((w[..., 2 * h] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * U32
        u2 = (w[..., 2 * h + 1] >> np.uint64(8)).astype(np.float64) * U32
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 2 * math.pi * u2
        for k, trig in ((0, np.cos), (1, np.sin)):
            v = rad * trig(ang)
            z[..., 2 * h + k] = v
            bound[..., 2 * h + k] = 2 * (rad * ((D2PI + U32) * ang + 8 * U32) + 10 * U32 * np.abs(v))
    return z, bound


def _counter(w0, b, domain, call):
    w0 = np.asarray(w0, dtype=np.uint64)
    c = np.empty(w0.shape + (4,), dtype=np.uint64)
    c[..., 0], c[..., 1], c[..., 2], c[..., 3] = w0, b + (domain << 24), call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF
    return c


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def quad_noise(seed, call, b, quads):
    """Domain 0 for the quad indices `quads` of sample b: (z [n, 4], bound [n, 4])."""
    return box_muller(philox4x32_10(_counter(quads, b, 0, call), _key(seed)))


def pixel_noise(seed, call, b, C, H, W):
    """Domain 0 over a whole sample: (z [C, H, W], bound [C, H, W]); W % 4 == 0."""
    assert W % 4 == 0
    z, bound = quad_noise(seed, call, b, np.arange(C * H * W // 4))
    return z.reshape(C, H, W), bound.reshape(C, H, W)


def rect_colours(seed, call, b, r):
    """Domain 1: the colours of rectangle r of sample b for channels 0..3: (z [4], bound [4])."""
    return box_muller(philox4x32_10(_counter(r, b, 1, call), _key(seed)))


def erase(x, rects, mode, seed, call):
    """The contract applied to a normalised batch x [B, C, H, W] (array-like, fp32 values): returns (out, inside, bound), float64
    [B, C, H, W] arrays -- out holds x outside the rectangles and the float64 fill inside, `inside` is the boolean mask of the erased
    elements, bound the per-element allowance of an fp32 evaluation (0 outside and for 'const')."""
    x = np.asarray(x, dtype=np.float64)
    rects = np.asarray(rects)
    B, C, H, W = x.shape
    assert rects.shape[0] == B and rects.shape[2] == 4 and mode in MODES and C <= 4
    out, inside, bound = x.copy(), np.zeros(x.shape, dtype=bool), np.zeros(x.shape)
    for b in range(B):
        noise = pixel_noise(seed, call, b, C, H, W) if mode == "pixel" and (rects[b, :, 0] < rects[b, :, 1]).any() else None
        for r, (y0, y1, x0, x1) in enumerate(rects[b]):
            if y0 >= y1 or x0 >= x1:
                continue
            inside[b, :, y0:y1, x0:x1] = True
            if mode == "pixel":
                out[b, :, y0:y1, x0:x1], bound[b, :, y0:y1, x0:x1] = noise[0][:, y0:y1, x0:x1], noise[1][:, y0:y1, x0:x1]
            elif mode == "rand":
                z, bd = rect_colours(seed, call, b, r)
                out[b, :, y0:y1, x0:x1], bound[b, :, y0:y1, x0:x1] = z[:C, None, None], bd[:C, None, None]
            else:
                out[b, :, y0:y1, x0:x1], bound[b, :, y0:y1, x0:x1] = 0.0, 0.0
    return out, inside, bound
