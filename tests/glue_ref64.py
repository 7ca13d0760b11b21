"""Contracts of the glue kernels of csrc/misc.hip, written from the statements of include/vitres_hip.h in float64 or as pure indexing
on the CPU; the launch paths of their launchers; per-element bounds from first principles; inputs, canaries and case lists shared by
tests/test_glue_ref_host.py (CPU) and tests/test_gpu_glue.py (device).

Two kinds of contract:
  exact   -- the output is a copy, a cast (torch's CPU .to(dtype): round to nearest even), or ONE fp32 operation followed by one cast.
             Compared as integers of the element width by mismatches(); NaN positions must agree, payloads are not compared.
  bounded -- a sum of fp32 terms whose order the contract leaves open (atomics, unrolled loads).  |got - ref64| <= bound per element,
             u = 2^-24, gamma(k) = k u / (1 - k u); a 16-bit output adds half an ulp of the result at that type.

Every output lives inside a larger allocation (guarded()): the guard zones, the pad columns and the rows a kernel must leave alone
hold ONE NaN bit pattern (0x7fd5 per 16 bits: a NaN as bf16, fp16 and fp32), and the expected tensor holds the same pattern there, so
"not written" is part of every integer comparison.  Input regions that must not reach a result (masked columns, rows below `first`,
unmapped rows, pad columns of src_ld, token rows) hold NaN as well."""
import math

import torch

U = 2.0 ** -24
CANARY16 = 0x7fd5
CANARY32 = 0x7fd57fd5
GUARD = 64                       # elements before and after a guarded view (a multiple of 16 bytes for every type)
VR_OK, VR_EINVAL, VR_EALIGN, VR_EUNSUPPORTED = 0, -1, -2, -3
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT3 = [F32, BF16, F16]


def gamma(k):
    return k * U / (1.0 - k * U)


def name(dt):
    return str(dt)[6:]


# ---- integer views, canaries, guarded buffers ---------------------------------------------------------------------------------------------
def ibits(t):
    if t.dtype in (torch.int32, torch.int16):
        return t
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def canary_int(t):
    return CANARY32 if t.element_size() == 4 else CANARY16


def canary(n, dtype):
    """n elements of the canary pattern"""
    if dtype == torch.int32:
        return torch.full((n,), CANARY32, dtype=torch.int32)
    if dtype == F32:
        return torch.full((n,), CANARY32, dtype=torch.int32).view(F32)
    return torch.full((n,), CANARY16, dtype=torch.int16).view(dtype)


def canary_like(t):
    return canary(t.numel(), t.dtype).view(t.shape)


def mismatches(got, exp):
    """bool tensor: elements of `got` that break an exact contract.  Equal bits pass; two NaNs pass unless either is the canary (an
    expected canary wants the canary's bits: the element was not to be written; a canary where a value was expected was not written)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    gi, ei = ibits(got), ibits(exp)
    if got.dtype in (torch.int32, torch.int16):
        return gi != ei
    can = canary_int(exp)
    nan_ok = torch.isnan(got) & torch.isnan(exp) & (ei != can) & (gi != can)
    return ~((gi == ei) | nan_ok)


def guarded(t, off=0, device=None):
    """-> (whole, view): `t` copied into a canary-filled flat allocation of GUARD + off + numel + GUARD elements; `view` has t's shape
    and starts `off` elements after the guard (off != 0 misaligns it where a launcher selects on alignment)."""
    n = t.numel()
    whole = canary(GUARD + off + n + GUARD, t.dtype)
    whole[GUARD + off:GUARD + off + n] = t.reshape(-1)
    if device is not None:
        whole = whole.to(device)
    return whole, whole[GUARD + off:GUARD + off + n].view(t.shape)


def guards_intact(whole, n, off=0):
    w = ibits(whole.cpu())
    can = CANARY32 if w.dtype == torch.int32 else CANARY16
    return bool((w[:GUARD + off] == can).all()) and bool((w[GUARD + off + n:] == can).all())


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def pattern32(n, salt=0):
    """fp32 values that are a function of the flat index alone: finite, every mantissa bit in use (so casts round), exponents 2^-10 .. 2^9,
    neighbours along any axis differ in sign, exponent and mantissa"""
    i = torch.arange(n, dtype=torch.int64) + salt * 7919
    bits = (((i * 2654435761) >> 3) & 0x007fffff) | ((117 + (i * 5) % 20) << 23) | (((i * 3 + (i >> 4)) & 1) << 31)
    return _i64_to_f32(bits)


def _i64_to_f32(bits):
    bits = bits & 0xffffffff
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(torch.int32).view(F32)


def from_bits32(words):
    return _i64_to_f32(torch.tensor(list(words), dtype=torch.int64))


def pattern16(n, dtype, salt=0):
    """16-bit values from the flat index: finite in bf16 and in fp16 (bits below 0x7800), distinct for n < 61440"""
    i = torch.arange(n, dtype=torch.int64) + salt * 131
    v = (i * 7 + 1) % 0x7800 | (((i // 0x7800) & 1) << 15)
    v = torch.where(v >= 2 ** 15, v - 2 ** 16, v)
    return v.to(torch.int16).view(dtype)


def pattern(n, dtype, salt=0):
    return pattern32(n, salt) if dtype == F32 else pattern16(n, dtype, salt)


def signed_unit(shape, seed, dtype=F32):
    """|x| in [0.5, 2) with random signs, representable in `dtype`: a dropped, doubled or misplaced term misses by >= 0.5"""
    g = torch.Generator().manual_seed(seed)
    mag = 0.5 + 1.5 * torch.rand(shape, generator=g, dtype=torch.float64)
    sgn = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    x = (mag * sgn).float().to(dtype)
    return torch.where(x.float().abs() >= 2.0, (sgn * 1.984375).to(dtype), x)          # (a magnitude that rounded up to 2)


def split_unit(B, C, seed, dtype=F32):
    """[B, C] with random signs, |x| in [0.5, 1) for even samples and [1.25, 2) for odd ones: a neighbouring sample's value misses by
    >= 0.25 in every element, 128 half-ulps of bf16 at the smaller one (vr_token_mean_bwd's only fault is the wrong sample)"""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand((B, C), generator=g, dtype=torch.float64)
    odd = (torch.arange(B) % 2 == 1).view(B, 1)
    mag = torch.where(odd, 1.25 + 0.734375 * r, 0.5 + 0.4921875 * r)
    sgn = torch.where(torch.rand((B, C), generator=g) < 0.5, -1.0, 1.0).double()
    x = (mag * sgn).float().to(dtype)
    assert bool(((x.float().abs() >= 0.5) & (x.float().abs() < 2.0)).all())
    return x


def balanced_tokens(B, n, C, seed, dtype):
    """Token rows for vr_token_mean, [B, n, C] with |y| in [0.5, 2) and random signs, whose mean is exactly (+-)2^-8 per sample (n > 1):
    the rows come in pairs (+a, -a) in a random order, and one pair is (1.5, -(1.5 - n 2^-8)).  The mean of 196 free random terms is ~0.1
    and half a bf16 ulp of it (1e-4) would hide one dropped term (0.5 / 196 = 2.6e-3 against the 100x margin the host test asserts);
    with the mean at 2^-8 the 16-bit rounding term is 2^-17 and neighbouring samples still differ by 2^-7.  n == 1: the row itself,
    magnitudes 0.75 / 1.75 alternating by sample."""
    g = torch.Generator().manual_seed(seed)
    if n == 1:
        y = torch.tensor([0.75, 1.75])[torch.arange(B) % 2].view(B, 1, 1).expand(B, 1, C).clone()
        sgn = torch.where(torch.rand(B, 1, C, generator=g) < 0.5, -1.0, 1.0)
        return (y * sgn).to(dtype)
    assert n % 2 == 0 and n * 2.0 ** -8 <= 0.875
    half = n // 2
    a = signed_unit((B, half, C), seed + 1, dtype).float()
    y = torch.cat([a, -a], 1)
    y[:, 0, :] = 1.5
    sm = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).view(B, 1)
    y[:, half, :] = -(1.5 - n * 2.0 ** -8)
    y[:, [0, half], :] *= sm[:, :, None]
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(B)])           # per-sample order
    y = torch.gather(y, 1, perm[:, :, None].expand(B, n, C))
    out = y.to(dtype)
    assert torch.equal(out.float(), y)
    return out


# fp32 bit patterns every converting kernel must get right, for both 16-bit types (torch's CPU cast is the expectation for each)
EDGE_BITS = [
    0x00000000, 0x80000000,                                       # +-0
    0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0xbf818000,   # bf16 ties above an even / an odd mantissa and their neighbours
    0x3f801000, 0x3f803000, 0x3f800fff, 0x3f801001, 0xbf803000,   # fp16 ties above an even / an odd mantissa and their neighbours
    0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7f8000,               # bf16: largest fp32 that stays finite, the threshold, FLT_MAX
    0x477fe000, 0x477fefff, 0x477ff000, 0xc77ff000,               # fp16: 65504, 65519.996, 65520 (-> inf)
    0x7f800000, 0xff800000,                                       # +-inf
    0x7fc00000, 0x7f800001, 0xffc00001, 0x7f80ffff, 0x7fffffff,   # quiet and signalling NaNs (low-bits-only payloads included)
    0x00000001, 0x007fffff, 0x807fffff, 0x00008000, 0x00018000, 0x00400000,   # fp32 denormals (bf16 ties among them)
    0x33800000, 0x33000000, 0x33000001, 0x32ffffff, 0x33c00000,   # fp16: 2^-24, the tie at 2^-25, just above, just below, 1.5 2^-24
    0x387fc000, 0x387fe000, 0x38800000, 0xb3000001,               # fp16: largest subnormal, the tie to 2^-14, 2^-14, -(2^-25)+
]


def edge_values():
    return from_bits32(EDGE_BITS)


def with_edges(x, positions):
    """x (flat fp32) with the edge values written from each of `positions` on (those that fit)"""
    e = edge_values()
    x = x.clone()
    for p in positions:
        k = max(0, min(e.numel(), x.numel() - p))
        x[p:p + k] = e[:k]
    return x


# ---- half an ulp of a float64 result at a 16-bit type --------------------------------------------------------------------------------------
def half_ulp(v, dtype):
    """half the spacing of `dtype` at |v| (float64 tensor): 2^(e - 8) for bf16, 2^(e - 11) for fp16 with e = floor(log2 |v|), e no less than
    the type's smallest normal exponent (below it the subnormal spacing holds: 2^-24 for fp16); 0 for fp32"""
    if dtype == F32:
        return torch.zeros_like(v)
    p, emin = (8, -126) if dtype == BF16 else (11, -14)
    _, ex = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(ex, emin), torch.clamp(ex - 1, min=emin))
    return torch.ldexp(torch.ones_like(v), e - p)


def out_bound(ref, b32, dtype):
    """bound of the fp32 arithmetic plus the rounding of the stored value (taken at |ref| + b32: the fp32 value may sit in the next binade)"""
    return b32 + half_ulp(ref.abs() + b32, dtype)


def ratio(got, ref, bound, where=None):
    """worst |got - ref| / bound over the elements of `where`; a NaN or an error with a zero bound gives inf"""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    if where is not None:
        r = r[where]
    return float(r.max()) if r.numel() else 0.0


WORST = {}                       # kernel -> worst ratio seen (printed last by the GPU suite)


def record(kernel, r):
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    return r


# ======== exact contracts =====================================================================================================================
def cast_contract(out_before, src, n):
    """dst[i] = dtype(src[i]) for i < n"""
    out = out_before.clone()
    out.view(-1)[:n] = src.view(-1)[:n].to(out.dtype)
    return out


def cast_transpose_contract(dst_before, src, descs):
    """dst[dst_off + c * ld_dst + r] = bf16(src[src_off + r * cols + c]); descs: (src_off, dst_off, rows, cols, ld_dst)"""
    out = dst_before.clone()
    for so, do, r, c, ld in descs:
        m = src[so:so + r * c].view(r, c)
        idx = do + torch.arange(c)[:, None] * ld + torch.arange(r)[None, :]
        out[idx] = m.t().to(out.dtype)
    return out


def zero_ranges_contract(words_before, base, ranges, gate=1):
    """int32 words: [base + lo, base + lo + count) = 0 for every range, when the gate is non-zero"""
    out = words_before.clone()
    if gate != 0:
        for lo, cnt in ranges:
            out[base + lo:base + lo + cnt] = 0
    return out


def _relayout_index(A, B, C, src_ld, dst_ld):
    a = torch.arange(A).view(A, 1, 1)
    b = torch.arange(B).view(1, B, 1)
    c = torch.arange(C).view(1, 1, C)
    return (a * src_ld + b * C + c).reshape(-1), (a * dst_ld + c * B + b).reshape(-1)


def relayout_contract(dst_before, src, A, B, C, src_ld, dst_ld):
    """dst[a * dst_ld + c * B + b] = dst_dtype(src[a * src_ld + b * C + c]); same type: the source's bits"""
    si, di = _relayout_index(A, B, C, src_ld, dst_ld)
    out = dst_before.clone()
    if out.dtype == src.dtype:
        ibits(out)[di] = ibits(src)[si]                 # (a view of out: words move, whatever they spell)
    else:
        out[di] = src[si].to(out.dtype)
    return out


def relayout_add_contract(dst_before, src, A, B, C, src_ld, dst_ld):
    """dst[...] += src[...]: one fp32 add per element"""
    si, di = _relayout_index(A, B, C, src_ld, dst_ld)
    out = dst_before.clone()
    out[di] = out[di] + src[si]
    return out


def conv_w_flip_contract(dst_before, src):
    """dst[ci, (kh, kw, co)] = dtype(src[co, ci, 2 - kh, 2 - kw])"""
    Co, Ci = src.shape[:2]
    out = dst_before.clone()
    for ci in range(Ci):
        for kh in range(3):
            for kw in range(3):
                out[ci, (kh * 3 + kw) * Co:(kh * 3 + kw + 1) * Co] = src[:, ci, 2 - kh, 2 - kw].to(out.dtype)
    return out


def scale_mask_cast_contract(out_before, x, scale, keep, rps):
    """out[m, c] = dtype(fp32(x[m, c] * scale[m / rps])) for c < keep[m / rps], +0 otherwise whatever x holds"""
    M, C = x.shape
    s = torch.arange(M) // rps
    prod = x * scale[s].view(M, 1) if scale is not None else x.clone()
    if keep is not None:
        prod = torch.where(torch.arange(C).view(1, C) < keep[s].view(M, 1).long(), prod, torch.zeros_like(prod))
    out = out_before.clone()
    out[:] = prod.to(out.dtype)
    return out


def embed_cls_contract(x_before, tokens, pos, keep, T):
    """x[b, t, c] = tokens[t, c] + pos[t, c] (one fp32 add) for c < keep[b], +0 otherwise, t < T; the other rows stay"""
    B, N, C = x_before.shape
    out = x_before.clone()
    row = tokens[:T] + pos[:T]
    for b in range(B):
        k = C if keep is None else int(keep[b])
        out[b, :T, :k] = row[:, :k]
        out[b, :T, k:] = 0.0
    return out


def mask_rows_contract(x_before, keep, rps):
    """x[m, c] = +0 for c >= keep[m / rps]; the other elements keep their bits"""
    out = x_before.clone()
    for m in range(out.shape[0]):
        out[m, int(keep[m // rps]):] = 0.0
    return out


def _sr_taps(g):
    """(tap, oh, ow, ih, iw) of every in-image tap of the 3x3 / stride 2 / pad 1 window, as index tensors"""
    go = g // 2
    tap, oh, ow = torch.meshgrid(torch.arange(9), torch.arange(go), torch.arange(go), indexing="ij")
    ih, iw = 2 * oh - 1 + tap // 3, 2 * ow - 1 + tap % 3
    ok = (ih >= 0) & (ih < g) & (iw >= 0) & (iw < g)
    return tap[ok], oh[ok], ow[ok], ih[ok], iw[ok]


def sr_im2col_contract(col_before, y, B, g, C, T):
    """col[(b, oh, ow), (kh, kw, c)] = y[b, T + (2 oh - 1 + kh) g + (2 ow - 1 + kw), c]: the element's bits, +0 outside the image"""
    go = g // 2
    out = torch.zeros_like(col_before)
    tap, oh, ow, ih, iw = _sr_taps(g)
    ibits(out).view(B, go, go, 9, C)[:, oh, ow, tap, :] = ibits(y).view(B, T + g * g, C)[:, T + ih * g + iw, :]
    return out


def sr_resid_bwd_contract(dx_before, dout, B, g, Cin, Cout, accumulate, T):
    """dx[b, t, :] (+)= dout[b, t, :Cin] for t < T; dx[b, T + (ih, iw), :] (+)= 0.25 dout[b, T + (ih/2, iw/2), :Cin]"""
    go = g // 2
    d = dout.view(B, T + go * go, Cout)[:, :, :Cin]
    v = torch.empty(B, T + g * g, Cin)
    v[:, :T] = d[:, :T]
    p = torch.arange(g * g)
    v[:, T:] = 0.25 * d[:, T + (p // g // 2) * go + (p % g) // 2]
    out = dx_before.clone().view(B, T + g * g, Cin)
    out[:] = out + v if accumulate else v
    return out.view(dx_before.shape)


def im2col_patch_contract(col_before, img, smap, P, ldk):
    """col[(b, py, px), (c, i, j)] = dtype(img[map[b], c, py P + i, px P + j]); columns Cin P P .. ldk are +0"""
    _, Cin, H, W = img.shape
    src = img if smap is None else img[smap]
    B = src.shape[0]
    gh, gw, Kc = H // P, W // P, Cin * P * P
    out = col_before.clone().view(B, gh, gw, ldk)
    out[..., Kc:] = 0.0
    for c in range(Cin):
        for i in range(P):
            k0 = (c * P + i) * P
            out[..., k0:k0 + P] = src[:, c, i::P, :].reshape(B, gh, gw, P).to(out.dtype)
    return out.view(col_before.shape)


# ======== bounded contracts: -> (ref64, fp32 bound) =================================================================================================
def map_rows(M, rm):
    m = torch.arange(M)
    if rm is None or rm[0] == 0:
        return m
    rpi, rps, off = rm
    return (m // rpi) * rps + off + m % rpi


def colsum_ref(x, out_before, M, N, rm):
    """out[n] += sum_m x[map(m), n]: at most min(M, 128) terms per partial sum and ceil(M / 128) additions into out, in any order"""
    xs = x[map_rows(M, rm)][:, :N].double()
    k = min(M, 128) + (M + 127) // 128
    return out_before.double() + xs.sum(0), gamma(k) * (out_before.double().abs() + xs.abs().sum(0))


def batchsum_path(B, inner):
    bper = 16 if B >= 64 else (8 if B >= 16 else B)
    chunks = (B + bper - 1) // bper
    last = B - (chunks - 1) * bper
    return bper, chunks, {(min(bper, B) // 8, min(bper, B) % 8), (last // 8, last % 8)}


def batchsum_ref(x, out_before):
    B = x.shape[0]
    bper, chunks, _ = batchsum_path(B, 1)
    xs = x.double()
    return out_before.double() + xs.sum(0), gamma(bper + chunks) * (out_before.double().abs() + xs.abs().sum(0))


def token_mean_ref(y, first):
    """out[b, c] = mean over n in [first, N) of y[b, n, c]: n - 1 additions, the rounding of 1 / n and one product"""
    ys = y[:, first:].double()
    n = ys.shape[1]
    return ys.mean(1), gamma(n + 2) * ys.abs().sum(1) / n


def token_mean_bwd_ref(dmean, n):
    """dy[b, t, c] = dmean[b, c] / n: the rounding of 1 / n and one product"""
    d = dmean.double()
    return d / n, 2 * U * d.abs() / n


def sr_col2im_ref(dcol, B, g, C):
    """dy[b, (ih, iw), c] = sum of the taps of dcol that read that pixel (scatter form; at most four of them) -> ref, bound, taps hit"""
    go = g // 2
    d = dcol.double().view(B, go, go, 9, C)
    ref = torch.zeros(B, g * g, C, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    tap, oh, ow, ih, iw = _sr_taps(g)
    ref.index_add_(1, ih * g + iw, d[:, oh, ow, tap, :])
    mag.index_add_(1, ih * g + iw, d[:, oh, ow, tap, :].abs())
    return ref, gamma(3) * mag


def sr_resid_ref(x, B, g, Cin, T):
    """patch rows: 0.25 (p00 + p01 + p10 + p11) of the 2x2 block -> ref [B, go go, Cin], bound"""
    go = g // 2
    p = x.double().view(B, T + g * g, Cin)[:, T:].view(B, go, 2, go, 2, Cin)
    return 0.25 * p.sum((2, 4)).view(B, go * go, Cin), gamma(3) * 0.25 * p.abs().sum((2, 4)).view(B, go * go, Cin)


def sr_resid_exact(out_before, x, B, g, Cin, Cout, T):
    """token rows out[b, t, :Cin] = x[b, t, :] and pad columns Cin.. = +0 (all rows); patch rows' kept columns are left as they were"""
    go = g // 2
    out = out_before.clone().view(B, T + go * go, Cout)
    out[:, :T, :Cin] = x.view(B, T + g * g, Cin)[:, :T]
    out[:, :, Cin:] = 0.0
    return out.view(out_before.shape)


# ======== launch paths (misc.hip's launchers, as read) =================================================================================================
def cast_path(n):
    """-> (workgroups, groups of eight on the vector form, trailing elements on the scalar form, grid-stride passes)"""
    blocks = max(1, min(4096, (n // 8 + 255) // 256))
    stride = blocks * 256 * 8
    return blocks, n // 8, n % 8, (n + stride - 1) // stride


def ct_path(desc):
    """(src_off, dst_off, rows, cols, ld_dst) -> (wide tiles, ragged tiles) of a matrix whose buffers are 16-byte aligned at offset 0"""
    so, do, r, c, ld = desc
    aligned = c % 4 == 0 and ld % 8 == 0 and so % 4 == 0 and do % 8 == 0
    tiles = ((r + 63) // 64) * ((c + 63) // 64)
    wide = (r // 64) * (c // 64) if aligned else 0
    return wide, tiles - wide


def zero_bx(counts):
    return max(1, min(4096, (max(counts) // 16 + 255) // 256))


def zero_path(word_addr, count, bx):
    """one range at word address `word_addr` (base + lo, in 4-byte words from a 16-byte boundary) in a launch of bx workgroups ->
    (head, n4, x4 iterations of thread 0, x4 iterations of the last thread, remainder iterations of thread 0, tail)"""
    stride = bx * 256
    head = min(count, (4 - (word_addr & 3)) & 3)
    n4 = (count - head) >> 2

    def walk(i):
        it, k = 0, i
        while k + 3 * stride < n4:
            it, k = it + 1, k + 4 * stride
        rem = 0
        while k < n4:
            rem, k = rem + 1, k + stride
        return it, rem
    (i0, r0), (i1, _) = walk(0), walk(stride - 1)
    return head, n4, i0, i1, r0, count - head - 4 * n4


def relayout_path(A, B, C):
    total = A * B * C
    grid = min(4096, (total + 255) // 256)
    return grid, (total + grid * 256 - 1) // (grid * 256)


def im2col_patch_path(Cin, W, P, ldk, dtype, col_off=0):
    """-> (load form, store form), or VR_EUNSUPPORTED above the 64 KiB of LDS"""
    if Cin * P * W * 4 > 64 * 1024:
        return VR_EUNSUPPORTED
    st8 = dtype != F32 and ldk % 8 == 0 and (col_off * 2) % 16 == 0
    return "ld4" if W % 4 == 0 else "ld1", "st8" if st8 else "st1"


def _v8_grid(total):
    blocks = (total + 255) // 256
    grid = min(16384, blocks)
    return grid, (total + grid * 256 - 1) // (grid * 256)


def sr_im2col_path(B, g, C, dtype, y_off=0, col_off=0):
    """-> ("v8", workgroups, passes) or ("scalar", workgroups, 1); offsets in elements from a 16-byte boundary"""
    if dtype in (BF16, F16) and C % 8 == 0 and (y_off * 2) % 16 == 0 and (col_off * 2) % 16 == 0:
        return ("v8",) + _v8_grid(B * (g // 2) ** 2 * 9 * (C // 8))
    return "scalar", B * (g // 2) ** 2 * 9, 1


def sr_col2im_path(B, g, C, dtype, dcol_off=0, dy_off=0):
    if dtype == F16:
        return VR_EUNSUPPORTED
    if dtype == BF16 and C % 8 == 0 and (dcol_off * 2) % 16 == 0 and (dy_off * 2) % 16 == 0:
        return ("v8",) + _v8_grid(B * g * g * (C // 8))
    return "scalar", B * g * g, 1


def colsum_path(M, N):
    """-> (column groups of 256, row chunks of 128, rows of the last chunk)"""
    return (N + 255) // 256, (M + 127) // 128, M - ((M + 127) // 128 - 1) * 128


def scale_mask_cast_path(M, C):
    """-> (workgroups of four rows, float4 per lane, lanes of the last float4 step that are live)"""
    return (M + 3) // 4, (C + 255) // 256, (C % 256) // 4


def token_mean_path(B, C):
    """-> (workgroups, columns per thread, threads live in the last step)"""
    return B, (C + 255) // 256, C % 256


# ======== case lists ===========================================================================================================================
CAST_N = [1, 7, 8, 9, 2047, 2048, 2049, 4096 + 3]
CAST_BIG = 8388608 + 8 * 3 + 5                       # second grid-stride pass, not a multiple of the pass

# one launch of vr_cast_transpose_batch: (src_off, dst_off, rows, cols, ld_dst); offsets are assigned by ct_layout()
CT_SHAPES = [(128, 64, 128, 0, 0),       # two wide tiles: the many-tile matrix
             (1, 1, 1, 0, 0),            # one ragged tile beside it: its second workgroup returns early
             (64, 66, 64, 0, 0),         # cols % 4 != 0
             (64, 64, 68, 0, 0),         # ld_dst % 8 != 0, canary pads between rows and ld_dst
             (64, 64, 72, 1, 0),         # src_off % 4 != 0
             (64, 64, 72, 0, 4),         # dst_off % 8 != 0
             (70, 68, 72, 0, 0),         # one wide tile, three ragged ones in the same matrix
             (1, 5, 8, 0, 0), (5, 1, 5, 0, 0),
             (64, 64, 64, 0, 0)]         # no pad at all


def ct_layout():
    """descriptors of CT_SHAPES with 16-byte aligned offsets (plus the misalignment each shape asks for) and canary gaps between matrices
    -> descs, src elements, dst elements"""
    descs, so, do = [], 0, 0
    for r, c, ld, ms, md in CT_SHAPES:
        descs.append((so + ms, do + md, r, c, ld))
        so += (ms + r * c + 4 + 7) // 8 * 8
        do += (md + c * ld + 8 + 7) // 8 * 8
    return descs, so, do


ZERO_COUNTS = [0, 1, 2, 3, 4, 5, 8, 4095, 4096, 4097, 4100]
ZERO_EDGE_COUNTS = [16 * 256 * k + d for k in (1, 2) for d in (-4, 0, 4, 5)]


def zero_launches():
    """-> [(tag, base word offset, [(lo, count)])]: every launch of the zero_ranges test.  Ranges of one launch are laid out in order with a
    gap of 5 untouched words (so the next lo's residue is set by hand), except the adjacent ones."""
    out = []
    for k, counts in enumerate((ZERO_COUNTS[:6], ZERO_COUNTS[6:])):                  # 24 + 20 ranges: lo % 4 x count
        ranges, at = [], 8
        for cnt in counts:
            for res in range(4):
                lo = (at + 3) // 4 * 4 + res
                ranges.append((lo, cnt))
                at = lo + cnt + 5
        out.append(("cross%d" % k, 0, ranges))
    for cnt in ZERO_EDGE_COUNTS:                                                     # alone in their launch: bx comes from them
        for res in range(4):
            out.append(("edge", 0, [(4 + res, cnt)]))
    out.append(("short+long", 0, [(5, 3), (16, 100000)]))
    out.append(("long+short", 0, [(8, 100000), (100000 + 8 + 6, 3), (100000 + 8 + 11, 2)]))
    out.append(("adjacent", 0, [(3, 7), (10, 4096), (4106, 1), (4107, 0), (4107, 9)]))
    out.append(("24 ranges", 0, [(9 * i + (i & 3), 5) for i in range(24)]))
    for b in (1, 2, 3):                                                              # a base that is only 4-byte aligned
        out.append(("base+%d" % b, b, [(0, 4097), (4100 + 3, 6), (4120, 4096)]))
    return out


def zero_words(n):
    """non-zero int32 words, distinct by index"""
    i = torch.arange(n, dtype=torch.int64)
    w = ((i * 2654435761) & 0x7fffffff) | 1
    return w.to(torch.int32)


# (A, B, C, src pad, dst pad)
RELAYOUT_CASES = [(3, 5, 7, 3, 5), (4, 1, 37, 3, 11), (1, 1, 1000, 0, 0), (2, 9, 4, 0, 1), (5, 3, 1, 2, 0), (1, 300, 3, 0, 0)]
RELAYOUT_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32), (F32, F16), (F16, F16), (F16, F32)]
RELAYOUT_BIG = (3, 7, 49933)                          # 1 048 593 elements: a second pass of 17
CONV_W_FLIP = [(7, 5), (5, 7), (1, 1)]                # Co x Ci x 9 = 315: two workgroups, the second partly filled

COLSUM_M, COLSUM_N = [1, 127, 128, 129, 300], [1, 255, 256, 257]
COLSUM_MAP = (5, 7, 2)
BATCHSUM_B, BATCHSUM_INNER = [1, 7, 8, 9, 15, 16, 17, 23, 63, 64, 65], [1, 255, 256, 257]
SMC_M, SMC_C = [1, 3, 4, 5, 9], [4, 252, 256, 260, 1028]
TM_FIRST, TM_N, TM_C = [0, 1, 2], [1, 2, 16, 196], [1, 255, 256, 257, 520]

# (Cin, H, W, P): H != W everywhere; W % 4 both ways for P = 2 and 14
PATCH_GEOM = [(3, 4, 6, 2), (3, 6, 4, 2), (3, 14, 21, 7), (3, 28, 42, 14), (3, 42, 28, 14), (2, 32, 48, 16)]
PATCH_MAP = [2, 0, 2]                                 # a repeat; image 1 is never read and holds NaN


def patch_ldks(Kc):
    return [Kc, (Kc + 7) // 8 * 8, Kc + 3]


SR_G, SR_T, SR_C = [2, 4, 6, 14], [1, 2], [8, 72, 76, 100]
SR_RESID = [(257, 257), (100, 257)]
SR_IM2COL_BIG = (9512, 14, 8)                         # 4 194 792 groups of eight: 488 into the second pass
SR_COL2IM_BIG = (21400, 14, 8)                        # 4 194 400 groups


def smc_keep(C, S):
    """keep counts of S samples cycling through {0, 1, 3, C - 1, C}: 1, 3 and C - 1 cut a float4"""
    vals = [0, 1, 3, C - 1, C]
    return torch.tensor([vals[(s + C // 4) % 5] for s in range(S)], dtype=torch.int32)


# ======== inputs of the bounded kernels (shared by the host and the device suite) ======================================================================
def colsum_inputs(M, N, rm, dt):
    """x [rows, ld] with NaN in the pad columns and in the rows the map skips; out_before non-zero -> x, out_before, ld"""
    ld = N + 3
    rows = map_rows(M, rm)
    x = canary((int(rows.max()) + 1) * ld, dt).view(-1, ld)
    x[rows, :N] = signed_unit((M, N), M * 1000 + N, dt)
    return x, signed_unit((N,), M + N), ld


def batchsum_inputs(B, inner):
    """x [B + 1, inner]: the row behind the batch is NaN (a chunk that runs one sample too far reads it); out_before non-zero"""
    x = canary((B + 1) * inner, F32).view(B + 1, inner)
    x[:B] = signed_unit((B, inner), B * 1000 + inner)
    return x, signed_unit((inner,), B + inner)


def token_inputs(first, n, C, dt, B=2):
    """y [B, first + n, C]: rows below `first` are NaN"""
    y = canary(B * (first + n) * C, dt).view(B, first + n, C)
    y[:, first:] = balanced_tokens(B, n, C, first * 1000 + n + C, dt)
    return y
