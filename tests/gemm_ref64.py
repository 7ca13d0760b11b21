"""float64 statement of vr_gemm's contract (include/vitres_hip.h) -- forward, data gradient and weight gradient, every epilogue -- with
derived per-element error bounds, the case table of tests/test_gpu_gemm.py and exact-probe operands.  CPU only.  Written from the header,
not from tests/emu_kernels.py: the emulation stays a second, independent statement (tests/test_gemm_ref_host.py holds the two together).

The contract
------------
forward / data gradient (a_trans = 0).  A is [*, lda] with K contiguous, logical row m is stored at a_map(m); B is [N, ldb] (b_trans = 0)
or [K, ldb] (b_trans = 1: the forward's weight as it is); output row m is stored at c_map(m), s = m // rows_in is the row's sample
(rows_in = 0: one sample), map(m) = (m // rpi) rps + off + m % rpi.  In this order:

    1. v = sum_k A[m, k] B[n, k]  (+ bias[n])  (+ pos[m % rows_in][n])
    2. act = 1: u = v;  C = u and C2 = gelu(u) (dual store),  C = gelu(u) alone without C2.   gelu(u) = u Phi(u) is taken from the fp32 u,
       act = 2 (no dact_u): C = gelu'(u) = Phi(u) + u phi(u), C2 = gelu(u).                    not from the rounded C.
       act = 3: C = relu(u), a NaN kept (v <= 0 ? 0 : v).
    3. dact_u given: v *= gelu'(dact_u[c_map(m), n])  (act = 0), or v *= dact_u[c_map(m), n] as it is (act = 2).
    4. keep_n: column n of row m is kept iff (n % n_period if n_period > 0 else n) < keep_n[s].  A masked element is exactly +0 -- of C
       and of C2, whatever v holds (NaN included): the kernels SELECT, they do not multiply by a 0 / 1 mask.
    5. A keep value -(k + 2) (the DropPath marker of a sample inside a group of width k) reads as keep 0; so does every negative keep.
    6. v *= scale[s]    (a product: a kept NaN or inf times scale 0 is NaN; a masked +0 times a finite scale stays 0)
    7. v += resid[c_map(m), n]    (fp32, ldc layout; may be C itself)
    8. round to the output type (nearest even; fp16 overflows to +-inf above 65504 + half an ulp, common.h).
    Steps 6 and 7 do not exist in the act forms (the kernels ignore scale / resid there; the tests never pass them).

weight gradient (a_trans = b_trans = 1).  A is [T, lda] (= dY, token t at a_map(t)), B is [T, ldb] (= X, token t at b_map(t)), K = T:

    G[m, n] = sum_t A[t, m] B[t, n],   g[m] = sum_t A[t, m]
    atomic = 1:  C[c_map(m), n] += G,  bias_grad[m] += g         atomic = 2:  C = G,  bias_grad = g  (overwritten, fully masked tiles are
    written as zeros: a destination full of NaN comes back finite)

Operand contract (what the caller promises; the case builders below keep every promise and fill everything outside it with NaN):
    * keep_k (k_period): A[m, k] == 0 for (k % k_period if k_period > 0 else k) >= keep_k[s(m)]; the kernels skip those K slices.
      Weight gradient: the samples are those of the tokens; keep_k promises A[t, m] == 0 for m beyond keep_k[s(t)] (output ROWS), keep_n
      promises B[t, n] == 0 for n beyond keep_n[s(t)] (output COLUMNS).  Rows / columns beyond the largest keep of the launch's samples
      are therefore exact zero gradients: unchanged under atomic = 1, zero under atomic = 2.
    * K-contiguous operand rows are READABLE AND ZERO in columns K .. roundup(K, chunk), chunk = 8 (16-bit) or 4 (fp32) elements -- one
      16-byte load; gemm_validate refuses lda / ldb below that.
    * Columns roundup(K, chunk) .. lda / ldb are never read (the builders put NaN there).  Contraction-major operands (b_trans, and both
      operands of the weight gradient) may be read in their row padding up to roundup(rows, 8): it only reaches outputs nobody stores.
    * What a launch must not write: ldc padding, rows beyond M, rows c_map does not hit.  The tests fill them with a NaN of a fixed
      bit pattern and compare bits.

The bounds
----------
u32 = 2^-24 (unit roundoff of an fp32 operation), MFMA = 2^-23 (stem_ref64), u = 2^-8 / 2^-11 / 0 for a bf16 / fp16 / fp32 output.  All
bounds are per element and first order, and are multiplied by 2 at the end -- the project's one margin -- and by nothing else.  With
S = sum_k |A[m, k]| |B[n, k]|:

MFMA sums.  attn_ref64's model, held on the MI355X for the 16-bit MFMAs: products of 16-bit operands are exact in fp32 and a K-term
accumulation costs  dacc = K 2^-23 S.  The fp32 kernel (mfma_f32_32x32x2f32, gemm.hip) rounds its products: one rounding per product and
one per add is 2 K u32 S -- the same number.  Nobody has measured that instruction's internal rounding: the fp32 bound rests on this
derivation, not on a measurement.  The 64-wide slices, the 16- / 32-deep MFMA steps and the tile shapes only re-order the same K terms.
K-split shares (k_shares 2 .. 4) add their fp32 partial tiles in share order, every partial sum at most S:  + (shares - 1) u32 S.
Weight gradients.  atomic = 1: `split` workgroups add their partial sums with fp32 atomics, in any order, onto `before`; every
intermediate is at most S + |before|:  + split u32 (S + |before|).  `split` is what the launch really uses: tn_split() restates
vr_gemm_tn_launch's rule, tn_group_splits() vr_gemm_tn_group_launch's, general_split() launch1's, with the CU count as an argument; the
tests mostly pass split_k themselves.  The share count is what vr_gemm_ntk_launch clamps to (lean_shares()).
atomic = 2: one workgroup per tile, nothing added.  bias_grad is the same sum with |A| for S (MFMAs against ones, or fp32 row sums).

Epilogue.  The bias add and the pos add round once each, relative to a value of at most |acc| + |bias| + |pos|:
    dpre = dacc + (#terms) u32 (|acc| + |bias| + |pos|)
store forms:  times d = gelu'(dact_u) or dact_u:  dv = dpre |d| + |pre| dd + u32 |v|   (dd: the evaluation error of gelu', 0 for act = 2)
    scale: dv |scale| + u32 |v scale|;   residual: + u32 |out|;   output: + u |out|.   Masked elements have bound 0 (resid is returned
    bit for bit); so have the exact probes.
GELU forms:   du = dpre;  C = u: du + u |u|;  gelu(u): LIP1 du + eg(u) + u |g|;  gelu'(u): LIP2 du + ed(u) + u |g'|;  relu: du + u |r|,
    LIP1 = sup |gelu'| < 1.13, LIP2 = sup |gelu''| < 0.8 (both checked on the grid of the host test).  gelu is smooth: no element of this
    suite is "undecided" -- every keep mask is decided by integers and relu is 1-Lipschitz.

GELU evaluation error, with x = |u| / sqrt 2, e = exp(-x^2), Phi(u) = 1 - tail or tail, tail = erfc(x) / 2:
  fp32 operands (gelu_f / dgelu_f: erff and __expf).  The HIP math API lists erff at 4 ULP = 8 u32 |erf|; its argument carries 2 u32 (the
    constant and the product), worth 2 u32 sup|x erf'(x)| < u32; 1 + erf rounds once:  dPhi = (8 + 1) u32 / 2 + u32 Phi <= 5.5 u32, ABSOLUTE
    (for u << 0 the sum 1 + erf cancels: the contract has to admit it).  eg = |u| dPhi + u32 |g|.  phi(u): the exponent -u^2/2 carries
    u32 from its product and 2 u32 inside __expf (rowstat_ref64), v_exp_f32 2 u32, the constant and its product 2 u32:
    dphi = phi u32 (1.5 u^2 + 4) + 2^-126;   ed = dPhi + |u| dphi + 2 u32 (Phi + |u| phi).
  16-bit operands (gelu_terms_fast: Abramowitz-Stegun 7.1.26 in fp32 with v_rcp_f32 and __expf).  The approximation itself is an
    algorithmic term the contract admits: |d Phi| <= AS_CDF = 0.75e-7 absolute -- half of A-S's 1.5e-7 for erf, NOT taken on trust: the
    host test evaluates the polynomial in float64 on a dense grid of |x| <= 10 against math.erf and asserts the maximum below AS_CDF.
    The fp32 evaluation: x 2 u32; t = rcp(fma(p, x, 1)): the fma 1, the argument's 2 (times p x / (1 + p x) < 1), v_rcp_f32 1 ULP = 2:
    5 u32 relative; e: x^2 carries 5 u32, __expf 2 u32 on the exponent, v_exp_f32 2 u32:  the = u32 (7 x^2 + 2);  P = t poly(t): the
    five Horner roundings are worth 5 u32 sum|a_i| (SA = 4.4753), t's error 5 u32 |t P'(t)| <= 5 u32 sum i |a_i| (TP = 16.198; crude,
    and still below the 16-bit output rounding wherever it matters);  0.5 poly t e: 3 u32 more;  1 - tail: u32 Phi:
        dtail = AS_CDF + tail (the + 3 u32) + (e / 2) 5 u32 (SA + TP) + 2^-126,     dPhi = dtail + u32 Phi
        eg = |u| dPhi + u32 |g|;    dphi = phi (the + 2 u32) + 2^-126;    ed = dPhi + |u| dphi + u32 |g'|  (one fma).
  Non-finite u, from the float64 formulas (and both device implementations agree): gelu(NaN) = gelu'(NaN) = NaN, gelu(+inf) = +inf,
    gelu(-inf) = -inf * 0 = NaN, gelu'(+-inf) = Phi + (+-inf) * 0 = NaN.  Finite |u| up to 40 is ordinary: e underflows to 0, Phi is 0 or 1.

Exact probes.  Operands are small integers -- A has at most 32 entries of +-1 per row, B holds 1 .. 3 with signs, bias / pos / resid are
small integers, scale and the saved derivative are powers of two -- so every partial sum, in any order, is an integer below 2^24 and
every final value is an integer of magnitude <= 256: exact in bf16, fp16 and fp32.  Their bound is 0: torch.equal against a reference
computed in any precision.  The workload-sized dispatch cases use them and need no float64 matmul.

`worst_ratio`, `F64`, `U32`, `f64`, `unit_roundoff` are rowstat_ref64's, `MFMA` and `nonfinite_ratio` stem_ref64's.
"""
import zlib

import torch

from rowstat_ref64 import F64, U32, TINY, f64, unit_roundoff, worst_ratio          # noqa: F401  (re-exported to the tests)
from stem_ref64 import MFMA, nonfinite_ratio, relu64                                # noqa: F401

F32 = torch.float32
BF16 = torch.bfloat16
F16 = torch.float16
DTYPES = [F32, BF16, F16]
NAN = float("nan")
SQRT1_2 = 0.70710678118654752
INV_SQRT_2PI = 0.39894228040143268

# Abramowitz-Stegun 7.1.26 as common.h writes it
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
AS_CDF = 0.75e-7                                   # asserted against math.erf on the grid (test_gemm_ref_host.py)
AS_SA = sum(abs(c) for c in AS_A)
AS_TP = sum((i + 1) * abs(c) for i, c in enumerate(AS_A))
LIP1 = 1.13                                        # sup |gelu'|
LIP2 = 0.8                                         # sup |gelu''|


def as_erfc_scaled(x):
    """t poly(t) of A-S 7.1.26 in float64: erfc(x) exp(x^2) for x >= 0 (tensor or float)"""
    t = 1.0 / (1.0 + AS_P * x)
    p = AS_A[4]
    for c in (AS_A[3], AS_A[2], AS_A[1], AS_A[0]):
        p = p * t + c
    return p * t


def cdf64(u):
    # erfc keeps the lower tail: 0.5 (1 + erf) would cancel, and the contract is the function, not one way to write it
    return 0.5 * torch.special.erfc(-u * SQRT1_2)


def pdf64(u):
    return INV_SQRT_2PI * torch.exp(-0.5 * u * u)


def gelu64(u):
    return u * cdf64(u)


def dgelu64(u):
    return cdf64(u) + u * pdf64(u)


def gelu_errors(u, fast):
    """-> (eg, ed): evaluation error bounds of gelu(u) and gelu'(u) for an exact fp32 u (float64 tensors), first order, no factor 2"""
    au = u.abs()
    cdf, pdf = cdf64(u), pdf64(u)
    g, d = u * cdf, cdf + u * pdf
    if not fast:
        dphi_c = 5.5 * U32
        dpdf = pdf * U32 * (1.5 * u * u + 4) + TINY
        return au * dphi_c + U32 * g.abs(), dphi_c + au * dpdf + 2 * U32 * (cdf + au * pdf)
    x2 = 0.5 * u * u
    e = torch.exp(-x2)
    the = U32 * (7 * x2 + 2)
    tail = torch.minimum(cdf, 1 - cdf)
    dtail = AS_CDF + tail * (the + 3 * U32) + 0.5 * e * 5 * U32 * (AS_SA + AS_TP) + TINY
    dphi_c = dtail + U32 * cdf
    dpdf = pdf * (the + 2 * U32) + TINY
    return au * dphi_c + U32 * g.abs(), dphi_c + au * dpdf + U32 * d.abs()


# ---- the launch rules of the weight gradient, restated (gemm_tn.hip vr_gemm_tn_launch, gemm.hip launch1) ---------------------------------
def group_pure(rows, G):
    return G > 1 and rows % G == 0


def group_split(split, T, m_groups, needs_pure=False):
    split = max(1, split)
    if not group_pure(T, m_groups):
        return split
    if split < m_groups and not needs_pure:
        return split
    return max(1, (split + m_groups // 2) // m_groups) * m_groups


def tn_split(No, Ki, T, n_cu, split_k=0, atomic=1, m_groups=0):
    """token splits of a single bf16 weight-gradient launch on gemm_tn.hip"""
    if atomic == 2:
        return 1
    tiles = ((No + 127) // 128) * ((Ki + 127) // 128)
    if split_k <= 0:
        split = ((T + 63) // 64 + 31) // 32
        by_fill = (4 * n_cu + tiles - 1) // tiles
        split_k = max(1, min(split, by_fill))
    return group_split(split_k, T, m_groups)


def tn_group_splits(dims, T, n_cu, atomics, sched=0, m_groups=0):
    """[split]: token splits of every problem of a vr_gemm_group launch (vr_gemm_tn_group_launch; dims = [(No, Ki)], one T and one
    m_groups, automatic splits, no unwritten-tile operands).  Store-form problems (atomic = 2) never split."""
    slices = (T + 63) // 64
    if 2 not in atomics and (sched & 0x10000):              # the 8-wave kernel: one split for the whole group, by its cost model
        tiles = sum(((No + 127) // 128) * ((Ki + 127) // 128) for No, Ki in dims)
        G = m_groups if group_pure(T, m_groups) else 1
        best, best_s, sq = -1, 1, 1
        while sq <= 64:
            per = (slices + sq - 1) // sq
            if per < 4 and sq > 1:
                break
            cost = ((tiles * sq + n_cu - 1) // n_cu) * (per + 40)
            if best < 0 or cost < best:
                best, best_s = cost, sq
            sq += (G - sq if sq < G else G) if G > 1 else 1
        return [best_s] * len(dims)
    tw = 64 if all(a == 2 for a in atomics) else 128
    work = sum(((No + tw - 1) // tw) * ((Ki + tw - 1) // tw) * slices for No, Ki in dims)
    spw = min(32, max(8, work // (2 * n_cu)))               # slices per workgroup: ~2 workgroups per CU in total, 8 - 32 slices each
    return [1 if a == 2 else group_split((slices + spw - 1) // spw, T, m_groups) for a in atomics]


def lean_shares(K, k_shares):
    """shares a lean-loop launch really uses (vr_gemm_ntk_launch): at most 4 and at most half the 64-wide slices"""
    return min(min(k_shares, 4), max(1, (K // 64) // 2)) if k_shares > 1 else 1


def general_split(No, Ki, T, split_k=0, shared=False):
    """-> (split, big): token splits and the 256 x 256 persistent tile of gemm.hip's weight gradient (launch1)"""
    big_tiles = ((No + 255) // 256) * ((Ki + 255) // 256)
    want = max(1, min(T // 512, 1 << 16))
    big = (not shared) and No >= 192 and Ki >= 192 and big_tiles * want >= 192
    tiles = big_tiles if big else ((No + 127) // 128) * ((Ki + 127) // 128)
    if split_k <= 0:
        split_k = max(1, min(want, max(1, 1024 // tiles)))
    return split_k, big


def tn_token_ranges(T, split, m_groups=0):
    """[(kbeg, kend)] of every split, as tn_body cuts them (64-token slices; a range may be empty)"""
    out = []
    if group_pure(T, m_groups) and split % m_groups == 0:
        kg, spg = T // m_groups, split // m_groups
        kper = ((kg + spg - 1) // spg + 63) // 64 * 64
        for g in range(m_groups):
            for zi in range(spg):
                kb = g * kg + zi * kper
                out.append((kb, max(kb, min(g * kg + kg, kb + kper))))
        return out
    kper = ((T + split - 1) // split + 63) // 64 * 64
    for z in range(split):
        out.append((z * kper, max(z * kper, min(T, z * kper + kper))))
    return out


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def rows_of(n, m):
    idx = torch.arange(n)
    if not m or m[0] == 0:
        return idx
    rpi, rps, off = m
    return (idx // rpi) * rps + off + idx % rpi


def roundup(x, m):
    return (x + m - 1) // m * m


def chunk_of(dtype):
    return 4 if dtype == F32 else 8


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def keep_rows(keep, rows, rows_in):
    """int64 [rows]: the keep value of every row's sample, markers / negatives read as 0; None -> None"""
    if keep is None:
        return None
    s = (torch.arange(rows) // rows_in) if rows_in > 0 else torch.zeros(rows, dtype=torch.int64)
    return keep.to(torch.int64)[s].clamp(min=0)


def kept_mask(keep, rows, cols, rows_in, period):
    """bool [rows, cols]"""
    if keep is None:
        return torch.ones(rows, cols, dtype=torch.bool)
    c = torch.arange(cols) % period if period > 0 else torch.arange(cols)
    return c[None, :] < keep_rows(keep, rows, rows_in)[:, None]


def _view(t, ld):
    return t.reshape(-1)[: (t.numel() // ld) * ld].view(-1, ld)


def operands64(a, b, kw):
    """-> (A [M, K], B [N, K]) float64 logical operands of a launch (forward: M rows; weight gradient: output rows x tokens)"""
    M, N, K = kw["M"], kw["N"], kw["K"]
    A2, B2 = _view(f64(a), kw["lda"]), _view(f64(b), kw["ldb"])
    if kw.get("a_trans"):
        return A2[rows_of(K, kw.get("a_map"))][:, :M].t(), B2[rows_of(K, kw.get("b_map"))][:, :N].t()
    A = A2[rows_of(M, kw.get("a_map"))][:, :K]
    B = B2[:K, :N].t() if kw.get("b_trans") else B2[:N, :K]
    return A, B


# ---- the contract ------------------------------------------------------------------------------------------------------------------------
def gemm64(a, b, kw, before=None, bias_grad_before=None):
    """The float64 contract of one launch and its bounds.  a, b: the operand buffers (any dtype: their values are exact inputs);
    kw: the keyword arguments of vitres.kernels.gemm (CPU tensors); before: the logical [M, N] part of C before the launch (atomic = 1).
    -> dict(C, bC, S, gain[, C2, bC2][, bias_grad, bBG, SA]): [M, N] float64 values BEFORE the output rounding (the bound carries it) and
    bounds for shares = 1 / split = 1; `bounds_for` adds the share / split terms.  fp16 overflow: see `round_out`."""
    M, N, K = kw["M"], kw["N"], kw["K"]
    in_dtype, out_dtype = a.dtype, kw["out_dtype"]
    u_out, fast = unit_roundoff(out_dtype), in_dtype != F32
    A, B = operands64(a, b, kw)
    acc = A @ B.t()
    S = A.abs() @ B.abs().t()
    dacc = K * MFMA * S
    r = dict(S=S)
    if kw.get("a_trans"):                                   # ---- weight gradient
        atomic = kw.get("atomic", 1)
        bef = f64(before) if (before is not None and atomic == 1) else torch.zeros_like(acc)
        r["C"], r["before"] = bef + acc, bef
        r["bC"], r["gain"] = 2 * dacc, torch.ones_like(S)
        if kw.get("bias_grad") is not None:
            bb = f64(bias_grad_before) if (bias_grad_before is not None and atomic == 1) else torch.zeros(M, dtype=F64)
            r["bias_grad"], r["bg_before"], r["SA"] = bb + A.sum(1), bb, A.abs().sum(1)
            r["bBG"] = 2 * K * MFMA * r["SA"]
        return r
    rows_in, act = kw.get("rows_in", 0), kw.get("act", 0)
    m = torch.arange(M)
    sample = (m // rows_in) if rows_in > 0 else torch.zeros(M, dtype=torch.int64)
    mloc = (m % rows_in) if rows_in > 0 else m
    orow = rows_of(M, kw.get("c_map"))
    mag, terms, pre = acc.abs(), 0, acc
    if kw.get("bias") is not None:
        bias = f64(kw["bias"]).view(1, N)
        pre, mag, terms = pre + bias, mag + bias.abs(), terms + 1
    if kw.get("pos") is not None:
        pos = _view(f64(kw["pos"]), N)[mloc]
        pre, mag, terms = pre + pos, mag + pos.abs(), terms + 1
    dpre = dacc + terms * U32 * mag
    mask = kept_mask(kw.get("keep_n"), M, N, rows_in, kw.get("n_period", 0))
    zero = torch.zeros_like(pre)
    dact = kw.get("dact_u")
    if act in (1, 2, 3) and dact is None:
        assert kw.get("scale") is None and kw.get("resid") is None
        if act == 3:
            C, bC, gain = relu64(pre), dpre + u_out * relu64(pre).abs(), torch.ones_like(S)
        else:
            eg, ed = gelu_errors(pre, fast)
            g, d = gelu64(pre), dgelu64(pre)
            bg = LIP1 * dpre + eg + u_out * g.abs()
            if kw.get("out2") is None:                      # single store: C = gelu(u)
                C, bC, gain = g, bg, torch.full_like(S, LIP1)
            else:
                if act == 2:
                    C, bC, gain = d, LIP2 * dpre + ed + u_out * d.abs(), torch.full_like(S, LIP2)
                else:
                    C, bC, gain = pre, dpre + u_out * pre.abs(), torch.ones_like(S)
                r["C2"], r["bC2"], r["gain2"] = torch.where(mask, g, zero), 2 * torch.where(mask, bg, zero), torch.where(mask, torch.full_like(S, LIP1), zero)
        r["C"], r["bC"], r["gain"] = torch.where(mask, C, zero), 2 * torch.where(mask, bC, zero), torch.where(mask, gain, zero)
        return r
    v, dv, gain = pre, dpre, torch.ones_like(S)
    if dact is not None:
        ud = _view(f64(dact), kw["ldu"])[orow][:, :N]
        if act == 2:
            d, dd = ud, torch.zeros_like(ud)
        else:
            d, dd = dgelu64(ud), gelu_errors(ud, fast)[1]
        dv = dpre * d.abs() + pre.abs() * dd + U32 * (pre * d).abs()
        v, gain = pre * d, d.abs()
    v, dv, gain = torch.where(mask, v, zero), torch.where(mask, dv, zero), torch.where(mask, gain, zero)
    if kw.get("scale") is not None:
        sc = f64(kw["scale"])[sample].view(M, 1)
        v, dv, gain = v * sc, dv * sc.abs() + torch.where(mask, U32 * (v * sc).abs(), zero), gain * sc.abs()
    if kw.get("resid") is not None:
        v = v + _view(f64(kw["resid"]), kw["ldc"])[orow][:, :N]
        dv = dv + torch.where(mask, U32 * v.abs(), zero)
    dv = dv + torch.where(mask, u_out * v.abs(), zero)
    r["C"], r["bC"], r["gain"] = v, 2 * dv, gain
    return r


def bounds_for(ref, which="C", shares=1, split=0):
    """bound of C / C2 / bias_grad for a launch with `shares` K-split shares (forward) or `split` token splits under atomic = 1"""
    if which == "bias_grad":
        return ref["bBG"] + 2 * split * U32 * (ref["SA"] + ref["bg_before"].abs())
    b = ref["bC" if which == "C" else "bC2"]
    g = ref["gain" if which == "C" else "gain2"]
    if shares > 1:
        b = b + 2 * (shares - 1) * U32 * ref["S"] * g
    if split > 0:
        b = b + 2 * split * U32 * (ref["S"] + ref["before"].abs())
    return b


def round_out(v, dtype):
    """a float64 contract value as the output type holds it when nothing else rounds (exact probes, masked zeros)"""
    return v.to(F32).to(dtype)


# ---- operands and the case table -----------------------------------------------------------------------------------------------------
FWD_SHAPES = [(1, 8, 64), (63, 64, 64), (65, 72, 128), (127, 128, 192), (129, 136, 256), (193, 200, 512), (64, 264, 4096), (130, 128, 4160),
              (66, 24, 40), (8, 24, 40), (34, 10, 37)]
FORMS = ["plain", "bias", "bias_resid", "bias_resid_alias", "bias_resid_scale", "resid_scale", "pos", "gelu_dual", "gelu_single", "gelu_pair", "relu",
         "dgrad", "dgrad_f32out", "dgrad_dact_erf", "dgrad_dact_saved", "dgradk_dact_erf", "dgradk_dact_saved"]
EXACT_FORMS = ["plain", "bias", "bias_resid_alias", "bias_resid_scale", "resid_scale", "pos", "relu", "dgrad", "dgrad_f32out", "dgrad_dact_saved",
               "dgradk_dact_saved"]
# dgradk_*: the data gradient times gelu' on a K-CONTIGUOUS weight (b_trans = 0: the transposed bf16 shadow of the forward's weight) -- the
# only data-gradient form the panel-resident kernel takes, and the general kernel's / gemm_nt.hip's dact_u epilogue without b_trans
MASK_FORMS = ["bias", "bias_resid_scale", "gelu_pair", "relu", "dgrad", "dgrad_dact_saved", "dgradk_dact_saved"]
PANEL_FORMS = ["plain", "bias", "gelu_dual", "gelu_single", "gelu_pair", "dgradk_dact_saved"]      # what vr_gemm_panel_launch covers
SCALES = [1.0 / 0.9, 0.0, 1.25, 1.0]
SCALES_EXACT = [2.0, 0.0, 0.5, 1.0]
ROUND_PROBE_OFFSET = {BF16: 384.0, F16: 3072.0}      # added to the bias of an exact probe: integer results where odd ones are ties


def form_ok(form, dtype):
    if dtype == F16 and form.startswith("dgrad"):
        return False                                        # fp16: the forward forms only
    if form == "dgrad_f32out":
        return dtype == BF16
    return True


def fwd_specs():
    """every forward / data-gradient case of the suite: dicts of plain values (tests parametrise over them by `name`)"""
    specs = []
    for i, (M, N, K) in enumerate(FWD_SHAPES):
        for form in FORMS:
            specs.append(dict(name="%s-M%dN%dK%d" % (form, M, N, K), form=form, M=M, N=N, K=K, pad_c=i % 2 == 0, pad_a=(i // 2) % 2 == 0))
    for form in PANEL_FORMS:                                # K in (256, 320]: the panel-resident kernel has its 80-row form only
        specs.append(dict(name="%s-M129N136K320" % form, form=form, M=129, N=136, K=320, pad_c=True, pad_a=False))
    for form in ("plain", "pos", "dgrad"):                  # row maps: A rows gathered, output rows scattered into a taller buffer
        specs.append(dict(name="%s-maps-M66N72K128" % form, form=form, M=66, N=72, K=128, pad_c=True, pad_a=False, rows_in=22,
                          a_map=(22, 30, 3), c_map=(22, 25, 2)))
    for form in MASK_FORMS:
        # 64-row tiles hold rows of several samples with different keeps; one sample carries the DropPath marker
        specs.append(dict(name="%s-mask-M136N136K192" % form, form=form, M=136, N=136, K=192, pad_c=True, pad_a=False, rows_in=17,
                          keep_n=[129, 0, 135, 8, -(64 + 2), 136, 63, 65], keep_k=[192, 1, 65, 191, 64, 0, 63, 192]))
        specs.append(dict(name="%s-mask-M195N200K128" % form, form=form, M=195, N=200, K=128, pad_c=False, pad_a=True, rows_in=65,
                          keep_n=[127, 199, 9], keep_k=[64, 128, 127], k_period=0))
        specs.append(dict(name="%s-mask-M136N192K256-periods" % form, form=form, M=136, N=192, K=256, pad_c=False, pad_a=False, rows_in=17,
                          keep_n=[0, 1, 33, 64, 33, 64, 1, 0], n_period=64, keep_k=[0, 1, 63, 64, 65, 127, 128, 64], k_period=128))
        specs.append(dict(name="%s-mask-M136N136K192-kp64" % form, form=form, M=136, N=136, K=192, pad_c=False, pad_a=False, rows_in=17,
                          keep_n=[7, 128, 136, 1, 64, 127, 9, 135], keep_k=[64, 0, 1, 63, 64, 1, 63, 64], k_period=64))
    # k_period below a slice: the lean loop refuses it, gemm_nt must take it
    specs.append(dict(name="bias-mask-M136N136K128-kp32", form="bias", M=136, N=136, K=128, pad_c=False, pad_a=False, rows_in=17,
                      keep_n=[136, 8, 65, 0, 136, 129, 64, 7], keep_k=[32, 0, 1, 31, 32, 31, 1, 0], k_period=32))
    return specs


def _fill(shape, dtype, g, exact, lo=-3, hi=3, scale=1.0):
    if exact:
        v = torch.randint(lo, hi + 1, shape, generator=g).to(F32)
        return v.to(dtype)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def exact_a(rows, K, dtype, g):
    """[rows, K] with +-1 at k = (r + j p) % K, p = max(1, K // 32): at most 32 entries per row, every slice of K used by some row"""
    p = max(1, K // 32)
    k, r = torch.arange(K)[None, :], torch.arange(rows)[:, None]
    sign = torch.randint(0, 2, (rows, K), generator=g).to(F32) * 2 - 1
    return torch.where((k + r) % p == 0, sign, torch.zeros(())).to(dtype)


def exact_b(rows, K, dtype, g):
    v = torch.randint(1, 4, (rows, K), generator=g).to(F32) * (torch.randint(0, 2, (rows, K), generator=g).to(F32) * 2 - 1)
    return v.to(dtype)


def _padded(logical, ld, zero_to, dtype):
    """[rows, ld]: the logical columns, zeros up to zero_to, NaN behind (never read)"""
    rows, cols = logical.shape
    t = torch.full((rows, ld), NAN, dtype=dtype)
    t[:, :zero_to] = 0
    t[:, :cols] = logical
    return t


def build_fwd(spec, dtype, exact=False):
    """-> dict(a, b, kw, out_rows, resid_alias) or None when the form does not exist in `dtype`.  kw holds every keyword of
    vitres.kernels.gemm except the output buffers: out_dtype names the type, `out2` is True where a second output is wanted."""
    form = spec["form"]
    if not form_ok(form, dtype):
        return None
    M, N, K = spec["M"], spec["N"], spec["K"]
    g = _gen(spec["name"], str(dtype), exact)
    ch = chunk_of(dtype)
    kpad = roundup(K, ch)
    lda = kpad + (2 * ch if spec.get("pad_a") else 0)
    bt = form.startswith("dgrad") and not form.startswith("dgradk")
    with_resid = form.startswith("bias_resid") or form == "resid_scale"      # resid_scale: no bias (gemm_nt.hip's run-time epilogue)
    out_dtype = F32 if (dtype == F32 or with_resid or form == "dgrad_f32out") else dtype
    ldc = N + (8 if spec.get("pad_c") else 0)
    rows_in = spec.get("rows_in", 0)
    if rows_in == 0 and form in ("pos", "bias_resid_scale", "resid_scale"):
        rows_in = max(1, (M + 2) // 3)
    nb = (M + rows_in - 1) // rows_in if rows_in else 1
    A = exact_a(M, K, dtype, g) if exact else _fill((M, K), dtype, g, False)
    keep_k = spec.get("keep_k")
    if keep_k is not None:                                  # the promise of keep_k: zeros beyond the keep
        A = torch.where(kept_mask(torch.tensor(keep_k), M, K, rows_in, spec.get("k_period", 0)), A, torch.zeros((), dtype=dtype))
    a_map, c_map = spec.get("a_map"), spec.get("c_map")
    a_rows = int(rows_of(M, a_map).max()) + 1 + (2 if a_map else 0)
    a = torch.full((a_rows, lda), NAN, dtype=dtype)         # rows no map reaches: NaN
    a[rows_of(M, a_map)] = _padded(A, lda, kpad, dtype)
    Bl = exact_b(N, K, dtype, g) if exact else _fill((N, K), dtype, g, False, scale=K ** -0.5)
    if bt:
        ldb = roundup(N, 8) + (8 if spec.get("pad_a") else 0)
        b = _padded(Bl.t().contiguous(), ldb, N, dtype)     # [K, ldb]: row padding may be read, it reaches no stored output
    else:
        ldb = lda
        b = _padded(Bl, ldb, kpad, dtype)
    kw = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, b_trans=bt, rows_in=rows_in, out_dtype=out_dtype)
    if a_map:
        kw["a_map"] = a_map
    if c_map:
        kw["c_map"] = c_map
    out_rows = int(rows_of(M, c_map).max()) + 1 + 3         # three rows beyond the last one written
    if form in ("bias", "bias_resid", "bias_resid_alias", "bias_resid_scale", "gelu_dual", "gelu_single", "gelu_pair", "relu"):
        kw["bias"] = _fill((N,), F32, g, exact, -16, 16)
    if form == "pos":
        kw["pos"] = _fill((rows_in, N), F32, g, exact, -8, 8)
    if with_resid:
        res = torch.full((out_rows, ldc), NAN)
        res[rows_of(M, c_map), :N] = _fill((M, N), F32, g, exact, -32, 32)
        kw["resid"] = res
    if form in ("bias_resid_scale", "resid_scale"):
        kw["scale"] = torch.tensor([(SCALES_EXACT if exact else SCALES)[s % 4] for s in range(nb)], dtype=F32)
    if form in ("gelu_dual", "gelu_pair"):
        kw["out2"] = True
    if form in ("gelu_dual", "gelu_single"):
        kw["act"] = 1
    if form == "gelu_pair":
        kw["act"] = 2
    if form == "relu":
        kw["act"] = 3
    if "_dact_" in form:
        du = torch.full((out_rows, ldc), NAN, dtype=dtype)
        if exact:
            pw = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (M, N), generator=g)]
            du[rows_of(M, c_map), :N] = pw.to(dtype)
        else:
            du[rows_of(M, c_map), :N] = _fill((M, N), dtype, g, False, scale=1.5)
        kw.update(dact_u=du, ldu=ldc, act=2 if form.endswith("_saved") else 0)
    if spec.get("keep_n") is not None:
        kw["keep_n"] = torch.tensor(spec["keep_n"], dtype=torch.int32)
        kw["n_period"] = spec.get("n_period", 0)
    if keep_k is not None:
        kw["keep_k"] = torch.tensor(keep_k, dtype=torch.int32)
        kw["k_period"] = spec.get("k_period", 0)
    return dict(a=a, b=b, kw=kw, out_rows=out_rows, resid_alias=form == "bias_resid_alias", spec=spec, exact=exact)


WGRAD_SHAPES = [(8, 8, 1), (64, 64, 63), (72, 136, 65), (128, 128, 64), (136, 264, 2049), (200, 328, 390)]


def wgrad_specs():
    specs = []
    for i, (No, Ki, T) in enumerate(WGRAD_SHAPES):
        specs.append(dict(name="wgrad-No%dKi%dT%d" % (No, Ki, T), No=No, Ki=Ki, T=T, pad_c=i % 2 == 0))
    specs.append(dict(name="wgrad-No10Ki24T130", No=10, Ki=24, T=130, pad_c=True))          # lda no multiple of 8: the general kernel
    specs.append(dict(name="wgrad-maps-No72Ki136T66", No=72, Ki=136, T=66, pad_c=False, a_map=(22, 30, 3), b_map=(22, 25, 2)))
    # token samples with their own kept rows / columns (65 tokens each); group-pure with m_groups = 2 or 3, interleaved with 4
    specs.append(dict(name="wgrad-keeps-No200Ki328T390", No=200, Ki=328, T=390, pad_c=False, rows_in=65,
                      keep_k=[200, 129, 64, 1, 0, 199], keep_n=[328, 65, 127, 0, 9, 264]))
    specs.append(dict(name="wgrad-keeps-No136Ki264T390-low", No=136, Ki=264, T=390, pad_c=True, rows_in=65,
                      keep_k=[63, 64, 8, 1, 0, 65], keep_n=[129, 65, 127, 0, 9, 128]))
    # 64-token samples: with 7 splits every token range is ONE sample; two of them keep no column at all (a layer whose input width is
    # 0) while their dY rows are kept -- the bias gradient still sums them
    specs.append(dict(name="wgrad-keeps-No72Ki136T384-nocols", No=72, Ki=136, T=384, pad_c=True, rows_in=64,
                      keep_k=[72, 8, 64, 40, 0, 71], keep_n=[136, 0, 129, 0, 9, 128]))
    return specs


def build_wgrad(spec, dtype, exact=False):
    No, Ki, T = spec["No"], spec["Ki"], spec["T"]
    g = _gen(spec["name"], str(dtype), exact)
    odd = No % 8 != 0
    lda, ldb = (No if odd else roundup(No, 8)), roundup(Ki, 8)
    rows_in = spec.get("rows_in", 0)
    A = exact_a(No, T, dtype, g).t().contiguous() if exact else _fill((T, No), dtype, g, False)
    B = exact_b(Ki, T, dtype, g).t().contiguous() if exact else _fill((T, Ki), dtype, g, False)
    if spec.get("keep_k") is not None:
        A = torch.where(kept_mask(torch.tensor(spec["keep_k"]), T, No, rows_in, 0), A, torch.zeros((), dtype=dtype))
        B = torch.where(kept_mask(torch.tensor(spec["keep_n"]), T, Ki, rows_in, 0), B, torch.zeros((), dtype=dtype))
    a_map, b_map = spec.get("a_map"), spec.get("b_map")
    a = torch.full((int(rows_of(T, a_map).max()) + 1, lda), NAN, dtype=dtype)
    a[rows_of(T, a_map)] = _padded(A, lda, lda, dtype)
    b = torch.full((int(rows_of(T, b_map).max()) + 1, ldb), NAN, dtype=dtype)
    b[rows_of(T, b_map)] = _padded(B, ldb, ldb, dtype)
    ldc = Ki + (4 if spec.get("pad_c") else 0)
    kw = dict(M=No, N=Ki, K=T, lda=lda, ldb=ldb, ldc=ldc, a_trans=True, b_trans=True, rows_in=rows_in, out_dtype=F32)
    if a_map:
        kw.update(a_map=a_map, b_map=b_map)
    if spec.get("keep_k") is not None:
        kw.update(keep_k=torch.tensor(spec["keep_k"], dtype=torch.int32), keep_n=torch.tensor(spec["keep_n"], dtype=torch.int32))
    before = _fill((No, Ki), F32, g, exact, -8, 8)
    bg_before = _fill((No,), F32, g, exact, -8, 8)
    return dict(a=a, b=b, kw=kw, out_rows=No + 3, before=before, bg_before=bg_before, spec=spec, exact=exact)


def wgrad_zero_region(spec):
    """bool [No, Ki]: rows / columns beyond the largest keep of the launch's samples (exact zero gradients)"""
    No, Ki = spec["No"], spec["Ki"]
    if spec.get("keep_k") is None:
        return torch.zeros(No, Ki, dtype=torch.bool)
    km, nm = max(max(spec["keep_k"]), 0), max(max(spec["keep_n"]), 0)
    return (torch.arange(No)[:, None] >= km) | (torch.arange(Ki)[None, :] >= nm)


# ---- launch buffers: what both the emulation and the device are handed -------------------------------------------------------------------
CANARY = {F32: (torch.int32, 0x7fc12345), BF16: (torch.int16, 0x7fc1), F16: (torch.int16, 0x7e01)}      # quiet NaNs with a payload


def canary(shape, dtype, device="cpu"):
    it, bits = CANARY[dtype]
    return torch.full(shape, bits, dtype=it, device=device).view(dtype)


def launch_buffers(case, device="cpu", atomic=None, before="rand"):
    """-> (a, b, out, out2, kw): tensors on `device`, outputs filled with the canary (weight gradients: the logical part holds `before`:
    'rand' the case's values, 'zero', or 'nan' for the store form), kw ready for emu_kernels.gemm / vitres.kernels.gemm"""
    kw = dict(case["kw"])
    out_dtype = kw.pop("out_dtype")
    M, N, ldc = kw["M"], kw["N"], kw["ldc"]
    out = canary((case["out_rows"], ldc), out_dtype)
    out2 = canary((case["out_rows"], ldc), out_dtype) if kw.pop("out2", None) else None
    if kw.get("a_trans"):
        kw["atomic"] = 1 if atomic is None else atomic
        out[:M, :N] = {"rand": case["before"], "zero": torch.zeros(M, N), "nan": torch.full((M, N), NAN)}[before]
    to = lambda v: v.to(device) if isinstance(v, torch.Tensor) else v
    kw = {k: to(v) for k, v in kw.items()}
    out = out.to(device)
    if case.get("resid_alias"):
        out.copy_(kw["resid"])                              # NaN outside the logical part either way: restore the canary there
        orow = rows_of(M, kw.get("c_map"))
        keep = torch.zeros(case["out_rows"], ldc, dtype=torch.bool)
        keep[orow, :N] = True
        out = torch.where(keep.to(device), out, canary((case["out_rows"], ldc), out_dtype, device))
        kw["resid"] = out
    if out2 is not None:
        kw["out2"] = out2.to(device)
    return case["a"].to(device), case["b"].to(device), out, kw.get("out2"), kw


def logical(buf, kw):
    """the [M, N] part of an output buffer a launch writes"""
    return buf[rows_of(kw["M"], kw.get("c_map")).to(buf.device), : kw["N"]]


def canary_intact(buf, kw):
    """every element outside the logical part still holds the canary's bits"""
    it, bits = CANARY[buf.dtype]
    b = buf.detach().cpu().view(it)
    wr = torch.zeros(b.shape, dtype=torch.bool)
    wr[rows_of(kw["M"], kw.get("c_map")), : kw["N"]] = True
    return bool(((b == bits) | wr).all())
