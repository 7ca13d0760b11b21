"""tests/gemm_ref64.py on the CPU: the float64 contract and tests/emu_kernels.gemm agree on every case of tests/test_gpu_gemm.py; an
fp32 emulation in the kernels' order (64-wide K slices, 16-deep MFMA steps inside a slice -- every k on its own for the fp32 kernel --,
K-split shares summed in share order, weight-gradient token splits added in a shuffled order) stays inside the derived bounds; the
injected faults leave them; the Abramowitz-Stegun constant, the Lipschitz constants and the split rules are checked, not trusted.

Prints (pytest -s) the worst emulation error / bound per form, the ratio every fault reaches and the A-S grid maximum."""
import math
import random

import pytest
import torch

import emu_kernels as E
import gemm_ref64 as G

F32, F64 = torch.float32, torch.float64


# ---- fp32 emulation in the kernels' order ---------------------------------------------------------------------------------------------------
def gelu_terms_fast32(u):
    """common.h gelu_terms_fast in torch fp32 (the fma contractions written as separately rounded products: inside the bound's roundings)"""
    x = u.abs() * F32_C(G.SQRT1_2)
    tt = 1.0 / (F32_C(G.AS_P) * x + 1.0)
    e = torch.exp((-x * x).to(F64)).to(F32)
    poly = F32_C(G.AS_A[4]) * tt + F32_C(G.AS_A[3])
    for c in (G.AS_A[2], G.AS_A[1], G.AS_A[0]):
        poly = poly * tt + F32_C(c)
    half_tail = 0.5 * poly * tt * e
    cdf = torch.where(u >= 0, 1.0 - half_tail, half_tail)
    return cdf, F32_C(G.INV_SQRT_2PI) * e


def F32_C(x):
    return torch.tensor(x, dtype=F32)


def gelu32(u, fast):
    if fast:
        cdf, pdf = gelu_terms_fast32(u)
        return u * cdf, u * pdf + cdf
    cdf = 0.5 * (1.0 + torch.erf((u * F32_C(G.SQRT1_2)).to(F64)).to(F32))
    pdf = F32_C(G.INV_SQRT_2PI) * torch.exp((-0.5 * u * u).to(F64)).to(F32)
    return 0.5 * u * (1.0 + torch.erf((u * F32_C(G.SQRT1_2)).to(F64)).to(F32)), cdf + u * pdf


def accumulate(A, B, lo, hi, in32):
    """fp32 [M, N] = sum over k in [lo, hi) of A[:, k] B[:, k] in the kernels' order, from zero"""
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=F32)
    if in32:
        for k in range(lo, hi):
            acc = acc + A[:, k, None] * B[None, :, k]                      # the product rounds, the add rounds
        return acc
    A64, B64 = A.to(F64), B.to(F64)
    for k0 in range(lo, hi, 16):                                           # one MFMA step: exact products, one rounding of the sum
        k1 = min(hi, k0 + 16)
        acc = (acc.to(F64) + A64[:, k0:k1] @ B64[:, k0:k1].t()).to(F32)
    return acc


def trunc16(v, dtype):
    """fp32 -> 16-bit by truncation (fault 10)"""
    h = v.to(dtype)
    over = h.to(F32).abs() > v.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(dtype), h)


def emulate(case, shares=1, split=1, atomic=None, before="rand", fault=None, seed=0):
    """-> dict(C[, C2][, bias_grad]): [M, N] tensors of the output type (NaN where nothing was stored).  fault: a name of FAULTS."""
    kw, a, b = case["kw"], case["a"], case["b"]
    M, N, K = kw["M"], kw["N"], kw["K"]
    in32, out_dtype = a.dtype == F32, kw["out_dtype"]
    kw2 = dict(kw)
    if fault == "rowmap_wrong_operand":
        kw2["a_map"], kw2["c_map"] = kw.get("c_map"), kw.get("a_map")
    A, B = (t.to(F32) for t in G.operands64(a, b, dict(kw2, c_map=None)))
    if kw.get("a_trans"):
        return emulate_wgrad(case, A, B, split, atomic, before, fault, seed)
    parts = []
    slices = (K + 63) // 64
    tile = (slice(max(0, (M - 1) // 64 * 64), M), slice(max(0, (N - 1) // 64 * 64), N))     # the last (short) tile
    bad = slices // 2
    for sh in range(shares):
        acc = torch.zeros(M, N, dtype=F32)
        for sl in range(sh, slices, shares):
            d = accumulate(A, B, sl * 64, min(K, sl * 64 + 64), in32)
            new = acc + d
            if sl == bad and fault == "slice_skipped":
                new[tile] = acc[tile]
            if sl == bad and fault == "slice_twice":
                new[tile] = (new + d)[tile]
            acc = new
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    rows_in, act = kw.get("rows_in", 0), kw.get("act", 0)
    m = torch.arange(M)
    sample = (m // rows_in) if rows_in > 0 else torch.zeros(M, dtype=torch.int64)
    mloc = (m % rows_in) if rows_in > 0 else m
    orow = G.rows_of(M, kw.get("c_map"))
    v = acc
    if kw.get("bias") is not None:
        bias = kw["bias"].clone()
        if fault == "bias_missing_last_tile":
            bias[(N - 1) // 64 * 64:] = 0
        v = v + bias.view(1, N)
    if kw.get("pos") is not None:
        pos = G._view(kw["pos"], N)
        v = v + (pos[m.clamp(max=pos.shape[0] - 1)] if fault == "pos_by_m" else pos[mloc])
    keep = kw.get("keep_n")
    if keep is not None:
        kv = keep.to(torch.int64)[sample]
        kv = torch.where(kv < 0, -(kv + 2), kv) if fault == "marker_as_k" else kv.clamp(min=0)
        kv = kv + (1 if fault == "keep_plus_one" else (-1 if fault == "keep_minus_one" else 0))
        np_ = kw.get("n_period", 0)
        c = torch.arange(N) % np_ if np_ > 0 else torch.arange(N)
        mask = c[None, :] < kv[:, None]
    else:
        mask = torch.ones(M, N, dtype=torch.bool)
    zero = torch.zeros((), dtype=F32)

    def store(t):
        o = trunc16(t, out_dtype) if (fault == "truncate" and out_dtype != F32) else t.to(out_dtype)
        if fault == "last_row_dropped":
            o[M - 1] = G.NAN
        if fault == "last_col_dropped":
            o[:, N - 1] = G.NAN
        return o

    dact, fast = kw.get("dact_u"), not in32
    if act in (1, 2, 3) and dact is None:
        if act == 3:
            return dict(C=store(torch.where(mask, torch.where(v <= 0, zero, v), zero)))
        src = v.to(out_dtype).to(F32) if fault == "gelu_of_rounded_u" else v
        g, _ = gelu32(src, fast)
        _, d = gelu32(v, fast)
        g = torch.where(mask, g, zero)
        if kw.get("out2") is None:
            return dict(C=store(g))
        return dict(C=store(torch.where(mask, d if act == 2 else v, zero)), C2=store(g))
    if dact is not None:
        ud = G._view(dact, kw["ldu"])[orow][:, :N].to(F32)
        v = v * (ud if act == 2 else gelu32(ud, fast)[1])
    res = G._view(kw["resid"], kw["ldc"])[orow][:, :N] if kw.get("resid") is not None else None
    sc = kw["scale"][sample].view(M, 1) if kw.get("scale") is not None else None
    if fault == "mask_after_resid":
        v = v * sc if sc is not None else v
        v = v + res if res is not None else v
        return dict(C=store(torch.where(mask, v, zero)))
    v = torch.where(mask, v, zero)
    if fault == "scale_on_resid":
        v = (v + res) * sc
    else:
        v = v * sc if sc is not None else v
        v = v + res if res is not None else v
    return dict(C=store(v))


def emulate_wgrad(case, A, B, split, atomic, before, fault, seed):
    kw = case["kw"]
    M, N, T = kw["M"], kw["N"], kw["K"]
    atomic = 1 if atomic is None else atomic
    bef = {"rand": case["before"], "zero": torch.zeros(M, N), "nan": torch.full((M, N), G.NAN)}[before].clone()
    bgb = case["bg_before"].clone() if before == "rand" else torch.zeros(M)
    ranges = G.tn_token_ranges(T, 1 if atomic == 2 else split, 0)
    ones = torch.ones(1, T, dtype=F32)
    parts = []
    in32 = case["a"].dtype == F32
    last = max(i for i, (lo, hi) in enumerate(ranges) if hi > lo)
    Abg = A
    if fault == "bias_grad_skips_colless_samples":          # the bug this suite found: tiles without a kept column left before their row sums
        colless = G.keep_rows(kw["keep_n"], T, kw["rows_in"]) == 0
        Abg = torch.where(colless[None, :], torch.zeros((), dtype=F32), A)
    for i, (lo, hi) in enumerate(ranges):
        if hi <= lo or (fault == "split_dropped" and i == last):
            continue
        bg_hi = lo + (hi - lo - 1) // 64 * 64 if (fault == "bias_grad_last_slice" and i == last) else hi
        parts.append((accumulate(A, B, lo, hi, in32), accumulate(Abg, ones, lo, bg_hi, in32)[:, 0]))
    random.Random(seed).shuffle(parts)
    if atomic == 2 and fault != "store_accumulates":
        C, bg = torch.zeros(M, N), torch.zeros(M)
    else:
        C, bg = bef, bgb
    for p, q in parts:
        C, bg = C + p, bg + q
    return dict(C=C, bias_grad=bg)


def ratio(case, ref, got, shares=1, split=0):
    r = G.worst_ratio(got["C"], ref["C"], G.bounds_for(ref, "C", shares, split))
    if "C2" in got:
        r = max(r, G.worst_ratio(got["C2"], ref["C2"], G.bounds_for(ref, "C2", shares, split)))
    if "bias_grad" in got and "bias_grad" in ref:
        r = max(r, G.worst_ratio(got["bias_grad"], ref["bias_grad"], G.bounds_for(ref, "bias_grad", split=split)))
    return r


_CASES = {}


def fwd_case(spec, dt):
    key = (spec["name"], dt)
    if key not in _CASES:
        c = G.build_fwd(spec, dt)
        _CASES[key] = (c, G.gemm64(c["a"], c["b"], c["kw"])) if c is not None else (None, None)
    return _CASES[key]


SPECS = G.fwd_specs()
WSPECS = G.wgrad_specs()


# ---- the contract against the torch statement ---------------------------------------------------------------------------------------------
def test_contract_and_emu_kernels_agree_on_every_case():
    worst = {}
    for spec in SPECS:
        for dt in G.DTYPES:
            c, ref = fwd_case(spec, dt)
            if c is None:
                continue
            a, b, out, out2, kw = G.launch_buffers(c)
            E.gemm(a, b, out, **kw)
            assert G.canary_intact(out, kw), spec["name"]
            got = dict(C=G.logical(out, kw))
            if out2 is not None:
                got["C2"] = G.logical(out2, kw)
            r = ratio(c, ref, got)
            worst[spec["form"]] = max(worst.get(spec["form"], 0.0), r)
            assert r <= 1.0, (spec["name"], dt, r)
    for spec in WSPECS:
        for dt in (F32, torch.bfloat16):
            c = G.build_wgrad(spec, dt)
            for atomic, before in ((1, "rand"), (2, "nan")):
                kwr = dict(c["kw"], atomic=atomic, bias_grad=True)
                ref = G.gemm64(c["a"], c["b"], kwr, before=c["before"], bias_grad_before=c["bg_before"])
                a, b, out, _, kw = G.launch_buffers(c, atomic=atomic, before=before)
                bg = c["bg_before"].clone() if atomic == 1 else torch.full((spec["No"],), G.NAN)
                E.gemm(a, b, out, bias_grad=bg, **kw)
                r = ratio(c, ref, dict(C=G.logical(out, kw), bias_grad=bg), split=1)
                worst["wgrad"] = max(worst.get("wgrad", 0.0), r)
                assert r <= 1.0 and G.canary_intact(out, kw), (spec["name"], dt, atomic, r)
    print("GEMM contract vs emu_kernels, worst error / bound per form: " + " ".join("%s=%.3f" % kv for kv in sorted(worst.items())))


# ---- the ordered fp32 emulation stays inside the bounds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", G.DTYPES, ids=lambda d: str(d)[6:])
def test_ordered_emulation_inside_the_bounds_forward(dt):
    worst = {}
    for spec in SPECS:
        c, ref = fwd_case(spec, dt)
        if c is None:
            continue
        share_list = [1] + ([2, 3, 4] if (dt == torch.bfloat16 and spec["K"] in (256, 512, 4096) and spec["K"] % 64 == 0) else [])
        for sh in sorted({G.lean_shares(spec["K"], s) for s in share_list}):          # (what the launcher clamps the request to)
            r = ratio(c, ref, emulate(c, shares=sh), shares=sh)
            key = spec["form"] + ("+shares" if sh > 1 else "")
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, (spec["name"], dt, sh, r)
    print("GEMM ordered emulation %s, worst error / bound per form: %s" % (str(dt)[6:], " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("dt", [F32, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_ordered_emulation_inside_the_bounds_wgrad(dt):
    worst = 0.0
    for spec in WSPECS:
        c = G.build_wgrad(spec, dt)
        slices = (spec["T"] + 63) // 64
        for split in sorted({1, 2, 3, 7, slices + 1}):
            for atomic, before in ((1, "rand"), (1, "zero"), (2, "nan")):
                if atomic == 2 and split > 1:
                    continue
                bef = c["before"] if before == "rand" else torch.zeros_like(c["before"])
                bgb = c["bg_before"] if before == "rand" else torch.zeros_like(c["bg_before"])
                ref = G.gemm64(c["a"], c["b"], dict(c["kw"], atomic=atomic, bias_grad=True), before=bef, bias_grad_before=bgb)
                for seed in (0, 1):
                    r = ratio(c, ref, emulate(c, split=split, atomic=atomic, before=before, seed=seed), split=split if atomic == 1 else 0)
                    worst = max(worst, r)
                    assert r <= 1.0, (spec["name"], dt, split, atomic, before, r)
    print("GEMM ordered emulation %s, weight gradients: worst error / bound %.3f" % (str(dt)[6:], worst))


# ---- injected faults leave the bounds --------------------------------------------------------------------------------------------------------
# name -> (which specs it can show on, dtype).  Every fault is run on all those cases; the largest ratio is printed.
def _has(*keys):
    return lambda s: all(s.get(k) is not None for k in keys)


FAULTS = {
    "slice_skipped": (lambda s: s["form"] in ("plain", "bias", "dgrad") and "mask" not in s["name"], torch.bfloat16),
    "slice_twice": (lambda s: s["form"] in ("plain", "bias", "dgrad") and "mask" not in s["name"], torch.bfloat16),
    "last_row_dropped": (lambda s: s["form"] == "plain", torch.bfloat16),
    "last_col_dropped": (lambda s: s["form"] == "plain", torch.bfloat16),
    "keep_plus_one": (_has("keep_n"), torch.bfloat16),
    "keep_minus_one": (_has("keep_n"), torch.bfloat16),
    "mask_after_resid": (lambda s: s["form"] == "bias_resid_scale" and s.get("keep_n") is not None, torch.bfloat16),
    "scale_on_resid": (lambda s: s["form"] == "bias_resid_scale", torch.bfloat16),
    "bias_missing_last_tile": (lambda s: s["form"] == "bias", torch.bfloat16),
    "pos_by_m": (lambda s: s["form"] == "pos", torch.bfloat16),
    "gelu_of_rounded_u": (lambda s: s["form"] in ("gelu_dual", "gelu_pair"), torch.bfloat16),
    "marker_as_k": (lambda s: s.get("keep_n") is not None and min(s["keep_n"]) < 0, torch.bfloat16),
    "rowmap_wrong_operand": (_has("a_map"), torch.bfloat16),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_injected_fault_leaves_the_bounds_forward(fault):
    pred, dt = FAULTS[fault]
    reached, n = 0.0, 0
    for spec in SPECS:
        if not pred(spec) or spec["K"] > 4096:
            continue
        c, ref = fwd_case(spec, dt)
        clean, bad = ratio(c, ref, emulate(c)), ratio(c, ref, emulate(c, fault=fault))
        assert clean <= 1.0
        reached, n = max(reached, bad), n + 1
    print("GEMM fault %s: error / bound %.3g on the worst of %d cases" % (fault, reached, n))
    assert n > 0 and reached > 1.0, (fault, reached)


def test_truncating_store_is_caught_by_the_rounding_probe_only():
    """Truncation moves a value by less than one ulp = 2 u |out|: exactly the random cases' output term with its factor 2, so no random
    case can see it.  The rounding probe does: exact integer results in (256, 512) (bf16) / (2048, 4096) (fp16), where every odd integer
    is a tie -- the device must return round-to-nearest-even bit for bit."""
    for dt in (torch.bfloat16, torch.float16):
        spec = dict(name="round-probe", form="bias", M=65, N=72, K=128, pad_c=True, pad_a=False)
        c = G.build_fwd(spec, dt, exact=True)
        c["kw"]["bias"] = c["kw"]["bias"] + G.ROUND_PROBE_OFFSET[dt]
        ref = G.round_out(G.gemm64(c["a"], c["b"], c["kw"])["C"], dt)
        assert torch.equal(emulate(c)["C"], ref)
        assert not torch.equal(emulate(c, fault="truncate")["C"], ref)
        spec_r = next(s for s in SPECS if s["name"] == "bias-M129N136K256")
        cr, rr = fwd_case(spec_r, dt)
        assert ratio(cr, rr, emulate(cr, fault="truncate")) <= 1.0           # ... and, as derived, stays inside a random case's bound


@pytest.mark.parametrize("fault", ["split_dropped", "bias_grad_last_slice", "store_accumulates", "bias_grad_skips_colless_samples"])
def test_injected_fault_leaves_the_bounds_wgrad(fault):
    reached = 0.0
    for spec in WSPECS:
        if fault == "bias_grad_skips_colless_samples" and not (spec.get("keep_n") and 0 in spec["keep_n"]):
            continue
        c = G.build_wgrad(spec, torch.bfloat16)
        atomic, before, split = (2, "rand", 1) if fault == "store_accumulates" else (1, "rand", 2)
        ref = G.gemm64(c["a"], c["b"], dict(c["kw"], atomic=atomic, bias_grad=True), before=c["before"], bias_grad_before=c["bg_before"])
        got = emulate(c, split=split, atomic=atomic, before=before, fault=fault)
        reached = max(reached, ratio(c, ref, got, split=split if atomic == 1 else 0))
    print("GEMM fault %s: error / bound %.3g" % (fault, reached))
    assert reached > 1.0


# ---- the constants -----------------------------------------------------------------------------------------------------------------------
def test_abramowitz_stegun_constant_and_lipschitz_constants_on_the_grid():
    x = torch.linspace(0, 10, 2_000_001, dtype=F64)
    erfc_as = G.as_erfc_scaled(x) * torch.exp(-x * x)
    err = float((0.5 * erfc_as - 0.5 * torch.special.erfc(x)).abs().max())
    for xv in (0.0, 0.3, 1.0, 2.5, 6.0):                                   # torch's erfc against math.erf, the stated reference
        assert abs(float(torch.special.erfc(torch.tensor(xv, dtype=F64))) - (1 - math.erf(xv))) < 1e-15
    print("GEMM A-S 7.1.26 grid maximum |d Phi| = %.4g (bound %.4g)" % (err, G.AS_CDF))
    assert err <= G.AS_CDF
    u = torch.linspace(-10, 10, 2_000_001, dtype=F64)
    d1 = G.dgelu64(u)
    d2 = 2 * G.pdf64(u) - u * u * G.pdf64(u)                               # gelu'' = phi (2 - u^2)
    print("GEMM sup|gelu'| = %.4f, sup|gelu''| = %.4f" % (float(d1.abs().max()), float(d2.abs().max())))
    assert float(d1.abs().max()) < G.LIP1 and float(d2.abs().max()) < G.LIP2
    num = (G.gelu64(u[2:]) - G.gelu64(u[:-2])) / (u[2:] - u[:-2])          # the formulas are the derivatives of one another
    assert float((num - d1[1:-1]).abs().max()) < 1e-8
    assert abs(G.AS_SA - 4.4753) < 1e-3 and abs(G.AS_TP - 16.198) < 1e-2


def test_split_rules_restated():
    """hand-evaluated from gemm_tn.hip / gemm.hip for a 256-CU device (and one 304-CU line)"""
    assert G.tn_split(136, 264, 2049, 256) == 2 and G.tn_split(136, 264, 2048, 256) == 1           # 33 token slices -> 2
    assert G.tn_split(128, 128, 64 * 32 * 40, 256) == 40 and G.tn_split(1024, 1024, 64 * 32 * 40, 256) == 16     # by_fill = ceil(1024 / 64)
    assert G.tn_split(1024, 1024, 64 * 32 * 40, 304) == 19
    assert G.tn_split(64, 64, 390, 256, split_k=7) == 7 and G.tn_split(64, 64, 390, 256, split_k=7, atomic=2) == 1
    assert G.tn_split(64, 64, 390, 256, split_k=3, m_groups=2) == 4 and G.tn_split(64, 64, 390, 256, split_k=1, m_groups=2) == 1
    assert G.tn_split(64, 64, 390, 256, split_k=3, m_groups=4) == 3                                   # 390 % 4: not group-pure
    assert G.general_split(10, 24, 130) == (1, False) and G.general_split(256, 256, 512 * 192) == (192, True)
    assert G.general_split(256, 256, 512 * 191) == (191, False) and G.general_split(192, 192, 512 * 192, shared=True)[1] is False
    assert G.tn_token_ranges(2049, 2) == [(0, 1088), (1088, 2049)] and G.tn_token_ranges(65, 3) == [(0, 64), (64, 65), (128, 128)]
    # vr_gemm_group at T = 390 (7 slices): spw clamps to 8 -> one split each; the 8-wave kernel's cost model: s = 1 -> 1 x 47, s = 2 -> 1 x 44,
    # s = 3 leaves 3 < 4 slices per split; on 8 CUs the 9 tiles: s = 1 -> 2 x 47, s = 2 -> 3 x 44
    dims = [(200, 328), (72, 136), (128, 128)]
    assert G.tn_group_splits(dims, 390, 256, [1, 1, 1]) == [1, 1, 1] and G.tn_group_splits(dims, 390, 256, [1, 2, 1], 0x10000) == [1, 1, 1]
    assert G.tn_group_splits(dims, 390, 256, [1, 1, 1], 0x10000) == [2, 2, 2] and G.tn_group_splits(dims, 390, 8, [1, 1, 1], 0x10000) == [1, 1, 1]
    # long T: 3 tiles x 65 slices = 195 slices of work on 2 x 4 CUs -> 24 per workgroup -> 3 splits; on 256 CUs the floor of 8 -> 9 splits,
    # 10 for two groups; the store form never splits
    assert G.tn_group_splits(dims[1:], 4100, 4, [1, 1]) == [3, 3] and G.tn_group_splits(dims[1:], 4100, 256, [1, 1]) == [9, 9]
    assert G.tn_group_splits(dims[1:], 4100, 4, [2, 2]) == [1, 1] and G.tn_group_splits(dims[1:], 4100, 256, [1, 1], m_groups=2) == [10, 10]
    assert [G.lean_shares(256, s) for s in (1, 2, 3, 4)] == [1, 2, 2, 2] and [G.lean_shares(512, s) for s in (2, 3, 4, 5)] == [2, 3, 4, 4]
    assert G.lean_shares(64, 4) == 1 and G.lean_shares(4096, 4) == 4
    assert G.tn_token_ranges(390, 4, 2) == [(0, 128), (128, 195), (195, 323), (323, 390)]
