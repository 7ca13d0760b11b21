"""tests/optim_ref64.py on the CPU: the bounds hold for an fp32 emulation of the three kernels of csrc/optim.hip, uncontracted and with
either fused multiply-add the compiler may form, and they (or the exact contracts beside them) reject injected faults, each at a case named here.  The emulation is numpy fp32 -- IEEE
after every +, -, *, /, sqrt -- in the kernels' own order: the grid-stride loop is element-wise for AdamW, and for the sum of squares the
eight fma chains per thread, the in-thread tree, the wave butterfly and the four-wave sum.  `pytest -s` prints the worst ratios."""
import decimal
import math

import numpy as np
import pytest
import torch

import optim_ref64 as R
from optim_ref64 import BC1, B1, B2, EPS, GS, LR, SBC2, WD
from vitres.optim import FlatAdamW

f32, f64 = np.float32, np.float64
ONE = f32(1.0)
N_SWEEP = 2056                                        # two workgroups, the second with one live thread


def fma(a, b, c):
    """round(a * b + c) once: the product of two fp32 is exact in float64 (the float64 sum rounds first, an innocuous double rounding)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


# ---- the emulation ----------------------------------------------------------------------------------------------------------------------------------
ADAMW_FAULTS = ["wd_coupled", "wd_after", "eps_in_sqrt", "eps_before_div", "no_bias_c1", "beta2_off", "group_shift", "update_255",
                "drop_last_thread", "shadow_trunc", "ema_old_p"]
NORM_FAULTS = ["sumsq_counts_255", "stale_partial", "coef_no_eps"]


def emu_adamw(a, gid, groups, coef=None, d=None, dev=False, contract=0, fault=None):
    """adamw_kernel<DEV, CLIP> on the CPU.  a: dict p, g, m, v, ema (fp32), shadow (uint16) -> the same dict after the launch.
    contract: 0 = every product and sum rounds; 1, 2 = `a * b + c * d` fused around its first / its second product (the compiler may
    take either), the parameter step fused in both."""
    gi = gid.astype(np.int64)
    if fault == "group_shift":                         # group i reads the byte of group i + 1
        gi = np.append(gi[1:], gi[-1:])
    live8 = gi != 255
    if fault == "update_255":
        gi, live8 = np.where(live8, gi, 0), np.ones_like(live8)
    if fault == "drop_last_thread":                    # `i < n8 - 1`: the last live thread of the last pass
        live8 = live8.copy()
        live8[-1] = False
    ge = np.repeat(np.where(live8, gi, 0), 8)
    live = np.repeat(live8, 8)
    h = np.asarray(groups, f32)[ge]
    if dev:
        live = live & (h[:, BC1] != 0)
    p, g, m, v = (a[k].astype(f32) for k in "pgmv")
    with np.errstate(all="ignore"):
        gr = g * h[:, GS]
        if coef is not None:
            gr = gr * f32(coef)
        fdec = ONE - h[:, LR] * h[:, WD]
        x = p * fdec
        c1, c2 = ONE - h[:, B1], ONE - h[:, B2]
        if fault == "wd_coupled":                      # torch.optim.Adam's L2 penalty instead of the decoupled decay
            gr, x = gr + h[:, WD] * p, p
        if fault == "beta2_off":
            c2 = (c2.astype(f64) * (1.0 + 2e-6)).astype(f32)
        m1 = [h[:, B1] * m + c1 * gr, fma(h[:, B1], m, c1 * gr), fma(c1, gr, h[:, B1] * m)][contract]
        v1 = [h[:, B2] * v + c2 * gr * gr, fma(h[:, B2], v, c2 * gr * gr), fma(c2 * gr, gr, h[:, B2] * v)][contract]
        if fault == "eps_in_sqrt":
            denom = np.sqrt(v1 + h[:, EPS]) / h[:, SBC2]
        elif fault == "eps_before_div":
            denom = (np.sqrt(v1) + h[:, EPS]) / h[:, SBC2]
        else:
            denom = np.sqrt(v1) / h[:, SBC2] + h[:, EPS]
        s = h[:, LR] if fault == "no_bias_c1" else h[:, LR] / h[:, BC1]
        r = m1 / denom
        if fault == "wd_after":
            p1 = (p - s * r) * fdec
        else:
            p1 = fma(-s, r, x) if contract else x - s * r
        out = {"g": a["g"], "p": np.where(live, p1, p), "m": np.where(live, m1, m), "v": np.where(live, v1, v)}
        sh = (R.bits(p1) >> 16).astype(np.uint16) if fault == "shadow_trunc" else R.bf16_rne(p1)
        out["shadow"] = np.where(live, sh, a["shadow"])
        if d is not None:
            dd, e = f32(d), a["ema"].astype(f32)
            src = p if fault == "ema_old_p" else p1
            e1 = [dd * e + (ONE - dd) * src, fma(dd, e, (ONE - dd) * src), fma(ONE - dd, src, dd * e)][contract]
            out["ema"] = np.where(live, e1, e)
        else:
            out["ema"] = a["ema"]
    return out


def emu_sumsq(g, gid, n_partials, max_blocks=0, before=None, fault=None):
    """sumsq_kernel: -> partials fp32 [n_partials]; before: the buffer's earlier contents (matter to a fault only)"""
    n8 = g.size // 8
    active, _, chain = R.sumsq_path(g.size, n_partials, max_blocks)
    keep = np.ones(n8, bool) if fault == "sumsq_counts_255" else gid != 255
    t = np.zeros((chain * active * 256, 8), f32)
    t[:n8] = np.where(keep[:, None], g.reshape(n8, 8), f32(0))       # (a skipped group is never read: fma(0, 0, acc) = acc)
    t = t.reshape(chain, active * 256, 8)
    acc = np.zeros((active * 256, 8), f32)
    for k in range(chain):
        acc = fma(t[k], t[k], acc)
    s = ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])) + ((acc[:, 4] + acc[:, 5]) + (acc[:, 6] + acc[:, 7]))
    s = s.reshape(active, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    w = s[:, :, 0]
    out = np.zeros(n_partials, f32) if before is None or fault != "stale_partial" else before.astype(f32).copy()
    out[:active] = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    return out


def emu_clip_finish(partials, max_norm, grad_scale, skipped, fault=None):
    """clip_finish_kernel: -> (norm, coef, skip, skipped)"""
    with np.errstate(all="ignore"):
        total = np.asarray(partials, f64).sum()
        norm = f32(f64(f32(grad_scale)) * np.sqrt(total))
        if not np.isfinite(norm):
            return norm, f32(0), 1, skipped + 1
        q = f32(max_norm) / (norm if fault == "coef_no_eps" else norm + f32(1e-6))
    return norm, (q if q < ONE else ONE), 0, skipped


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
def arena(n, seed=3):
    a = R.adamw_inputs(n, seed)
    a["shadow"] = np.full(n, R.CANARY16, np.uint16)
    return a


def run_case(n, h, holes=(), dev=False, contract=0, fault=None, zero_group=None):
    """-> {(output, family): ratio} plus ("shadow", None) and ("untouched", None)"""
    t, kind, gs, coef, d = h
    groups = R.groups_f32(kind, t, gs)
    if zero_group is not None:
        groups[zero_group] = 0
    gid = R.group_bytes(n, len(groups), holes)
    a = arena(n)
    got = emu_adamw(a, gid, groups, coef, d, dev, contract, fault)
    fam = R.family_of(n)
    out = {}
    for fi, name in enumerate(R.FAMILIES):
        for k, r in R.adamw_verdict(a, got, gid, groups, coef, d, dev, where=fam == fi).items():
            if k in ("shadow", "untouched"):
                out[(k, None)] = max(out.get((k, None), 0.0), r)
            else:
                out[(k, name)] = r
    return out


HONEST = {}


def honest_sweep():
    """every hyper set at N_SWEEP, uncontracted and both contractions -> {(contract, hyper, output, family): ratio}; computed once"""
    if not HONEST:
        for h in R.hyper_sets():
            for contract in (0, 1, 2):
                for key, r in run_case(N_SWEEP, h, contract=contract).items():
                    HONEST[(contract, h) + key] = r
                    if key[1] is not None:
                        R.record(("adamw emu fma=%d" % contract, key[0]), r)
    return HONEST


def test_honest_emulation_stays_inside_every_bound():
    sweep = honest_sweep()
    assert len(sweep) >= 3 * 96 * (3 * 6 + 2)
    worst = max(sweep.items(), key=lambda kv: kv[1])
    assert worst[1] <= 1.0, worst
    for contract in (0, 1, 2):
        for k in ("p", "m", "v", "ema"):
            assert 0.0 < R.WORST[("adamw emu fma=%d" % contract, k)] <= 1.0
    # no bound is slack by construction: the uncontracted emulation comes within a factor of four of every one of them
    assert all(R.WORST[("adamw emu fma=0", k)] > 0.25 for k in ("p", "m", "v", "ema")), R.WORST


@pytest.mark.parametrize("n,cap", R.ADAMW_CASES)
def test_honest_emulation_on_every_path_size_with_holes_and_a_zero_group(n, cap):
    n8 = n // 8
    holes = [(0, 1)] if n8 < 4 else [(0, 2), (n8 // 2, n8 // 2 + 3), (n8 - 1, n8)]
    for h in [(1, "two", 1.0, None, 0.99996), (10, "sixteen", 0.125, 0.37, 0.99)]:
        for kw in (dict(), dict(holes=holes), dict(dev=True, zero_group=1)):
            for contract in (0, 1, 2):
                out = run_case(n, h, contract=contract, **kw)
                assert max(out.values()) <= 1.0, (n, h, kw, contract, out)


# fault -> the case that must expose it: (hyper set, output, family); family None for the two exact verdicts.  Faults of the formula are
# named at the families where they bite: exact zeros of p (every family has them) for what moves the step, `cold` (v' is the new term alone)
# for beta2.  t = 1 is what shows eps_before_div and no_bias_c1: at t = 100000 both corrections are exactly 1 in fp32.
H1 = (1, "two", 1.0, None, 0.99996)
H2 = (2, "two", 0.125, 0.37, 0.99)
FAULT_CASES = {
    "wd_coupled": (H1, "p", "typ"),
    "wd_after": (H1, "p", "big"),
    "eps_in_sqrt": (H1, "p", "typ"),
    "eps_before_div": (H1, "p", "tiny"),
    "no_bias_c1": (H2, "p", "typ"),
    "beta2_off": (H1, "v", "cold"),
    "group_shift": (H1, "p", "typ"),
    "ema_old_p": (H1, "ema", "big"),
    "shadow_trunc": (H1, "shadow", None),
}


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_each_formula_fault_leaves_its_bound_at_the_named_case(fault):
    h, k, fam = FAULT_CASES[fault]
    for contract in (0, 1, 2):
        r = run_case(N_SWEEP, h, contract=contract, fault=fault)[(k, fam)]
        print("OPTIM fault %-18s fma=%d %s %s/%s: err/bound %.3g" % (fault, contract, R.hyper_name(h), k, fam, r))
        assert r > 1.0, (fault, contract, r)
        assert honest_sweep()[(contract, h, k, fam)] <= 1.0


@pytest.mark.parametrize("fault", ["eps_before_div", "no_bias_c1"])
def test_the_faults_that_need_a_small_t_are_invisible_at_t_100000(fault):
    """why t = 1 and t = 2 are in the list: with both bias corrections at exactly 1 these two forms ARE the contract"""
    for h in [(100000, "two", 1.0, None, 0.99996), (100000, "sixteen", 0.125, 0.37, 0.99)]:
        assert R.groups_f32(h[1], h[0], h[2])[0, BC1] == 1.0 and R.groups_f32(h[1], h[0], h[2])[0, SBC2] == 1.0
        assert max(run_case(N_SWEEP, h, fault=fault).values()) <= 1.0
    assert max(run_case(N_SWEEP, (10, "two", 1.0, None, None), fault=fault).values()) > 1.0


def test_structural_faults_are_caught():
    assert set(FAULT_CASES) | {"update_255", "drop_last_thread"} == set(ADAMW_FAULTS)          # every fault has its named case
    n, h = 4104, H1
    n8 = n // 8
    holes = [(0, 2), (n8 // 2, n8 // 2 + 3), (n8 - 1, n8)]
    assert run_case(n, h, holes=holes, fault="update_255")[("untouched", None)] == math.inf
    assert run_case(n, h, holes=holes)[("untouched", None)] == 0.0
    for n, cap in R.ADAMW_CASES:                       # the dropped thread: at every path size the last group of eight keeps its input
        out = run_case(n, h, fault="drop_last_thread")
        assert max(v for (k, _), v in out.items() if k in ("p", "m", "v", "ema")) > 1.0, n
    # the neighbour's group byte: also with sixteen groups, and invisible only where neighbours share their byte
    assert max(run_case(N_SWEEP, (1, "sixteen", 1.0, None, None), fault="group_shift").values()) > 1.0


# ---- the gradient norm ------------------------------------------------------------------------------------------------------------------------------
def sumsq_case(kind, n, n_partials, cap, holes=(), fault=None):
    g = R.sumsq_inputs(kind, n)
    gid = R.group_bytes(n, 2, holes)
    if holes:
        g = g.copy()
        for lo, hi in holes:
            g[lo * 8:hi * 8] = 1e3                     # a counted hole is worth 1e6 per element
    before = R.canary32(n_partials)
    got = emu_sumsq(g, gid, n_partials, cap, before, fault)
    ref, bound, active = R.sumsq_contract(g, gid, n_partials, cap)
    zeros_ok = bool((R.bits(got[active:]) == 0).all())
    return R.ratio(got[:active], ref[:active], bound[:active]), zeros_ok, got


@pytest.mark.parametrize("n,n_partials,cap", R.SUMSQ_CASES)
def test_sumsq_emulation_stays_inside_its_bound(n, n_partials, cap):
    for kind in R.SUMSQ_FAMILIES:
        r, zeros_ok, _ = sumsq_case(kind, n, n_partials, cap)
        R.record(("sumsq emu", kind), r)
        assert r <= 1.0 and zeros_ok, (kind, r)


def test_norm_faults_are_caught_at_their_named_cases():
    caught = []
    # a counted 255 stretch: case (2056, 2, 0) with the last group of eight a hole
    r, _, _ = sumsq_case("randn", 2056, 2, 0, holes=[(256, 257)], fault="sumsq_counts_255")
    assert r > 1.0
    caught.append("sumsq_counts_255")
    assert sumsq_case("randn", 2056, 2, 0, holes=[(256, 257)])[0] <= 1.0
    # a stale slot: case (8, 5, 0), four workgroups without work
    assert R.sumsq_path(8, 5, 0)[1] == 4
    assert not sumsq_case("randn", 8, 5, 0, fault="stale_partial")[1] and sumsq_case("randn", 8, 5, 0)[1]
    caught.append("stale_partial")
    # torch's 1e-6: case randn (2048, 1, 0), max_norm a quarter of the norm
    _, _, part = sumsq_case("randn", 2048, 1, 0)
    for fault, same in ((None, True), ("coef_no_eps", False)):
        norm, coef, skip, skipped = emu_clip_finish(part, 0.02, 1.0, 3, fault)
        assert R.norm_matches(norm, part, 1.0) and skip == 0 and skipped == 3
        want = R.clip_outputs(norm, 0.02, 3)
        assert (R.bits(coef) == R.bits(want[0])) == same and 0.1 < float(want[0]) < 1.0
    caught.append("coef_no_eps")
    assert caught == NORM_FAULTS


def test_clip_finish_emulation_at_the_edges():
    z = np.zeros(4, f32)
    for part, max_norm, gs, want_skip in ((z, 1.0, 1.0, 0), (z + f32(1e-6), math.inf, 1.0, 0), (z + f32(3e38), 1.0, 1e20, 1),
                                          (np.array([1, np.nan, 1, 1], f32), 1.0, 1.0, 1)):
        norm, coef, skip, skipped = emu_clip_finish(part, max_norm, gs, 7)
        assert R.norm_matches(norm, part, gs)
        assert (R.bits(coef), skip, skipped) == (R.bits(R.clip_outputs(norm, max_norm, 7)[0]),) + R.clip_outputs(norm, max_norm, 7)[1:]
        assert skip == want_skip and skipped == 7 + want_skip and float(coef) == (0.0 if want_skip else 1.0)


# ---- tables, the tie to torch, the host's own arithmetic -----------------------------------------------------------------------------------------
def test_gpu_path_tables_match_the_code_and_cover_every_path():
    import test_gpu_optim
    test_gpu_optim.check_path_tables()


def tiny_optimizer(cls=FlatAdamW, dtype=torch.float32):
    torch.manual_seed(0)
    ws = [torch.nn.Parameter(torch.randn(16, dtype=dtype) * 0.02), torch.nn.Parameter(torch.randn(24, dtype=dtype) * 0.02)]
    spec = [{"params": [w], "lr": lr, "weight_decay": wd} for w, (lr, wd) in zip(ws, R.group_rows("two"))]
    model = torch.nn.Module()
    model.ws = torch.nn.ParameterList(ws)
    args = (model, spec) if cls is FlatAdamW else (spec,)
    return ws, cls(*args, betas=(0.9, 0.999), eps=1e-8)


def test_contract_is_torch_adamw_in_float64():
    """five steps over two groups: torch.optim.AdamW on float64 CPU tensors against the contract fed the same doubles, the bias
    corrections as FlatAdamW computes them before their fp32 rounding"""
    ws, topt = tiny_optimizer(torch.optim.AdamW, torch.float64)
    _, fopt = tiny_optimizer()
    gid = np.array([0, 0, 1, 1, 1], np.uint8)
    m, v = np.zeros(40), np.zeros(40)
    gen = torch.Generator().manual_seed(1)
    for t in range(1, 6):
        groups = []
        for pg in fopt.param_groups:
            bc1, sbc2 = fopt._bias_corrections(pg["betas"][0], pg["betas"][1], t)
            groups.append([pg["lr"], pg["betas"][0], pg["betas"][1], pg["eps"], pg["weight_decay"], bc1, sbc2, 1.0])
        for w in ws:
            w.grad = torch.randn(w.shape, generator=gen, dtype=torch.float64) * 1e-3
        before = {"p": torch.cat([w.detach() for w in ws]).numpy().copy(), "g": torch.cat([w.grad for w in ws]).numpy().copy(), "m": m, "v": v}
        topt.step()
        ref, _, live = R.adamw_contract(before, gid, np.array(groups, f64))
        assert live.all()
        want = {"p": torch.cat([w.detach() for w in ws]).numpy(),
                "m": torch.cat([topt.state[w]["exp_avg"] for w in ws]).numpy(),
                "v": torch.cat([topt.state[w]["exp_avg_sq"] for w in ws]).numpy()}
        for k in "pmv":
            rel = np.abs(ref[k] - want[k]) / np.abs(want[k])
            assert rel.max() <= 1e-12, (t, k, rel.max())
        m, v = ref["m"], ref["v"]


def test_group_structs_hold_the_bias_corrections_to_one_fp32_rounding():
    _, opt = tiny_optimizer()
    decimal.getcontext().prec = 60
    opt.grad_scale = 0.125
    for t in R.T_LIST:
        arr = opt._group_structs(t)
        c1 = 1 - decimal.Decimal(0.9) ** t
        c2 = (1 - decimal.Decimal(0.999) ** t).sqrt()
        for gi, (lr, wd) in enumerate(R.group_rows("two")):
            assert abs(decimal.Decimal(arr[gi].bias_c1) - c1) <= c1 * decimal.Decimal(R.U)
            assert abs(decimal.Decimal(arr[gi].sqrt_bias_c2) - c2) <= c2 * decimal.Decimal(R.U)
            assert arr[gi].bias_c1 != 0                                    # an all-zero block alone means "no update"
            want = R.groups_f32("two", t, 0.125)[gi]
            assert [getattr(arr[gi], k) for k in R.FIELDS] == [float(x) for x in want]      # the structs of the suite are the host's own


def test_ema_weights_sum_to_one_and_differ_from_the_double_rounded_weight():
    """recorded in optim_ref64's docstring: 1 - fp32(d) against fp32(1 - d) at the reference's default decay"""
    d = f32(0.99996)
    ours, theirs = float(ONE - d), float(f32(1.0 - 0.99996))
    assert float(d) + ours == 1.0 and float(d) + theirs != 1.0
    assert 1.2e-4 < abs(ours - theirs) / theirs < 1.4e-4


def test_zz_worst_ratios():
    honest_sweep()
    for key in sorted(R.WORST, key=str):
        print("OPTIM WORST %-22s %-8s err/bound %.3f" % (key[0], key[1], R.WORST[key]))
    assert R.WORST and max(R.WORST.values()) <= 1.0
