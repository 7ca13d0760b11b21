"""tests/rowstat_ref64.py on the CPU: the bounds hold for an emulation of the kernels' rounding points, and they (or the structural
probes built on them) reject injected faults.  The emulation is torch fp32 on the CPU -- IEEE fp32 after every operation, which is what
float64 with a round to fp32 after each +, -, *, /, sqrt gives -- in the lane / shuffle summation order of ln.hip and misc.hip, with
16-bit output rounding; exp and log are float64 values rounded to fp32 (inside the 1 ULP of v_exp_f32 / v_log_f32)."""
import math

import pytest
import torch

import emu_kernels as E
import rowstat_ref64 as R

F32 = torch.float32
LANE = torch.arange(64)
LOG2E = torch.tensor(0x3fb8aa3b, dtype=torch.int32).view(F32)         # the constant hipcc multiplies by before v_exp_f32
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def wave_sum(s):
    """[M, 64] per-lane partials -> [M]: the xor butterfly of common.h"""
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, LANE ^ o]
    return s[:, 0]


def lanes(t, C):
    """[M, C] -> [M, nv, 64, 4]: lane l holds float4 l + 64 j; zero beyond C"""
    M, nv = t.shape[0], (C + 255) // 256
    out = torch.zeros(M, nv * 256, dtype=F32)
    out[:, :C] = t
    return out.view(M, nv, 64, 4)


def row_sum(t, C):
    """s += x + y + z + w per float4, then the butterfly"""
    q = lanes(t, C)
    s = torch.zeros(t.shape[0], 64, dtype=F32)
    for j in range(q.shape[1]):
        s = s + (((q[:, j, :, 0] + q[:, j, :, 1]) + q[:, j, :, 2]) + q[:, j, :, 3])
    return wave_sum(s)


def emu_ln_fwd(x, w, b, keep, rps, eps, out_dtype, fault=None):
    """-> y [M, C] out_dtype, mean, rstd fp32.  fault = (name, row)"""
    C = x.shape[-1]
    X, w, b = x.reshape(-1, C).to(F32), w.to(F32), b.to(F32)
    M = X.shape[0]
    p = R.rows_keep(keep, M, C, rps)
    if fault and fault[0] == "neighbour_keep":          # row m normalised with the next sample's keep
        p = p.clone()
        p[fault[1]] = int(keep[(fault[1] // rps + 1) % keep.numel()])
    mask = torch.arange(C)[None, :] < p[:, None]
    if fault and fault[0] == "partial_group":           # component p of a partly kept float4 group let through
        assert int(p[fault[1]]) % 4 != 0
        mask = mask.clone()
        mask[fault[1], int(p[fault[1]])] = True
    Xm = torch.where(mask, X, torch.zeros((), dtype=F32))
    pf = p.to(F32)
    inv_n = torch.where(p > 0, 1.0 / pf.clamp(min=1), torch.zeros_like(pf))
    mu = row_sum(Xm, C) * inv_n
    if keep is not None:
        var = row_sum(Xm * Xm, C) * inv_n - mu * mu
    else:
        d = Xm - mu[:, None]
        var = row_sum(d * d, C) * inv_n
    if not (fault and fault[0] == "no_clamp"):
        var = var.clamp(min=0)
    rs = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    if fault and fault[0] == "tail_stats":              # the clamped tail load (row M - 1) being stored for row m
        mu, rs = mu.clone(), rs.clone()
        mu[fault[1]], rs[fault[1]] = mu[M - 1], rs[M - 1]
    y = torch.where(mask, w * ((Xm - mu[:, None]) * rs[:, None]) + b, torch.zeros((), dtype=F32))
    return y.to(out_dtype), mu, rs


def emu_ln_bwd(dy, x, w, mean, rstd, keep, rps, dx_in, copies, dw0=None, db0=None, fault=None):
    """-> dx [M, C], dw, db (after vr_ln_grad_reduce when copies > 1; the partial rows start at 0, dw / db at dw0 / db0 or 0)"""
    C = x.shape[-1]
    X, G, w = x.reshape(-1, C).to(F32), dy.reshape(-1, C).to(F32), w.to(F32)
    M = X.shape[0]
    p = R.rows_keep(keep, M, C, rps)
    mask = torch.arange(C)[None, :] < p[:, None]
    pf = p.to(F32)
    inv_n = torch.where(p > 0, 1.0 / pf.clamp(min=1), torch.zeros_like(pf))
    mu, rs = mean.to(F32)[:, None], rstd.to(F32)[:, None]
    a = torch.where(mask, G, torch.zeros((), dtype=F32))
    z = (torch.where(mask, X, mu.expand(M, C)) - mu) * rs
    g = a * w
    s1 = (row_sum(g, C) * inv_n)[:, None]
    s2 = (row_sum(g * z, C) * inv_n)[:, None]
    dx = (g - (s1 + z * s2)) * rs
    if dx_in is not None:
        dx = dx + dx_in.reshape(-1, C).to(F32)
    dx = torch.where(mask, dx, torch.zeros((), dtype=F32))
    cw, cb = a * z, a.clone()
    if fault and fault[0] == "drop_row":
        cw[fault[1]], cb[fault[1]] = 0.0, 0.0
    if fault and fault[0] == "row_twice":
        cw[fault[1]], cb[fault[1]] = 2 * cw[fault[1]], 2 * cb[fault[1]]
    _, _, rows, wgs = R.ln_bwd_path(M, C, copies)
    c = max(copies, 1)
    outs = []
    for contrib, base in ((cw, dw0), (cb, db0)):
        t = torch.zeros(wgs * rows, C, dtype=F32)
        t[:M] = contrib
        t = t.view(wgs, rows // 4, 4, C)                 # row rr of a workgroup belongs to wave rr % 4, walked in ascending order
        acc = torch.zeros(wgs, 4, C, dtype=F32)
        for i in range(rows // 4):
            acc = acc + t[:, i]
        wg = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
        dst = base.to(F32).clone() if base is not None else torch.zeros(C, dtype=F32)
        part = torch.zeros(c, C, dtype=F32) if c > 1 else dst[None, :]
        for k in range((wgs + c - 1) // c):              # workgroup b adds into row b % copies (here: in workgroup order)
            blk = wg[k * c:(k + 1) * c]
            part[:blk.shape[0]] += blk
        if c > 1:                                         # ln_grad_reduce_kernel: four chains over groups of 16, the rest into chain 0
            ch = [torch.zeros(C, dtype=F32) for _ in range(4)]
            k = 0
            while k + 16 <= c:
                for u_ in range(0, 16, 4):
                    for e in range(4):
                        ch[e] = ch[e] + part[k + u_ + e]
                k += 16
            for k in range(k, c):
                ch[0] = ch[0] + part[k]
            dst = dst + ((ch[0] + ch[1]) + (ch[2] + ch[3]))
        else:
            dst = part[0]
        outs.append(dst)
    return dx, outs[0], outs[1]


def fexp(d):
    return torch.exp2((d * LOG2E).to(torch.float64)).to(F32)


def emu_softce(x, t, K, ld, gscale, loss_scale, acc0, path, grad_dtype, fault=None):
    """t already gathered [R, K].  path 'pass' (vr_softce and the pass-by-pass train kernel) or 'reg'.  -> loss [R], grad [R, ld], acc"""
    X, T = x.to(F32), t.to(F32)
    Rn = X.shape[0]
    mx = X.max(dim=1, keepdim=True).values
    e = fexp(X - mx)
    if path == "pass":
        n = (K + 63) // 64
        pad = lambda v: torch.cat([v, torch.zeros(Rn, n * 64 - K, dtype=F32)], 1).view(Rn, n, 64)
        ee, tt, tx = pad(e), pad(T), pad(T * X)
        se = st = stx = torch.zeros(Rn, 64, dtype=F32)
        for i in range(n):
            se, st, stx = se + ee[:, i], st + tt[:, i], stx + tx[:, i]
    else:
        pad = lambda v: torch.cat([v, torch.zeros(Rn, 1024 - K, dtype=F32)], 1).view(Rn, 4, 64, 4)
        ee, tt, tx = pad(e), pad(T), pad(T * X)
        if fault and fault[0] == "pad_exp0":             # a -inf padding lane contributing exp(0)
            assert K < 1024
            ee = ee.clone()
            ee.view(Rn, 1024)[fault[1], K] = 1.0
        quad = lambda q: (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
        se = st = stx = torch.zeros(Rn, 64, dtype=F32)
        for v in range(4):
            se, st, stx = se + quad(ee[:, v]), st + quad(tt[:, v]), stx + quad(tx[:, v])
    se, st, stx = wave_sum(se), wave_sum(st), wave_sum(stx)
    lse = mx[:, 0] + torch.log(se.to(torch.float64)).to(F32)
    loss = lse * st - stx
    if path == "pass":
        g = gscale * (e * (1.0 / se)[:, None] * st[:, None] - T)
    else:
        g = gscale * (e * (st / se)[:, None] - T)
    acc = torch.tensor(acc0, dtype=F32)
    for r in range(Rn):
        acc = acc + loss[r] * torch.tensor(loss_scale, dtype=F32)
    grad = torch.zeros(Rn, ld, dtype=F32)
    grad[:, :K] = g
    return loss, grad.to(grad_dtype), acc.reshape(1)


WORST = {}


def note(key, ratios):
    for k, v in ratios.items():
        WORST[(key, k)] = max(WORST.get((key, k), 0.0), v)


# ---- the emulation stays inside the bounds on every case family of the GPU test ---------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M,C,rps", R.LN_FWD_CASES)
def test_ln_fwd_emulation_within_bounds(M, C, rps, masked):
    x, w, b = R.ln_inputs(M * 7 + C, M, C)
    keep = R.keep_cycle(C, (M + rps - 1) // rps, start=M % 5) if masked else None
    ref = R.layernorm_fwd64(x, w, b, keep, rps, R.EPS)
    for dt in DTYPES:
        bd = R.layernorm_fwd_bounds(x, w, b, keep, rps, R.EPS, R.unit_roundoff(dt), ref)
        assert bool(bd["valid"].all())
        y, mu, rs = emu_ln_fwd(x, w, b, keep, rps, R.EPS, dt)
        r = R.check_ln_fwd(y, mu, rs, x, w, b, keep, rps, R.EPS, R.unit_roundoff(dt), ref, bd)
        note("ln_fwd", r)
        assert all(v < 1.0 for v in r.values()), (dt, r)
    # tests/emu_kernels.py states the same contract
    y, mu, rs = E.ln_fwd(x, w, b, keep, rps, R.EPS, torch.float32)
    r = R.check_ln_fwd(y, mu, rs, x, w, b, keep, rps, R.EPS, 0.0, ref)
    assert all(v < 1.0 for v in r.values()), r


bwd_case = R.ln_bwd_inputs


@pytest.mark.parametrize("i", range(len(R.LN_BWD_CASES)))
def test_ln_bwd_emulation_within_bounds(i):
    M, C, copies, rps = R.LN_BWD_CASES[i]
    masked, dtype, with_dx_in = i % 2 == 0, (torch.bfloat16 if i % 3 else torch.float32), i % 4 < 2
    x, w, keep, dy, dx_in, mean_in, rstd_in = bwd_case(M, C, copies, rps, masked, dtype, with_dx_in)
    ref = R.layernorm_bwd64(dy, x, w, mean_in, rstd_in, keep, rps, dx_in)
    dx, dw, db = emu_ln_bwd(dy, x, w, mean_in, rstd_in, keep, rps, dx_in, copies)
    r = R.check_ln_bwd(dx, dw, db, ref, C, copies)
    note("ln_bwd", r)
    assert all(v < 1.0 for v in r.values()), r
    dwe, dbe = torch.zeros(C), torch.zeros(C)
    dxe = E.ln_bwd(dy, x, w, mean_in, rstd_in, keep, rps, dx_in, dwe, dbe)
    r = R.check_ln_bwd(dxe, dwe, dbe, ref, C, 1)
    assert all(v < 1.0 for v in r.values()), r


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ratio", [0, 3, 30])
@pytest.mark.parametrize("C", [32, 260, 1288, 2048])
def test_offset_rows_emulation_within_bounds(C, ratio, masked):
    M, rps = 23, 5
    x, w, b = R.offset_inputs(C + ratio, M, C, float(ratio))
    keep = torch.tensor([C, C - 1, C // 2 + 1, C - 3, 5 if ratio < 30 else C - 2], dtype=torch.int32) if masked else None
    ref = R.layernorm_fwd64(x, w, b, keep, rps, R.EPS)
    bd = R.layernorm_fwd_bounds(x, w, b, keep, rps, R.EPS, 0.0, ref)
    assert bool(bd["valid"].all())
    y, mu, rs = emu_ln_fwd(x, w, b, keep, rps, R.EPS, torch.float32)
    r = R.check_ln_fwd(y, mu, rs, x, w, b, keep, rps, R.EPS, 0.0, ref, bd)
    note("ln_offset", r)
    assert all(v < 1.0 for v in r.values()), r


SOFTCE_HOST = [(K, R.LOGIT_FAMILIES[i % 5], R.TARGET_FAMILIES[(i // 2 + j) % 5]) for i, K in enumerate(R.SOFTCE_K) for j in range(2)] + \
              [(1000, lf, tf) for lf in R.LOGIT_FAMILIES for tf in R.TARGET_FAMILIES] + \
              [(37, lf, "softmax") for lf in R.LOGIT_FAMILIES] + [(1536, lf, "smooth") for lf in R.LOGIT_FAMILIES]


@pytest.mark.parametrize("K,lf,tf", SOFTCE_HOST)
def test_softce_emulation_within_bounds(K, lf, tf):
    Rn, rps = 8, 4
    x, t = R.softce_logits(lf, K, Rn, K), R.softce_targets(tf, K + 1, Rn, K)
    smap = torch.tensor([1, 0])
    ld = R.softce_ld(K)
    for dt in (torch.float32, torch.bfloat16):
        ref = R.softce_train64(x, t, smap, rps, ld, 1.0 / Rn, 1.0 / Rn, 0.5)
        bd = R.softce_bounds(ref, R.unit_roundoff(dt))
        tg = t[R.target_rows(Rn, rps, smap)]
        loss, grad, acc = emu_softce(x, tg, K, ld, 1.0 / Rn, 1.0 / Rn, 0.5, R.softce_train_path(K, ld), dt)
        r = dict(loss=R.worst_ratio(loss, ref["loss"], bd["loss"]), grad=R.worst_ratio(grad, ref["grad"], bd["grad"]),
                 acc=R.worst_ratio(acc, ref["acc"], bd["acc"]))
        note("softce", r)
        assert all(v < 1.0 for v in r.values()), (dt, r)
    # vr_softce's order (pass by pass, no pad) and the emulation of tests/emu_kernels.py
    ref = R.softce64(x, tg, 0.25)
    bd = R.softce_bounds(ref, 0.0)
    loss, grad, _ = emu_softce(x, tg, K, K, 0.25, 1.0, 0.0, "pass", torch.float32)
    assert R.worst_ratio(loss, ref["loss"], bd["loss"]) < 1.0 and R.worst_ratio(grad, ref["grad"], bd["grad"]) < 1.0
    le, ge = E.softce(x, tg, 0.25)
    assert R.worst_ratio(le, ref["loss"], bd["loss"]) < 1.0 and R.worst_ratio(ge, ref["grad"], bd["grad"]) < 1.0
    acc_e = torch.full((1,), 0.5)
    ge = E.softce_train(x, t, smap, rps, acc_e, torch.float32)
    ref = R.softce_train64(x, t, smap, rps, ld, 1.0 / Rn, 1.0 / Rn, 0.5)
    bd = R.softce_bounds(ref, 0.0)
    assert R.worst_ratio(ge, ref["grad"], bd["grad"]) < 1.0 and R.worst_ratio(acc_e, ref["acc"], bd["acc"]) < 1.0


# ---- injected faults exceed the bound on the inputs the GPU test uses for that edge ---------------------------------------------------
def _fwd_fault(M, C, rps, fault, row_of):
    x, w, b = R.ln_inputs(M * 7 + C, M, C)
    keep = R.keep_cycle(C, (M + rps - 1) // rps, start=M % 5)
    ref = R.layernorm_fwd64(x, w, b, keep, rps, R.EPS)
    row = row_of(ref["p"])
    y, mu, rs = emu_ln_fwd(x, w, b, keep, rps, R.EPS, torch.bfloat16, fault=(fault, row))
    return R.check_ln_fwd(y, mu, rs, x, w, b, keep, rps, R.EPS, 2.0 ** -8, ref)


@pytest.mark.parametrize("M,C,rps", [(16384 + 5, 32, 17), (8192 + 3, 776, 17), (85, 32, 5)])
def test_fault_neighbour_keep(M, C, rps):
    """the last row of a sample normalised with the next sample's keep (a wave's RU rows straddling the boundary)"""
    def row_of(p):
        cand = [m for m in range(rps - 1, M - 1, rps) if p[m] != p[m + 1] and p[m] > 1 and p[m + 1] > 1]
        return cand[len(cand) // 2]
    r = _fwd_fault(M, C, rps, "neighbour_keep", row_of)
    assert r["y"] > 1.0 and r["mean"] > 1.0, r


@pytest.mark.parametrize("M,C,rps", [(16384 + 5, 32, 17), (16384 + 5, 260, 5), (8192 + 3, 32, 5)])
def test_fault_tail_statistics_stored(M, C, rps):
    r = _fwd_fault(M, C, rps, "tail_stats", lambda p: int(torch.nonzero(p[:M - 1] == C)[-1]))      # the last fully kept row before M - 1
    assert r["mean"] > 1.0 and r["y"] > 1.0, r
    x = R.ramp_inputs(M, C)                             # the structural probe: mean[m] names the row
    w, b = torch.ones(C), torch.zeros(C)
    y, mu, rs = emu_ln_fwd(x, w, b, None, M, R.EPS, torch.float32, fault=("tail_stats", M - 3))
    assert R.check_ln_fwd(y, mu, rs, x, w, b, None, M, R.EPS, 0.0)["mean"] > 1.0
    y, mu, rs = emu_ln_fwd(x, w, b, None, M, R.EPS, torch.float32)
    assert R.check_ln_fwd(y, mu, rs, x, w, b, None, M, R.EPS, 0.0)["mean"] < 1.0


@pytest.mark.parametrize("M,C,rps", [(85, 32, 5), (9, 1796, 5), (16384 + 5, 260, 5)])
def test_fault_partial_group_component(M, C, rps):
    r = _fwd_fault(M, C, rps, "partial_group", lambda p: int(torch.nonzero((p % 4 != 0) & (p > 4))[0]))
    assert r["y"] == math.inf, r                        # the channel beyond keep must be exactly 0


probe_inputs = R.probe_inputs


@pytest.mark.parametrize("fault", ["drop_row", "row_twice"])
@pytest.mark.parametrize("M,C,copies,rps", [(85, 32, 1, 17), (32768 + 7, 32, 1, 5), (8192 + 5, 260, 64, 5)])
def test_fault_row_missing_or_twice_in_dw_db(M, C, copies, rps, fault):
    """Under random inputs the summation-depth bound widens with M while one row's share of dw / db does not: the fault reaches a ratio of
    1.4e4 at M = 85 but only 3.5 .. 4 at M = 32775 (printed).  The structural probe (exact inputs, equality) catches it at every M."""
    x, w, keep, dy, dx_in, mean_in, rstd_in = bwd_case(M, C, copies, rps, True, torch.float32, False)
    ref = R.layernorm_bwd64(dy, x, w, mean_in, rstd_in, keep, rps, None)
    live = torch.nonzero(ref["p"] >= C - 3)
    row = int(live[len(live) // 2])
    dx, dw, db = emu_ln_bwd(dy, x, w, mean_in, rstd_in, keep, rps, None, copies, fault=(fault, row))
    r = R.check_ln_bwd(dx, dw, db, ref, C, copies)
    print("ROWSTAT-FAULT %s M%d C%d copies%d random inputs: dw %.3f db %.3f" % (fault, M, C, copies, r["dw"], r["db"]))
    assert r["dw"] > 1.0 and r["db"] > 1.0, r
    xp, dyp, mu0, rs1, chosen = probe_inputs(M, C, rps, copies)
    refp = R.layernorm_bwd64(dyp, xp, torch.ones(C), mu0, rs1, None, rps, None)
    assert float(refp["db"][0]) == 2.0 ** len(chosen) - 1
    for m in (chosen[0], chosen[-1], chosen[len(chosen) // 2]):
        _, dwp, dbp = emu_ln_bwd(dyp, xp, torch.ones(C), mu0, rs1, None, rps, None, copies, fault=(fault, m))
        assert not torch.equal(dwp.double(), refp["dw"]) and not torch.equal(dbp.double(), refp["db"])
    _, dwp, dbp = emu_ln_bwd(dyp, xp, torch.ones(C), mu0, rs1, None, rps, None, copies)
    assert torch.equal(dwp.double(), refp["dw"]) and torch.equal(dbp.double(), refp["db"])


@pytest.mark.parametrize("value", [3.3, 10.1, 100.3])
@pytest.mark.parametrize("C", [32, 260, 1280])
def test_fault_masked_variance_outside_the_validity_condition(C, value):
    """rows of value + 1e-4 randn: the masked formula loses var entirely; `valid` is false there and the unclamped formula gives NaN or an
    rstd above eps^-1/2 -- which is why such rows are asserted separately, and never against drstd."""
    M = 16
    x, w, b = R.degenerate_inputs(C, M, C, value, 1e-4)
    keep = torch.full((M,), C, dtype=torch.int32)
    ref = R.layernorm_fwd64(x, w, b, keep, 1, R.EPS)
    bd = R.layernorm_fwd_bounds(x, w, b, keep, 1, R.EPS, 0.0, ref)
    assert not bool(bd["valid"].any())
    y, mu, rs = emu_ln_fwd(x, w, b, keep, 1, R.EPS, torch.float32, fault=("no_clamp", 0))
    # judged by what the tests assert on such rows (not by drstd, which does not hold there): var < 0 gives a NaN, or an rstd above eps^-1/2
    limit = R.EPS ** -0.5 * (1 + 4 * R.U32)
    assert bool(torch.isnan(rs).any()) or float(rs.max()) > limit
    print("ROWSTAT-FAULT no_clamp C%d value %g: NaN rstd rows %d / %d, largest finite rstd %.1f" %
          (C, value, int(torch.isnan(rs).sum()), M, float(rs[~torch.isnan(rs)].max()) if bool((~torch.isnan(rs)).any()) else float("nan")))
    # with the clamp: finite, 0 < rstd <= eps^-1/2 (1 + 4 u32), mean inside its bound
    y, mu, rs = emu_ln_fwd(x, w, b, keep, 1, R.EPS, torch.float32)
    assert bool(torch.isfinite(y).all()) and bool((rs > 0).all()) and float(rs.max()) <= R.EPS ** -0.5 * (1 + 4 * R.U32)
    assert R.worst_ratio(mu, ref["mean"], bd["mean"]) <= 1.0


@pytest.mark.parametrize("K", [252, 1000, 1020])
def test_fault_softce_pad_lane_and_ungathered_target(K):
    Rn, rps = 8, 4
    ld = R.softce_ld(K)
    assert R.softce_train_path(K, ld) == "reg"
    x, t = R.softce_logits("randn2", K, Rn, K), R.softce_targets("softmax", K + 1, Rn, K)
    smap = torch.tensor([1, 0])
    ref = R.softce_train64(x, t, smap, rps, ld, 1.0 / Rn, 1.0 / Rn, 0.5)
    bd = R.softce_bounds(ref, 0.0)
    tg = t[R.target_rows(Rn, rps, smap)]
    loss, grad, acc = emu_softce(x, tg, K, ld, 1.0 / Rn, 1.0 / Rn, 0.5, "reg", torch.float32, fault=("pad_exp0", 3))
    assert R.worst_ratio(loss, ref["loss"], bd["loss"]) > 1.0 and R.worst_ratio(grad, ref["grad"], bd["grad"]) > 1.0
    assert R.worst_ratio(acc, ref["acc"], bd["acc"]) > 1.0
    tg2 = tg.clone()
    tg2[5] = t[5]                                       # row 5 read without sample_map
    loss, grad, acc = emu_softce(x, tg2, K, ld, 1.0 / Rn, 1.0 / Rn, 0.5, "reg", torch.float32)
    assert R.worst_ratio(loss, ref["loss"], bd["loss"]) > 1.0 and R.worst_ratio(grad, ref["grad"], bd["grad"]) > 1.0


def test_launch_paths_cover_every_template():
    fwd = {R.ln_fwd_path(M, C)[1:] for M, C, _ in R.LN_FWD_CASES}
    assert {ru for _, ru in fwd} == {1, 2, 4} and {t for t, _ in fwd} == {1, 2, 3, 4, 5, 8}
    assert {R.ln_fwd_path(M, C)[0] for M, C, _ in R.LN_FWD_CASES} == {1, 2, 3, 4, 5, 6, 7, 8}
    bwd = {R.ln_bwd_path(M, C, cp)[1:3] for M, C, cp, _ in R.LN_BWD_CASES}
    assert {rows for _, rows in bwd} == {4, 8, 16, 32, 64} and {ru for ru, _ in bwd} == {1, 2, 4}
    assert {R.softce_train_path(K, R.softce_ld(K)) for K in R.SOFTCE_K} == {"reg", "pass"}
    assert R.softce_train_path(1024, 1024) == "reg" and R.softce_train_path(1028, 1032) == "pass"
    assert not R.ln_supported(30) and not R.ln_supported(2052) and R.ln_supported(2048) and R.ln_supported(4)


def test_worst_ratios_are_reported(capsys):
    """A report, not a check (every case above asserts its own ratios): prints what the emulation reached per family and output, for
    the cases that ran in this session."""
    with capsys.disabled():
        for (fam, out), v in sorted(WORST.items()):
            print("ROWSTAT-EMU %s %s worst ratio %.3f" % (fam, out, v))
