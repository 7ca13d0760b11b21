"""vr_ln_fwd / vr_ln_bwd / vr_ln_grad_reduce, the LayerNorm epilogues of vr_gemm_ln and vr_softce / vr_softce_train against the float64
contracts of tests/rowstat_ref64.py: per-element derived bounds on every launch path (rows per wave, rows per workgroup, float4 per lane,
the two soft-CE kernels), keep counts that cut through a float4 group, structural probes with exact inputs, rows whose mean is large
against their spread, and non-finite logits.  Output buffers belong to the test and start as NaN: a row nobody writes fails.

vr_gemm_ln takes ln_keep from device memory and masks per component, so it accepts keep counts that are no multiple of 4 (nothing to
refuse on the host): those cases are bounded like vr_ln_fwd's."""
import math

import pytest
import torch

import rowstat_ref64 as R
import vitres.kernels as K
from vitres import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]

# The launch paths, read from ln.hip: vr_ln_fwd takes nv = ceil(C / 256) float4 per lane (templates 1..5 and 8), RU = 4 (nv <= 2) / 2
# (nv <= 4) / 1 rows per wave, halved while M < 4 RU 1024; vr_ln_bwd takes BWD_ROWS from M and copies and RU = 4 / 2 / 1 for nv = 1 / 2 /
# more.  (M, C) -> (nv, template, RU)
FWD_PATHS = {(16389, 32): (1, 1, 4), (16389, 260): (2, 2, 4), (8195, 32): (1, 1, 2), (8195, 776): (4, 4, 2),
             (1, 32): (1, 1, 1), (2, 32): (1, 1, 1), (3, 32): (1, 1, 1), (5, 32): (1, 1, 1), (85, 32): (1, 1, 1),
             (7, 4): (1, 1, 1), (9, 252): (1, 1, 1), (7, 256): (1, 1, 1), (7, 520): (3, 3, 1), (9, 1024): (4, 4, 1), (7, 1028): (5, 5, 1),
             (6, 1280): (5, 5, 1), (7, 1288): (6, 8, 1), (7, 1540): (7, 8, 1), (9, 1796): (8, 8, 1), (7, 2048): (8, 8, 1)}
# (M, C, copies) -> (nv, inner RU, BWD_ROWS)
BWD_PATHS = {(85, 32, 1): (1, 4, 4), (2051, 32, 1): (1, 4, 8), (8197, 32, 1): (1, 4, 32), (32775, 32, 1): (1, 4, 64),
             (2051, 32, 7): (1, 4, 8), (8197, 32, 64): (1, 4, 16), (2051, 32, 64): (1, 4, 8), (8197, 32, 7): (1, 4, 16),
             (85, 260, 1): (2, 2, 4), (2051, 260, 7): (2, 2, 8), (8197, 260, 64): (2, 2, 16), (8197, 260, 1): (2, 2, 32),
             (85, 776, 1): (4, 1, 4), (2051, 776, 64): (4, 1, 8), (8197, 776, 7): (4, 1, 16), (2051, 776, 1): (4, 1, 8),
             (8197, 776, 1): (4, 1, 32)}
# K -> kernel behind vr_softce_train at ld_grad = K rounded up to 8
SOFTCE_PATHS = {4: "reg", 8: "reg", 37: "pass", 252: "reg", 256: "reg", 260: "reg", 1000: "reg", 1001: "pass", 1020: "reg", 1024: "reg",
                1028: "pass", 1536: "pass"}


def test_path_table_matches_the_code_and_covers_every_path():
    assert set(FWD_PATHS) == {(M, C) for M, C, _ in R.LN_FWD_CASES} and set(BWD_PATHS) == {(M, C, cp) for M, C, cp, _ in R.LN_BWD_CASES}
    assert all(R.ln_fwd_path(M, C) == v for (M, C), v in FWD_PATHS.items())
    assert all(R.ln_bwd_path(M, C, cp)[:3] == v for (M, C, cp), v in BWD_PATHS.items())
    assert set(SOFTCE_PATHS) == set(R.SOFTCE_K) and all(R.softce_train_path(k, R.softce_ld(k)) == v for k, v in SOFTCE_PATHS.items())
    assert {v[2] for v in FWD_PATHS.values()} == {1, 2, 4} and {v[1] for v in FWD_PATHS.values()} == {1, 2, 3, 4, 5, 8}
    assert {v[0] for v in FWD_PATHS.values()} == {1, 2, 3, 4, 5, 6, 7, 8}
    assert {v[2] for v in BWD_PATHS.values()} == {4, 8, 16, 32, 64} and {v[1] for v in BWD_PATHS.values()} == {1, 2, 4}
    assert {(v[1], v[2]) for (M, C, cp), v in BWD_PATHS.items() if cp > 1} >= {(4, 8), (4, 16), (2, 8), (2, 16), (1, 8), (1, 16)}
    assert set(SOFTCE_PATHS.values()) == {"reg", "pass"}


def cu(t):
    return None if t is None else t.to(DEV)


def ln_fwd(x, w, b, keep, rps, eps, out_dtype):
    """vr_ln_fwd on NaN-filled outputs owned by the caller -> rc, y, mean, rstd"""
    M, C = x.shape
    y = torch.full((M, C), NAN, dtype=out_dtype, device=DEV)
    mean, rstd = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
    rc = _lib.lib().vr_ln_fwd(K._p(x), K._p(w), K._p(b), K._p(y), K._p(mean), K._p(rstd), K._p(keep), M, C, rps, eps, K._dtcode(out_dtype),
                              K._stream())
    torch.cuda.synchronize()
    return rc, y, mean, rstd


def ln_bwd(dy, x, w, mean, rstd, keep, rps, dx_in, dw, db, copies, next_cast=None):
    """vr_ln_bwd on NaN-filled dx / gt -> rc, dx, gt"""
    M, C = x.shape
    dx = torch.full((M, C), NAN, device=DEV)
    gt = torch.full((M, C), NAN, dtype=dy.dtype, device=DEV) if next_cast is not None else None
    sc, kp = next_cast if next_cast is not None else (None, None)
    rc = _lib.lib().vr_ln_bwd(K._p(dy), K._p(x), K._p(w), K._p(mean), K._p(rstd), K._p(keep), K._p(dx_in), K._p(dx), K._p(dw), K._p(db),
                              K._p(gt), K._p(sc), K._p(kp), M, C, rps, K._dt(dy), copies, K._stream())
    torch.cuda.synchronize()
    return rc, dx, gt


def show(tag, what, r):
    print("ROWSTAT %s %s: %s" % (tag, what, " ".join("%s=%.3f" % kv for kv in r.items())))


def fwd_case(tag, x, w, b, keep, rps, dtypes=DTYPES):
    ref = R.layernorm_fwd64(x, w, b, keep, rps, R.EPS)
    xd, wd, bd_, kd = cu(x), cu(w), cu(b), cu(keep)
    for dt in dtypes:
        u = R.unit_roundoff(dt)
        bd = R.layernorm_fwd_bounds(x, w, b, keep, rps, R.EPS, u, ref)
        assert bool(bd["valid"].all())
        rc, y, mean, rstd = ln_fwd(xd, wd, bd_, kd, rps, R.EPS, dt)
        assert rc == 0, rc
        r = R.check_ln_fwd(y, mean, rstd, x, w, b, keep, rps, R.EPS, u, ref, bd)
        show(tag, "M%d C%d rps%d %s %s" % (x.shape[0], x.shape[1], rps, "masked" if keep is not None else "plain", str(dt)[6:]), r)
        assert all(v <= 1.0 for v in r.values()), (dt, r)


# ---- LayerNorm forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M,C,rps", R.LN_FWD_CASES)
def test_ln_fwd_random(M, C, rps, masked):
    x, w, b = R.ln_inputs(M * 7 + C, M, C)
    keep = R.keep_cycle(C, (M + rps - 1) // rps, start=M % 5) if masked else None
    fwd_case("ln_fwd", x, w, b, keep, rps)


@pytest.mark.parametrize("rps", [1, 5, 17])
@pytest.mark.parametrize("M,C", [(16384 + 5, 32), (8192 + 3, 32), (85, 260)])
def test_ln_fwd_sample_boundaries_inside_a_wave(M, C, rps):
    """every rps against every rows-per-wave: keep changes between the RU rows of a wave and between the waves of a workgroup"""
    x, w, b = R.ln_inputs(M + C + rps, M, C)
    fwd_case("ln_fwd_rps", x, w, b, R.keep_cycle(C, (M + rps - 1) // rps, start=rps), rps, dtypes=[torch.bfloat16])


@pytest.mark.parametrize("C", [2052, 30])
def test_ln_refuses_unsupported_widths(C):
    x, w, b = R.ln_inputs(C, 3, C)
    with pytest.raises(RuntimeError, match="vr_ln_fwd failed"):
        K.ln_fwd(cu(x), cu(w), cu(b), None, 3, R.EPS, torch.float32)
    z = torch.zeros(3, device=DEV)
    with pytest.raises(RuntimeError, match="vr_ln_bwd failed"):
        K.ln_bwd(cu(x), cu(x), cu(w), z, z, None, 3, None, torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))
    assert not R.ln_supported(C)


@pytest.mark.parametrize("M,C", [(16384 + 5, 32), (16384 + 5, 260), (8192 + 3, 32), (8192 + 3, 776), (85, 32), (5, 1796)])
def test_ln_fwd_ramp_rows_name_the_row_that_was_read(M, C):
    """row m = m + c / 1024: mean[m] = m + (C - 1) / 2048, a neighbour's (or the clamped row M - 1's) statistics miss by >= 1"""
    x = R.ramp_inputs(M, C)
    w, b = torch.ones(C), torch.zeros(C)
    ref = R.layernorm_fwd64(x, w, b, None, M, R.EPS)
    rc, y, mean, rstd = ln_fwd(cu(x), cu(w), cu(b), None, M, R.EPS, torch.float32)
    assert rc == 0
    r = R.check_ln_fwd(y, mean, rstd, x, w, b, None, M, R.EPS, 0.0, ref)
    show("ln_ramp", "M%d C%d" % (M, C), r)
    assert r["mean"] <= 1.0 and r["rstd"] <= 1.0 and r["y"] <= 1.0, r
    assert float((mean.cpu().double() - ref["mean"]).abs().max()) < 0.25


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ratio", [0, 3, 30])
@pytest.mark.parametrize("C", [32, 260, 1288, 2048])
def test_ln_fwd_offset_rows(C, ratio, masked):
    """mean / std up to 30, inside the validity condition: the cancellation term of dvar is what lets the masked path pass"""
    M, rps = 23, 5
    x, w, b = R.offset_inputs(C + ratio, M, C, float(ratio))
    keep = torch.tensor([C, C - 1, C // 2 + 1, C - 3, 5 if ratio < 30 else C - 2], dtype=torch.int32) if masked else None
    fwd_case("ln_offset%d" % ratio, x, w, b, keep, rps, dtypes=[torch.float32, torch.bfloat16])


def degenerate_checks(tag, x, keep, rps, mean, rstd, y):
    ref = R.layernorm_fwd64(x, torch.ones(x.shape[1]), torch.zeros(x.shape[1]), keep, rps, R.EPS)
    bd = R.layernorm_fwd_bounds(x, torch.ones(x.shape[1]), torch.zeros(x.shape[1]), keep, rps, R.EPS, 0.0, ref)
    nonfinite = int((~torch.isfinite(mean)).sum() + (~torch.isfinite(rstd)).sum() + (~torch.isfinite(y.float())).sum())
    rm = R.worst_ratio(mean, ref["mean"], bd["mean"])
    print("ROWSTAT %s: non-finite %d, rstd in [%.4g, %.4g], mean ratio %.3f, rows valid %d / %d" %
          (tag, nonfinite, float(rstd.min()), float(rstd.max()), rm, int(bd["valid"].sum()), x.shape[0]))
    assert nonfinite == 0
    assert float(rstd.min()) > 0 and float(rstd.max()) <= R.EPS ** -0.5 * (1 + 4 * R.U32)
    assert rm <= 1.0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("spread", [1e-4, 0.0])
@pytest.mark.parametrize("value", [0.0, 0.3, 3.3, 10.1, 100.3])
def test_ln_fwd_degenerate_rows_stay_finite(value, spread, masked):
    """rows of value + 1e-4 randn and exactly constant rows: the masked E[x^2] - mean^2 goes negative in fp32 (var + eps < 0 from value
    3.3 on); with the variance clamped at 0 mean, rstd and y are finite and rstd stays within (0, eps^-1/2]"""
    for C in (8, 32, 260, 1280):
        M, rps = 16, 4
        x, w, b = R.degenerate_inputs(C + int(value), M, C, value, spread)
        keep = torch.tensor([C, C - 1, C // 2 + 1, C - 3], dtype=torch.int32) if masked else None
        rc, y, mean, rstd = ln_fwd(cu(x), cu(w), cu(b), cu(keep), rps, R.EPS, torch.bfloat16)
        assert rc == 0
        degenerate_checks("ln_degenerate v%g s%g C%d %s" % (value, spread, C, "masked" if masked else "plain"), x, keep, rps,
                          mean.cpu(), rstd.cpu(), y.cpu())


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("i", range(len(R.LN_BWD_CASES)))
def test_ln_bwd_random(i, dtype):
    M, C, copies, rps = R.LN_BWD_CASES[i]
    masked, with_dx_in, based = i % 2 == 0, i % 4 < 2, i % 3 == 1
    x, w, keep, dy, dx_in, mean_in, rstd_in = R.ln_bwd_inputs(M, C, copies, rps, masked, dtype, with_dx_in)
    ref = R.layernorm_bwd64(dy, x, w, mean_in, rstd_in, keep, rps, dx_in)
    g = torch.Generator().manual_seed(i)
    dw0, db0 = (torch.randn(C, generator=g), torch.randn(C, generator=g)) if based else (None, None)
    dw = cu(dw0) if based else torch.zeros(C, device=DEV)
    db = cu(db0) if based else torch.zeros(C, device=DEV)
    B = (M + rps - 1) // rps
    nc = (cu(torch.tensor([1.0, 0.0, 1.25, 0.5])[torch.arange(B) % 4].contiguous()), cu(R.keep_cycle(C, B, start=3)))
    args = (cu(dy), cu(x), cu(w), cu(mean_in), cu(rstd_in), cu(keep), rps, cu(dx_in))
    if copies > 1:
        part = torch.zeros(2, copies, C, device=DEV)
        rc, dx, gt = ln_bwd(*args, part[0], part[1], copies, next_cast=nc)
        assert rc == 0
        assert torch.equal(dw, cu(dw0) if based else torch.zeros(C, device=DEV))            # untouched until the reduce
        K.ln_grad_reduce([(part[0], part[1], dw, db)], copies)
        torch.cuda.synchronize()
        assert float(part.abs().max()) == 0.0                                              # partial rows are left exactly 0
    else:
        rc, dx, gt = ln_bwd(*args, dw, db, copies, next_cast=nc)
        assert rc == 0
    r = R.check_ln_bwd(dx, dw, db, ref, C, copies, dw0, db0)
    show("ln_bwd", "M%d C%d copies%d rps%d %s %s%s" % (M, C, copies, rps, "masked" if masked else "plain", str(dtype)[6:],
                                                        " dx_in" if with_dx_in else ""), r)
    assert all(v <= 1.0 for v in r.values()), r
    want = K.scale_mask_cast(dx, nc[0], nc[1], rps, dtype)                                  # the existing exact rule, bit for bit
    assert torch.equal(gt, want)
    rc, dx2, _ = ln_bwd(*args, torch.zeros(max(copies, 1), C, device=DEV), torch.zeros(max(copies, 1), C, device=DEV), copies)
    assert rc == 0 and torch.equal(dx2, dx)


@pytest.mark.parametrize("M,C,copies,rps", R.LN_BWD_CASES)
def test_ln_bwd_dw_db_count_every_row_once(M, C, copies, rps):
    """exact inputs (rowstat_ref64.probe_inputs): dw and db must equal the chosen rows' contributions bit for bit"""
    x, dy, mu0, rs1, chosen = R.probe_inputs(M, C, rps, copies)
    w = torch.ones(C)
    ref = R.layernorm_bwd64(dy, x, w, mu0, rs1, None, rps, None)
    assert float(ref["db"][0]) == 2.0 ** len(chosen) - 1
    c = max(copies, 1)
    part = torch.zeros(2, c, C, device=DEV)
    rc, dx, _ = ln_bwd(cu(dy), cu(x), cu(w), cu(mu0), cu(rs1), None, rps, None, part[0], part[1], copies)
    assert rc == 0
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    if copies > 1:
        K.ln_grad_reduce([(part[0], part[1], dw, db)], copies)
    else:
        dw, db = part[0, 0], part[1, 0]
    torch.cuda.synchronize()
    assert torch.equal(db.cpu().double(), ref["db"]) and torch.equal(dw.cpu().double(), ref["dw"])
    r = R.check_ln_bwd(dx, dw, db, ref, C, copies)
    assert r["dx"] <= 1.0, r


# ---- vr_gemm_ln: the LayerNorm epilogues of the fused Linear ------------------------------------------------------------------------------
def _bf(t):
    return t.to(torch.bfloat16)


FUSED = [(2, 33, 8, 72, False), (3, 50, 192, 256, False), (3, 50, 192, 256, True), (5, 17, 448, 128, True), (2, 33, 8, 72, True)]


def fused_keeps(B, C):
    return torch.tensor([(C, C - 1, C - 2, C // 2 + 1, C - 3)[i % 5] for i in range(B)], dtype=torch.int32)


@pytest.mark.parametrize("B,Nt,C,Kd,masked", FUSED)
def test_gemm_ln_forward_statistics(B, Nt, C, Kd, masked):
    """mode 0: the float64 LayerNorm contract applied to the kernel's OWN residual output `out` bounds mean, rstd and y as for vr_ln_fwd"""
    M = B * Nt
    g = torch.Generator().manual_seed(C + Kd)
    a, wt = _bf(torch.randn(M, Kd, generator=g)), _bf(torch.randn(C, Kd, generator=g) * Kd ** -0.5)
    bias, resid = torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    lw, lb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ln_keep = fused_keeps(B, C) if masked else None
    out = torch.full((M, C), NAN, device=DEV)
    assert K.gemm_ln_supported(cu(a), C, C)
    y, mu, rs = K.gemm_ln_fwd(cu(a), cu(wt), out, cu(lw), cu(lb), cu(ln_keep), R.EPS, M=M, N=C, K=Kd, lda=Kd, ldb=Kd, ldc=C, bias=cu(bias),
                              resid=cu(resid), rows_in=Nt)
    torch.cuda.synchronize()
    x = out.cpu()
    u = R.unit_roundoff(torch.bfloat16)
    ref = R.layernorm_fwd64(x, lw, lb, ln_keep, Nt, R.EPS)
    bd = R.layernorm_fwd_bounds(x, lw, lb, ln_keep, Nt, R.EPS, u, ref)
    assert bool(bd["valid"].all())
    r = R.check_ln_fwd(y, mu, rs, x, lw, lb, ln_keep, Nt, R.EPS, u, ref, bd)
    show("gemm_ln_fwd", "B%d Nt%d C%d K%d %s" % (B, Nt, C, Kd, "masked" if masked else "plain"), r)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,Nt,C,Kd", [(2, 33, 8, 72), (3, 50, 192, 256)])
def test_gemm_ln_forward_degenerate_rows_stay_finite(B, Nt, C, Kd, masked):
    """a = 0 and bias = 0: `out` is the residual, rows of value + 1e-4 randn (and constant rows) -- finite with the clamped variance"""
    M = B * Nt
    for value in (0.0, 0.3, 3.3, 10.1, 100.3):
        for spread in (1e-4, 0.0):
            resid, lw, lb = R.degenerate_inputs(C + int(value), M, C, value, spread)
            a, wt = torch.zeros(M, Kd, dtype=torch.bfloat16), _bf(torch.randn(C, Kd, generator=torch.Generator().manual_seed(1)))
            ln_keep = fused_keeps(B, C) if masked else None
            out = torch.full((M, C), NAN, device=DEV)
            y, mu, rs = K.gemm_ln_fwd(cu(a), cu(wt), out, cu(lw), cu(lb), cu(ln_keep), R.EPS, M=M, N=C, K=Kd, lda=Kd, ldb=Kd, ldc=C,
                                      bias=torch.zeros(C, device=DEV), resid=cu(resid), rows_in=Nt)
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), resid)
            degenerate_checks("gemm_ln_degenerate v%g s%g C%d %s" % (value, spread, C, "masked" if masked else "plain"), resid, ln_keep, Nt,
                              mu.cpu(), rs.cpu(), y.cpu())


@pytest.mark.parametrize("B,Nt,C,Kd,masked", FUSED)
def test_gemm_ln_backward_against_the_contract(B, Nt, C, Kd, masked):
    """mode 1: dy is the float64 GEMM of the bf16 operands; its fp32 accumulation error K u32 |du| |wt|^T enters the bounds through the
    backward's linear terms.  That term is orders above the LayerNorm's own roundings (the kernel sits at 0.003 of the bound), so this is
    a check of structure -- every row and channel routed, masked and summed once -- not of rounding.  dw / db depth: a workgroup sums 64
    rows (N <= 320) or 32 (wider), one workgroup per row tile; 64 + 2 + ceil(M / 32) covers both."""
    M = B * Nt
    g = torch.Generator().manual_seed(C + Kd + 1)
    du, wt = _bf(torch.randn(M, Kd, generator=g)), _bf(torch.randn(C, Kd, generator=g) * Kd ** -0.5)
    x, dx_in = torch.rand(M, C, generator=g) - 0.4, torch.randn(M, C, generator=g)
    lw = 1 + 0.1 * torch.randn(C, generator=g)
    ln_keep = fused_keeps(B, C) if masked else None
    f = R.layernorm_fwd64(x, lw, torch.zeros(C), ln_keep, Nt, R.EPS)
    mean_in, rstd_in = f["mean"].float(), f["rstd"].float()
    dy = du.double() @ wt.double().t()
    ddy = Kd * R.U32 * (du.double().abs() @ wt.double().abs().t())
    ref = R.layernorm_bwd64(dy, x, lw, mean_in, rstd_in, ln_keep, Nt, dx_in)
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = K.gemm_ln_bwd(cu(du), cu(wt), cu(x), cu(lw), cu(mean_in), cu(rstd_in), cu(ln_keep), cu(dx_in), dw, db, M=M, N=C, K=Kd, lda=Kd,
                       ldb=Kd, rows_in=Nt)
    torch.cuda.synchronize()
    r = R.check_ln_bwd(dx, dw, db, ref, C, 1, ddy=ddy, depth=64 + 2 + (M + 31) // 32)
    show("gemm_ln_bwd", "B%d Nt%d C%d K%d %s" % (B, Nt, C, Kd, "masked" if masked else "plain"), r)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("masked", [False, True])
def test_gemm_ln_fold_degenerate_rows_stay_finite(masked, monkeypatch):
    """the third place that forms the variance: the row routine of vr_gemm_ln_fold (gemm_ntk.hip), a = 0 and bias = 0 as above"""
    monkeypatch.setattr(K, "LN_FOLD", True)
    B, Nt, C, Kd = 4, 17, 2048, 256
    M = B * Nt
    for value in (3.3, 100.3):
        for spread in (1e-4, 0.0):
            resid, lw, lb = R.degenerate_inputs(C + int(value), M, C, value, spread)
            a, wt = torch.zeros(M, Kd, dtype=torch.bfloat16), _bf(torch.randn(C, Kd, generator=torch.Generator().manual_seed(1)))
            ln_keep = torch.tensor([C, C - 1, C // 2 + 1, C - 3], dtype=torch.int32) if masked else None
            out = torch.full((M, C), NAN, device=DEV)
            got = K.gemm_ln_fold_fwd(cu(a), cu(wt), out, cu(lw), cu(lb), cu(ln_keep), R.EPS, M=M, N=C, K=Kd, lda=Kd, ldb=Kd, ldc=C,
                                     bias=torch.zeros(C, device=DEV), resid=cu(resid), rows_in=Nt)
            assert got is not None, "the form must be covered"
            torch.cuda.synchronize()
            y, mu, rs = got
            assert torch.equal(out.cpu(), resid)
            degenerate_checks("gemm_ln_fold_degenerate v%g s%g %s" % (value, spread, "masked" if masked else "plain"), resid, ln_keep, Nt,
                              mu.cpu(), rs.cpu(), y.cpu())


@pytest.mark.parametrize("bad", [NAN, math.inf])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("C", [32, 260])
def test_ln_fwd_propagates_non_finite_rows(C, masked, bad):
    """a NaN or inf among a row's KEPT channels: that row's mean, rstd and kept y are non-finite (the variance clamp lets a NaN variance
    through); one beyond keep is ignored; every other row stays inside its bounds"""
    M, rps, row, row2 = 12, 3, 4, 7
    x, w, b = R.ln_inputs(C + 5, M, C)
    keep = torch.tensor([C, C - 1, C // 2 + 1, C - 3], dtype=torch.int32) if masked else None
    xb = x.clone()
    xb[row, 2] = bad
    x0 = x.clone()
    if masked:
        p2 = int(keep[row2 // rps])
        xb[row2, p2], x0[row2, p2] = bad, 0.0                # beyond keep: as good as any other value there
    ref = R.layernorm_fwd64(x0, w, b, keep, rps, R.EPS)
    bd = R.layernorm_fwd_bounds(x0, w, b, keep, rps, R.EPS, 0.0, ref)
    rc, y, mean, rstd = ln_fwd(cu(xb), cu(w), cu(b), cu(keep), rps, R.EPS, torch.float32)
    assert rc == 0
    y, mean, rstd = y.cpu(), mean.cpu(), rstd.cpu()
    p = int(ref["p"][row])
    assert not math.isfinite(float(mean[row])) and not math.isfinite(float(rstd[row])) and not bool(torch.isfinite(y[row, :p]).any())
    assert float(y[row, p:].abs().sum()) == 0.0
    others = [m for m in range(M) if m != row]
    assert R.worst_ratio(mean[others], ref["mean"][others], bd["mean"][others]) <= 1.0
    assert R.worst_ratio(rstd[others], ref["rstd"][others], bd["rstd"][others]) <= 1.0
    assert R.worst_ratio(y[others], ref["y"][others], bd["y"][others]) <= 1.0


# ---- soft-target cross entropy ---------------------------------------------------------------------------------------------------------
def softce_train(x, t, smap, rps, ld, dt, acc0=0.5):
    Rn, Kc = x.shape
    d = torch.full((Rn, ld), NAN, dtype=dt, device=DEV)
    acc = torch.full((1,), acc0, device=DEV)
    rc = _lib.lib().vr_softce_train(K._p(x), K._p(t), K._p(smap), rps, K._p(acc), K._p(d), ld, K._dtcode(dt), Rn, Kc, 1.0 / Rn, 1.0 / Rn,
                                    K._stream())
    torch.cuda.synchronize()
    return rc, d, acc


def softce_one(tag, x, t, smap, rps, worst):
    Rn, Kc = x.shape
    ld = R.softce_ld(Kc)
    xd, td, sd = cu(x), cu(t), cu(smap)
    ref = R.softce_train64(x, t, smap, rps, ld, 1.0 / Rn, 1.0 / Rn, 0.5)
    for dt in (torch.float32, torch.bfloat16):
        bd = R.softce_bounds(ref, R.unit_roundoff(dt))
        rc, d, acc = softce_train(xd, td, sd, rps, ld, dt)
        assert rc == 0
        assert ld == Kc or float(d[:, Kc:].float().abs().max()) == 0.0                     # pad columns exactly 0
        r = dict(grad=R.worst_ratio(d, ref["grad"], bd["grad"]), acc=R.worst_ratio(acc, ref["acc"], bd["acc"]))
        for k, v in r.items():
            worst["train_" + k] = max(worst.get("train_" + k, 0.0), v)
        assert all(v <= 1.0 for v in r.values()), (tag, dt, r)
    tg = t[R.target_rows(Rn, rps, smap)].contiguous()
    ref = R.softce64(x, tg, 0.25)
    bd = R.softce_bounds(ref, 0.0)
    loss, d = K.softce(xd, cu(tg), 0.25)
    torch.cuda.synchronize()
    r = dict(loss=R.worst_ratio(loss, ref["loss"], bd["loss"]), grad=R.worst_ratio(d, ref["grad"], bd["grad"]))
    for k, v in r.items():
        worst["softce_" + k] = max(worst.get("softce_" + k, 0.0), v)
    assert all(v <= 1.0 for v in r.values()), (tag, r)


def softce_layout(Rn, j):
    """(rps, sample_map or None, target rows): rps in {1, 4}, permuted map and None; a partial last sample when rps does not divide R"""
    rps = (1, 4)[j % 2] if Rn > 1 else 1
    B = (Rn + rps - 1) // rps
    smap = torch.randperm(B, generator=torch.Generator().manual_seed(Rn + j)) if (j // 2) % 2 == 0 else None
    return rps, smap, B * rps


@pytest.mark.parametrize("Kc", R.SOFTCE_K)
def test_softce_families(Kc):
    """every logit family against every target family at R = 8, the diagonal at R = 1, 5, 66; both vr_softce_train kernels' gradient
    dtypes and vr_softce; loss_acc pre-filled with 0.5"""
    worst, j = {}, 0
    for Rn in R.SOFTCE_R:
        for li, lf in enumerate(R.LOGIT_FAMILIES):
            for ti, tf in enumerate(R.TARGET_FAMILIES):
                if Rn != 8 and li != ti:
                    continue
                rps, smap, Tn = softce_layout(Rn, j)
                j += 1
                x, t = R.softce_logits(lf, Kc + Rn, Rn, Kc), R.softce_targets(tf, Kc + Rn + 1, Tn, Kc)
                softce_one("K%d R%d rps%d %s %s %s" % (Kc, Rn, rps, "map" if smap is not None else "nomap", lf, tf), x, t, smap, rps, worst)
    show("softce", "K%d (%s)" % (Kc, SOFTCE_PATHS[Kc]), worst)


@pytest.mark.parametrize("bad", [NAN, math.inf])
@pytest.mark.parametrize("Kc", [37, 1000, 1028])
def test_softce_propagates_non_finite_logits(Kc, bad):
    """a NaN or +inf in one logit row: that row's gradient and loss_acc are non-finite, every other row stays inside its bounds"""
    Rn, row = 8, 5
    x, t = R.softce_logits("randn2", Kc, Rn, Kc), R.softce_targets("softmax", Kc + 1, Rn, Kc)
    xb = x.clone()
    xb[row, Kc // 2] = bad
    ld = R.softce_ld(Kc)
    ref = R.softce_train64(x, t, None, 1, ld, 1.0 / Rn, 1.0 / Rn, 0.5)
    others = [r for r in range(Rn) if r != row]
    for dt in (torch.float32, torch.bfloat16):
        bd = R.softce_bounds(ref, R.unit_roundoff(dt))
        rc, d, acc = softce_train(cu(xb), cu(t), None, 1, ld, dt)
        assert rc == 0
        assert not bool(torch.isfinite(d[row, :Kc].float()).any()) and not math.isfinite(acc.item())
        assert R.worst_ratio(d[others], ref["grad"][others], bd["grad"][others]) <= 1.0
        assert ld == Kc or float(d[others][:, Kc:].float().abs().max()) == 0.0
    loss, d = K.softce(cu(xb), cu(t), 1.0)
    torch.cuda.synchronize()
    ref = R.softce64(x, t, 1.0)
    bd = R.softce_bounds(ref, 0.0)
    assert not math.isfinite(float(loss[row])) and not bool(torch.isfinite(d[row]).any())
    assert R.worst_ratio(loss[others], ref["loss"][others], bd["loss"][others]) <= 1.0
    assert R.worst_ratio(d[others], ref["grad"][others], bd["grad"][others]) <= 1.0
