"""The contracts, launch-path functions, bounds and inputs of tests/glue_ref64.py, checked on the CPU:

  * every contract agrees with a second statement of the operation (torch.nn.functional.unfold / fold / avg_pool2d, tests/emu_kernels.py)
    and the spatial-reduction pairs satisfy their adjoint identities in float64;
  * the path functions equal the literal tables of tests/test_gpu_glue.py and the case lists reach every form and pass count;
  * for every bounded kernel and case, fp32 emulations of the kernel's summation in three orders stay inside the bound, and every
    injected fault leaves it by a factor >= 100 (the figure is the worst element of the case: the device test fails when one element does);
  * a fault on an exact contract's output fails the integer comparison.

No test here needs a device."""
import ast
import math
import os

import torch
import torch.nn.functional as F

import emu_kernels as E
import glue_ref64 as R
import test_gpu_glue as T
from glue_ref64 import BF16, F16, F32

MIN_FAULT_RATIO = 100.0


def test_path_tables_match_the_code_and_cover_every_path():
    T.check_path_tables()


def test_no_case_is_left_out():
    """neither glue suite skips or expects a failure: no decorator, call or attribute of that name in their syntax trees"""
    here = os.path.dirname(os.path.abspath(__file__))
    for fn in ("test_gpu_glue.py", "test_glue_ref_host.py", "glue_ref64.py"):
        tree = ast.parse(open(os.path.join(here, fn)).read())
        names = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} | {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
        assert not names & {"skip", "skipif", "xfail", "importorskip"}, fn


# ---- canaries and the integer comparison ---------------------------------------------------------------------------------------------------------
def test_canary_is_a_nan_in_every_type_and_guards_detect_a_write():
    for dt in R.DT3:
        c = R.canary(4, dt)
        assert bool(torch.isnan(c).all())
        whole, view = R.guarded(torch.zeros(5, dtype=dt), off=3)
        assert R.guards_intact(whole, 5, 3) and view.data_ptr() == whole[R.GUARD + 3:].data_ptr()
        for i in (0, R.GUARD + 2, R.GUARD + 3 + 5, whole.numel() - 1):
            w = whole.clone()
            w[i] = 0.0
            assert not R.guards_intact(w, 5, 3)
        w = whole.clone()
        R.ibits(w)[1] ^= 1                                     # another NaN payload in a guard word
        assert not R.guards_intact(w, 5, 3)


def test_mismatches_compares_bits_nan_positions_and_canaries():
    exp = torch.tensor([1.0, 0.0, float("nan"), 2.0])
    exp = torch.cat([exp, R.canary(1, F32)])
    assert not R.mismatches(exp.clone(), exp).any()
    got = exp.clone()
    got[2] = R.from_bits32([0x7f800001])[0]                    # another NaN where a NaN is expected
    assert not R.mismatches(got, exp).any()
    for i, v in ((1, -0.0), (0, 1.0000001), (2, 1.0), (3, float("nan")), (4, 0.0), (4, float("nan"))):
        got = exp.clone()
        got[i] = v
        assert R.mismatches(got, exp).nonzero().view(-1).tolist() == [i], (i, v)
    got = exp.clone()
    got[2] = R.canary(1, F32)[0]                               # the canary where a written NaN was expected: not written
    assert R.mismatches(got, exp).tolist() == [False, False, True, False, False]


def test_half_ulp():
    v = torch.tensor([1.0, 1.99, 2.0, 0.0, 2.0 ** -14, 2.0 ** -20, 65504.0, 3.0e-40], dtype=torch.float64)
    assert R.half_ulp(v, BF16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -134, 2.0 ** -22, 2.0 ** -28, 2.0 ** 7, 2.0 ** -134]
    assert R.half_ulp(v, F16).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** 4, 2.0 ** -25]
    assert not R.half_ulp(v, F32).any()
    for dt in (BF16, F16):                                     # rounding any float64 to the type stays inside half an ulp
        x = torch.cat([R.signed_unit((4096,), 1).double() * 3.0, R.signed_unit((4096,), 2).double() * 2.0 ** -16])
        assert bool(((x.to(dt).double() - x).abs() <= R.half_ulp(x, dt)).all())


def test_edge_values_are_what_their_comments_say():
    e = R.edge_values()
    assert e.numel() == len(set(R.EDGE_BITS)) == len(R.EDGE_BITS)
    b, h = e.to(BF16), e.to(F16)
    i = R.EDGE_BITS.index
    bb, hb = R.ibits(b).tolist(), R.ibits(h).tolist()
    assert (bb[i(0x3f808000)], bb[i(0x3f818000)], bb[i(0x3f807fff)], bb[i(0x3f808001)]) == (0x3f80, 0x3f82, 0x3f80, 0x3f81)
    assert (hb[i(0x3f801000)], hb[i(0x3f803000)], hb[i(0x3f800fff)], hb[i(0x3f801001)]) == (0x3c00, 0x3c02, 0x3c00, 0x3c01)
    assert (bb[i(0x7f7f7fff)], bb[i(0x7f7f8000)]) == (0x7f7f, 0x7f80) and (hb[i(0x477fe000)], hb[i(0x477fefff)], hb[i(0x477ff000)]) == (0x7bff, 0x7bff, 0x7c00)
    assert (bb[i(0x80000000)] & 0xffff, hb[i(0x80000000)] & 0xffff) == (0x8000, 0x8000)
    assert (bb[i(0x007fffff)], bb[i(0x00008000)], bb[i(0x00018000)], bb[i(0x00000001)]) == (0x0080, 0x0000, 0x0002, 0x0000)
    assert (hb[i(0x33800000)], hb[i(0x33000000)], hb[i(0x33000001)], hb[i(0x32ffffff)], hb[i(0x33c00000)]) == (1, 0, 1, 0, 2)
    assert (hb[i(0x387fc000)], hb[i(0x387fe000)], hb[i(0x38800000)]) == (0x03ff, 0x0400, 0x0400)
    for k in (0x7fc00000, 0x7f800001, 0xffc00001, 0x7f80ffff, 0x7fffffff):
        assert math.isnan(float(b[i(k)])) and math.isnan(float(h[i(k)]))
    assert math.isinf(float(b[i(0x7f800000)])) and math.isinf(float(h[i(0xff800000)]))


def test_inputs_have_distinct_neighbours():
    x = R.pattern32(40000)
    assert R.ibits(x).unique().numel() == 40000 and bool(torch.isfinite(x).all())
    for step in (1, 3, 7, 8, 64, 100, 257):
        assert bool((R.ibits(x)[step:] != R.ibits(x)[:-step]).all())
    assert bool(((x.abs() >= 2.0 ** -10) & (x.abs() < 2.0 ** 10)).all()) and 0.3 < float((x < 0).float().mean()) < 0.7
    for dt in (BF16, F16):
        y = R.pattern16(60000, dt)
        assert R.ibits(y).unique().numel() == 60000 and bool(torch.isfinite(y.float()).all())
    for dt in R.DT3:
        s = R.signed_unit((5000,), 3, dt).float()
        assert bool(((s.abs() >= 0.5) & (s.abs() < 2.0)).all()) and 0.4 < float((s < 0).float().mean()) < 0.6
        for n in R.TM_N:
            y = R.balanced_tokens(2, n, 5, 7, dt).double()
            assert bool(((y.abs() >= 0.5) & (y.abs() < 2.0)).all())
            if n > 1:
                assert torch.equal(y.mean(1), torch.tensor([[2.0 ** -8] * 5, [-2.0 ** -8] * 5], dtype=torch.float64))


# ---- contracts against a second statement ------------------------------------------------------------------------------------------------------------
def test_im2col_patch_contract_is_unfold_at_non_square_geometry_with_a_map():
    for Cin, H, W, P in R.PATCH_GEOM:
        assert H != W
        img = R.pattern32(3 * Cin * H * W, H).view(3, Cin, H, W)
        Kc = Cin * P * P
        for smap in (None, torch.tensor(R.PATCH_MAP), torch.tensor([1, 2, 0])):
            for dt in R.DT3:
                for ldk in R.patch_ldks(Kc):
                    rows = 3 * (H // P) * (W // P)
                    got = R.im2col_patch_contract(R.canary(rows * ldk, dt).view(rows, ldk), img, smap, P, ldk)
                    src = img if smap is None else img.index_select(0, smap)
                    u = F.unfold(src, kernel_size=P, stride=P).transpose(1, 2).reshape(rows, Kc)
                    assert torch.equal(got[:, :Kc], u.to(dt)) and not R.ibits(got[:, Kc:]).any()
                    assert torch.equal(got, E.im2col_patch(img, P, ldk, dt, sample_map=smap))


def test_sr_contracts_are_unfold_fold_and_avg_pool_and_adjoint():
    B = 2
    for g in R.SR_G:
        go = g // 2
        for T_ in R.SR_T:
            for C in (8, 13):
                y = torch.zeros(B, T_ + g * g, C, dtype=BF16)
                y[:, T_:] = R.pattern16(B * g * g * C, BF16, g).view(B, g * g, C)
                col = R.sr_im2col_contract(R.canary(B * go * go * 9 * C, BF16), y, B, g, C, T_).view(B * go * go, 9 * C)
                assert torch.equal(col, E.sr_im2col(y, B, g, C, T_))
                d = R.signed_unit((B * go * go, 9 * C), g + C).double()
                ref, bound = R.sr_col2im_ref(d, B, g, C)
                u = d.view(B, go * go, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, go * go)
                dy = F.fold(u, output_size=(g, g), kernel_size=3, stride=2, padding=1).flatten(2).transpose(1, 2)
                assert float((dy - ref).abs().max()) < 1e-12 and bool((bound <= R.gamma(3) * 8.0).all())
                dy32 = torch.zeros(B, T_ + g * g, C)
                E.sr_col2im(d.float(), dy32, B, g, C, T_)
                assert R.ratio(dy32[:, T_:], ref, bound) <= 1.0 and not dy32[:, :T_].any()
                # <sr_im2col(y), d> == <y, sr_col2im(d)>
                lhs = float((col.double() * d).sum())
                rhs = float((y[:, T_:].double() * ref).sum())
                assert abs(lhs - rhs) <= 1e-12 * float((col.double() * d).abs().sum())
        for Cin, Cout in ((5, 5), (5, 9)):
            for T_ in R.SR_T:
                x = R.signed_unit((B, T_ + g * g, Cin), g + Cin)
                ref, _ = R.sr_resid_ref(x, B, g, Cin, T_)
                img = x[:, T_:].double().transpose(1, 2).reshape(B, Cin, g, g)
                assert float((F.avg_pool2d(img, 2, 2).flatten(2).transpose(1, 2) - ref).abs().max()) < 1e-15
                out = R.sr_resid_exact(R.canary(B * (T_ + go * go) * Cout, F32).view(B, T_ + go * go, Cout), x, B, g, Cin, Cout, T_)
                emu = E.sr_resid(x, B, g, Cin, Cout, T_)
                assert torch.equal(out[:, :T_], emu[:, :T_]) and torch.equal(out[:, T_:, Cin:], emu[:, T_:, Cin:])
                dout = R.signed_unit((B, T_ + go * go, Cout), g + Cout)
                dx = R.sr_resid_bwd_contract(torch.zeros(B, T_ + g * g, Cin), dout, B, g, Cin, Cout, 0, T_)
                assert torch.equal(dx, E.sr_resid_bwd(dout, B, g, Cin, Cout, T_))
                acc0 = R.signed_unit((B, T_ + g * g, Cin), 77)
                assert torch.equal(R.sr_resid_bwd_contract(acc0, dout, B, g, Cin, Cout, 1, T_), acc0 + dx)
                # <sr_resid(x), dout> == <x, sr_resid_bwd(dout)> over the columns that carry the residual
                full = torch.cat([x[:, :T_].double(), ref], 1)
                lhs = float((full * dout[:, :, :Cin].double()).sum())
                rhs = float((x.double() * dx.double()).sum())
                assert abs(lhs - rhs) <= 1e-12 * float((x.double() * dx.double()).abs().sum())


def test_exact_contracts_agree_with_the_emulated_kernels():
    descs, ns, nd = R.ct_layout()
    src = R.pattern32(ns)
    exp = R.cast_transpose_contract(R.canary(nd, BF16), src, descs)
    assert not R.mismatches(E.cast_transpose_batch(src, R.canary(nd, BF16), (None, 0, descs)), exp).any()
    assert int((R.ibits(exp) == R.CANARY16).sum()) == nd - sum(r * c for _, _, r, c, _ in descs)      # pads and gaps untouched
    for n in R.CAST_N:
        x = R.with_edges(R.pattern32(n), [0])
        for dt in (BF16, F16):
            assert not R.mismatches(R.cast_contract(R.canary(n, dt), x, n), E.cast_bf16(x, torch.empty(n, dtype=dt))).any()
    for tag, base, ranges in R.zero_launches():
        n = base + max(lo + c for lo, c in ranges) + 8
        w = R.zero_words(n)
        exp = R.zero_ranges_contract(w, base, ranges)
        assert torch.equal(exp[base:], E.zero_ranges(w.clone()[base:], [(lo, lo + c) for lo, c in ranges]))
        inside = torch.zeros(n, dtype=torch.bool)
        for lo, c in ranges:
            inside[base + lo:base + lo + c] = True
        assert bool((exp[inside] == 0).all()) and torch.equal(exp[~inside], w[~inside]) and bool((w != 0).all())
        assert torch.equal(R.zero_ranges_contract(w, base, ranges, gate=0), w)
    for A, B, C, sp, dp in R.RELAYOUT_CASES:
        for sd, dd in R.RELAYOUT_PAIRS:
            s = R.pattern(A * (B * C + sp), sd)
            exp = R.relayout_contract(R.canary(A * (B * C + dp), dd), s, A, B, C, B * C + sp, B * C + dp)
            emu = E.relayout(s, R.canary(A * (B * C + dp), dd), A, B, C, dst_ld=B * C + dp, src_ld=B * C + sp)
            assert not R.mismatches(emu, exp).any()
        s, d = R.pattern32(A * (B * C + sp), 1), R.pattern32(A * (B * C + dp), 2)
        exp = R.relayout_add_contract(d, s, A, B, C, B * C + sp, B * C + dp)
        assert torch.equal(exp, d + E.relayout(s, torch.zeros_like(d), A, B, C, dst_ld=B * C + dp, src_ld=B * C + sp))
    for Co, Ci in R.CONV_W_FLIP:
        w = R.pattern32(Co * Ci * 9).view(Co, Ci, 3, 3)
        for dt in (F32, BF16):
            assert torch.equal(R.conv_w_flip_contract(R.canary(Ci * 9 * Co, dt).view(Ci, 9 * Co), w), E.conv_w_flip(w, dt))
    for M in R.SMC_M:
        for C in R.SMC_C:
            x = R.pattern32(M * C, M).view(M, C)
            S = (M + 1) // 2
            scale, keep = torch.tensor([1.0, 0.5, -0.5, 1.7, 3.0e-5])[torch.arange(S) % 5], R.smc_keep(C, S)
            for dt in R.DT3:
                for sc, kp in ((scale, keep), (None, keep), (scale, None)):
                    exp = R.scale_mask_cast_contract(R.canary(M * C, dt).view(M, C), x, sc, kp, 2)
                    assert bool((exp == E.scale_mask_cast(x, sc, kp, 2, dt)).all())                # values: the emulation leaves -0
    for T_ in (1, 2):
        C, B = 9, 3
        tok, pos, keep = R.pattern32(T_ * C).view(T_, C), R.pattern32((T_ + 2) * C, 1).view(T_ + 2, C), torch.tensor([0, 4, C], dtype=torch.int32)
        before = R.canary(B * (T_ + 2) * C, F32).view(B, T_ + 2, C)
        for kp in (None, keep):
            exp = R.embed_cls_contract(before, tok, pos, kp, T_)
            emu = E.embed_cls(tok, pos, before.clone(), kp, T_)
            assert bool((emu[:, :T_] == exp[:, :T_]).all()) and not R.mismatches(emu[:, T_:], exp[:, T_:]).any()   # (the emulation leaves -0)
            assert not R.mismatches(exp[:, T_:], before[:, T_:]).any() and not bool((R.ibits(exp[:, :T_]) == R.CANARY32).any())
    x = R.pattern32(5 * 12).view(5, 12).clone()
    kp = torch.tensor([0, 12, 5], dtype=torch.int32)
    assert bool((R.mask_rows_contract(x, kp, 2) == E.mask_rows(x.clone(), kp, 2)).all())


# ---- fp32 emulations of the kernels' sums, and the faults ----------------------------------------------------------------------------------------
def fsum(terms, order):
    """sum of fp32 tensors in the kernel's sequential order, reversed, or pairwise"""
    t = list(terms)
    if not t:
        return None
    if order == "rev":
        t = t[::-1]
    if order == "pair":
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return t[0]
    s = t[0]
    for v in t[1:]:
        s = s + v
    return s


ORDERS = ("seq", "rev", "pair")


def emu_colsum(x, out0, M, N, rm, order, fault=None):
    rows = R.map_rows(M, (rm[0], rm[1], 0) if fault == "wrong_row" else rm)               # the map's offset lost: rows the map skips
    xs = x[rows][:, :N].float()
    parts = []
    for m0 in range(0, M, 128):
        t = list(xs[m0:min(M, m0 + 128)])
        if fault == "drop" and m0 <= M // 2 < m0 + 128:
            del t[M // 2 - m0]
        if fault == "skip_last" and m0 == 0:
            del t[-1]
        p = fsum(t, order)
        parts.append(torch.zeros(N) if p is None else p)
    if fault == "twice":
        parts.insert(1, parts[0])
    return fsum([out0] + parts, order)


def emu_batchsum(x, out0, B, order, fault=None):
    bper, chunks, _ = R.batchsum_path(B, 1)
    parts = []
    for k in range(chunks):
        b0, b1 = k * bper, min(B, (k + 1) * bper)
        if fault == "wrong_row" and k == chunks - 1:
            b0, b1 = b0 + 1, b1 + 1                                                      # one sample too far: the NaN row behind the batch
        t = list(x[b0:b1])
        if fault == "drop" and b0 <= B // 2 < b1:
            del t[B // 2 - b0]
        if fault == "skip_last" and k == 0:
            del t[-1]
        if order == "seq":                                                               # the kernel: trees of eight, then one by one
            s, i = torch.zeros_like(out0), 0
            while i + 8 <= len(t):
                s = s + (((t[i] + t[i + 1]) + (t[i + 2] + t[i + 3])) + ((t[i + 4] + t[i + 5]) + (t[i + 6] + t[i + 7])))
                i += 8
            for v in t[i:]:
                s = s + v
        else:
            s = fsum(t, order)
            s = torch.zeros_like(out0) if s is None else s
        parts.append(s)
    if fault == "twice":
        parts.insert(1, parts[0])
    return fsum([out0] + parts, order)


def emu_token_mean(y, first, dt, order, fault=None):
    B, N, C = y.shape
    n = N - first
    t = list(y[:, first - 1 if fault == "first" else first:].float().unbind(1))
    if fault == "drop":
        del t[n // 2]
    s = fsum(t, order)
    s = torch.zeros(B, C) if s is None else s
    if fault == "wrong_row":
        s = s.roll(1, 0)
    return (s * (torch.tensor(1.0) / float(n))).to(dt)


def emu_token_mean_bwd(dmean, n, dt, fault=None):
    d = dmean.float().roll(1, 0) if fault == "wrong_row" else dmean.float()
    return (d * (torch.tensor(1.0) / float(n))).to(dt)


def emu_sr_col2im(dcol, B, g, C, dt, order, fault=None):
    go = g // 2
    d = dcol.float().view(B, go, go, 9, C)
    tap, oh, ow, ih, iw = R._sr_taps(g)
    parts = []
    for k in range(9):
        sel = tap == k
        if fault == "drop" and k == 4:
            continue
        p = torch.zeros(B, g * g, C)
        src_tap = (k % 3) * 3 + k // 3 if fault == "transposed" else k
        p.index_add_(1, (ih * g + iw)[sel], d[:, oh[sel], ow[sel], src_tap, :])
        parts.append(p)
        if fault == "twice" and k == 4:
            parts.append(p)
    return fsum(parts, order).to(dt)


def emu_sr_resid(x, B, g, Cin, T_, order, fault=None):
    go = g // 2
    p = x.float().view(B, T_ + g * g, Cin)[:, T_:].view(B, go, 2, go, 2, Cin)
    if fault == "wrong_row":
        p = p.roll(1, 0)
    t = [p[:, :, 0, :, 0], p[:, :, 0, :, 1], p[:, :, 1, :, 0], p[:, :, 1, :, 1]]
    if fault == "drop":
        del t[3]
    return (0.25 * fsum(t, order)).reshape(B, go * go, Cin)


def bounded_cases():
    """(kernel, tag, dtype, ref, fp32 bound, emulate(order, fault), faults) for every bounded kernel and case of the device suite"""
    for dt in (F32, BF16):
        for M in R.COLSUM_M:
            for N in R.COLSUM_N:
                for rm in (None, R.COLSUM_MAP):
                    x, out0, _ = R.colsum_inputs(M, N, rm, dt)
                    ref, b32 = R.colsum_ref(x, out0, M, N, rm)
                    yield ("colsum", "%s M%d N%d %s" % (R.name(dt), M, N, rm), F32, ref, b32,
                           lambda o, f, a=(x, out0, M, N, rm): emu_colsum(*a, o, f), ["drop", "twice", "skip_last"] + (["wrong_row"] if rm else []))
    for B in R.BATCHSUM_B:
        for inner in R.BATCHSUM_INNER:
            x, out0 = R.batchsum_inputs(B, inner)
            ref, b32 = R.batchsum_ref(x[:B], out0)
            yield ("batchsum", "B%d inner%d" % (B, inner), F32, ref, b32, lambda o, f, a=(x, out0, B): emu_batchsum(*a, o, f),
                   ["drop", "twice", "skip_last", "wrong_row"])
    for dt in R.DT3:
        for n in R.TM_N:
            for first in R.TM_FIRST:
                for C in R.TM_C:
                    y = R.token_inputs(first, n, C, dt)
                    ref, b32 = R.token_mean_ref(y, first)
                    yield ("token_mean", "%s first%d n%d C%d" % (R.name(dt), first, n, C), dt, ref, b32,
                           lambda o, f, a=(y, first, dt): emu_token_mean(*a, o, f), ["drop", "wrong_row"] + (["first"] if first else []))
                    if dt != F16 and first == 0:
                        dm = R.split_unit(2, C, n + C + first, dt)
                        ref, b32 = R.token_mean_bwd_ref(dm, n)
                        yield ("token_mean_bwd", "%s n%d C%d" % (R.name(dt), n, C), dt, ref, b32,
                               lambda o, f, a=(dm, n, dt): emu_token_mean_bwd(*a, f), ["wrong_row"])
    for dt in (F32, BF16):
        for g in R.SR_G:
            for C in R.SR_C:
                dcol = R.signed_unit((2 * (g // 2) ** 2, 9 * C), g * 100 + C + 1, dt)
                ref, b32 = R.sr_col2im_ref(dcol, 2, g, C)
                yield ("sr_col2im", "%s g%d C%d" % (R.name(dt), g, C), dt, ref, b32, lambda o, f, a=(dcol, 2, g, C, dt): emu_sr_col2im(*a, o, f),
                       ["drop", "twice"] + (["transposed"] if g > 2 else []))
    for Cin, _ in R.SR_RESID:
        for T_ in R.SR_T:
            for g in (2, 6):
                x = R.signed_unit((2, T_ + g * g, Cin), g + T_ + Cin)
                ref, b32 = R.sr_resid_ref(x, 2, g, Cin, T_)
                yield ("sr_resid", "g%d T%d Cin%d" % (g, T_, Cin), F32, ref, b32, lambda o, f, a=(x, 2, g, Cin, T_): emu_sr_resid(*a, o, f),
                       ["drop", "wrong_row"])


def test_bounds_hold_in_three_orders_and_every_fault_leaves_them_by_100():
    worst, least, count = {}, {}, {}
    for kernel, tag, dt, ref, b32, emu, faults in bounded_cases():
        bound = R.out_bound(ref, b32, dt)
        assert bool((bound >= 0).all()) and faults
        for order in ORDERS:
            r = R.ratio(emu(order, None), ref, bound)
            worst[kernel] = max(worst.get(kernel, 0.0), r)
            assert r <= 1.0, (kernel, tag, order, r)
        for fault in faults:
            r = R.ratio(emu("seq", fault), ref, bound)
            if r < least.get(kernel, (math.inf,))[0]:
                least[kernel] = (r, tag, fault)
            assert r >= MIN_FAULT_RATIO, (kernel, tag, fault, r)
        count[kernel] = count.get(kernel, 0) + 1
    for k in sorted(worst):
        print("GLUE HOST %-16s %4d cases: worst emulation/bound %.3f, least fault/bound %.1f (%s, %s)" % ((k, count[k], worst[k]) + least[k]))
    assert set(count) == {"colsum", "batchsum", "token_mean", "token_mean_bwd", "sr_col2im", "sr_resid"}
    assert min(v[0] for v in least.values()) >= MIN_FAULT_RATIO


# ---- faults on exact contracts -------------------------------------------------------------------------------------------------------------------
def test_faults_on_exact_outputs_fail_the_integer_comparison():
    e = R.edge_values()
    for dt in (BF16, F16):
        exp = R.cast_contract(R.canary(e.numel(), dt), e, e.numel())
        # ties rounded away from zero
        half = 0x8000 if dt == BF16 else 0x1000
        away = R.from_bits32([((b & 0x7fffffff) + half) & ~(2 * half - 1) | (b & 0x80000000) if (b & 0x7f800000) != 0x7f800000 else b
                              for b in R.EDGE_BITS]).to(dt)
        bad = R.mismatches(away, exp)
        tie = R.EDGE_BITS.index(0x3f808000 if dt == BF16 else 0x3f801000)
        assert bool(bad[tie]) and not bool(bad[R.EDGE_BITS.index(0x3f818000 if dt == BF16 else 0x3f803000)])
        # fp32 denormals flushed before the cast
        flushed = torch.where(e.abs() < 2.0 ** -126, torch.zeros_like(e) * e, e).to(dt)
        if dt == BF16:
            assert bool(R.mismatches(flushed, exp)[R.EDGE_BITS.index(0x007fffff)])
        # a NaN turned into inf, the sign of zero lost
        g = exp.clone()
        g[R.EDGE_BITS.index(0x7f800001)] = float("inf")
        g[R.EDGE_BITS.index(0x80000000)] = 0.0
        assert int(R.mismatches(g, exp).sum()) == 2
    # a masked column that holds -0 (x * 0 for a negative x)
    x = -R.pattern32(8).abs().view(2, 4)
    keep = torch.tensor([2], dtype=torch.int32)
    exp = R.scale_mask_cast_contract(R.canary(8, BF16).view(2, 4), x, None, keep, 2)
    neg0 = (x * (torch.arange(4) < 2)).to(BF16)
    assert bool((neg0 == exp).all()) and R.mismatches(neg0, exp).tolist() == [[False, False, True, True]] * 2
    # the patch matrix one column off, its pad written, H and W exchanged
    Cin, H, W, P = R.PATCH_GEOM[2]
    img = R.pattern32(3 * Cin * H * W).view(3, Cin, H, W)
    ldk = Cin * P * P + 3
    rows = 3 * (H // P) * (W // P)
    exp = R.im2col_patch_contract(R.canary(rows * ldk, F32).view(rows, ldk), img, None, P, ldk)
    assert int(R.mismatches(exp.roll(1, 1), exp).sum()) >= rows * Cin * P * P
    swapped = R.im2col_patch_contract(R.canary(rows * ldk, F32).view(rows, ldk), img.reshape(3, Cin, W, H), None, P, ldk)
    assert int(R.mismatches(swapped, exp).sum()) > rows * Cin * P * P // 2
    g = R.im2col_patch_contract(R.canary(rows * (ldk + 2), F32).view(rows, ldk + 2), img, None, P, ldk + 2)[:, :ldk + 0]
    assert not R.mismatches(g.contiguous(), exp).any()
    # sr_im2col with kh and kw exchanged, and with a token row read as the first patch row
    B, g_, C, T_ = 2, 4, 8, 1
    y = R.canary(B * (T_ + g_ * g_) * C, BF16).view(B, T_ + g_ * g_, C)
    y[:, T_:] = R.pattern16(B * g_ * g_ * C, BF16).view(B, g_ * g_, C)
    n = B * 4 * 9 * C
    exp = R.sr_im2col_contract(R.canary(n, BF16), y, B, g_, C, T_).view(B, 2, 2, 9, C)
    tr = exp.view(B, 2, 2, 3, 3, C).transpose(3, 4).reshape(B, 2, 2, 9, C)
    assert int(R.mismatches(tr.contiguous(), exp).sum()) > n // 3
    y0 = torch.cat([y[:, :1], y], 1)[:, :T_ + g_ * g_]                                   # every row one too early
    off = R.sr_im2col_contract(R.canary(n, BF16), y0.contiguous(), B, g_, C, T_).view(B, 2, 2, 9, C)
    assert int(R.mismatches(off, exp).sum()) > n // 3 and bool(torch.isnan(off.float()).any())
    # relayout with b and c exchanged; a pad column written
    A, B_, C_ = 3, 5, 7
    s = R.pattern32(A * 40)
    exp = R.relayout_contract(R.canary(A * 38, BF16), s, A, B_, C_, 40, 38)
    assert int(R.mismatches(R.relayout_contract(R.canary(A * 38, BF16), s, A, C_, B_, 40, 38), exp).sum()) > A * 20
    g = exp.clone()
    g[36] = 0.0
    assert R.mismatches(g, exp).nonzero().view(-1).tolist() == [36]
    # zero_ranges one word long or one word short
    w = R.zero_words(64)
    exp = R.zero_ranges_contract(w, 1, [(5, 9)])
    assert int(R.mismatches(R.zero_ranges_contract(w, 1, [(5, 10)]), exp).sum()) == 1
    assert int(R.mismatches(R.zero_ranges_contract(w, 1, [(6, 8)]), exp).sum()) == 1
