"""The conv patch-embedding stem -- conv3x3.hip (vr_conv3x3 and its residual / bias + ReLU / patch-order forms, vr_conv1_direct,
vr_conv3x3_wgrad), the BatchNorm and layout kernels of stem.hip, vr_conv_w_flip and the ReLU epilogue of vr_gemm -- against the float64
contracts of tests/stem_ref64.py.  Every assertion is `worst error / derived bound <= 1` or bit-for-bit equality; the cases are the lists
of stem_ref64, the ones tests/test_stem_ref_host.py runs through an fp32 emulation: H and W around the 16 x 16 tile (and the 8 x 32 tile of
conv1_direct), every Cin (padded contraction slots, LDS stride padded or not), Cout either side of the second n-tile, more weight-gradient
tiles than persistent workgroups, BatchNorm row counts around rows_par, the four-row unroll and a second workgroup, exact integer and one-
hot probes, batch-isolation inputs and planted non-finite values.  Output buffers belong to the test and start as NaN: an element nobody
writes fails.

Out of scope: the 2048-workgroup cap of vr_bn_stats / vr_bn_bwd needs R > 2048 * 64 * rows_par rows (about 1 GB of input at C = 256): too
slow for this suite."""
import types

import pytest
import torch

import stem_ref64 as S
import vitres.kernels as K
from vitres import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
INF = float("inf")
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def cu(t):
    return None if t is None else t.to(DEV)


def nan_out(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def call(name, *args):
    rc = getattr(_lib.lib(), name)(*args, K._stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)


class Gpu:
    """the entry points behind stem_ref64's `impl` interface: CPU tensors in, NaN-filled device outputs, CPU tensors out.  Every device
    operand stays in a local until the call has synchronised: a temporary freed right after K._p() would hand its block to the next one"""

    def conv3x3(self, a, w, B, H, W, Cin, Cout, out_dtype):
        out, ad, wd = nan_out((B * H * W, Cout), out_dtype), cu(a), cu(w)
        call("vr_conv3x3", K._p(ad), K._p(wd), K._p(out), B, H, W, Cin, Cout, K._dtcode(out_dtype))
        return out.cpu()

    def conv3x3_res(self, a, w, res, B, H, W, Cin, Cout, out_dtype):
        out, r, ad, wd = nan_out((B * H * W, Cout), out_dtype), cu(res), cu(a), cu(w)
        call("vr_conv3x3_res", K._p(ad), K._p(wd), K._p(r), K._p(out), B, H, W, Cin, Cout, K._dtcode(out_dtype))
        return out.cpu()

    def conv3x3_res_patch(self, a, w, res_col, B, H, W, Cin, Cout, P, out_dtype):
        out, r, ad, wd = nan_out((B * H * W, Cout), out_dtype), cu(res_col), cu(a), cu(w)
        call("vr_conv3x3_res_patch", K._p(ad), K._p(wd), K._p(r), K._p(out), B, H, W, Cin, Cout, K._dtcode(out_dtype), P)
        return out.cpu()

    def conv3x3_bias_relu(self, a, w, bias, res, B, H, W, Cin, Cout, out_dtype):
        out, r, bs, ad, wd = nan_out((B * H * W, Cout), out_dtype), cu(res), cu(bias), cu(a), cu(w)
        call("vr_conv3x3_bias_relu", K._p(ad), K._p(wd), K._p(bs), K._p(r), K._p(out), B, H, W, Cin, Cout, K._dtcode(out_dtype))
        return out.cpu()

    def conv3x3_bias_relu_patch(self, a, w, bias, res, B, H, W, Cin, Cout, P, out_dtype):
        out, r, bs, ad, wd = nan_out((B * (H // P) * (W // P), P * P * Cout), out_dtype), cu(res), cu(bias), cu(a), cu(w)
        call("vr_conv3x3_bias_relu_patch", K._p(ad), K._p(wd), K._p(bs), K._p(r), K._p(out), B, H, W, Cin, Cout, P, K._dtcode(out_dtype))
        return out.cpu()

    def conv_w_flip(self, w4, out_dtype):
        Co, Ci = w4.shape[0], w4.shape[1]
        out, wd = nan_out((Ci, 9 * Co), out_dtype), cu(w4.contiguous())
        call("vr_conv_w_flip", K._p(wd), K._p(out), Co, Ci, K._dtcode(out_dtype))
        return out.cpu()

    def conv1_direct(self, img, w, bias, relu, out_dtype):
        B, _, H, W = img.shape
        Cout = w.shape[0]
        out, bs, im, wd = nan_out((B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1), Cout), out_dtype), cu(bias), cu(img), cu(w)
        call("vr_conv1_direct", K._p(im), K._p(wd), K._p(bs), K._p(out), B, H, W, Cout, int(bool(relu)), K._dtcode(out_dtype))
        return out.cpu()

    def conv3x3_wgrad(self, a, dz, dw, B, H, W, Cin, Cout):
        d, ad, gd = cu(dw), cu(a), cu(dz)
        call("vr_conv3x3_wgrad", K._p(ad), K._p(gd), K._p(d), B, H, W, Cin, Cout)
        return d.cpu()

    def bn_stats(self, z, s, q):
        zd, sd, qd = cu(z), cu(s), cu(q)
        call("vr_bn_stats", K._p(zd), K._p(sd), K._p(qd), z.shape[0], z.shape[1], K._dt(zd))
        return sd.cpu(), qd.cpu()

    def bn_finalize(self, s, q, n, w, b, eps, momentum, rmean, rvar, nbt, update):
        C = s.shape[0]
        bn = types.SimpleNamespace(weight=cu(w), bias=cu(b), eps=eps, running_mean=cu(rmean), running_var=cu(rvar), num_batches_tracked=cu(nbt))
        out = K.bn_finalize(torch.stack([s, q]).to(DEV), n, bn, momentum, update)
        torch.cuda.synchronize()
        return tuple(t.cpu() for t in out) + (bn.running_mean.cpu(), bn.running_var.cpu(), bn.num_batches_tracked.cpu())

    def bn_relu(self, z, scale, shift, res, out_dtype):
        R, C = z.shape
        out, zd, r, sc, sh = nan_out((R, C), out_dtype), cu(z), cu(res), cu(scale), cu(shift)
        call("vr_bn_relu", K._p(zd), K._p(sc), K._p(sh), K._p(r), K._p(out), R, C, K._dtcode(out_dtype), K._dt(zd))
        return out.cpu()

    def bn_relu_patch(self, z, scale, shift, res, B, H, W, P, out_dtype):
        C = z.shape[1]
        out, zd, r, sc, sh = nan_out((B * (H // P) * (W // P), P * P * C), out_dtype), cu(z), cu(res), cu(scale), cu(shift)
        call("vr_bn_relu_patch", K._p(zd), K._p(sc), K._p(sh), K._p(r), K._p(out), B, H, W, P, C, K._dtcode(out_dtype), K._dt(zd))
        return out.cpu()

    def bn_bwd(self, da, z, scale, shift, mean, rstd, sg, sgz, training, patch=None):
        R, C = z.shape
        t = [cu(x) for x in (da, z, scale, shift, mean, rstd, sg, sgz)]
        dz = nan_out((R, C), da.dtype)
        if patch is None:
            call("vr_bn_bwd", *[K._p(x) for x in t], K._p(dz), R, C, int(training), K._dt(t[0]), K._dt(t[1]))
        else:
            B, H, W, P = patch
            call("vr_bn_bwd_patch", *[K._p(x) for x in t], K._p(dz), B, H, W, P, C, int(training), K._dt(t[0]), K._dt(t[1]))
        return dz.cpu(), t[6].cpu(), t[7].cpu()

    def bn_bwd_patch(self, dcol, z, scale, shift, mean, rstd, sg, sgz, training, B, H, W, P):
        return self.bn_bwd(dcol, z, scale, shift, mean, rstd, sg, sgz, training, patch=(B, H, W, P))

    def im2col3x3(self, a, B, H, W, C):
        col, ad = nan_out((B * H * W, 9 * C), a.dtype), cu(a)
        call("vr_im2col3x3", K._p(ad), K._p(col), B, H, W, C, 1, 0, 9 * C, K._dt(ad))
        return col.cpu()

    def im2col3x3_image(self, img, stride, ld, dtype):
        B, C, H, W = img.shape
        col, im = nan_out((B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), ld), dtype), cu(img)
        call("vr_im2col3x3", K._p(im), K._p(col), B, H, W, C, stride, 1, ld, K._dtcode(dtype))
        return col.cpu()

    def col2im3x3(self, dcol, B, H, W, C):
        d, dc = nan_out((B * H * W, C), dcol.dtype), cu(dcol)
        call("vr_col2im3x3", K._p(dc), K._p(d), B, H, W, C, K._dt(dc))
        return d.cpu()

    def patch_unfold(self, a, B, gh, gw, P, C):
        col, ad = nan_out((B * gh * gw, P * P * C), a.dtype), cu(a)
        call("vr_patch_unfold", K._p(ad), K._p(col), B, gh, gw, P, C, 0, K._dt(ad))
        return col.cpu()

    def patch_fold(self, col, B, gh, gw, P, C):
        a, cd = nan_out((B * gh * P * gw * P, C), col.dtype), cu(col)
        call("vr_patch_unfold", K._p(a), K._p(cd), B, gh, gw, P, C, 1, K._dt(cd))
        return a.cpu()


GPU = Gpu()


class Worst:
    def __init__(self, tag):
        self.tag, self.w = tag, {}

    def __call__(self, q, r, ctx=None):
        for k, v in (r.items() if isinstance(r, dict) else [("", r)]):
            name = q + ("." + k if k else "")
            self.w[name] = max(self.w.get(name, 0.0), v)
            assert v <= 1.0, (name, v, ctx)

    def show(self):
        print("STEM gpu %s: %s" % (self.tag, "  ".join("%s=%.3f" % kv for kv in sorted(self.w.items()))))


# ---- conv3x3 family ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", S.CONV_CIN)
def test_conv3x3_family(Cin):
    """every (H, W) x B x Cout in fp32 and bf16, fp16 operands, the residual / bias + ReLU / patch-order forms, batch isolation"""
    w = Worst("conv3x3 Cin%d" % Cin)
    for kw in S.conv_cases(Cin):
        w("conv3x3_" + kw.get("form", "plain"), S.run_conv3x3(GPU, **kw), kw)
    w.show()


@pytest.mark.parametrize("Cin", S.CONV_CIN)
def test_conv3x3_exact_probes(Cin):
    """integer operands: bit-for-bit the float64 result; one-hot inputs: the weights' taps at exactly the 9 neighbours"""
    for H, W in S.CONV_HW:
        for Cout in (4, 20, 32):
            assert S.run_conv3x3_int(GPU, 3, H, W, Cin, Cout) == 0.0, (H, W, Cout)
            assert S.run_conv3x3_onehot(GPU, 3, H, W, Cin, Cout) == 0.0, (H, W, Cout)


def test_conv3x3_data_gradient_is_the_transposed_convolution():
    w = Worst("dgrad")
    for kw in S.dgrad_cases():
        w("dgrad", S.run_dgrad(GPU, **kw), kw)
    w.show()


# ---- conv1_direct -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", S.CONV1_COUT)
def test_conv1_direct(Cout):
    w = Worst("conv1 Cout%d" % Cout)
    for kw in S.conv1_cases(Cout):
        w("conv1", S.run_conv1(GPU, **kw), kw)
    for H, W in S.CONV1_HW:
        assert S.run_conv1_int(GPU, 2, H, W, Cout) == 0.0 and S.run_conv1_onehot(GPU, 2, H, W, Cout) == 0.0, (H, W)
    w.show()


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", S.CONV_CIN)
def test_conv3x3_wgrad(C):
    """into a non-zero dw; the integer probe bit for bit"""
    w = Worst("wgrad C%d" % C)
    for kw in S.wgrad_cases(C):
        w("wgrad", S.run_wgrad(GPU, **kw), kw)
    w.show()


def test_conv3x3_wgrad_more_tiles_than_workgroups():
    """B = 257 at 17 x 17: 1028 tiles on 1024 persistent workgroups -- four workgroups take a second tile (the loop's second barrier)"""
    B, H, W = S.WGRAD_BIG
    assert B * ((H + 15) // 16) * ((W + 15) // 16) > 1024
    w = Worst("wgrad persistent")
    w("wgrad", S.run_wgrad(GPU, B, H, W, 32))
    w("wgrad_int", S.run_wgrad(GPU, B, H, W, 24, integer=True))
    w.show()


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", S.BN_C)
def test_bn_stats_and_finalize(C):
    """sums into non-zero accumulators; mean / rstd / scale / shift and the running statistics against BatchNorm2d's; update_running
    False leaves the three buffers' bits alone; offset channels up to |mean| / std = 30; a constant channel"""
    w = Worst("bn forward C%d" % C)
    for kw in S.bn_forward_cases(C):
        w("bn", S.run_bn_forward(GPU, **kw), kw)
    w.show()


@pytest.mark.parametrize("C", S.BN_C)
def test_bn_relu(C):
    w = Worst("bn_relu C%d" % C)
    for kw in S.bn_relu_cases(C):
        w("bn_relu", S.run_bn_relu(GPU, **kw), kw)
    w.show()


@pytest.mark.parametrize("C", S.BN_C)
def test_bn_bwd(C):
    """training and evaluation, sg / sgz accumulated into non-zero buffers, the undecided mask elements on either branch"""
    w = Worst("bn_bwd C%d" % C)
    for kw in S.bn_bwd_cases(C):
        w("bn_bwd", S.run_bn_bwd(GPU, **kw), kw)
    w.show()


def test_bn_patch_forms_and_the_strict_mask():
    w = Worst("bn patch")
    for kw, od in S.bn_patch_cases():
        w("bn_relu_patch", S.run_bn_relu(GPU, out_dtype=od, with_res=True, **kw), kw)
        for training in (True, False):
            w("bn_bwd_patch", S.run_bn_bwd(GPU, da_dtype=od, training=training, **kw), kw)
    w("zero_probe", S.run_bn_zero_probe(GPU))
    w("zero_probe_eval", S.run_bn_zero_probe(GPU, training=False))
    w.show()


# ---- layout kernels ---------------------------------------------------------------------------------------------------------------------
def test_layout_kernels_bit_for_bit():
    w = Worst("layout")
    for kw in S.layout_cases():
        w("layout", S.run_layouts(GPU, **kw), kw)
    for H, W, P in S.PATCH_SHAPES:
        for C in (8, 24, 32):
            for dt in (F32, BF):
                w("patch", S.run_unfold(GPU, 3, H, W, P, C, dt), (H, W, P, C, dt))
    for kw in S.image_cases():
        w("im2col_image", S.run_im2col_image(GPU, **kw), kw)
    w.show()


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------------------
# Ordinary data: a NaN (or a +inf that turns into NaN downstream) must come out as NaN in exactly the outputs whose float64 contract is NaN,
# and every other output stays inside its bound.
@pytest.mark.parametrize("patch", [False, True])
@pytest.mark.parametrize("zd,od", S.BN_DTYPES)
def test_bn_relu_propagates_non_finite_inputs(zd, od, patch):
    B, H, W, P, C = 2, 14, 14, 7, 24
    inp = S.bn_inputs(B * H * W, C, zd)
    scale, shift, _, _ = S.bn_handed(inp)
    z = inp["z"].clone()
    z[3, 5] = NAN
    z[200, 0] = NAN
    z[77, 9], scale[9] = INF, 0.0                    # inf * 0 = NaN
    shift[17] = NAN                                  # a whole channel
    res = inp["res"].to(od)
    ref, bd = S.bn_relu64(z, scale, shift, res, B, H, W, P if patch else 0)
    assert int(torch.isnan(ref).sum()) == 3 + B * H * W and not bool(torch.isinf(ref).any())
    got = GPU.bn_relu_patch(z, scale, shift, res, B, H, W, P, od) if patch else GPU.bn_relu(z, scale, shift, res, od)
    assert S.nonfinite_ratio(got, ref, S.out_bound(ref, bd, S.unit_roundoff(od))) <= 1.0


@pytest.mark.parametrize("form,P", [("bias_relu", 0), ("bias_relu_res", 0), ("bias_relu_patch", 7), ("bias_relu_patch_res", 2)])
@pytest.mark.parametrize("Cin,Cout,od,op", [(16, 12, F32, BF), (24, 24, BF, BF), (32, 20, F16, F16)])
def test_conv3x3_bias_relu_propagates_non_finite_inputs(Cin, Cout, od, op, form, P):
    B, H, W = (2, 28, 42) if P == 7 else (2, 16, 32) if P == 2 else (2, 17, 33)
    a, w, bias, res = S.conv_inputs(B, H, W, Cin, Cout, op)
    a[(1 * H + 9) * W + 16, 3] = NAN                 # a pixel on the tile seam of image 1
    w[1, 4 * Cin + 2] = NAN                          # the centre tap of output channel 1
    bias[Cout - 1] = NAN
    ref, bd = S.conv3x3_64(a, w, B, H, W, bias=bias, relu=True, res=res if form.endswith("res") else None, out_patch=P)
    n = int(torch.isnan(ref).sum())
    assert n == 2 * B * H * W + 9 * (Cout - 2) and not bool(torch.isinf(ref).any())
    r = S.check_conv3x3(GPU, a, w, bias, res, B, H, W, od, form, P, ratio=S.nonfinite_ratio)
    assert r <= 1.0, r


@pytest.mark.parametrize("od,op", [(F32, BF), (BF, BF), (F16, F16)])
@pytest.mark.parametrize("Cout", [4, 20])
def test_conv1_direct_relu_propagates_non_finite_inputs(Cout, od, op):
    img, w, bias = S.conv1_inputs(2, 33, 65, Cout, op)
    img[1, 2, 16, 63] = NAN                          # an odd pixel: a tap of 1 x 1 ... 2 x 2 outputs
    w[1, 13] = NAN
    bias[Cout - 1] = NAN
    ref, bd = S.conv1_64(img, w, op, bias, True)
    assert int(torch.isnan(ref).sum()) >= 2 * 2 * 17 * 33 and not bool(torch.isinf(ref).any())
    got = GPU.conv1_direct(img, w, bias, True, od)
    assert S.nonfinite_ratio(got, ref, S.out_bound(ref, bd, S.unit_roundoff(od))) <= 1.0


def gemm_relu64(a, w, bias):
    """relu(a w^T + bias) term by term -> (out, bound at u = 0): K products summed in fp32 (MFMA: K 2^-23, which also covers the fp32
    kernel's fmaf chain at K u32), the bias add"""
    A, Wt = S.f64(a), S.f64(w)
    pre, mag = torch.zeros(A.shape[0], Wt.shape[0], dtype=S.F64), torch.zeros(A.shape[0], Wt.shape[0], dtype=S.F64)
    for n in range(Wt.shape[0]):
        pre[:, n] = (A * Wt[n]).sum(-1)
        mag[:, n] = (A.abs() * Wt[n].abs()).sum(-1)
    pre = pre + S.f64(bias)
    return S.relu64(pre), A.shape[1] * S.MFMA * mag + S.U32 * pre.abs()


# The three shapes of test_gemm_relu_epilogue in bf16 all take vr_gemm_nt_launch (bf16, act = 3, a 16-bit result): the ReLU of
# gemm_nt_parts.h.  The two ReLUs of gemm.hip belong to the general kernel: epilogue_all (16-bit result; reached with sched bit 4, which
# skips the NT kernels) and epilogue_lds (fp32 operands and result on the 128 x 128 tile) -- one more launch each.
@pytest.mark.parametrize("M,N,Kd,dt,sched", [(1000, 24, 32, BF, 0), (300, 256, 192, BF, 0), (130, 72, 200, BF, 0), (130, 72, 200, BF, 4),
                                             (130, 72, 200, F32, 0), (300, 256, 192, F16, 0)])
def test_gemm_relu_epilogue_propagates_non_finite_inputs(M, N, Kd, dt, sched):
    g = torch.Generator().manual_seed(M + N)
    a, w = torch.randn(M, Kd, generator=g).to(dt), (torch.randn(N, Kd, generator=g) * Kd ** -0.5).to(dt)
    bias = torch.randn(N, generator=g)
    a[M // 2, 5] = NAN
    w[3, Kd - 1] = NAN
    bias[N - 1] = NAN
    ref, bd = gemm_relu64(a, w, bias)
    assert int(torch.isnan(ref).sum()) == N + 2 * M - 2
    out = nan_out((M, N), dt)
    K.gemm(cu(a), cu(w), out, M=M, N=N, K=Kd, lda=Kd, ldb=Kd, ldc=N, bias=cu(bias), act=3, sched=sched)
    torch.cuda.synchronize()
    assert S.nonfinite_ratio(out.cpu(), ref, S.out_bound(ref, bd, S.unit_roundoff(dt))) <= 1.0


@pytest.mark.parametrize("zd", [F32, BF])
@pytest.mark.parametrize("C", [24, 256])
def test_bn_statistics_propagate_non_finite_inputs(C, zd):
    """a channel holding a NaN: its mean, rstd, scale, shift and running statistics are NaN; a channel holding +inf: mean and running_mean
    +inf, the rest NaN (inf - inf); every other channel inside its bound"""
    R = S.bn_rows(C)[5]
    inp = S.bn_inputs(R, C, zd)
    z = inp["z"].clone()
    z[R // 3, 2] = NAN
    z[R - 1, 5] = INF
    s, q = GPU.bn_stats(z, torch.zeros(C), torch.zeros(C))
    scale, shift, mean, rstd, rm, rv, nbt = GPU.bn_finalize(s, q, R, inp["w"], inp["b"], S.BN_EPS, S.BN_MOMENTUM, inp["rmean"].clone(),
                                                            inp["rvar"].clone(), torch.tensor(0), True)
    f = S.bn_finalize64(z, inp["w"], inp["b"], rmean0=inp["rmean"], rvar0=inp["rvar"])
    bad = torch.zeros(C, dtype=torch.bool)
    bad[2] = bad[5] = True
    assert bool(f["valid"][~bad].all())
    got = dict(mean=mean, rstd=rstd, scale=scale, shift=shift, rmean=rm, rvar=rv)
    for k, v in got.items():
        assert bool(torch.isnan(f[k][2])) and (bool(torch.isnan(f[k][5])) or float(f[k][5]) == INF), k
        assert S.nonfinite_ratio(v, f[k], f["b" + k]) <= 1.0, k
    assert int(nbt) == 1


@pytest.mark.parametrize("Cin,Cout", [(16, 4), (24, 20), (32, 32)])
def test_conv3x3_zero_weight_slots_do_not_spread_an_infinity(Cin, Cout):
    """+inf in channel 0 of one pixel: the padded contraction slots (zero weights, they read tap 0 / chunk 0 of the lane's own window) and
    the zero rows of a partly filled n-tile see it inside the MFMA, but only the 9 outputs whose window holds the pixel may leave finite
    values behind -- every other output of the tile, its halo neighbours included, stays inside its bound"""
    B, H, W = 2, 17, 33
    for y, x in ((5, 5), (8, 16), (16, 15)):
        a, w, _, _ = S.conv_inputs(B, H, W, Cin, Cout)
        a[(1 * H + y) * W + x, 0] = INF
        ref, bd = S.conv3x3_64(a, w, B, H, W)
        hit = ~torch.isfinite(ref)
        assert 0 < int(hit.any(-1).sum()) <= 9
        got = S.f64(GPU.conv3x3(a, w, B, H, W, Cin, Cout, F32))
        assert not bool(torch.isfinite(got[hit]).any())
        z = torch.zeros_like(ref)
        assert S.worst_ratio(torch.where(hit, z, got), torch.where(hit, z, ref), torch.where(hit, z, S.out_bound(ref, bd, 0.0))) <= 1.0


def test_conv1_direct_zero_weight_slots_do_not_spread_an_infinity():
    img, w, _ = S.conv1_inputs(2, 33, 65, 20)
    img[1, 0, 9, 31] = INF
    ref, bd = S.conv1_64(img, w, BF)
    hit = ~torch.isfinite(ref)
    assert 0 < int(hit.any(-1).sum()) <= 4
    got = S.f64(GPU.conv1_direct(img, w, None, False, F32))
    assert not bool(torch.isfinite(got[hit]).any())
    z = torch.zeros_like(ref)
    assert S.worst_ratio(torch.where(hit, z, got), torch.where(hit, z, ref), torch.where(hit, z, S.out_bound(ref, bd, 0.0))) <= 1.0


def test_relu_returns_plus_zero_for_negative_inputs_and_minus_zero():
    """the bits of the zeros: +0 from negatives and from -0 (z = -0 with scale = 1, shift = -0 gives a pre-activation of -0)"""
    C = 8
    z = torch.tensor([[-0.0, -3.0, 2.0, -1e-30, 0.0, -0.0, 5.0, -7.0]])
    out = GPU.bn_relu(z, torch.ones(C), torch.full((C,), -0.0), None, F32)
    assert out.view(torch.int32).tolist() == torch.tensor([[0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 5.0, 0.0]]).view(torch.int32).tolist()
