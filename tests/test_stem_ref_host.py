"""Host checks of tests/stem_ref64.py, the float64 contracts and bounds of the conv patch-embedding stem.  No GPU.

1. An fp32 emulation in the kernels' order -- 16-bit operands, fp32 accumulation over (tap, channel chunk) in MFMA step order for the
   convolutions, per-tile partial sums per persistent workgroup for the weight gradient, per-thread chains, the rows_par fold and the per-
   block adds for BatchNorm -- stays inside every bound on the very cases tests/test_gpu_stem.py runs (the lists of stem_ref64).
2. Numerical errors injected INTO THE EMULATION push some case above 1: the bounds are tight enough to see them.
3. The undecided share of the BatchNorm mask is within its cap on every seeded input.
4. The contracts agree with torch.nn.BatchNorm2d, torch.nn.functional.conv2d / conv_transpose2d and torch.nn.grad.conv2d_weight in float64."""
import math

import pytest
import torch

import stem_ref64 as S

F32 = torch.float32


class Emu:
    """the stem's entry points in fp32, in the kernels' order; `inject` names one deliberate error"""

    def __init__(self, inject=None):
        self.inject = inject

    # ---- conv3x3 family -------------------------------------------------------------------------------------------------------------
    def _shift(self, x, kh, kw):
        """x [B, H, W, C] fp32 -> the tap's shifted view, zero outside the image"""
        B, H, W, _ = x.shape
        if self.inject == "swap_khkw":
            kh, kw = kw, kh
        iy, ix = torch.arange(H) + kh - 1, torch.arange(W) + kw - 1
        oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
        if self.inject == "clamp_pad":                          # right / bottom edge: the clamped coordinate instead of zero
            oky, okx = iy >= 0, ix >= 0
        s = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)] * (oky[:, None] & okx[None, :])[None, :, :, None]
        if self.inject == "halo_next_image" and kh == 2 and B > 1:     # the row below the image: row 0 of the next image
            s = s.clone()
            s[:-1, H - 1] = x[1:, 0][:, ix.clamp(0, W - 1)] * okx[None, :, None]
        return s

    def _conv(self, a, w, B, H, W):
        Cout = w.shape[0]
        x, wt = a.float().reshape(B, H, W, -1), w.float().reshape(Cout, 9, -1)
        NC = x.shape[-1] // 8
        acc = torch.zeros(B, H, W, Cout)
        for chunk in range(9 * NC):                              # step ks = chunk / 4, lane group g = chunk % 4
            if self.inject == "drop_chunk" and chunk == 7:       # the last chunk of MFMA step 1
                continue
            tap, cc = chunk // NC, chunk % NC
            s = self._shift(x, tap // 3, tap % 3)[..., cc * 8:cc * 8 + 8]
            acc = acc + (s[:, :, :, None, :] * wt[:, tap, cc * 8:cc * 8 + 8]).sum(-1)
        return acc.reshape(-1, Cout)

    def conv3x3(self, a, w, B, H, W, Cin, Cout, out_dtype):
        return self._conv(a, w, B, H, W).to(out_dtype)

    def conv3x3_res(self, a, w, res, B, H, W, Cin, Cout, out_dtype):
        return (self._conv(a, w, B, H, W) + res.float()).to(out_dtype)

    def conv3x3_res_patch(self, a, w, res_col, B, H, W, Cin, Cout, P, out_dtype):
        r = res_col.float().reshape(-1, Cout) if self.inject == "res_nhwc" else S.from_patch(res_col.float(), B, H, W, P)
        return (self._conv(a, w, B, H, W) + r).to(out_dtype)

    def conv3x3_bias_relu(self, a, w, bias, res, B, H, W, Cin, Cout, out_dtype):
        y = torch.relu(self._conv(a, w, B, H, W) + bias)
        return (y + res.float() if res is not None else y).to(out_dtype)

    def conv3x3_bias_relu_patch(self, a, w, bias, res, B, H, W, Cin, Cout, P, out_dtype):
        return S.to_patch(self.conv3x3_bias_relu(a, w, bias, res, B, H, W, Cin, Cout, out_dtype), B, H, W, P)

    def conv_w_flip(self, w4, out_dtype):
        f = w4 if self.inject == "no_flip" else w4.flip(2, 3)
        return f.permute(1, 2, 3, 0).reshape(w4.shape[1], 9 * w4.shape[0]).to(out_dtype).contiguous()

    def conv1_direct(self, img, w, bias, relu, out_dtype):
        B, _, H, W = img.shape
        Cout = w.shape[0]
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        I = torch.nn.functional.pad(img.to(w.dtype).float(), (1, 2, 1, 2))
        wt = w.float()
        acc = torch.zeros(B, Ho, Wo, Cout)
        for k in range(27):                                      # one MFMA: k = (kh, kw, c) in order
            tap, c = k // 3, k % 3
            acc = acc + I[:, c, tap // 3:tap // 3 + 2 * Ho:2, tap % 3:tap % 3 + 2 * Wo:2][..., None] * wt[:, k]
        y = acc.reshape(-1, Cout)
        if bias is not None:
            y = y + bias
        return (torch.relu(y) if relu else y).to(out_dtype)

    def conv3x3_wgrad(self, a, dz, dw, B, H, W, Cin, Cout):
        col = S.im2col_nhwc(a.float(), B, H, W)                  # exact: a selection of bf16 values and zeros
        g = dz.float()
        ty, tx = (H + 15) // 16, (W + 15) // 16
        pix = torch.arange(B * H * W)
        tile = ((pix // (H * W)) * ty + ((pix // W) % H) // 16) * tx + (pix % W) // 16
        order = torch.argsort(tile, stable=True)
        counts = torch.bincount(tile, minlength=B * ty * tx).tolist()
        ntiles, grid = len(counts), min(len(counts), 1024)
        parts, o = [], 0
        for n in counts:
            idx = order[o:o + n]
            parts.append(g[idx].t() @ col[idx])                  # a tile's 256 pixels in the MFMA accumulators
            o += n
        out = dw.clone()
        for j in range(grid):                                    # a persistent workgroup: its tiles, then one atomic add
            acc = torch.zeros(Cout, 9 * Cin)
            for n, t in enumerate(range(j, ntiles, grid)):
                if self.inject == "skip_tile" and j == 0 and n == 1:
                    continue
                acc = acc + parts[t]
            out = out + acc
        return out

    # ---- BatchNorm ------------------------------------------------------------------------------------------------------------------
    def _reduce(self, x, acc0):
        """column sums of x [R, C] fp32 in bn_stats_kernel's order: per-thread chains, the rows_par fold, the per-block adds"""
        R, C = x.shape
        rp, blocks, chain = S.bn_path(R, C)
        if self.inject == "drop_tail_row":                      # the last row of an unrolled trip's tail (u > 0) is not summed
            k = (R - 1) // (blocks * rp)
            if k % 4:
                x = x.clone()
                x[R - 1] = 0.0
        pad = torch.zeros(chain * blocks * rp, C)
        pad[:R] = x
        pad = pad.reshape(chain, blocks, rp, C)
        t = torch.zeros(blocks, rp, C)
        for k in range(chain):
            t = t + pad[k]
        b = torch.zeros(blocks, C)
        for r in range(rp):
            b = b + t[:, r]
        out = acc0.clone().float()
        for j in range(blocks):
            out = out + b[j]
        return out

    def bn_stats(self, z, s, q):
        x = z.float()
        return self._reduce(x, s), self._reduce(x * x, q)

    def bn_finalize(self, s, q, n, w, b, eps, momentum, rmean, rvar, nbt, update):
        n32, eps, m = torch.tensor(float(n), dtype=F32), torch.tensor(eps, dtype=F32), torch.tensor(momentum, dtype=F32)
        mu = s / n32
        var = q / n32 - mu * mu
        var = torch.where(var < 0, torch.zeros_like(var), var)
        if update:
            f = torch.tensor(1.0) if self.inject == "biased_rvar" else n32 / torch.clamp(n32 - 1, min=1.0)
            rmean = rmean * (1 - m) + m * mu
            rvar = rvar * (1 - m) + m * (var * f)
            nbt = nbt + 1
        rs = 1.0 / torch.sqrt(var + eps)
        sc = w * rs
        return sc, b - mu * sc, mu, rs, rmean, rvar, nbt

    def bn_relu(self, z, scale, shift, res, out_dtype):
        y = torch.relu(z.float() * scale + shift)
        return (y + res.float() if res is not None else y).to(out_dtype)

    def bn_relu_patch(self, z, scale, shift, res, B, H, W, P, out_dtype):
        return S.to_patch(self.bn_relu(z, scale, shift, res, out_dtype), B, H, W, P)

    def bn_bwd(self, da, z, scale, shift, mean, rstd, sg, sgz, training):
        x, g = z.float(), da.float().reshape(z.shape)
        pre = x * scale + shift
        gg = torch.where(pre >= 0 if self.inject == "mask_ge" else pre > 0, g, torch.zeros_like(g))
        zh = (x - mean) * rstd
        sg, sgz = self._reduce(gg, sg), self._reduce(gg * (x - mean) * rstd, sgz)
        inv_n = (torch.tensor(1.0) / torch.tensor(float(z.shape[0]))) if training else torch.tensor(0.0)
        t1 = 0.0 if self.inject == "no_sg_term" else sg * inv_n
        return (scale * (gg - t1 - zh * sgz * inv_n)).to(da.dtype), sg, sgz

    def bn_bwd_patch(self, dcol, z, scale, shift, mean, rstd, sg, sgz, training, B, H, W, P):
        return self.bn_bwd(S.from_patch(dcol, B, H, W, P), z, scale, shift, mean, rstd, sg, sgz, training)

    # ---- layout ---------------------------------------------------------------------------------------------------------------------
    def im2col3x3(self, a, B, H, W, C):
        return S.im2col_nhwc(a, B, H, W)

    def col2im3x3(self, dcol, B, H, W, C):
        d = dcol.float().reshape(B, H, W, 9, C)
        p = torch.nn.functional.pad(d, (0, 0, 0, 0, 1, 1, 1, 1))
        acc = torch.zeros(B, H, W, C)
        for t in range(9):
            acc = acc + p[:, 2 - t // 3:2 - t // 3 + H, 2 - t % 3:2 - t % 3 + W, t]
        return acc.reshape(-1, C).to(dcol.dtype)


EMU = Emu()
WORST = {}


def note(q, r):
    WORST[q] = max(WORST.get(q, 0.0), S.worst_of(r))
    if isinstance(r, dict):
        for k, v in r.items():
            WORST[q + "." + k] = max(WORST.get(q + "." + k, 0.0), v)
    return S.worst_of(r)


def report(prefix):
    print("STEM emulation worst error / bound: " + "  ".join("%s=%.3f" % kv for kv in sorted(WORST.items()) if kv[0].startswith(prefix)))


# ---- 1. the emulation is inside every bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", S.CONV_CIN)
def test_emulated_conv3x3_family_is_inside_the_bounds(Cin):
    for kw in S.conv_cases(Cin):
        assert note("conv3x3_" + kw.get("form", "plain"), S.run_conv3x3(EMU, **kw)) <= 1.0, kw
    for H, W in S.CONV_HW:
        for Cout in (4, 20, 32):
            assert S.run_conv3x3_int(EMU, 3, H, W, Cin, Cout) == 0.0 and S.run_conv3x3_onehot(EMU, 3, H, W, Cin, Cout) == 0.0
    report("conv3x3")


def test_emulated_data_gradient_is_inside_the_bounds():
    for kw in S.dgrad_cases():
        assert note("dgrad", S.run_dgrad(EMU, **kw)) <= 1.0, kw
    report("dgrad")


@pytest.mark.parametrize("Cout", S.CONV1_COUT)
def test_emulated_conv1_direct_is_inside_the_bounds(Cout):
    for kw in S.conv1_cases(Cout):
        assert note("conv1", S.run_conv1(EMU, **kw)) <= 1.0, kw
    for H, W in S.CONV1_HW:
        assert S.run_conv1_int(EMU, 2, H, W, Cout) == 0.0 and S.run_conv1_onehot(EMU, 2, H, W, Cout) == 0.0
    report("conv1")


@pytest.mark.parametrize("C", S.CONV_CIN)
def test_emulated_wgrad_is_inside_the_bounds(C):
    for kw in S.wgrad_cases(C):
        assert note("wgrad", S.run_wgrad(EMU, **kw)) <= 1.0, kw
    if C == 32:
        assert note("wgrad_persistent", S.run_wgrad(EMU, *S.WGRAD_BIG, C)) <= 1.0
    report("wgrad")


@pytest.mark.parametrize("C", S.BN_C)
def test_emulated_batchnorm_is_inside_the_bounds(C):
    for kw in S.bn_forward_cases(C):
        assert note("bn_fwd", S.run_bn_forward(EMU, **kw)) <= 1.0, kw
    for kw in S.bn_relu_cases(C):
        assert note("bn_relu", S.run_bn_relu(EMU, **kw)) <= 1.0, kw
    for kw in S.bn_bwd_cases(C):
        assert note("bn_bwd", S.run_bn_bwd(EMU, **kw)) <= 1.0, kw
    report("bn_")


def test_emulated_patch_forms_and_probes_are_inside_the_bounds():
    for kw, od in S.bn_patch_cases():
        assert note("bn_relu_patch", S.run_bn_relu(EMU, out_dtype=od, with_res=True, **kw)) <= 1.0, kw
        for training in (True, False):
            assert note("bn_bwd_patch", S.run_bn_bwd(EMU, da_dtype=od, training=training, **kw)) <= 1.0, kw
    assert S.worst_of(S.run_bn_zero_probe(EMU)) <= 1.0 and S.worst_of(S.run_bn_zero_probe(EMU, training=False)) <= 1.0
    for kw in S.layout_cases():
        assert note("layout", S.run_layouts(EMU, **kw)) <= 1.0, kw
    report("bn_")
    report("layout")


# ---- 2. injected errors are seen ----------------------------------------------------------------------------------------------------------
def _conv_probe(impl):
    return max(S.run_conv3x3(impl, B=3, H=H, W=W, Cin=Cin, Cout=Cout, out_dtype=dt, isolate=iso)
               for (H, W), Cin, Cout, dt, iso in [((16, 16), 16, 16, F32, True), ((15, 17), 24, 12, torch.bfloat16, False),
                                                  ((33, 16), 32, 32, torch.bfloat16, True)])


INJECTED = {
    "halo_next_image": _conv_probe,
    "clamp_pad": _conv_probe,
    "drop_chunk": _conv_probe,
    "swap_khkw": _conv_probe,
    "no_flip": lambda e: S.run_dgrad(e, 3, 15, 17, 24, 32)["dx"],
    "res_nhwc": lambda e: S.run_conv3x3(e, B=3, H=28, W=42, Cin=24, Cout=24, out_dtype=torch.bfloat16, form="res_patch", P=7),
    "mask_ge": lambda e: S.worst_of(S.run_bn_zero_probe(e)),
    "no_sg_term": lambda e: S.run_bn_bwd(e, 65, 32, F32, torch.bfloat16, True)["dz"],
    "biased_rvar": lambda e: S.run_bn_forward(e, 9, 256)["rvar"],
    "skip_tile": lambda e: S.run_wgrad(e, *S.WGRAD_BIG, 32),
    "drop_tail_row": lambda e: max(S.run_bn_forward(e, R, C)["sum+"] for C in (24, 256) for R in S.bn_rows(C)[3:]),
}


@pytest.mark.parametrize("name", sorted(INJECTED))
def test_injected_error_is_outside_the_bounds(name):
    clean, broken = INJECTED[name](EMU), INJECTED[name](Emu(name))
    print("STEM injected %s: %.3f -> %.3g" % (name, clean, broken))
    assert clean <= 1.0 < broken


def test_every_injection_of_the_emulation_is_exercised():
    import inspect
    src = inspect.getsource(Emu)
    assert all('"%s"' % name in src for name in INJECTED)


# ---- 3. the undecided share of the BatchNorm mask ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", S.BN_C)
def test_undecided_mask_elements_are_within_the_cap(C):
    total = 0
    for kw in S.bn_bwd_cases(C):
        _, ref = S.bn_bwd_case(**kw)
        assert ref["undecided"] <= S.undecided_cap(ref["numel"]), kw
        total += ref["undecided"]
    if C in (24, 32):
        for kw, od in S.bn_patch_cases():
            if kw["C"] == C:
                _, ref = S.bn_bwd_case(da_dtype=od, training=True, **kw)
                assert ref["undecided"] <= S.undecided_cap(ref["numel"]), kw
    print("STEM undecided elements at C = %d: %d" % (C, total))


# ---- 4. the contracts are the operations torch names ----------------------------------------------------------------------------------------
def test_relu_contract_propagates_nan_and_returns_plus_zero():
    r = S.relu64(torch.tensor([float("nan"), -0.0, -3.0, 2.0, float("inf"), float("-inf")], dtype=S.F64))
    assert math.isnan(float(r[0])) and r[1:].tolist() == [0.0, 0.0, 2.0, float("inf"), 0.0]
    assert not bool(torch.signbit(r[1:4]).any())                     # +0, not -0


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(3, 15, 17, 24, 20), (1, 1, 1, 16, 4), (2, 33, 16, 32, 32)])
def test_conv_contracts_are_torch_conv2d(B, H, W, Cin, Cout):
    a, w, bias, res = S.conv_inputs(B, H, W, Cin, Cout)
    x = S.f64(a).reshape(B, H, W, Cin).permute(0, 3, 1, 2)
    w4 = S.f64(w).reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, w4, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    tol = 1e-13 * float(y.abs().max() + 1)
    assert float((S.conv3x3_64(a, w, B, H, W)[0] - y).abs().max()) <= tol
    full = torch.relu(y + S.f64(bias)) + S.f64(res)
    assert float((S.conv3x3_64(a, w, B, H, W, bias=bias, relu=True, res=res)[0] - full).abs().max()) <= tol
    # the NaN-safe (term by term) path states the same numbers
    a2 = a.clone()
    a2[0, 0] = float("nan")
    got = S.conv3x3_64(a2, w, B, H, W)[0]
    keep = ~torch.isnan(got).any(-1)
    assert float((got[keep] - y[keep]).abs().max() if keep.any() else 0.0) <= tol and bool(torch.isnan(got[0]).all())
    # data gradient: the transposed convolution, and the flipped-weight convolution that computes it
    dz = a[:, :Cout] if Cout <= Cin else torch.cat([a, a], 1)[:, :Cout]
    w4g = S.f64(w).reshape(Cout, 9, Cin)[:, :, :].permute(0, 2, 1).reshape(Cout, Cin, 3, 3)
    t = torch.nn.functional.conv_transpose2d(S.f64(dz).reshape(B, H, W, Cout).permute(0, 3, 1, 2), w4g, padding=1)
    t = t.permute(0, 2, 3, 1).reshape(-1, Cin)
    assert float((S.dgrad64(dz, w4g, B, H, W)[0] - t).abs().max()) <= tol
    assert float((S.conv3x3_64(dz, S.w_flip64(w4g), B, H, W)[0] - t).abs().max()) <= tol
    # weight gradient
    if Cin == Cout:
        gw = torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), S.f64(res).reshape(B, H, W, Cout).permute(0, 3, 1, 2), padding=1)
        ref, _ = S.wgrad64(a, res, torch.zeros(Cout, 9 * Cin), B, H, W)
        assert float((ref - gw.permute(0, 2, 3, 1).reshape(Cout, -1)).abs().max()) <= 1e-12 * float(gw.abs().max() + 1)


@pytest.mark.parametrize("H,W", [(1, 1), (16, 17), (33, 65)])
def test_conv1_contract_is_torch_conv2d_on_the_rounded_image(H, W):
    img, w, bias = S.conv1_inputs(2, H, W, 20)
    w4 = S.f64(w)[:, :27].reshape(20, 3, 3, 3).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(S.f64(img.to(torch.bfloat16)), w4, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, 20)
    assert float((S.conv1_64(img, w, torch.bfloat16)[0] - y).abs().max()) <= 1e-13 * float(y.abs().max() + 1)
    full = torch.relu(y + S.f64(bias))
    assert float((S.conv1_64(img, w, torch.bfloat16, bias, True)[0] - full).abs().max()) <= 1e-13 * float(y.abs().max() + 1)


@pytest.mark.parametrize("R,C", [(1, 8), (9, 256), (2051, 256), (65, 32)])
def test_finalize_contract_is_torch_batchnorm2d(R, C):
    inp = S.bn_inputs(R, C)
    bn = torch.nn.BatchNorm2d(C, eps=S.f32v(S.BN_EPS), momentum=S.f32v(S.BN_MOMENTUM)).double()
    with torch.no_grad():
        bn.weight.copy_(inp["w"]); bn.bias.copy_(inp["b"]); bn.running_mean.copy_(inp["rmean"]); bn.running_var.copy_(inp["rvar"])
    bn.train()
    x = S.f64(inp["z"]).t().reshape(1, C, R, 1)
    if R == 1:
        with pytest.raises(ValueError):                          # torch refuses one value per channel; the kernel's n = 1 factor is 1
            bn(x)
        f = S.bn_finalize64(inp["z"], inp["w"], inp["b"], rmean0=inp["rmean"], rvar0=inp["rvar"])
        assert float(f["var"].abs().max()) == 0.0 and torch.allclose(f["rvar"], (1 - S.f32v(0.1)) * S.f64(inp["rvar"]), rtol=1e-14)
        return
    y = bn(x).reshape(C, R).t()
    f = S.bn_finalize64(inp["z"], inp["w"], inp["b"], rmean0=inp["rmean"], rvar0=inp["rvar"])
    assert torch.allclose(S.f64(inp["z"]) * f["scale"] + f["shift"], y.detach(), rtol=1e-10, atol=1e-10)
    assert torch.allclose(f["rmean"], bn.running_mean, rtol=1e-12, atol=1e-13) and torch.allclose(f["rvar"], bn.running_var, rtol=1e-12, atol=1e-13)
    assert int(bn.num_batches_tracked) == 1


def test_bn_backward_contract_is_autograd_of_batchnorm_relu():
    R, C = 65, 32
    inp = S.bn_inputs(R, C)
    z = S.f64(inp["z"]).requires_grad_(True)
    w, b = S.f64(inp["w"]), S.f64(inp["b"])
    mean, var = z.mean(0), z.var(0, unbiased=False)
    out = torch.relu((z - mean) * (var + S.f32v(S.BN_EPS)) ** -0.5 * w + b)
    out.backward(S.f64(inp["da"]))
    f = S.bn_finalize64(inp["z"], w, b)
    ref = S.bn_bwd64(inp["da"], inp["z"], f["scale"], f["shift"], f["mean"], f["rstd"], torch.zeros(C), torch.zeros(C), True, 0.0)
    assert torch.allclose(ref["dz"], z.grad, rtol=1e-6, atol=1e-9)          # (inv_n is the fp32 1 / R: 6e-8 relative)


def test_layout_statements_are_the_permutations():
    B, H, W, P, C = 2, 14, 21, 7, 8
    a = torch.arange(B * H * W * C, dtype=F32).reshape(B * H * W, C)
    col = S.to_patch(a, B, H, W, P)
    ref = a.reshape(B, H // P, P, W // P, P, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // P) * (W // P), P * P * C)
    assert torch.equal(col, ref) and torch.equal(S.from_patch(col, B, H, W, P), a)
    x = a.reshape(B, H, W, C).permute(0, 3, 1, 2)
    unf = torch.nn.functional.unfold(x, 3, padding=1).reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)
    assert torch.equal(S.im2col_nhwc(a, B, H, W), unf)
    img = torch.randn(2, 3, 9, 12)
    for stride in (1, 2):
        u = torch.nn.functional.unfold(img, 3, padding=1, stride=stride)
        L = u.shape[-1]
        u = u.reshape(2, 3, 9, L).permute(0, 3, 2, 1).reshape(2 * L, 27)
        got = S.im2col_image(img, stride, 32, F32)
        assert torch.equal(got[:, :27], u) and float(got[:, 27:].abs().max()) == 0.0
    w4 = torch.randn(5, 3, 3, 3)
    wf = S.w_flip64(w4).reshape(3, 3, 3, 5)
    assert all(float(wf[ci, kh, kw, co]) == float(w4[co, ci, 2 - kh, 2 - kw]) for ci in range(3) for kh in range(3) for kw in range(3) for co in range(5))
