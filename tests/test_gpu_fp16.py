"""The fp16 evaluation mode on the GPU: every forward kernel instantiated for fp16 (GEMM forms and epilogues, the fused LayerNorm
GEMM, attention, the element-wise entries, the evaluation stem) against torch on fp16-rounded operands; model-level eval logits
against the fp32 HIP path next to the bf16 error; C5 candidate scoring; the same kernel sequence as bf16; switching modes on a
trained model; the training guard."""
import os
import subprocess

import numpy as np
import pytest
import torch

import emu_kernels as E
import recipe
import vitres
import vitres.kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
H16 = torch.float16


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relerr(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


def within_ulp(out, ref, ulps=1):
    """Elements of out (fp16) farther than `ulps` fp16 ulps from the fp16-rounded fp32 reference.  The reference's own fp32
    summation order differs from the kernel's, and the 16-bit GELU epilogue's erf carries an absolute 1.5e-7: results that cancel
    (or sit in GELU's negative tail) below that noise -- 2e-6 of the largest value -- are compared at that floor instead."""
    r32 = ref.detach().cpu().float()
    r = r32.to(H16).float()
    o = out.detach().cpu().float()
    ulp = torch.clamp(torch.exp2(torch.floor(torch.log2(r.abs().clamp(min=2.0 ** -14))) - 10), min=2.0 ** -24)
    noise = 2e-6 * float(r32.abs().max())
    bad = (o - r).abs() > ulps * ulp + noise
    return int(bad.sum())


# ---- 1. GEMM -------------------------------------------------------------------------------------------------
# (M, N, K, sched): K % 64 == 0 -> gemm_ntk.hip; K tails / odd strides -> gemm_nt.hip; sched bit 4 -> the generic kernel
GEMM_SHAPES = [(257 * 3, 576, 192, 0), (2176, 768, 3072, 0), (257 * 2, 320, 168, 0), (130, 1000, 96, 0), (64, 24, 40, 0),
               (257 * 2, 256, 128, 4), (130, 200, 72, 4)]


@pytest.mark.parametrize("M,N,K_,sched", GEMM_SHAPES)
def test_gemm_fp16_forward_epilogues(M, N, K_, sched):
    rows_in = 257 if M % 257 == 0 else 0
    Bn = max(M // rows_in, 1) if rows_in else 1
    a = rnd(M, K_, seed=1).to(H16)
    b = rnd(N, K_, seed=2, scale=K_ ** -0.5).to(H16)
    bias = rnd(N, seed=3)
    keep = torch.randint(1, N + 1, (Bn,), generator=torch.Generator().manual_seed(4)).int()
    scale = torch.rand(Bn, generator=torch.Generator().manual_seed(5)) + 0.5
    resid = rnd(M, N, seed=6)
    to = lambda v: v.to(DEV) if isinstance(v, torch.Tensor) else v
    for variant in ("plain", "nobias", "resid", "gelu", "relu", "gelu2", "f32"):
        out_dtype = torch.float32 if variant in ("resid", "f32") else H16
        kw = dict(M=M, N=N, K=K_, lda=K_, ldb=K_, ldc=N, bias=None if variant == "nobias" else bias, rows_in=rows_in,
                  keep_n=keep if rows_in else None, sched=sched)
        if variant == "resid":
            kw.update(scale=scale if rows_in else None, resid=resid)
        if variant in ("gelu", "relu", "gelu2"):
            kw.update(act={"gelu": 1, "relu": 3, "gelu2": 2}[variant])
        out2 = out2_ref = None
        if variant == "gelu2":                          # C = gelu'(u), C2 = gelu(u)
            out2, out2_ref = torch.zeros(M, N, dtype=H16, device=DEV), torch.zeros(M, N, dtype=torch.float32)
        ekw = {k: v for k, v in kw.items() if k != "sched"}
        ref = E.gemm(a, b, torch.zeros(M, N, dtype=torch.float32), out2=out2_ref, **ekw)
        real = K.gemm(a.to(DEV), b.to(DEV), torch.zeros(M, N, dtype=out_dtype, device=DEV), out2=out2, **{k: to(v) for k, v in kw.items()})
        torch.cuda.synchronize()
        if out_dtype == torch.float32:
            assert relerr(real, ref) < 1e-4, (variant, relerr(real, ref))
        else:
            assert within_ulp(real, ref, 1) == 0, (variant, within_ulp(real, ref, 1))      # one fp16 ulp of the rounded reference
        if out2 is not None:
            assert within_ulp(out2, out2_ref, 1) == 0


def test_gemm_fp16_pos_and_row_maps():
    """The patch-embedding form: positional embedding, output row map (class-token rows skipped), fp32 result -- gemm_nt.hip's general
    epilogue; and an A row map (the token rows of a spatial reduction)."""
    B, P, T, C, Kp = 6, 64, 1, 192, 592
    col = rnd(B * P, Kp, seed=1).to(H16)
    w = rnd(C, Kp, seed=2, scale=Kp ** -0.5).to(H16)
    bias, pos = rnd(C, seed=3), rnd(P, C, seed=4)
    keep = torch.tensor([192, 128, 64, 192, 96, 160], dtype=torch.int32)
    kw = dict(M=B * P, N=C, K=Kp, lda=Kp, ldb=Kp, ldc=C, bias=bias, pos=pos, keep_n=keep, rows_in=P, c_map=(P, P + T, T))
    ref = E.gemm(col, w, torch.full((B, P + T, C), 7.0), **kw)
    out = K.gemm(col.to(DEV), w.to(DEV), torch.full((B, P + T, C), 7.0, device=DEV),
                 **{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    assert relerr(out, ref) < 1e-4
    assert float((out[:, 0].cpu() - 7.0).abs().max()) == 0.0            # rows outside the map untouched
    y = rnd(B * 17, C, seed=5).to(H16)
    kw2 = dict(M=B, N=C, K=C, lda=C, ldb=C, ldc=C, bias=bias, a_map=(1, 17, 0))
    ref2 = E.gemm(y, w[:, :C].contiguous(), torch.zeros(B, C), **kw2)
    out2 = K.gemm(y.to(DEV), w[:, :C].contiguous().to(DEV), torch.zeros(B, C, device=DEV),
                  **{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw2.items()})
    assert relerr(out2, ref2) < 1e-4


@pytest.mark.parametrize("tile", [1, 2, 3])
def test_gemm_fp16_masked_tiles_unwritten(tile):
    """Write skipping (sched 0x40000) with the per-group grid, as for bf16: tiles beyond a group's width are left untouched."""
    G, spg, rows_in, N, K_ = 4, 2, 65, 512, 256
    M = G * spg * rows_in
    widths = [512, 256, 128, 0]
    keep = torch.tensor([w for w in widths for _ in range(spg)], dtype=torch.int32)
    a, b = rnd(M, K_, seed=1).to(H16), rnd(N, K_, seed=2, scale=K_ ** -0.5).to(H16)
    bias = rnd(N, seed=3)
    kw = dict(M=M, N=N, K=K_, lda=K_, ldb=K_, ldc=N, bias=bias, keep_n=keep, rows_in=rows_in)
    ref = E.gemm(a, b, torch.zeros(M, N), **kw)
    kw_d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    BN = 64 if tile == 3 else 128
    K.M_GROUPS[0] = G
    try:
        for skip in (False, True):
            K.WRITE_SKIP[0] = skip
            out = K.gemm(a.to(DEV), b.to(DEV), torch.full((M, N), float("nan"), dtype=H16, device=DEV), sched=tile << 11, **kw_d).cpu()
            for g_, w in enumerate(widths):
                rows = slice(g_ * spg * rows_in, (g_ + 1) * spg * rows_in)
                wr = (w + BN - 1) // BN * BN if skip else N
                assert torch.isfinite(out[rows, :wr]).all(), (skip, g_)
                if wr:
                    assert within_ulp(out[rows, :wr], ref[rows, :wr], 1) == 0, (skip, g_)
                assert torch.isnan(out[rows, wr:]).all(), (skip, g_)
    finally:
        K.M_GROUPS[0] = 1
        K.WRITE_SKIP[0] = False


def test_gemm_fp16_refuses_what_it_does_not_implement():
    a = torch.zeros(128, 128, dtype=H16, device=DEV)
    bb = torch.zeros(128, 128, dtype=torch.bfloat16, device=DEV)
    o32 = torch.zeros(128, 128, device=DEV)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):          # fp16 in, bf16 out
        K.gemm(a, a, torch.zeros(128, 128, dtype=torch.bfloat16, device=DEV), M=128, N=128, K=128, lda=128, ldb=128, ldc=128)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):          # weight gradient
        K.gemm(a, a, o32, M=128, N=128, K=128, lda=128, ldb=128, ldc=128, a_trans=True, b_trans=True, atomic=True)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):          # data gradient (b_trans)
        K.gemm(a, a, torch.zeros(128, 128, dtype=H16, device=DEV), M=128, N=128, K=128, lda=128, ldb=128, ldc=128, b_trans=True)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):          # the opt-in K-split form
        K.gemm(a, a, o32, M=128, N=128, K=128, lda=128, ldb=128, ldc=128, k_shares=2)
    with pytest.raises(AssertionError):
        K.gemm(a, bb, o32, M=128, N=128, K=128, lda=128, ldb=128, ldc=128)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.attn_bwd(torch.zeros(2, 17, 3 * 64, dtype=H16, device=DEV), torch.zeros(2, 17, 64, dtype=H16, device=DEV),
                   torch.zeros(2, 17, 64, dtype=H16, device=DEV), torch.zeros(2, 1, 17, device=DEV), None, 2, 17, 1, 64, 0.125)


# ---- 2. fused LayerNorm GEMM ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Nt,C,Kd,masked", [(4, 257, 256, 768, True), (3, 65, 320, 960, False), (2, 257, 192, 104, True)])
def test_gemm_ln_fp16_equals_separate_kernels(B, Nt, C, Kd, masked):
    M = B * Nt
    g = torch.Generator().manual_seed(7)
    a = rnd(M, Kd, seed=1).to(H16).to(DEV)
    w = rnd(C, Kd, seed=2, scale=Kd ** -0.5).to(H16).to(DEV)
    bias, resid = rnd(C, seed=3).to(DEV), rnd(B, Nt, C, seed=4).to(DEV)
    lw, lb = (1 + 0.1 * rnd(C, seed=5)).to(DEV), (0.1 * rnd(C, seed=6)).to(DEV)
    keep = torch.randint(C // 2, C + 1, (B,), generator=g).int().to(DEV) if masked else None
    kk = torch.randint(Kd // 2, Kd + 1, (B,), generator=g).int().to(DEV) if masked else None
    scale = (torch.rand(B, generator=g) + 0.5).to(DEV)
    assert K.gemm_ln_supported(a, C, C)
    x1 = torch.empty(B, Nt, C, device=DEV)
    y, mean, rstd = K.gemm_ln_fwd(a, w, x1, lw, lb, keep, 1e-6, M=M, N=C, K=Kd, lda=Kd, ldb=Kd, ldc=C, bias=bias, scale=scale,
                                  keep_n=keep, resid=resid, rows_in=Nt, keep_k=kk)
    x2 = torch.empty(B, Nt, C, device=DEV)
    K.gemm(a, w, x2, M=M, N=C, K=Kd, lda=Kd, ldb=Kd, ldc=C, bias=bias, scale=scale, keep_n=keep, resid=resid, rows_in=Nt, keep_k=kk)
    y2, mean2, rstd2 = K.ln_fwd(x2, lw, lb, keep, Nt, 1e-6, H16)
    assert y.dtype == H16
    assert relerr(x1, x2) < 1e-5 and relerr(mean, mean2) < 1e-4 and relerr(rstd, rstd2) < 1e-4
    assert within_ulp(y, y2.float(), 1) == 0


# ---- 3. attention -------------------------------------------------------------------------------------------------
def _attn_ref(qkv, keep, B, N, H, D, scale):
    q, k, v = qkv.float().view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    p = torch.softmax((q * scale) @ k.transpose(-1, -2), -1)
    o = (p @ v).transpose(1, 2).reshape(B, N, H * D)
    if keep is not None:
        for b in range(B):
            o[b, :, int(keep[b]):] = 0
    return o


@pytest.mark.parametrize("N,H,D,masked", [(257, 4, 64, True), (65, 8, 32, False), (17, 6, 48, True), (257, 5, 48, False),
                                          (785, 4, 64, True), (785, 6, 32, False), (50, 3, 16, True)])
def test_attention_fp16_forward(N, H, D, masked):
    """D = 16 exists in attn.hip only; N = 785 is the hi-res (long-sequence) form."""
    B = 3
    qkv = rnd(B, N, 3 * H * D, seed=N + D).to(H16)
    keep = torch.tensor([H * D, (H - 1) * D, D], dtype=torch.int32)[:B] if masked else None
    scale = D ** -0.5
    o, lse = K.attn_fwd(qkv.to(DEV), None if keep is None else keep.to(DEV), B, N, H, D, scale)
    assert o.dtype == H16
    ref = _attn_ref(qkv, keep, B, N, H, D, scale)
    assert relerr(o, ref) < 2e-3, relerr(o, ref)


# ---- 4. element-wise entries and the cast -----------------------------------------------------------------------
def test_cast_is_torch_half_bit_for_bit():
    x = torch.cat([rnd(4093, seed=1) * 3000, torch.tensor([65504.0, 65519.9, 65520.0, 1e6, -1e6, float("inf"), float("-inf"),
                                                          float("nan"), 2.0 ** -25, 3 * 2.0 ** -26, 1e-8, -0.0])])
    n = x.numel() // 8 * 8 + 8
    src = torch.zeros(n)
    src[:x.numel()] = x
    out = K.cast_f16(src.to(DEV), torch.empty(n, dtype=H16, device=DEV)).cpu()
    want = src.half()
    assert torch.equal(out.view(torch.int16)[~want.isnan()], want.view(torch.int16)[~want.isnan()])
    assert bool(out[want.isnan()].isnan().all())
    odd = K.cast_f16(src[:n - 8].to(DEV), torch.empty(n - 8, dtype=H16, device=DEV)).cpu()     # (tail handled element by element)
    assert torch.equal(odd[:100].view(torch.int16), want[:100].view(torch.int16))


def test_elementwise_entries_fp16():
    B, N, C = 3, 17, 64
    x = rnd(B, N, C, seed=1) * 40
    x[0, 0, :4] = torch.tensor([1e6, -1e6, float("nan"), 65519.0])
    sc = torch.tensor([0.5, 2.0, 1.25])
    keep = torch.tensor([64, 40, 8], dtype=torch.int32)
    out = K.scale_mask_cast(x.to(DEV), sc.to(DEV), keep.to(DEV), N, H16).cpu()
    want = (x * sc.view(B, 1, 1)).masked_fill(torch.arange(C).view(1, 1, C) >= keep.view(B, 1, 1), 0).half()
    same = lambda a, b: torch.equal(a.view(torch.int16)[~b.isnan()], b.view(torch.int16)[~b.isnan()]) and bool(a[b.isnan()].isnan().all())
    assert same(out, want)
    y = rnd(B, N, C, seed=2).half()
    tm = K.token_mean(y.to(DEV), 1).cpu()
    assert same(tm, (y.float()[:, 1:].sum(1) * (1.0 / (N - 1))).half()) or within_ulp(tm, y.float()[:, 1:].mean(1), 1) == 0
    img = rnd(2, 3, 56, 56, seed=3)
    col = K.im2col_patch(img.to(DEV), 14, 592, H16).cpu()
    ref = torch.zeros(2 * 16, 592)
    ref[:, :588] = img.unfold(2, 14, 14).unfold(3, 14, 14).permute(0, 2, 3, 1, 4, 5).reshape(32, 588)
    assert same(col, ref.half())
    yy = rnd(2, 1 + 8 * 8, 32, seed=4).half()
    sr = K.sr_im2col(yy.to(DEV), 2, 8, 32).cpu()
    assert same(sr, E.sr_im2col(yy.float(), 2, 8, 32).half())
    w = rnd(24, 16, 9, seed=5)
    r = K.relayout(w.to(DEV), torch.empty(24, 9 * 16, dtype=H16, device=DEV), 24, 16, 9).cpu()
    assert same(r, w.permute(0, 2, 1).reshape(24, 144).half())
    r2 = K.relayout(r.to(DEV), torch.empty(24, 144, dtype=H16, device=DEV), 24, 9, 16).cpu()
    assert same(r2, w.reshape(24, 144).half())
    r3 = K.relayout(r.to(DEV), torch.empty(24, 144, device=DEV), 24, 1, 144).cpu()
    assert torch.equal(r3, r.float())
    xl = rnd(B, N, 320, seed=6) * 3 + 1
    lw, lb = 1 + 0.1 * rnd(320, seed=7), 0.1 * rnd(320, seed=8)
    kl = torch.tensor([320, 200, 64], dtype=torch.int32)
    yl, _, _ = K.ln_fwd(xl.to(DEV), lw.to(DEV), lb.to(DEV), kl.to(DEV), N, 1e-6, H16)
    yr, _, _ = K.ln_fwd(xl.to(DEV), lw.to(DEV), lb.to(DEV), kl.to(DEV), N, 1e-6, torch.float32)
    assert yl.dtype == H16 and within_ulp(yl, yr.cpu(), 1) == 0


def test_eval_stem_kernels_fp16():
    """conv1_direct, im2col3x3 of the image, conv3x3_bias_relu and its _patch form with fp16 operands against conv2d on the same
    fp16 values."""
    B, H, W, m = 2, 56, 56, 24
    img = rnd(B, 3, H, W, seed=1)
    w1 = torch.zeros(m, 32)
    w1[:, :27] = rnd(m, 27, seed=2) * 0.2
    w1 = w1.half()
    t1 = 0.1 * rnd(m, seed=3)
    a1 = K.conv1_direct(img.to(DEV), w1.to(DEV), t1.to(DEV), True, H16)
    wt = w1.float()[:, :27].view(m, 3, 3, 3).permute(0, 3, 1, 2)
    ref1 = torch.relu(torch.nn.functional.conv2d(img.half().float(), wt, stride=2, padding=1) + t1.view(1, m, 1, 1))
    ref1 = ref1.permute(0, 2, 3, 1).reshape(-1, m)
    assert a1.dtype == H16 and relerr(a1, ref1) < 2e-3
    col = K.im2col3x3_image(img.to(DEV), 2, 32, H16)
    a1g = K.gemm(col, w1.to(DEV), torch.empty(col.shape[0], m, dtype=H16, device=DEV), M=col.shape[0], N=m, K=32, lda=32, ldb=32,
                 ldc=m, bias=t1.to(DEV), act=3)
    assert relerr(a1g, ref1) < 2e-3
    Hm, Wm = H // 2, W // 2
    a = a1.cpu()
    w2 = (rnd(m, 9 * m, seed=4) * (9 * m) ** -0.5).half()
    t2 = 0.1 * rnd(m, seed=5)
    ref2 = E.conv3x3_bias_relu(a, w2, t2, a, B, Hm, Wm, m, m, torch.float32)
    out2 = K.conv3x3_bias_relu(a1, w2.to(DEV), t2.to(DEV), a1, B, Hm, Wm, m, m, H16)
    assert out2.dtype == H16 and relerr(out2, ref2) < 2e-3
    outp = K.conv3x3_bias_relu_patch(a1, w2.to(DEV), t2.to(DEV), a1, B, Hm, Wm, m, m, 7, H16).cpu()
    assert torch.equal(outp, K.patch_unfold(out2, B, Hm // 7, Wm // 7, 7, m).cpu())


# ---- 5. model level -----------------------------------------------------------------------------------------------
def _make(name, nd, space, epa, img=224, classes=1000, cfg=None):
    from vitres import supernet_config
    kw = {}
    if space or cfg is not None:
        kw = dict(num_channels_to_keep=cfg if cfg is not None else getattr(supernet_config, space).num_channels_to_keep,
                  example_per_arch=epa, num_warmup_epochs=30)
    return vitres.create_model(name + ("_supernet" if kw else ""), img_size=img, num_classes=classes, network_def=nd,
                               drop_path_rate=0.0, **kw)


MODEL_CASES = {
    "C2_ref_tiny_b128": ("flexible_vit_sr_patch14_224_patch_output", recipe.REF_TINY_DEF, None, 128, 64, 224, 1000, None),
    "C3_sr_tiny_b128": ("flexible_vit_sr_patch14_224_patch_output", recipe.SR_TINY_DEF, "sr_tiny", 128, 64, 224, 1000, None),
    "C4_sr_small_b64": ("flexible_vit_sr_patch14_224_patch_output", recipe.SR_SMALL_DEF, "sr_small", 64, 32, 224, 1000, None),
    "sr_tiny_mh_b32": ("flexible_vit_sr_patch14_224_patch_output", recipe.SR_TINY_MH_DEF, "sr_tiny_mh", 32, 16, 224, 1000, None),
    "distill_micro": ("flexible_vit_sr_distill_patch14_224", recipe.MICRO_DEFS[4], "micro", 8, 2, recipe.MICRO_IMG,
                      recipe.MICRO_CLASSES, None),
    "patch16_micro": ("flexible_vit_patch16_224", recipe.VIT16_DEF, "vit16", 8, 2, recipe.VIT16_IMG, recipe.MICRO_CLASSES, None),
}
MEASURED = {}


def _eval_logits(prod, sd, dt, x, B, space):
    prod.set_compute_dtype(dt)
    prod.load_state_dict(sd)
    with torch.no_grad():
        torch.manual_seed(4)
        out = prod(x)
    out = out[0] if isinstance(out, tuple) else out
    return out.float().cpu(), (torch.stack(prod.last_keeps).clone() if space and prod.last_keeps else None)


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_fp16_eval_logits_vs_fp32_hip_path(name):
    """Eval-mode logits of the fp16 path against the fp32 HIP path on the same weights, inputs and keeps: <= 4e-3 relative and
    <= 0.35x the bf16 path's error measured here (fp16 carries 3 more mantissa bits).  Keep vectors bit-exact."""
    factory, nd, space, B, epa, img, classes, _ = MODEL_CASES[name]
    cfg = {"micro": recipe.micro_keep_config(), "vit16": recipe.vit16_keep_config()}.get(space)
    prod = _make(factory, nd, None if space in ("micro", "vit16") else space, epa, img, classes, cfg=cfg)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in prod.state_dict().items()], 5150)
    prod.load_state_dict(sd)
    prod = prod.to(DEV).eval()
    if space:
        prod.set_epoch(31)
    x = recipe.inputs(21, B, img, classes, 16)[0].to(DEV)
    res = {dt: _eval_logits(prod, sd, dt, x, B, space) for dt in (torch.float32, torch.bfloat16, H16)}
    f, b, h = res[torch.float32], res[torch.bfloat16], res[H16]
    if f[1] is not None:
        assert torch.equal(f[1], h[1]) and torch.equal(f[1], b[1])
    eb, eh = relerr(b[0], f[0]), relerr(h[0], f[0])
    MEASURED[name] = (eb, eh)
    print("%s: logits vs fp32 HIP -- bf16 %.3e, fp16 %.3e (ratio %.3f)" % (name, eb, eh, eh / max(eb, 1e-12)))
    assert torch.isfinite(h[0]).all()
    assert eh <= 4e-3 and eh <= 0.35 * eb, (eb, eh)


# ---- 6. C5 ----------------------------------------------------------------------------------------------------------
def test_c5_candidates_fp16_match_sliced_subnets():
    """The sr_small candidates of the C5 test (resident supernet, conv stem, removed blocks) in fp16 against the prefix-sliced oracle
    sub-networks: <= 5e-3 (bf16's band is 3e-2); score_population runs in fp16."""
    import vitres_oracle as O
    from vitres import evo_eval, supernet_config
    from vitres.network_utils.compute_flop_mac import ComputationEstimator
    from vitres.search_utils import gen_utils
    sp = supernet_config.sr_small
    sup = _make("flexible_vit_sr_patch14_224_patch_output", recipe.SR_SMALL_DEF, "sr_small", 2)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in sup.state_dict().items()], 4444)
    sup.load_state_dict(sd)
    sup = sup.to(DEV).eval().set_compute_dtype(H16)
    est = ComputationEstimator(distill=False, input_resolution=224, patch_size=14)
    np.random.seed(3)
    cands = [gen_utils.gen_random_network_def(sp.network_def, sp.num_channels_to_keep, 2.9e9, est) for _ in range(8)]
    x, _, _, labels = recipe.inputs(31, 4, 224, 1000, 16)
    worst = 0.0
    for ci, nd in enumerate(cands):
        sub = O.OracleViTSR(nd, img_size=224, num_classes=1000, patch_output=True)
        sub.load_state_dict(O.sub_state_dict(sd, sub.state_dict()))
        sub.eval()
        with torch.no_grad():
            want = sub(x)
            got = sup(x.to(DEV), plan=evo_eval.plan_for_subnet(sup, nd, 4))
        want = want[0] if isinstance(want, tuple) else want
        worst = max(worst, relerr(got, want))
        assert relerr(got, want) < 5e-3, (ci, relerr(got, want))
    print("C5 fp16: worst candidate logits vs sliced oracle %.3e" % worst)
    scores = evo_eval.score_population(sup, cands, [(x.to(DEV), labels.to(DEV))])
    assert sup.compute_dtype == H16
    assert len(scores) == 8 and all(0.0 <= s_ <= 100.0 for s_ in scores)


# ---- 7. same kernels ------------------------------------------------------------------------------------------------
def _demangle(names):
    if not any(n.startswith("_Z") for n in names):
        return names
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, timeout=60).stdout.splitlines()
        return out if len(out) == len(names) else names
    except (OSError, subprocess.SubprocessError):
        return names


def _kernel_names(prod, x):
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad():
        prod(x)                                            # (weight shadow cast, workspaces: the steady state is profiled)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            prod(x)
            torch.cuda.synchronize()
    ev = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA), key=lambda e: e.time_range.start)
    return _demangle([e.name for e in ev])


def test_fp16_eval_launches_the_bf16_kernels():
    """One eval forward of C3 in bf16 and in fp16: the same kernels, in the same order, once the element type in the names is
    mapped (bf16_t is `unsigned short` in a kernel's name, the fp16 element type `f16_t`)."""
    factory, nd, space, B, epa, img, classes, _ = MODEL_CASES["C3_sr_tiny_b128"]
    prod = _make(factory, nd, space, epa)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in prod.state_dict().items()], 5150)
    prod.load_state_dict(sd)
    prod = prod.to(DEV).eval()
    prod.set_epoch(31)
    x = recipe.inputs(21, B, img, classes, 16)[0].to(DEV)
    names = {}
    for dt in (torch.bfloat16, H16):
        prod.set_compute_dtype(dt)
        torch.manual_seed(4)
        names[dt] = _kernel_names(prod, x)
    hip = lambda ns: [n for n in ns if "elementwise" not in n.lower() and "copy" not in n.lower()]
    nb = hip(names[torch.bfloat16])
    nh = [n.replace("f16_t", "unsigned short") for n in hip(names[H16])]
    assert len(nb) > 50, nb[:5]
    assert sum("f16_t" in n for n in names[H16]) > 20
    assert nb == nh, [(a, c) for a, c in zip(nb, nh) if a != c][:5]


# ---- 8. switching modes ---------------------------------------------------------------------------------------------
def test_switching_modes_on_a_trained_model():
    from vitres import engine
    from vitres.losses import SoftTargetCrossEntropy
    from vitres.optim import FlatAdamW
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    name, nd = "flexible_vit_sr_patch14_224_patch_output_supernet", recipe.MICRO_DEFS[0]

    def make():
        return vitres.create_model(name, img_size=recipe.MICRO_IMG, num_classes=recipe.MICRO_CLASSES, network_def=nd,
                                   drop_path_rate=0.0, **kw)
    prod = make()
    sd0 = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in prod.state_dict().items()], 100)
    prod.load_state_dict(sd0)
    prod = prod.to(DEV).set_compute_dtype(torch.bfloat16)
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    prod.train()
    prod.set_epoch(31)
    prod.load_state_dict(sd0)
    opt = FlatAdamW(prod, engine.param_groups_weight_decay(prod, 0.05), lr=2e-3)
    opt.own_shadow()
    g = engine.GraphedTrainStep(prod, SoftTargetCrossEntropy(), x, t, pt, "seq", optimizer=opt)
    for it in range(3):
        torch.manual_seed(900 + it)
        opt.prepare_step()
        g(x, t, pt, epoch=31, train_iter=it, arch_sample=None)
    torch.cuda.synchronize()

    def evaluate(m):
        m.eval()
        with torch.no_grad():
            torch.manual_seed(5)
            out = m(x)
        m.train()
        return (out[0] if isinstance(out, tuple) else out).float().cpu()
    L = evaluate(prod)
    prod.set_compute_dtype(H16)
    L16 = evaluate(prod)
    fresh = make()
    fresh.load_state_dict({k: v.detach().cpu() for k, v in prod.state_dict().items()})
    fresh = fresh.to(DEV).set_compute_dtype(H16)
    fresh.set_epoch(31)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in prod.state_dict().items()})
    assert torch.equal(L16, evaluate(fresh))
    assert not torch.equal(L16, L)
    with pytest.raises(NotImplementedError):
        g(x, t, pt, epoch=31, train_iter=3, arch_sample=None)
    prod.set_compute_dtype(torch.bfloat16)
    assert torch.equal(evaluate(prod), L)
    torch.manual_seed(903)
    opt.prepare_step()
    loss = g(x, t, pt, epoch=31, train_iter=3, arch_sample=None)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert torch.equal(prod._arena["shadow"].float(), prod._arena["flat"].bfloat16().float())


# ---- 9. guard --------------------------------------------------------------------------------------------------------
def test_fp16_training_raises_before_anything_is_enqueued():
    from vitres import engine
    from vitres.losses import SoftTargetCrossEntropy
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    prod = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                               num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0, **kw)
    prod = prod.to(DEV).set_compute_dtype(H16)
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    prod.train()
    torch.cuda.synchronize()
    arena_before = prod._arena
    for call in (lambda: prod(x), lambda: prod.loss_and_grad(x, t, pt, "seq"),
                 lambda: engine.GraphedTrainStep(prod, SoftTargetCrossEntropy(), x, t, pt, "seq")):
        with pytest.raises(NotImplementedError, match="fp16 is eval-only; train in bf16 or fp32"):
            call()
    assert prod._arena is arena_before is None           # not even the parameter arena was built
