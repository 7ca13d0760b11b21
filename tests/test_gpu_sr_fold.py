"""The spatial-reduction block's glue passes folded into their consumers, against the launch sequences they replace.

Forward: the conv GEMM adds the pooled shortcut in its epilogue, applies the outer mask last and stores the token-row copies, the token
GEMM adds those as its residual and masks its own term: the result must be the bits of vr_sr_resid -> conv GEMM -> token GEMM ->
vr_mask_rows.  The patch-embedding GEMM stores the token rows of the embedding: the bits of GEMM + vr_embed_cls.

Backward: vr_ln_bwd_sr gathers the LayerNorm backward's dy from the conv data gradient (col2im) and from the token data gradient, and
its dx_in from the incoming gradient (the pooled shortcut's backward): dx_out and gt_out must be the bits of vr_sr_col2im -> token data
gradient -> vr_sr_resid_bwd -> vr_ln_bwd, and dgamma / dbeta (fp32 atomics, any order) must hold the float64 contract of
tests/rowstat_ref64.py under its derived bound.

Loss: vr_softce_train's register kernel adds one atomic per workgroup instead of one per row: its gradient must be the bits recorded
from the kernel before that change, its loss sum within the soft-CE contract's bound."""
import os

import numpy as np
import pytest
import torch

import rowstat_ref64 as R
import vitres.functional as F
import vitres.kernels as K
from vitres import _lib
from test_gpu_model import _micro_bf16_step, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF = torch.bfloat16

# g = 2: one pooled pixel, every tap row at an edge; g = 4: odd rows / columns with both taps and the bottom / right edge without.
# B = 3: 15 - 54 rows, fewer than a tile; B = 33 at g = 4: 132 pooled patch rows (across a 128-row tile), 561 / 594 input rows.
# Input rows: 15, 18, 51, 54, 561, 594 -- none a multiple of vr_ln_bwd's 4 rows per workgroup: the last workgroup is always partial.
GRID = [(B, g, T, Cin, Cout) for (B, g) in ((3, 2), (3, 4), (33, 4)) for T in (1, 2) for (Cin, Cout) in ((64, 64), (64, 128))]


def mixed_keep(B, C, start=0):
    """per-sample keep counts: 0, a value that is no multiple of 8 (40) and the full width"""
    vals = [C, 40, 0, C - 8, 24]
    return torch.tensor([vals[(start + i) % len(vals)] for i in range(B)], dtype=torch.int32, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def poison(shape):
    """leave a freed NaN block of this fp32 shape with the caching allocator: the torch.empty of the same size that follows gets it (the
    other form's result is still alive, so it cannot be handed out again and pass for rows nobody wrote)"""
    t = torch.full(shape, NAN, device=DEV)
    torch.cuda.synchronize()
    del t


def launches(monkeypatch, names):
    """count the calls of vitres.kernels.<name> from here on -> dict name -> [count]"""
    seen = {}
    for name in names:
        fn, cnt = getattr(K, name), [0]

        def wrap(*a, _fn=fn, _cnt=cnt, **kw):
            _cnt[0] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(K, name, wrap)
        seen[name] = cnt
    return seen


# ---- forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, torch.float16])
@pytest.mark.parametrize("B,g,T,Cin,Cout", GRID)
def test_sr_fwd_folded_is_resid_gemm_gemm_mask(B, g, T, Cin, Cout, dt, monkeypatch):
    gen = torch.Generator().manual_seed(7000 + 100 * B + 10 * g + T + Cout)
    P, Ni, No = (g // 2) ** 2, T + g * g, T + (g // 2) ** 2
    x = (torch.rand(B, Ni, Cin, generator=gen) - 0.4).to(DEV)
    rnd = lambda *sh, sc=1.0: (sc * torch.randn(*sh, generator=gen)).to(DEV)
    wr, wt = rnd(Cout, 9 * Cin, sc=0.05).to(dt), rnd(Cout, Cin, sc=0.1).to(dt)
    p = {"nw": 1 + rnd(Cin, sc=0.1), "nb": rnd(Cin, sc=0.1), "pos": rnd(P, Cout, sc=0.02),
         "reduce": F.Weights(None, rnd(Cout, sc=0.1), wr, 9 * Cin), "token": F.Weights(None, rnd(Cout, sc=0.1), wt, Cin)}
    cfg = {"grid": g, "tokens": T, "cout": Cout, "dtype": dt, "eps": R.EPS}
    embed_keep = mixed_keep(B, Cin, start=1)
    for new_keep in (mixed_keep(B, Cout), None):
        outs = {}
        for fuse in (False, True):
            with monkeypatch.context() as m:
                m.setattr(F, "FUSE_SR", fuse)
                seen = launches(m, ["sr_resid", "mask_rows"])
                poison((B, No, Cout))
                out, _ = F.sr_fwd(x, p, cfg, embed_keep, new_keep, False)
                torch.cuda.synchronize()
                assert seen["sr_resid"][0] == (0 if fuse else 1) and seen["mask_rows"][0] == (0 if fuse or new_keep is None else 1)
            outs[fuse] = out
        assert torch.isfinite(outs[True]).all()
        assert torch.equal(bits(outs[True]), bits(outs[False])), (B, g, T, Cin, Cout, new_keep is None)
        if new_keep is not None:
            cols = torch.arange(Cout, device=DEV)[None, None, :] >= new_keep.long()[:, None, None]
            assert float(outs[True][cols.expand(B, No, Cout)].abs().max()) == 0.0          # (B = 3 holds keep 0, 40 and Cout)


@pytest.mark.parametrize("dt", [BF, torch.float16])
@pytest.mark.parametrize("B,P,T,C", [(3, 4, 1, 64), (3, 16, 2, 64), (33, 4, 2, 64), (5, 49, 1, 136), (130, 1, 2, 64)])
def test_embedding_token_rows_from_the_patch_gemm(B, P, T, C, dt, monkeypatch):
    """(130, 1, 2): one patch per sample -- a 128-row tile holds the first rows of 128 samples, the next tile those of two"""
    gen = torch.Generator().manual_seed(9000 + B + P + T + C)
    ldk = 56
    col = torch.randn(B * P, ldk, generator=gen).to(dt).to(DEV)
    rnd = lambda *sh, sc=1.0: (sc * torch.randn(*sh, generator=gen)).to(DEV)
    p = {"proj": F.Weights(None, rnd(C, sc=0.1), rnd(C, ldk, sc=0.1).to(dt), ldk), "pos": rnd(1, P + T, C, sc=0.02), "tokens": rnd(1, T, C)}
    cfg = {"tokens": T, "patches": P, "dim": C, "dtype": dt, "patch": 4}
    img = torch.zeros(B, 1, device=DEV)
    for keep in (mixed_keep(B, C), None):
        outs = {}
        for fuse in (False, True):
            with monkeypatch.context() as m:
                m.setattr(F, "FUSE_SR", fuse)
                seen = launches(m, ["embed_cls"])
                poison((B, P + T, C))
                out, _ = F.embed0_fwd(img, p, cfg, keep, False, col=col)
                torch.cuda.synchronize()
                assert seen["embed_cls"][0] == (0 if fuse else 1)
            outs[fuse] = out
        assert torch.isfinite(outs[True]).all()                        # every row written, token rows included
        assert torch.equal(bits(outs[True]), bits(outs[False])), (B, P, T, C, keep is None)


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def sr_bwd_inputs(B, g, T, Cin, Cout):
    gen = torch.Generator().manual_seed(1000 * B + 100 * g + 10 * T + Cout)
    P, Ni, No = (g // 2) ** 2, T + g * g, T + (g // 2) ** 2
    x, w, b = R.ln_inputs(B + g + T + Cout, B * Ni, Cin)
    x = x.view(B, Ni, Cin).to(DEV)
    keep = mixed_keep(B, Cin)
    _, mean, rstd = K.ln_fwd(x, w.to(DEV), b.to(DEV), keep, Ni, R.EPS, BF)
    dcol = torch.randn(B * P, 9 * Cin, generator=gen).to(BF).to(DEV)
    gt = torch.randn(B, No, Cout, generator=gen).to(BF).to(DEV)              # the masked, cast incoming gradient the token Linear reads
    wt = (0.1 * torch.randn(Cout, Cin, generator=gen)).to(BF).to(DEV)        # token Linear weight [out, in]
    gout = torch.randn(B, No, Cout, generator=gen).to(DEV)
    nc = (torch.tensor([1.0, 0.0, 1.25, 0.5])[torch.arange(B) % 4].contiguous().to(DEV), mixed_keep(B, Cin, start=3))
    return x, w.to(DEV), keep, mean, rstd, dcol, gt, wt, gout, nc


@pytest.mark.parametrize("copies", [1, 64])
@pytest.mark.parametrize("B,g,T,Cin,Cout", GRID)
def test_ln_bwd_sr_is_col2im_token_dgrad_resid_bwd_ln_bwd(B, g, T, Cin, Cout, copies):
    x, w, keep, mean, rstd, dcol, gt, wt, gout, nc = sr_bwd_inputs(B, g, T, Cin, Cout)
    Ni, No, M = T + g * g, T + (g // 2) ** 2, B * (T + g * g)
    assert M % R.ln_bwd_path(M, Cin, copies)[2] != 0                         # a partial last workgroup
    tok = dict(M=B * T, N=Cin, K=Cout, lda=Cout, ldb=Cin, b_trans=True, a_map=(T, No, 0), rows_in=T)
    # the sequence it replaces
    dy = torch.full((B, Ni, Cin), NAN, dtype=BF, device=DEV)
    K.sr_col2im(dcol, dy, B, g, Cin, T)
    K.gemm(gt, wt, dy, ldc=Cin, c_map=(T, Ni, 0), **tok)
    gres = K.sr_resid_bwd(gout, B, g, Cin, Cout, T)
    part = torch.zeros(2, copies, Cin, device=DEV)
    dx, gto = K.ln_bwd(dy, x, w, mean, rstd, keep, Ni, gres, part[0], part[1], next_cast=nc, copies=copies)
    # the folded form
    dy_tok = torch.full((B * T, Cin), NAN, dtype=BF, device=DEV)
    K.gemm(gt, wt, dy_tok, ldc=Cin, **tok)
    part2 = torch.zeros(2, copies, Cin, device=DEV)
    dx2, gto2 = K.ln_bwd_sr(dcol, dy_tok, gout, x, w, mean, rstd, keep, g, T, part2[0], part2[1], next_cast=nc, copies=copies)
    torch.cuda.synchronize()
    assert torch.equal(dy[:, :T].reshape(B * T, Cin), dy_tok)
    assert torch.isfinite(dx2).all() and torch.equal(dx2, dx)
    assert torch.equal(gto2.view(torch.int16), gto.view(torch.int16))
    # dgamma / dbeta of both forms against the float64 contract, through the fold of the partial rows when there are any
    ref = R.layernorm_bwd64(dy.reshape(M, Cin), x.reshape(M, Cin), w, mean, rstd, keep, Ni, gres.reshape(M, Cin))
    for tag, pr in (("separate", part), ("folded", part2)):
        dw, db = torch.zeros(Cin, device=DEV), torch.zeros(Cin, device=DEV)
        if copies > 1:
            K.ln_grad_reduce([(pr[0], pr[1], dw, db)], copies)
        else:
            dw, db = pr[0, 0], pr[1, 0]
        torch.cuda.synchronize()
        r = R.check_ln_bwd(dx2, dw, db, ref, Cin, copies)
        print("SRFOLD ln_bwd_sr B%d g%d T%d %d->%d copies%d %s: %s" % (B, g, T, Cin, Cout, copies, tag,
                                                                      " ".join("%s=%.3f" % kv for kv in r.items())))
        assert all(v <= 1.0 for v in r.values()), (tag, r)


def test_ln_bwd_sr_refuses_what_it_cannot_read():
    B, g, T, Cin, Cout = 3, 4, 1, 64, 64
    x, w, keep, mean, rstd, dcol, gt, wt, gout, nc = sr_bwd_inputs(B, g, T, Cin, Cout)
    dy_tok = torch.zeros(B * T, Cin, dtype=BF, device=DEV)
    dx, dw, db = torch.empty_like(x), torch.zeros(Cin, device=DEV), torch.zeros(Cin, device=DEV)

    def call(g_, C_, Cout_):
        return _lib.lib().vr_ln_bwd_sr(K._p(dcol), K._p(dy_tok), K._p(gout), K._p(x), K._p(w), K._p(mean), K._p(rstd), K._p(keep), K._p(dx),
                                       K._p(dw), K._p(db), None, None, None, B, g_, C_, Cout_, T, 1, K._stream())
    assert call(3, Cin, Cout) == -3 and call(g, 36, Cout) == -3 and call(g, Cin, 32) == -3 and call(g, Cin, 66) == -3
    assert call(g, Cin, Cout) == 0
    torch.cuda.synchronize()


def test_fuse_sr_at_model_level(monkeypatch):
    """One bf16 training step of the micro supernet with the folded spatial-reduction kernels (the default) and with the launch
    sequence they replace: masks, logits and loss are equal -- nothing on the way to them is summed by atomics -- and every parameter
    gradient stays inside the band test_opt_in_forms_at_model_level gives the atomic-summed weight gradients."""
    assert F.FUSE_SR is True
    glue = ["sr_resid", "mask_rows", "sr_col2im", "sr_resid_bwd", "embed_cls", "ln_bwd_sr"]
    with monkeypatch.context() as m:
        seen = launches(m, glue)
        ref = _micro_bf16_step()
    assert seen["ln_bwd_sr"][0] >= 1 and all(seen[k][0] == 0 for k in glue[:-1]), {k: v[0] for k, v in seen.items()}
    with monkeypatch.context() as m:
        m.setattr(F, "FUSE_SR", False)
        seen = launches(m, glue)
        got = _micro_bf16_step()
    assert seen["ln_bwd_sr"][0] == 0 and all(seen[k][0] >= 1 for k in glue[:-1]), {k: v[0] for k, v in seen.items()}
    assert len(got["keeps"]) == len(ref["keeps"])
    for a, b in zip(got["keeps"], ref["keeps"]):
        assert (a is None and b is None) or torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    assert torch.equal(got["cls"], ref["cls"]) and torch.equal(got["pat"], ref["pat"]) and got["loss"] == ref["loss"]
    worst = max(rel(g, ref["grads"][n]) for n, g in got["grads"].items())
    print("SRFOLD model step: worst gradient rel %.2e" % worst)
    assert worst < 2e-2, worst


# ---- soft-target cross entropy: one loss atomic per workgroup ---------------------------------------------------------------------------
SOFTCE_GOLDEN = "sr_fold_softce_train.npz"
SOFTCE_CASES = [(9, 1000, 1), (66, 1000, 4), (5, 256, 1)]     # (rows, classes, rows per sample): 9 and 5 leave the last workgroup short


def softce_case(Rn, Kc, rps):
    B = (Rn + rps - 1) // rps
    x = R.softce_logits("randn2", 31 * Kc + Rn, Rn, Kc)
    t = R.softce_targets("smooth", 31 * Kc + Rn + 1, B * rps, Kc)
    smap = torch.randperm(B, generator=torch.Generator().manual_seed(Rn + Kc))
    return x, t, smap


def run_softce_train(x, t, smap, rps, dt, acc0=0.5):
    Rn, Kc = x.shape
    ld = R.softce_ld(Kc)
    d = torch.full((Rn, ld), NAN, dtype=dt, device=DEV)
    acc = torch.full((1,), acc0, device=DEV)
    xd, td, sd = x.to(DEV), t.to(DEV), smap.to(DEV)
    rc = _lib.lib().vr_softce_train(K._p(xd), K._p(td), K._p(sd), rps, K._p(acc), K._p(d), ld, K._dtcode(dt), Rn, Kc, 1.0 / Rn, 1.0 / Rn,
                                    K._stream())
    torch.cuda.synchronize()
    assert rc == 0
    return d, acc


@pytest.mark.parametrize("Rn,Kc,rps", SOFTCE_CASES)
def test_softce_train_gradient_bits_and_loss_sum(Rn, Kc, rps):
    """dlogits: the bits vr_softce_train's register kernel produced before its loss atomics were gathered per workgroup (recorded on an
    MI355X from that kernel on softce_case's inputs; the gradient does not depend on how the loss is summed).  loss_acc: the float64
    sum under rowstat_ref64.softce_bounds -- its R roundings relative to the partial sum bound any order of the R terms, also the
    (w0 + w1) + (w2 + w3) of a workgroup followed by one atomic."""
    assert R.softce_train_path(Kc, R.softce_ld(Kc)) == "reg"
    gold = np.load(os.path.join(G, SOFTCE_GOLDEN))
    x, t, smap = softce_case(Rn, Kc, rps)
    ref = R.softce_train64(x, t, smap, rps, R.softce_ld(Kc), 1.0 / Rn, 1.0 / Rn, 0.5)
    for dt, key in ((torch.float32, "f32"), (BF, "bf16")):
        d, acc = run_softce_train(x, t, smap, rps, dt)
        want = torch.from_numpy(gold["%s_R%d_K%d" % (key, Rn, Kc)])
        got = d.cpu().view(torch.int32 if dt == torch.float32 else torch.int16)
        assert torch.equal(got, want), (Rn, Kc, key)
        bd = R.softce_bounds(ref, R.unit_roundoff(dt))
        r = R.worst_ratio(acc, ref["acc"], bd["acc"])
        print("SRFOLD softce R%d K%d %s: acc ratio %.3f" % (Rn, Kc, key, r))
        assert r <= 1.0, r
