"""vr_attn_fwd / vr_attn_bwd against the float64 contract of tests/attn_ref64.py: per-element derived bounds at every dispatch
boundary of N, grids that switch the XCD block remap on, and structural probes (uniform rows, permutation routing, logit edges,
repeatability).  Output buffers belong to the test and start as NaN: a row nobody writes fails.  The backward is tested in isolation
on o_in = round(o64), lse_in = fp32(lse64); one case chains the forward kernel's own o and lse into it as the product does."""
import pytest
import torch

import attn_ref64 as R
import vitres.kernels as K
from vitres import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def attn_fwd(qkv, keep, B, N, H, D, scale):
    """K.attn_fwd on NaN-filled outputs owned by the caller; returns the raw status too (0 = VR_OK)"""
    o = torch.full((B, N, H * D), NAN, dtype=qkv.dtype, device=DEV)
    lse = torch.full((B, H, N), NAN, dtype=torch.float32, device=DEV)
    rc = _lib.lib().vr_attn_fwd(K._p(qkv), K._p(o), K._p(lse), K._p(keep), B, N, H, D, scale, K._dt(qkv), K._stream())
    torch.cuda.synchronize()
    return rc, o, lse


def attn_bwd(qkv, o, d_o, lse, keep, B, N, H, D, scale):
    dqkv = torch.full_like(qkv, NAN)
    delta = torch.full((B, H, N), NAN, dtype=torch.float32, device=DEV)
    rc = _lib.lib().vr_attn_bwd(K._p(qkv), K._p(o), K._p(d_o), K._p(lse), K._p(delta), K._p(dqkv), K._p(keep), B, N, H, D, scale,
                                K._dt(qkv), K._stream())
    torch.cuda.synchronize()
    return rc, dqkv


def all_finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


def run_case(tag, qkv, d_o, keep, B, N, H, D, backward=True):
    """forward and isolated backward of one input against the bounds -> (ratios, o, lse, dqkv); asserts ratio <= 1 and finiteness"""
    scale = D ** -0.5
    u = R.unit_roundoff(qkv.dtype)
    ref = R.forward64(qkv, keep, B, N, H, D, scale)
    kd = keep.to(DEV) if keep is not None else None
    rc, o, lse = attn_fwd(qkv.to(DEV), kd, B, N, H, D, scale)
    assert rc == 0, rc
    r = R.check_forward(o, lse, qkv, keep, B, N, H, D, scale, u, ref=ref)
    dqkv = None
    if backward:
        o_in, lse_in = R.unheads(ref[3]).to(qkv.dtype), ref[1].float()
        rc, dqkv = attn_bwd(qkv.to(DEV), o_in.to(DEV), d_o.to(DEV), lse_in.to(DEV), kd, B, N, H, D, scale)
        assert rc == 0, rc
        r.update(R.check_backward(dqkv, qkv, o_in, d_o, lse_in, keep, B, N, H, D, scale, u))
    print("ATTNRATIO %s B%d N%d H%d D%d %s: %s" % (tag, B, N, H, D, str(qkv.dtype)[6:], " ".join("%s=%.3f" % kv for kv in r.items())))
    assert all(v <= 1.0 for v in r.values()), r
    assert all_finite(o, lse) and (dqkv is None or all_finite(dqkv))
    return r, o, lse, dqkv


# ---- a. random inputs at the dispatch boundaries of N ----------------------------------------------------------------------------
# N -> head dims; every (size class, D) pair is hit: NKP = 1 (N <= 32), NKP = 3 (33..96: FULL above 64), NKP = 9 (97..288: FULL above
# 256; D = 32 takes the one-launch backward there), and the long kernels (N > 288: 128-query workgroups, 256-key blocks)
BF16_ND = {1: (32,), 2: (48,), 15: (64,), 16: (32,), 17: (32, 48, 64), 31: (48,), 32: (64,), 33: (32, 64), 64: (48,),
           65: (32, 48, 64), 95: (32,), 96: (48,), 97: (64,), 128: (32,), 129: (48,), 255: (64,), 256: (32,), 257: (32, 48, 64),
           287: (48,), 288: (64,), 289: (32,), 384: (48,), 385: (64,), 512: (32,), 513: (48,), 785: (64,)}
# the fp32 kernels of attn.hip: N <= 320 and the head's K, V (+ scratch) within 160 KB of LDS, which D = 64 leaves at N >= 287
F32_ND = {1: (16,), 2: (32,), 15: (48,), 16: (64,), 17: (16, 32, 48, 64), 31: (16,), 32: (32,), 33: (48,), 64: (64,),
          65: (16, 32, 48, 64), 95: (16,), 96: (32,), 97: (48,), 128: (64,), 129: (16,), 255: (32,), 256: (48,),
          257: (16, 32, 48, 64), 287: (16,), 288: (32,), 289: (48,)}


def nd_cases(table):
    return [(n, d) for n, ds in table.items() for d in ds]


@pytest.mark.parametrize("qscale", [1.0, 3.0])
@pytest.mark.parametrize("N,D", nd_cases(BF16_ND))
def test_random_bf16_boundary_n(N, D, qscale):
    B, H = 2, 2
    qkv, d_o = R.random_inputs(1000 + 7 * N + D, B, N, H, D, qscale)
    run_case("a-bf16-s%g" % qscale, qkv, d_o, torch.tensor([H * D, D], dtype=torch.int32), B, N, H, D)


@pytest.mark.parametrize("qscale", [1.0, 3.0])
@pytest.mark.parametrize("N,D", nd_cases(F32_ND))
def test_random_fp32_boundary_n(N, D, qscale):
    B, H = 2, 2
    qkv, d_o = R.random_inputs(2000 + 7 * N + D, B, N, H, D, qscale, dtype=torch.float32)
    run_case("a-fp32-s%g" % qscale, qkv, d_o, torch.tensor([H * D, D], dtype=torch.int32), B, N, H, D)


def test_fp32_beyond_320_is_unsupported():
    B, N, H, D = 2, 321, 2, 32
    qkv, d_o = R.random_inputs(1, B, N, H, D, dtype=torch.float32)
    qkv, d_o = qkv.to(DEV), d_o.to(DEV)
    rc, o, lse = attn_fwd(qkv, None, B, N, H, D, D ** -0.5)
    assert rc == -3                                                     # VR_EUNSUPPORTED, nothing launched
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(lse).all())
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        _lib.check(rc, "vr_attn_fwd")
    rc, dqkv = attn_bwd(qkv, torch.zeros_like(d_o), d_o, torch.zeros(B, H, N, device=DEV), None, B, N, H, D, D ** -0.5)
    assert rc == -3 and bool(torch.isnan(dqkv).all())
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.attn_fwd(qkv, None, B, N, H, D, D ** -0.5)


@pytest.mark.parametrize("qscale", [1.0, 3.0])
@pytest.mark.parametrize("D", [32, 48, 64])
@pytest.mark.parametrize("N", [17, 65, 257, 289])
def test_random_fp16_forward(N, D, qscale):
    B, H = 2, 2
    qkv, d_o = R.random_inputs(3000 + 7 * N + D, B, N, H, D, qscale, dtype=torch.float16)
    run_case("a-fp16-s%g" % qscale, qkv, d_o, torch.tensor([H * D, D], dtype=torch.int32), B, N, H, D, backward=False)


@pytest.mark.parametrize("N,D", [(65, 48), (257, 64), (257, 32), (385, 32)])
def test_forward_chained_into_backward(N, D):
    """the product's use: the backward consumes the forward kernel's own o and lse -- and is held to the contract on THOSE inputs"""
    B, H, scale = 2, 2, D ** -0.5
    keep = torch.tensor([H * D, D], dtype=torch.int32)
    qkv, d_o = R.random_inputs(4000 + N + D, B, N, H, D)
    rc, o, lse = attn_fwd(qkv.to(DEV), keep.to(DEV), B, N, H, D, scale)
    assert rc == 0
    rc, dqkv = attn_bwd(qkv.to(DEV), o, d_o.to(DEV), lse, keep.to(DEV), B, N, H, D, scale)
    assert rc == 0
    r = R.check_backward(dqkv, qkv, o.cpu(), d_o, lse.cpu(), keep, B, N, H, D, scale, 2.0 ** -8)
    print("ATTNRATIO a-chain B%d N%d H%d D%d: %s" % (B, N, H, D, " ".join("%s=%.3f" % kv for kv in r.items())))
    assert all(v <= 1.0 for v in r.values()), r
    assert all_finite(o, lse, dqkv)


# ---- b. grids of 15 .. 27 workgroups: the XCD block remap (identity below 16) ----------------------------------------------------
@pytest.mark.parametrize("B,H", [(8, 2), (17, 1), (5, 3), (23, 1), (8, 3), (9, 3)])
@pytest.mark.parametrize("N,D", [(17, 64), (65, 48), (65, 32), (17, 32)])
def test_xcd_remapped_grids(N, D, B, H):
    """every sample has its own data (one generator stream over the whole batch) and its own keep, so a workgroup that picks up
    another one's (b, h) is a per-element mismatch; dropped heads (bound 0) must be exact zeros in o, lse and the three gradients"""
    qkv, d_o = R.random_inputs(5000 + 100 * B + 10 * H + N + D, B, N, H, D)
    cyc = [H * D, D, 0, -(H * D + 2)]
    keep = torch.tensor([cyc[b % 4] for b in range(B)], dtype=torch.int32)
    r, o, lse, dqkv = run_case("b-grid%d" % (B * H), qkv, d_o, keep, B, N, H, D)
    dropped = ~R.kept_mask(keep, B, H, D)
    assert bool(dropped.any())
    gq, gk, gv = R.split_qkv(dqkv, B, N, H, D)
    for t in (R.heads(o, H, D), gq, gk, gv):
        assert float(t[dropped].abs().max()) == 0.0
    assert float(lse.cpu()[dropped].abs().max()) == 0.0


# ---- c. uniform rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(17, 64), (65, 48), (96, 32), (257, 32), (257, 64), (289, 48), (513, 32)])
def test_uniform_rows_count_every_key_and_query_once(N, D):
    import math
    B, H = 2, 2
    qkv, d_o = R.uniform_inputs(6000 + N + D, B, N, H, D)
    s, lse64, P, o64 = R.forward64(qkv, None, B, N, H, D, D ** -0.5)
    cnt = torch.bincount(torch.arange(N) % D, minlength=D).double() / N
    assert float(s.abs().max()) == 0.0 and float((lse64 - math.log(N)).abs().max()) < 1e-12
    assert float((o64 - cnt).abs().max()) < 1e-12                       # the reference states the counting argument
    r, o, lse, dqkv = run_case("c-uniform", qkv, d_o, None, B, N, H, D)
    assert float(R.split_qkv(dqkv, B, N, H, D)[1].abs().max()) == 0.0   # dK = dS^T q with q = 0


# ---- d. permutation routing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(1, 32), (2, 64), (17, 64), (33, 32), (65, 48), (257, 32), (257, 64), (288, 32), (401, 32), (785, 64)])
def test_permutation_routing_is_bit_exact(N, D):
    B, H, scale = 2, 2, D ** -0.5
    qkv, d_o, pi = R.permutation_inputs(7000 + N + D, B, N, H, D)
    # the test is sound on the reference alone: a 20-logit margin, and the rounded float64 results are the routed rows
    s, lse64, P, o64 = R.forward64(qkv, None, B, N, H, D, scale)
    if N > 1:
        top2 = s.topk(2, dim=-1).values
        assert float((top2[..., 0] - top2[..., 1]).min()) >= 20.0
    assert torch.equal(s.argmax(-1), pi)
    v = R.split_qkv(qkv, B, N, H, D)[2]
    idx = lambda p: p[..., None].expand(B, H, N, D)
    v_pi = torch.gather(v, 2, idx(pi))
    do_inv = torch.gather(R.heads(d_o, H, D), 2, idx(torch.argsort(pi, dim=-1)))
    o_in, lse_in = R.unheads(o64).to(torch.bfloat16), lse64.float()
    _, _, dQ, dK, dV = R.backward64(qkv, o_in, d_o, lse_in, None, B, N, H, D, scale)
    assert torch.equal(o_in, R.unheads(v_pi).to(torch.bfloat16)) and torch.equal(R.heads(o_in, H, D), v_pi)
    assert torch.equal(dV.to(torch.bfloat16).double(), do_inv)
    assert float(dQ.abs().max()) < 1e-6 and float(dK.abs().max()) < 1e-6
    r, o, lse, dqkv = run_case("d-perm", qkv, d_o, None, B, N, H, D)
    assert torch.equal(R.heads(o, H, D), v_pi)
    assert torch.equal(R.split_qkv(dqkv, B, N, H, D)[2], do_inv)


# ---- e. logit edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["neg", "pos", "mixed"])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("N", [17, 65, 257, 289])
def test_logit_edges(N, D, kind):
    """Ordinary finite bf16 data whose logits are far from zero.  'neg': every logit < -100, so lse < -88.7 and exp(-lse) -- the P a
    kernel computes for a zero-padded key -- overflows fp32; softmax is shift invariant and the float64 gradients are ~0.1."""
    B, H, scale = 2, 2, D ** -0.5
    qkv, d_o = R.logit_edge_inputs(kind, 8000 + N + D, B, N, H, D)
    s, lse64, P, o64 = R.forward64(qkv, None, B, N, H, D, scale)
    if kind == "neg":
        assert float(s.max()) < -100.0
    elif kind == "pos":
        assert float(s.min()) > 100.0
    else:
        assert float(s[:, :, 0, 0].min()) > 75.0 and (N == 1 or float(s[:, :, 0, 1:].max()) < -75.0)
    grads = R.backward64(qkv, R.unheads(o64).to(torch.bfloat16), d_o, lse64.float(), None, B, N, H, D, scale)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) < 1e30 for t in (s, lse64, P, o64) + tuple(grads))
    assert float(grads[2].abs().max()) > 1e-3                            # a real gradient, not an underflowed one
    run_case("e-" + kind, qkv, d_o, None, B, N, H, D)


# ---- f. repeatability ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(65, 48), (257, 64), (257, 32)])
def test_repeatable_bit_for_bit(N, D):
    B, H, scale = 8, 3, D ** -0.5                                       # 24 workgroups: remapped
    qkv, d_o = R.random_inputs(9000 + N + D, B, N, H, D)
    qkv, d_o = qkv.to(DEV), d_o.to(DEV)
    keep = torch.tensor([H * D, D] * (B // 2), dtype=torch.int32, device=DEV)
    rc, o1, l1 = attn_fwd(qkv, keep, B, N, H, D, scale)
    rc2, o2, l2 = attn_fwd(qkv, keep, B, N, H, D, scale)
    assert rc == 0 and rc2 == 0 and torch.equal(o1, o2) and torch.equal(l1, l2)
    rc, g1 = attn_bwd(qkv, o1, d_o, l1, keep, B, N, H, D, scale)
    rc2, g2 = attn_bwd(qkv, o1, d_o, l1, keep, B, N, H, D, scale)
    assert rc == 0 and rc2 == 0 and torch.equal(g1, g2)
    assert all_finite(o1, l1, g1)
