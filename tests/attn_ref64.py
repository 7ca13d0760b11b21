"""float64 statement of the attention contract (vr_attn_fwd / vr_attn_bwd) with derived per-element error bounds.  CPU only.

The contract
------------
qkv is [B, N, 3, H, D] (q, k, v of every head), o is [B, N, H * D], lse is fp32 [B, H, N].  For a kept head (h * D < keep_hd[b])

    s = scale * q k^T,   lse_i = log sum_j exp(s_ij),   P = exp(s - lse),   o = P v

and the backward, as a function of the tensors it is HANDED (o_in and lse_in are inputs, not recomputed):

    P     = exp(s - lse_in)
    delta = rowsum(dO * o_in)
    dS    = P * (dO v^T - delta) * scale
    dQ = dS k,   dK = dS^T q,   dV = P^T dO

A dropped head (h * D >= keep_hd[b]: this covers keep = 0 and the negative DropPath encoding -(k + 2)) gives o = 0, lse = 0 and
zero gradients.  Everything here is float64 on exact upcasts of the bf16 / fp16 / fp32 tensors the kernel gets; tensors are returned in
head layout [B, H, N, D] (`heads` / `split_qkv` convert the kernel's layouts).  backward64 is the explicit formula, not autograd
through a recomputed o: once o_in is rounded to 16 bits the two differ by 5e-4 .. 6e-3 of max|dQ|, and that difference belongs to the
caller of the kernel, not to the kernel.

The bounds
----------
u is the unit roundoff of the 16-bit type (2^-8 bf16, 2^-11 fp16, 0 on the fp32 path).  The kernels round in these places and
nowhere else: the forward rounds the unnormalised p <= 1 (the P operand of the P v MFMA) and the final o; the backward rounds P (operand
of dV), dS (operand of dQ and dK) and the three outputs.  All sums are fp32.

fp32 slack.  The exponent x_ij = s_ij - lse_i is formed in fp32 from a dot product of D exact products (the operands are 16-bit, their
products are exact in fp32) accumulated linearly, |fl(q.k) - q.k| <= D 2^-24 |q|.|k| (1 + ...) <= D 2^-23 |q|.|k| (|q|.|k| is the dot
product of the absolute values), then scaled; s * c, lse * log2(e) and the exp2 itself round once each, relative to |s|, |lse| and 1:

    eps_ij = D 2^-23 (|q_i| . |k_j|) scale + 2^-22 (|s_ij| + |lse_i| + 1)          absolute error of the exponent
    gamma  = D 2^-23                                                             relative error of the dO.v and dO.o dot products

so the computed P is P (1 + theta), |theta| <= eps (first order; eps <= 1e-3 on every input of the suite).

forward.  o = sum_j p_j v_j / sum_j p_j with p_j = exp(s_j - m).  Rounding p_j in the numerator costs u p_j |v_j| each, i.e. u (P |v|)
after normalisation; rounding o costs u |o|; the exponent error moves numerator and denominator by (P o eps) each, the denominator's
share multiplies |o| <= P |v|:

    |o - o64|     <= 2 u (|o64| + P |v|) + 2 (P o eps) |v|
    |lse - lse64| <= 2 max_j eps_ij + 2^-19        (m * scale, log(sum) and their sum round in fp32; sum is a mean of (1 + theta))

backward.  dV = P^T dO: rounding P costs u P^T |dO|, the output u |dV|, the exponent (P o eps)^T |dO|:

    |dV - dV64| <= 2 u (P^T |dO| + |dV64|) + (P o eps)^T |dO|

dS = P (dP - delta) scale with dP = dO v^T: P carries eps, dP and delta carry gamma relative to their absolute sums:

    E = |dS| o eps + P scale gamma (|dO| |v|^T + rowsum(|dO| |o_in|))
    |dQ - dQ64| <= 2 u (|dS| |k| + |dQ64|) + E |k|
    |dK - dK64| <= 2 u (|dS|^T |q| + |dK64|) + E^T |q|

The factor 2 on the u terms is the only margin: with factor 1 a float64 emulation of exactly these roundings reaches 0.33 .. 0.93 of
the bound (tests/test_attention_ref_host.py), so 2 is the smallest round number with headroom, and far below what a structural error
(a key dropped, counted twice, routed to the wrong slot) produces.  Every element is checked: `worst_ratio` returns max |got - ref| /
bound over the whole tensor, with 0 / 0 = 0 and x / 0 = inf (dropped heads and exactly-zero results have bound 0: they must be exact),
and inf for any non-finite element.
"""
import math

import torch

F64 = torch.float64


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}[dtype]


def heads(x, H, D):
    """[B, N, H * D] -> float64 [B, H, N, D]"""
    B, N = x.shape[0], x.shape[1]
    return x.detach().cpu().to(F64).reshape(B, N, H, D).permute(0, 2, 1, 3).contiguous()


def unheads(x):
    """[B, H, N, D] -> [B, N, H * D]"""
    B, H, N, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * D).contiguous()


def split_qkv(qkv, B, N, H, D):
    """[B, N, 3 * H * D] -> three float64 [B, H, N, D]"""
    # (not detached: the host test differentiates through forward64)
    x = qkv.cpu().to(F64).reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4).contiguous()
    return x[0], x[1], x[2]


def kept_mask(keep_hd, B, H, D):
    """bool [B, H]: head h of sample b is kept iff h * D < keep_hd[b] (None: dense)"""
    if keep_hd is None:
        return torch.ones(B, H, dtype=torch.bool)
    k = keep_hd.detach().cpu().to(torch.int64).reshape(B, 1)
    return (torch.arange(H).reshape(1, H) * D) < k


def _mask4(kept):
    return kept.to(F64)[:, :, None, None]


def forward64(qkv, keep_hd, B, N, H, D, scale):
    """-> s [B,H,N,N], lse [B,H,N], P [B,H,N,N], o [B,H,N,D]; dropped heads: o = 0, lse = 0 (s and P are left as computed)."""
    q, k, v = split_qkv(qkv, B, N, H, D)
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    o = P @ v
    kept = kept_mask(keep_hd, B, H, D)
    return s, lse * kept.to(F64)[:, :, None], P, o * _mask4(kept)


def backward64(qkv, o_in, d_o, lse_in, keep_hd, B, N, H, D, scale):
    """o_in, d_o: [B, N, H * D]; lse_in: [B, H, N].  -> P, dS [B,H,N,N], dQ, dK, dV [B,H,N,D]; dropped heads give zeros."""
    q, k, v = split_qkv(qkv, B, N, H, D)
    oi, g = heads(o_in, H, D), heads(d_o, H, D)
    m4 = _mask4(kept_mask(keep_hd, B, H, D))
    s = (q @ k.transpose(-1, -2)) * scale
    P = torch.exp(s - lse_in.detach().cpu().to(F64)[..., None]) * m4
    delta = (g * oi).sum(-1, keepdim=True)
    dS = P * (g @ v.transpose(-1, -2) - delta) * scale
    return P, dS, dS @ k, dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ g


def _eps(q, k, s, lse, D, scale):
    return D * 2.0 ** -23 * (q.abs() @ k.abs().transpose(-1, -2)) * scale + 2.0 ** -22 * (s.abs() + lse.abs()[..., None] + 1.0)


def forward_bounds(qkv, keep_hd, B, N, H, D, scale, u):
    """-> dict(o=[B,H,N,D], lse=[B,H,N]) of per-element bounds (0 on dropped heads)"""
    q, k, v = split_qkv(qkv, B, N, H, D)
    s, lse, P, o = forward64(qkv, None, B, N, H, D, scale)
    eps = _eps(q, k, s, lse, D, scale)
    kept = kept_mask(keep_hd, B, H, D)
    bo = 2 * u * (o.abs() + P @ v.abs()) + 2 * ((P * eps) @ v.abs())
    bl = 2 * eps.max(dim=-1).values + 2.0 ** -19
    return dict(o=bo * _mask4(kept), lse=bl * kept.to(F64)[:, :, None])


def backward_bounds(qkv, o_in, d_o, lse_in, keep_hd, B, N, H, D, scale, u):
    """-> dict(dq=, dk=, dv=) of per-element bounds [B,H,N,D] (0 on dropped heads)"""
    q, k, v = split_qkv(qkv, B, N, H, D)
    oi, g = heads(o_in, H, D), heads(d_o, H, D)
    l_in = lse_in.detach().cpu().to(F64)
    P, dS, dQ, dK, dV = backward64(qkv, o_in, d_o, lse_in, keep_hd, B, N, H, D, scale)
    s = (q @ k.transpose(-1, -2)) * scale
    eps = _eps(q, k, s, l_in, D, scale)
    gamma = D * 2.0 ** -23
    E = dS.abs() * eps + P * scale * gamma * (g.abs() @ v.abs().transpose(-1, -2) + (g.abs() * oi.abs()).sum(-1, keepdim=True))
    aS, T = dS.abs(), lambda x: x.transpose(-1, -2)
    return dict(dq=2 * u * (aS @ k.abs() + dQ.abs()) + E @ k.abs(),
                dk=2 * u * (T(aS) @ q.abs() + dK.abs()) + T(E) @ q.abs(),
                dv=2 * u * (T(P) @ g.abs() + dV.abs()) + T(P * eps) @ g.abs())


def worst_ratio(got, ref, bound):
    """max over every element of |got - ref| / bound; 0 / 0 = 0, x / 0 = inf, non-finite got = inf"""
    got = got.detach().cpu().to(F64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return float(r.max())


def check_forward(o, lse, qkv, keep_hd, B, N, H, D, scale, u, ref=None):
    """o [B,N,H*D], lse [B,H,N] from the code under test -> dict(o=ratio, lse=ratio)"""
    s, lse64, P, o64 = ref if ref is not None else forward64(qkv, keep_hd, B, N, H, D, scale)
    bd = forward_bounds(qkv, keep_hd, B, N, H, D, scale, u)
    return dict(o=worst_ratio(heads(o, H, D), o64, bd["o"]), lse=worst_ratio(lse, lse64, bd["lse"]))


def split_grad(dqkv, B, N, H, D):
    return split_qkv(dqkv, B, N, H, D)


def check_backward(dqkv, qkv, o_in, d_o, lse_in, keep_hd, B, N, H, D, scale, u):
    """dqkv [B,N,3*H*D] from the code under test -> dict(dq=ratio, dk=ratio, dv=ratio)"""
    _, _, dQ, dK, dV = backward64(qkv, o_in, d_o, lse_in, keep_hd, B, N, H, D, scale)
    bd = backward_bounds(qkv, o_in, d_o, lse_in, keep_hd, B, N, H, D, scale, u)
    gq, gk, gv = split_grad(dqkv, B, N, H, D)
    return dict(dq=worst_ratio(gq, dQ, bd["dq"]), dk=worst_ratio(gk, dK, bd["dk"]), dv=worst_ratio(gv, dV, bd["dv"]))


# ---- the inputs of the attention tests (shared by the host test and the GPU test) ------------------------------------------
def random_inputs(seed, B, N, H, D, qscale=1.0, dtype=torch.bfloat16):
    """qkv ~ qscale * N(0, 1), dO ~ N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, N, 3 * H * D, generator=g) * qscale).to(dtype)
    d_o = torch.randn(B, N, H * D, generator=g).to(dtype)
    return qkv, d_o


def pack_qkv(q, k, v):
    """three [B, H, N, D] -> [B, N, 3 * H * D]"""
    return torch.cat([unheads(q), unheads(k), unheads(v)], dim=-1).contiguous()


def uniform_inputs(seed, B, N, H, D, dtype=torch.bfloat16):
    """q = 0 (s = 0, P = 1 / N exactly), v_j = onehot(j mod D), dO_i = onehot(i mod D), k random: o[i, d] = #{j = d mod D} / N and
    dV[j, d] = #{i = d mod D} / N -- every key and every query is counted exactly once or the count is off by 1 / N."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, H, N, D, generator=g)
    hot = torch.zeros(N, D)
    hot[torch.arange(N), torch.arange(N) % D] = 1.0
    hot = hot.expand(B, H, N, D)
    return pack_qkv(torch.zeros(B, H, N, D), k, hot).to(dtype), unheads(hot).to(dtype)


def permutation_inputs(seed, B, N, H, D):
    """k_j = bf16(4 g_j / |g_j|), q_i = 32 k_pi(i) (exact in bf16), v and dO random bf16: query i attends to key pi(i) alone, so
    bf16(o) = v[pi] and bf16(dV) = dO[pi^-1] bit for bit.  -> qkv, dO, pi [B, H, N]"""
    g = torch.Generator().manual_seed(seed)
    gk = torch.randn(B, H, N, D, generator=g)
    k = (4.0 * gk / gk.norm(dim=-1, keepdim=True)).to(torch.bfloat16).float()
    pi = torch.stack([torch.randperm(N, generator=g) for _ in range(B * H)]).reshape(B, H, N)
    q = 32.0 * torch.gather(k, 2, pi[..., None].expand(B, H, N, D))
    v = torch.randn(B, H, N, D, generator=g)
    d_o = torch.randn(B, N, H * D, generator=g).to(torch.bfloat16)
    qkv = pack_qkv(q, k, v).to(torch.bfloat16)
    assert torch.equal(split_qkv(qkv, B, N, H, D)[0].float(), q)
    return qkv, d_o, pi


def logit_edge_inputs(kind, seed, B, N, H, D):
    """Finite, ordinary bf16 data whose logits sit far from 0.  scale = D^-0.5 is assumed.
    'neg': q = -a + 0.25 randn, k = +a + 0.25 randn with a^2 sqrt(D) = 128 (a = 4 at D = 64): every logit is near -125;
    'pos': q = +a + 0.25 randn as well: every logit near +125;
    'mixed': small random q and k, but query 0 of every head sees key 0 at +80 and every other key at -80."""
    g = torch.Generator().manual_seed(seed)
    a = math.sqrt(128.0 / math.sqrt(D))
    q = 0.25 * torch.randn(B, H, N, D, generator=g)
    k = 0.25 * torch.randn(B, H, N, D, generator=g)
    v = torch.randn(B, H, N, D, generator=g)
    d_o = torch.randn(B, N, H * D, generator=g).to(torch.bfloat16)
    if kind == "neg":
        q, k = q - a, k + a
    elif kind == "pos":
        q, k = q + a, k + a
    elif kind == "mixed":
        # first coordinate carries the edge: q_0 = (c, 0, ...), k_0 = (+c, ..), k_j = (-c, ..) with c^2 D^-0.5 = 80; other coordinates of q_0
        # are zero, so the random part of k does not reach row 0's logits
        c = math.sqrt(80.0 * math.sqrt(D))
        c = float(torch.tensor(c).to(torch.bfloat16))
        q[:, :, 0, :] = 0.0
        q[:, :, 0, 0] = c
        k[:, :, :, 0] = -c
        k[:, :, 0, 0] = c
    else:
        raise ValueError(kind)
    return pack_qkv(q, k, v).to(torch.bfloat16), d_o
