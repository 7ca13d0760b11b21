"""float64 statement of the row-statistic kernels' contracts -- LayerNorm (vr_ln_fwd / vr_ln_bwd / vr_ln_grad_reduce and the LayerNorm
epilogues of vr_gemm_ln) and soft-target cross entropy (vr_softce / vr_softce_train) -- with derived per-element error bounds.  CPU only.

The contracts
-------------
LayerNorm forward.  x is [M, C] fp32, row m belongs to sample m // rps, p = keep[sample] (or C when keep is None):

    mean = sum_{c<p} x_c / p,   var = sum_{c<p} (x_c - mean)^2 / p,   rstd = (var + eps)^-1/2,
    y_c  = w_c (x_c - mean) rstd + b_c   for c < p,   y_c = 0 for c >= p;      p = 0:  mean = 0, rstd = eps^-1/2, y = 0.

`var` is the true variance of the kept channels: the masked kernel path forms it as E[x^2] - mean^2 and the plain path in two passes, and
both state this one quantity.  Channels >= p of x are ignored whatever they hold.

LayerNorm backward, a function of the tensors it is HANDED (mean_in and rstd_in are inputs, not recomputed), ln.hip's formulas:

    a = dy (c < p), z = (x - mean_in) rstd_in (c < p), g = a w, s1 = sum g / p, s2 = sum g z / p,
    dx_c = (g_c - (s1 + z_c s2)) rstd_in + dx_in_c  for c < p,  dx_c = 0 exactly for c >= p (the residual gradient included),
    dw_c = sum_m a_mc z_mc,   db_c = sum_m a_mc                                  (sums over ALL rows)

Soft CE.  Row r of the logits x [R, K] meets target row  tr = (sample_map[r // rps] or r // rps) * rps + r % rps:

    lse = log sum_k exp(x_k),  loss_r = lse sum(t) - sum(t x),  grad_k = gscale (softmax(x)_k sum(t) - t_k),  grad = 0 in the pad columns
    K .. ld_grad,  loss_acc += loss_scale sum_r loss_r.

The bounds
----------
u32 = 2^-24 is the unit roundoff of every fp32 operation (hipcc divides and takes square roots correctly rounded), u = 2^-8 / 2^-11 / 0
that of a bf16 / fp16 / fp32 output.  Everything below is a first-order bound on |computed - float64|, per element, and every bound is
then multiplied by 2 -- the one margin, as in attn_ref64 -- and by nothing else.

Sums.  A row sum is formed by a wave: nv = ceil(C / 256) float4 per lane, `s += x + y + z + w` is 4 nv sequential adds, then 6 xor
shuffle levels.  Adding an exact zero does not round, so a sum of p non-zero terms costs at most min(4 nv + 6, p - 1) roundings:

    D = min(4 nv + 6, max(p - 1, 0)),      |fl(sum) - sum| <= D u32 sum|term|.

forward.  inv_n = fl(1 / p) and the product with it round once each:

    dmean = D u32 sum|x| / p + 2 u32 |mean|
    masked path (keep given), var = fl(fl(S2 inv_n) - fl(mu mu)); the squares round before they are summed (D + 1), inv_n twice more:
        dvar = (D + 3) u32 E[x^2] + 2 |mean| dmean + dmean^2 + u32 mean^2 + u32 var
      -- the cancellation term is proportional to u32 E[x^2] = u32 (var + mean^2), NOT to var: a row whose mean is large against its
      spread loses var entirely (and gave a negative var + eps, a NaN rstd, before the kernels clamped var at 0);
    plain path (two passes), sum (x - mu)^2 / p = var + (mu - mean)^2 exactly; x - mu, its square, the sum and inv_n round:
        dvar = (D + 5) u32 (var + dmean^2) + dmean^2                        -- proportional to var.
    rstd = 1 / sqrt(var + eps): the add, the root and the division round (3 roundings), the rest is the derivative:
        drstd = rstd^3 dvar / 2 + 3 u32 rstd
      The first-order term is used only where dvar <= (var + eps) / 4 (`valid`): there (1 - 1/4)^-1/2 = 1.155 against the first order's
      1.125, inside the factor 2.  The tests ASSERT `valid` on every row of every random-input case; rows outside it are tested as
      degenerate rows (finite, 0 < rstd <= eps^-1/2 (1 + 4 u32), mean within dmean).  max(var, 0) can only move var towards var64 >= 0.
    y = fl(w fl(fl(x - mu) rs) + b), with d = x - mean, z = d rstd:
        dy = |w| (rstd (dmean + u32 |d|) + |d| drstd + u32 |z|) + u32 (|w z| + |y|) + u |y|
    Channels >= p and the mean and y of p = 0 rows have bound 0: they must be exact.  (rstd of a p = 0 row keeps its three roundings.)

backward.  a, w, x, mean_in, rstd_in are exact inputs; z = fl(fl(x - mu) rs) carries 2 u32 |z|, g = fl(a w) one u32 |g|:
        ds1 = (D + 3) u32 sum|g| / p                       (g's rounding, the sum, inv_n twice)
        ds2 = (D + 6) u32 sum|g z| / p                     (g 1, z 2, the product 1, the sum, inv_n twice)
        t   = g - (s1 + z s2),   dx = t rstd + dx_in
        ddx = rstd (u32 |g| + ds1 + |z| ds2 + 3 u32 |z s2| + u32 (|s1| + |z s2|) + 2 u32 |t|) + u32 |dx|
    dw, db.  A workgroup sums BWD_ROWS rows (BWD_ROWS / 4 sequentially per wave, then 3 adds across the waves: <= BWD_ROWS + 2), then
    ceil(workgroups / copies) workgroups add into one address with atomics (any order: n terms cost n - 1 roundings in every order);
    with copies > 1 vr_ln_grad_reduce adds the partial rows in 4 chains, 4 adds per chain and full group of 16 rows, the copies % 16 rows
    left over one by one into chain 0; two adds join the chains and one folds into dw:
        depth = BWD_ROWS + 2 + ceil(workgroups / copies) + (4 floor(copies / 16) + copies % 16 + 3 if copies > 1)
        ddw = (depth + 3) u32 sum_m |a z| (+ depth u32 |dw before|),     ddb = depth u32 sum_m |a| (+ depth u32 |db before|)
    dy in bf16 is upcast exactly; dx, dw, db are fp32, so no u term.  gt_out is checked bit for bit against vr_scale_mask_cast(dx).

soft CE.  hipcc -O3 for gfx950 turns __expf(d) into  v_mul_f32 d, 0x3fb8aa3b (log2 e);  v_exp_f32  -- nothing else, no range scaling --
and __logf(s) into v_log_f32 followed by a two-term (hi / lo fma) product with ln 2 and a denormal rescale that does not fire for s >= 1.
The CDNA ISA documents v_exp_f32 and v_log_f32 at 1 ULP = 2^-23 relative = 2 u32.  With d = x - mx <= 0 (mx, the row maximum, is exact):
the subtraction, the constant's own rounding and the product move the exponent by 3 u32 |d| (absolute, in nats); v_exp_f32 adds 2 u32
relative, and a result below 2^-126 may be flushed:
        theta_k = u32 (3 |d_k| + 2),      |fl(e_k) - e_k| <= e_k theta_k + 2^-126                                     (attn_ref64's eps_ij)
    The sums se = sum e_k, st = sum t_k, stx = sum t_k x_k take ceil(K / 64) sequential adds per lane in vr_softce / the pass-by-pass
    kernel and 3 per float4 in the register kernel, then 6 shuffle levels:  Ds = min(max(ceil(K / 64), 3 ceil(K / 256)) + 6, K - 1).
        rse  = sum_k p_k theta_k + Ds u32                     relative error of se          (p = softmax(x); the 2^-126 enters as K 2^-126 / se)
        dlse = rse + 6 u32 log(se) + u32 |lse|                (v_log 2 u32, the ln 2 product and its rounding: 6 u32 in all; the add mx + log)
        dst  = Ds u32 sum|t|,   dstx = (Ds + 1) u32 sum|t x|
        dloss = dlse |st| + |lse| dst + dstx + u32 (|lse st| + |loss|)
        dgrad_k = |gscale| (p_k (|st| (theta_k + rse + 3 u32) + dst) + 2^-126) + 2 u32 |grad_k| + u |grad_k|
      (1 / se or st / se, and the products, are the 3 u32; the subtraction and gscale the 2 u32 |grad|; u the bf16 output.)
    loss_acc: each row's atomic add rounds once, relative to a partial sum that is at most |acc0| + sum_r |loss_scale loss_r|:
        dacc = sum_r |loss_scale| (dloss_r + u32 |loss_r|) + R u32 (|acc0| + sum_r |loss_scale loss_r|)
    Pad columns and rows with sum|t| = 0 have bound 0: exact zeros.

`worst_ratio(got, ref, bound)` is attn_ref64's: max |got - ref| / bound over every element, 0 / 0 = 0, x / 0 = inf, non-finite = inf.
"""
import math

import torch

F64 = torch.float64
U32 = 2.0 ** -24
TINY = 2.0 ** -126
MAXV_LIMIT = 8


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}[dtype]


def f64(t):
    return t.detach().cpu().to(F64)


def worst_ratio(got, ref, bound):
    """max over every element of |got - ref| / bound; 0 / 0 = 0, x / 0 = inf, non-finite got = inf"""
    got = f64(got)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return float(r.max())


# ---- launch paths, re-derived from ln.hip (vr_ln_fwd, vr_ln_bwd) and misc.hip (vr_softce_train) ---------------------------------------
def ln_supported(C):
    return C % 4 == 0 and 0 < C <= 64 * 4 * MAXV_LIMIT


def ln_fwd_path(M, C):
    """-> (nv, template float4 count, rows per wave RU)"""
    nv = (C + 255) // 256
    ru = 4 if nv <= 2 else (2 if nv <= 4 else 1)
    while ru > 1 and M < 4 * ru * 1024:
        ru >>= 1
    return nv, (nv if nv <= 5 else 8), ru


def ln_bwd_path(M, C, copies):
    """-> (nv, inner rows in flight RU, BWD_ROWS, workgroups)"""
    nv = (C + 255) // 256
    ru = 4 if nv == 1 else (2 if nv == 2 else 1)
    if copies > 1:
        rows = 16 if M >= 8192 else (8 if M >= 2048 else 4)
    else:
        rows = 64 if M >= 32768 else (32 if M >= 8192 else (8 if M >= 2048 else 4))
    return nv, ru, rows, (M + rows - 1) // rows


def softce_ld(K):
    return (K + 7) // 8 * 8


def softce_train_path(K, ld_grad):
    """'reg' (register-resident rows) or 'pass' (pass by pass); pointers from torch are 16-byte aligned"""
    return "reg" if K % 4 == 0 and K <= 1024 and ld_grad % 4 == 0 and ld_grad <= 1024 else "pass"


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def rows_keep(keep, M, C, rps):
    """int64 [M]: kept channels of every row"""
    if keep is None:
        return torch.full((M,), C, dtype=torch.int64)
    return keep.detach().cpu().to(torch.int64)[torch.arange(M) // rps]


def _mask(p, C):
    return (torch.arange(C)[None, :] < p[:, None]).to(F64)


def _depth(p, C):
    nv = (C + 255) // 256
    return torch.minimum(torch.full_like(p, 4 * nv + 6), (p - 1).clamp(min=0)).to(F64)


def layernorm_fwd64(x, w, b, keep, rps, eps, out_dtype=None):
    """-> dict(mean [M], var [M], rstd [M], y [M, C], p [M]); out_dtype is not applied (the bound carries it)"""
    C = x.shape[-1]
    X, w, b = f64(x).reshape(-1, C), f64(w), f64(b)
    M = X.shape[0]
    p = rows_keep(keep, M, C, rps)
    m, pf = _mask(p, C), p.clamp(min=1).to(F64)
    mean = (X * m).sum(1) / pf
    d = (X - mean[:, None]) * m
    var = (d * d).sum(1) / pf
    rstd = (var + float(eps)) ** -0.5
    y = (w * d * rstd[:, None] + b) * m
    return dict(mean=mean, var=var, rstd=rstd, y=y, p=p)


def layernorm_fwd_bounds(x, w, b, keep, rps, eps, u, ref=None):
    """-> dict(mean, rstd [M], y [M, C], dvar [M], valid bool [M])"""
    C = x.shape[-1]
    X, w = f64(x).reshape(-1, C), f64(w)
    ref = ref if ref is not None else layernorm_fwd64(x, w, b, keep, rps, eps)
    p, mean, var, rstd, y = ref["p"], ref["mean"], ref["var"], ref["rstd"], ref["y"]
    m, pf, D = _mask(p, C), p.clamp(min=1).to(F64), _depth(p, C)
    Xm = X * m
    dmean = D * U32 * Xm.abs().sum(1) / pf + 2 * U32 * mean.abs()
    if keep is not None:
        e2 = (Xm * Xm).sum(1) / pf
        dvar = (D + 3) * U32 * e2 + 2 * mean.abs() * dmean + dmean ** 2 + U32 * mean ** 2 + U32 * var
    else:
        dvar = (D + 5) * U32 * (var + dmean ** 2) + dmean ** 2
    drstd = 0.5 * rstd ** 3 * dvar + 3 * U32 * rstd
    d = (X - mean[:, None]) * m
    z = d * rstd[:, None]
    by = w.abs() * (rstd[:, None] * (dmean[:, None] + U32 * d.abs()) + d.abs() * drstd[:, None] + U32 * z.abs()) \
        + U32 * ((w * z).abs() + y.abs()) + u * y.abs()
    return dict(mean=2 * dmean, rstd=2 * drstd, y=2 * by * m, dvar=dvar, valid=dvar <= (var + float(eps)) / 4)


def check_ln_fwd(y, mean, rstd, x, w, b, keep, rps, eps, u, ref=None, bounds=None):
    """-> dict(mean=ratio, rstd=ratio, y=ratio)"""
    C = x.shape[-1]
    ref = ref if ref is not None else layernorm_fwd64(x, w, b, keep, rps, eps)
    bd = bounds if bounds is not None else layernorm_fwd_bounds(x, w, b, keep, rps, eps, u, ref)
    return dict(mean=worst_ratio(mean, ref["mean"], bd["mean"]), rstd=worst_ratio(rstd, ref["rstd"], bd["rstd"]),
                y=worst_ratio(f64(y).reshape(-1, C), ref["y"], bd["y"]))


def layernorm_bwd64(dy, x, w, mean_in, rstd_in, keep, rps, dx_in):
    """-> dict(dx [M, C], dw [C], db [C]) and the intermediates the bound needs"""
    C = x.shape[-1]
    X, G, w = f64(x).reshape(-1, C), f64(dy).reshape(-1, C), f64(w)
    mu, rs = f64(mean_in), f64(rstd_in)
    M = X.shape[0]
    p = rows_keep(keep, M, C, rps)
    m, pf = _mask(p, C), p.clamp(min=1).to(F64)
    live = (p > 0).to(F64)
    a = G * m
    z = (X - mu[:, None]) * rs[:, None] * m
    g = a * w
    s1, s2 = g.sum(1) / pf * live, (g * z).sum(1) / pf * live
    t = g - (s1[:, None] + z * s2[:, None])
    dx = t * rs[:, None]
    if dx_in is not None:
        dx = dx + f64(dx_in).reshape(-1, C)
    return dict(dx=dx * m, dw=(a * z).sum(0), db=a.sum(0), a=a, z=z, g=g, s1=s1, s2=s2, t=t, p=p, rs=rs, w=w)


def dwdb_depth(M, C, copies):
    _, _, rows, wgs = ln_bwd_path(M, C, copies)
    c = max(copies, 1)
    return rows + 2 + (wgs + c - 1) // c + (4 * (c // 16) + c % 16 + 3 if c > 1 else 0)


def layernorm_bwd_bounds(ref, C, copies, dw0=None, db0=None, ddy=None, depth=None):
    """ref: layernorm_bwd64's dict.  -> dict(dx [M, C], dw [C], db [C]); dw0 / db0: what the gradient buffers held before.
    ddy [M, C]: absolute error of the dy the kernel forms itself (vr_gemm_ln mode 1: K u32 |du| |wt|^T), carried through the linear terms;
    depth: the dw / db summation depth when it is not vr_ln_bwd's (vr_gemm_ln: 64 rows per workgroup, ceil(M / 64) workgroups)."""
    a, z, g, s1, s2, t, p, rs = (ref[k] for k in ("a", "z", "g", "s1", "s2", "t", "p", "rs"))
    M = a.shape[0]
    m, pf, D = _mask(p, C), p.clamp(min=1).to(F64), _depth(p, C)
    ds1 = (D + 3) * U32 * g.abs().sum(1) / pf
    ds2 = (D + 6) * U32 * (g * z).abs().sum(1) / pf
    zs2 = (z * s2[:, None]).abs()
    bdx = rs.abs()[:, None] * (U32 * g.abs() + ds1[:, None] + z.abs() * ds2[:, None] + 3 * U32 * zs2
                               + U32 * (s1.abs()[:, None] + zs2) + 2 * U32 * t.abs()) + U32 * ref["dx"].abs()
    depth = depth if depth is not None else dwdb_depth(M, C, copies)
    bw = (depth + 3) * U32 * (a * z).abs().sum(0) + (depth * U32 * f64(dw0).abs() if dw0 is not None else 0.0)
    bb = depth * U32 * a.abs().sum(0) + (depth * U32 * f64(db0).abs() if db0 is not None else 0.0)
    if ddy is not None:
        da = ddy * m
        dg = da * ref["w"].abs()
        bdx = bdx + rs.abs()[:, None] * (dg + (dg.sum(1) / pf)[:, None] + z.abs() * ((dg * z.abs()).sum(1) / pf)[:, None])
        bw, bb = bw + (da * z.abs()).sum(0), bb + da.sum(0)
    return dict(dx=2 * bdx * m, dw=2 * bw, db=2 * bb)


def check_ln_bwd(dx, dw, db, ref, C, copies, dw0=None, db0=None, ddy=None, depth=None):
    """dw / db: the buffers AFTER the backward (and the reduce); dw0 / db0 what they held before"""
    bd = layernorm_bwd_bounds(ref, C, copies, dw0, db0, ddy, depth)
    rw = ref["dw"] + (f64(dw0) if dw0 is not None else 0.0)
    rb = ref["db"] + (f64(db0) if db0 is not None else 0.0)
    return dict(dx=worst_ratio(f64(dx).reshape(-1, C), ref["dx"], bd["dx"]), dw=worst_ratio(dw, rw, bd["dw"]),
                db=worst_ratio(db, rb, bd["db"]))


# ---- soft CE ------------------------------------------------------------------------------------------------------------------------
def target_rows(R, rps, sample_map):
    s = torch.arange(R) // rps
    src = sample_map.detach().cpu().to(torch.int64)[s] if sample_map is not None else s
    return src * rps + torch.arange(R) % rps


def softce64(x, t, gscale):
    """x, t [R, K] (t already gathered) -> dict(loss [R], grad [R, K], ...)"""
    X, T = f64(x), f64(t)
    mx = X.max(dim=1, keepdim=True).values
    e = torch.exp(X - mx)
    se = e.sum(1)
    lse = mx[:, 0] + torch.log(se)
    st = T.sum(1)
    loss = lse * st - (T * X).sum(1)
    P = e / se[:, None]
    return dict(loss=loss, grad=gscale * (P * st[:, None] - T), P=P, se=se, lse=lse, st=st, d=X - mx, X=X, T=T, gscale=gscale)


def softce_train64(x, t, sample_map, rps, ld_grad, gscale, loss_scale, acc0):
    """-> dict(grad [R, ld_grad] with zero pad columns, acc = acc0 + loss_scale sum_r loss_r, ...)"""
    R, K = x.shape
    ref = softce64(x, f64(t).reshape(-1, K)[target_rows(R, rps, sample_map)], gscale)
    g = torch.zeros(R, ld_grad, dtype=F64)
    g[:, :K] = ref["grad"]
    ref.update(grad=g, acc=torch.tensor([acc0 + loss_scale * float(ref["loss"].sum())], dtype=F64), acc0=acc0, loss_scale=loss_scale)
    return ref


def softce_bounds(ref, u):
    """-> dict(loss [R], grad [R, K or ld_grad], acc [1] when ref has one)"""
    P, se, lse, st, d, X, T, gscale = (ref[k] for k in ("P", "se", "lse", "st", "d", "X", "T", "gscale"))
    R, K = X.shape
    Ds = min(max((K + 63) // 64, 3 * ((K + 255) // 256)) + 6, K - 1)
    theta = U32 * (3 * d.abs() + 2)
    rse = (P * theta).sum(1) + Ds * U32 + K * TINY / se
    dlse = rse + 6 * U32 * torch.log(se) + U32 * lse.abs()
    dst = Ds * U32 * T.abs().sum(1)
    dstx = (Ds + 1) * U32 * (T * X).abs().sum(1)
    dloss = dlse * st.abs() + lse.abs() * dst + dstx + U32 * ((lse * st).abs() + ref["loss"].abs())
    live = (T.abs().sum(1) > 0).to(F64)[:, None]                       # all-zero target rows: exact zeros
    gk = ref["grad"][:, :K]
    dg = abs(gscale) * (P * (st.abs()[:, None] * (theta + rse[:, None] + 3 * U32) + dst[:, None]) + TINY) * live + (2 * U32 + u) * gk.abs()
    bg = torch.zeros_like(ref["grad"])
    bg[:, :K] = 2 * dg
    out = dict(loss=2 * dloss * live[:, 0], grad=bg)
    if "acc" in ref:
        ls = abs(ref["loss_scale"])
        mag = abs(ref["acc0"]) + ls * float(ref["loss"].abs().sum())
        out["acc"] = torch.tensor([2 * (ls * float((dloss * live[:, 0] + U32 * ref["loss"].abs()).sum()) + R * U32 * mag)], dtype=F64)
    return out


# ---- the inputs of the row-statistic tests (shared by the host test and the GPU test) ------------------------------------------------
EPS = 1e-6


def keep_cycle(C, B, start=0):
    """per-sample keep counts: every partly kept float4 group (C-1, C-2, C-3, C/2+1, 5, 1), the full and the empty row, and the float4-
    per-lane boundaries 255 / 256 / 257 where they fit"""
    vals = [v for v in (C, C - 1, C - 2, C - 3, C // 2 + 1, 5, 1, 0, 256, 257, 255) if 0 <= v <= C]
    return torch.tensor([vals[(start + i) % len(vals)] for i in range(B)], dtype=torch.int32)


def ln_inputs(seed, M, C):
    """x uniform in [-0.4, 0.6] (a keep = 1 row has var = 0, and the masked formula's cancellation term 8 u32 x^2 must stay under
    (0 + eps) / 4: |x| <= 0.7), w = 1 + 0.1 randn, b = 0.1 randn.  Channels beyond keep are NOT zeroed: the kernels mask them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, C, generator=g) - 0.4
    return x, 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def offset_inputs(seed, M, C, ratio):
    """rows of ratio + randn: mean / std = ratio"""
    g = torch.Generator().manual_seed(seed)
    return ratio + torch.randn(M, C, generator=g), 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def degenerate_inputs(seed, M, C, value, spread):
    """rows of value + spread * randn (spread = 0: exactly constant rows)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((M, C), float(value)) + spread * torch.randn(M, C, generator=g)
    return x, 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def ln_bwd_inputs(M, C, copies, rps, masked, dtype, with_dx_in):
    """-> x, w, keep, dy (dtype), dx_in or None, mean_in, rstd_in (fp32 roundings of the float64 statistics)"""
    x, w, b = ln_inputs(M * 3 + C + copies, M, C)
    keep = keep_cycle(C, (M + rps - 1) // rps, start=M % 7) if masked else None
    g = torch.Generator().manual_seed(M + C)
    dy = torch.randn(M, C, generator=g).to(dtype)
    dx_in = torch.randn(M, C, generator=g) if with_dx_in else None
    f = layernorm_fwd64(x, w, b, keep, rps, EPS)
    return x, w, keep, dy, dx_in, f["mean"].float(), f["rstd"].float()


def probe_inputs(M, C, rps, copies):
    """Structural probe of dw / db: mean_in = 0, rstd_in = 1, w = 1, x in {1, 2, 3}, dy = 2^i in the i-th chosen row and 0 elsewhere:
    every product and partial sum is a small integer, so fp32 is exact in any order and db = 2^n - 1 in every column, bit for bit.  The
    chosen rows: first, last, the tail rows of the last workgroup, both sides of a sample boundary and of a workgroup boundary.
    -> x, dy, mean_in, rstd_in, chosen"""
    _, _, rows, wgs = ln_bwd_path(M, C, copies)
    last = (wgs - 1) * rows
    chosen = sorted(set(m for m in (0, M - 1, last, last + 1, M - 2, rps - 1, rps, (M // rps) * rps - 1, (M // rps) * rps, rows, rows - 1)
                        if 0 <= m < M))
    g = torch.Generator().manual_seed(M + C)
    x = torch.randint(1, 4, (M, C), generator=g).float()
    dy = torch.zeros(M, C)
    for i, m in enumerate(chosen):
        dy[m] = 2.0 ** i
    return x, dy, torch.zeros(M), torch.ones(M), chosen


def ramp_inputs(M, C):
    """row m = m + c / 1024 (exact in fp32 for m < 2^13 C <= 2048; beyond, still distinct): mean[m] names the row that was read"""
    return (torch.arange(M, dtype=torch.float32)[:, None] + torch.arange(C, dtype=torch.float32)[None, :] / 1024.0).contiguous()


# forward: (M, C, rps); the first four reach RU = 4 and RU = 2, the rest RU = 1 at every nv and the small-M tails
LN_FWD_CASES = [(16384 + 5, 32, 17), (16384 + 5, 260, 5), (8192 + 3, 32, 5), (8192 + 3, 776, 17),
                (1, 32, 1), (2, 32, 1), (3, 32, 5), (5, 32, 17), (85, 32, 5),
                (7, 4, 1), (9, 252, 5), (7, 256, 1), (7, 520, 5), (9, 1024, 5), (7, 1028, 1), (6, 1280, 5), (7, 1288, 1), (7, 1540, 5), (9, 1796, 5), (7, 2048, 1)]
# backward: (M, C, copies, rps)
LN_BWD_CASES = [(85, 32, 1, 17), (2048 + 3, 32, 1, 5), (8192 + 5, 32, 1, 17), (32768 + 7, 32, 1, 5),
                (2048 + 3, 32, 7, 17), (8192 + 5, 32, 64, 5), (2048 + 3, 32, 64, 1), (8192 + 5, 32, 7, 17),
                (85, 260, 1, 5), (2048 + 3, 260, 7, 17), (8192 + 5, 260, 64, 5), (8192 + 5, 260, 1, 17),
                (85, 776, 1, 17), (2048 + 3, 776, 64, 5), (8192 + 5, 776, 7, 17), (2048 + 3, 776, 1, 1), (8192 + 5, 776, 1, 5)]
# (BWD_ROWS = 64 needs M >= 32768: 34 MB of fp32 at C = 260 and 100 MB at C = 776, beyond what a quick test should hold, so the inner RU = 2
# and RU = 1 loops meet row walks up to 32 and the 64-row walk runs at C = 32)

SOFTCE_K = [4, 8, 37, 252, 256, 260, 1000, 1001, 1020, 1024, 1028, 1536]
SOFTCE_R = [1, 5, 8, 66]
LOGIT_FAMILIES = ["randn2", "equal", "equal1e4", "one80", "spread40"]
TARGET_FAMILIES = ["softmax", "onehot", "smooth", "half", "zero"]


def softce_logits(kind, seed, R, K):
    g = torch.Generator().manual_seed(seed)
    if kind == "randn2":
        return 2.0 * torch.randn(R, K, generator=g)
    if kind == "equal":
        return torch.full((R, K), 0.75)
    if kind == "equal1e4":
        return torch.full((R, K), 1e4)
    if kind == "one80":                              # one logit 80 above the rest
        x = torch.randn(R, K, generator=g)
        x[torch.arange(R), torch.randint(0, K, (R,), generator=g)] += 80.0 + 4.0
        return x
    if kind == "spread40":
        return 80.0 * torch.rand(R, K, generator=g) - 40.0
    raise ValueError(kind)


def softce_targets(kind, seed, R, K):
    g = torch.Generator().manual_seed(seed)
    hot = torch.zeros(R, K)
    hot[torch.arange(R), torch.randint(0, K, (R,), generator=g)] = 1.0
    if kind == "softmax":
        return torch.softmax(torch.randn(R, K, generator=g), -1)
    if kind == "onehot":
        return hot
    if kind == "smooth":                             # label smoothing 0.1 blended with a second class (mixup): sum = 1
        hot2 = torch.zeros(R, K)
        hot2[torch.arange(R), torch.randint(0, K, (R,), generator=g)] = 1.0
        return 0.9 * (0.7 * hot + 0.3 * hot2) + 0.1 / K
    if kind == "half":
        return 0.5 * torch.softmax(torch.randn(R, K, generator=g), -1)
    if kind == "zero":
        return torch.zeros(R, K)
    raise ValueError(kind)
