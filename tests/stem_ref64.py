"""float64 statement of the conv patch-embedding stem's contracts -- the direct convolutions of conv3x3.hip (vr_conv3x3 and its _res /
_res_patch / _bias_relu / _bias_relu_patch forms, vr_conv1_direct, vr_conv3x3_wgrad), the BatchNorm and layout kernels of stem.hip and
vr_conv_w_flip -- with derived per-element error bounds.  CPU only.

The contracts (on exact upcasts of the tensors the kernel is handed)
-------------------------------------------------------------------
conv3x3.  a is NHWC [B*H*W, Cin], w [Cout, (kh, kw, ci)], both 16-bit (bf16; fp16 for the VR_F16 forms); A = a zero padded by one pixel:

    conv[b, y, x, co] = sum_{kh, kw, ci} w[co, kh, kw, ci] A[b, y + kh, x + kw, ci]            (pad 1, stride 1)
    out = conv                                         vr_conv3x3
    out = conv + res                                   _res;  _res_patch: res is stored in patch order (patch_unfold's layout)
    out = relu(conv + bias) (+ res)                    _bias_relu;  _bias_relu_patch: out is stored in patch order

A pixel outside the image is the value 0: with finite weights it contributes exactly 0 (and a NaN weight meets it as 0 x NaN = NaN, in the
kernel's MFMA as in torch's conv2d).  relu(NaN) = NaN, relu(-0) = relu(negative) = +0.  The data gradient of the convolution is the same
kernel on dz with vr_conv_w_flip's weights, wf[ci, (kh, kw, co)] = w[co, ci, 2 - kh, 2 - kw]: the transposed convolution.

conv1_direct.  img fp32 NCHW [B, 3, H, W] is rounded to the operand type FIRST (RNE; the contract is on the rounded image I, zero padded),
w is [Cout, 32] with k = (kh, kw, c) in its first 27 slots and zeros in the rest, Ho = (H - 1) / 2 + 1:

    out[b, oy, ox, co] = sum_{kh, kw, c} w[co, (kh, kw, c)] I[b, c, 2 oy + kh, 2 ox + kw]  (+ bias[co])  (then relu)     bias, relu independent

wgrad.   dw[co, (kh, kw, ci)] += sum_{b, y, x} dz[b, y, x, co] A[b, y + kh, x + kw, ci].

bn_stats.     sum[c] += sum_r z[r, c],  sumsq[c] += sum_r z[r, c]^2            (z fp32 or bf16 [R, C])
bn_finalize.  torch.nn.BatchNorm2d in training: mean = sum / n, var = sumsq / n - mean^2 (biased, >= 0), rstd = (var + eps)^-1/2,
    scale = w rstd, shift = b - mean scale, running_mean <- (1 - m) running_mean + m mean, running_var <- (1 - m) running_var +
    m var n / max(n - 1, 1), num_batches_tracked += 1; eps and m are the fp32 values the kernel is handed.  A NaN statistic stays NaN.
    The tests state it on z itself (bn_stats -> bn_finalize), i.e. against the true statistics.
bn_relu.      out = relu(z scale[c] + shift[c]) (+ res);  _patch: out in patch order.  relu(NaN) = NaN.
bn_bwd.       a function of the scale, shift, mean and rstd it is HANDED:  pre = z scale + shift,  g = da [pre > 0] (strict: pre = 0 is masked),
    zhat = (z - mean) rstd,  sg[c] += sum_r g,  sgz[c] += sum_r g zhat,  dz = scale (g - sg inv_n - zhat sgz inv_n) with the sg / sgz the buffers
    hold AFTER the accumulation and inv_n = fl(1 / R) in training, 0 in evaluation;  _patch: da is read in patch order.
layout.       vr_im2col3x3 (NHWC; NCHW image with stride and ld; the 3-channel row kernel), vr_patch_unfold / fold, vr_conv_w_flip are
    permutations and RNE casts: bit for bit.  vr_col2im3x3 sums at most 9 terms in fp32 and rounds to the type.

The bounds
----------
u32 = 2^-24, u = 2^-8 / 2^-11 / 0 for a bf16 / fp16 / fp32 output (rowstat_ref64's).  First-order, per element; every bound is multiplied
by 2 at the end -- the one margin -- and by nothing else.

MFMA sums (attn_ref64's model, held on the MI355X): products of 16-bit operands are exact in fp32, a K-term accumulation costs
K 2^-23 sum|w||a| (the sum over the taps inside the image: padded pixels contribute |0|):
    conv3x3:  K = 9 Cin;   conv1_direct: K = 27
    d(out) = K 2^-23 sum|w||a| + u32 |conv + bias| (bias add) + u32 |out| (residual add) + u |out|;  relu is 1-Lipschitz and adds nothing.
wgrad:  a persistent workgroup accumulates ceil(tiles / grid) tiles of 256 pixels, grid = min(tiles, 1024) workgroups add with atomics:
    depth = 256 ceil(tiles / grid) + grid,    d(dw) = depth u32 (sum|dz a| + |dw before|).
bn_stats:  rows_par = 256 / (C / 8) (integer), blocks = min(ceil(R / (64 rows_par)), 2048); a thread sums ceil(R / (blocks rows_par)) rows
    (the four-row unroll keeps the order), rows_par LDS adds, blocks atomics; adding an exact zero does not round, so R terms cost at most
    R - 1 roundings (R when they join a non-zero `before`):   depth = min(ceil(R / (blocks rows_par)) + rows_par + blocks, R - 1 or R),
    d(sum) = depth u32 (sum|z| + |before|),  d(sumsq) = (depth + 1) u32 (sum z^2 + |before|)   (the squares round before they are summed).
bn_finalize (on true statistics, so the bn_stats depth enters):
    dmean = depth u32 E|z| + u32 |mean|
    dvar  = (depth + 2) u32 E[z^2] + 2 |mean| dmean + dmean^2 + u32 mean^2 + u32 var
      -- the cancellation term is proportional to u32 depth E[z^2] = u32 depth (var + mean^2), not to var (rowstat_ref64's masked path).
    drstd = rstd^3 dvar / 2 + 3 u32 rstd, used only where dvar <= (var + eps) / 4 (`valid`, ASSERTED on every random-input channel);
      constant channels (and every channel of an R = 1 launch) are degenerate: finite, 0 < rstd <= eps^-1/2 (1 + 4 u32), with mean and the
      running statistics, which do not pass through rstd, still inside their bounds.  The clamp can only move var towards var64 >= 0.
    dscale = |w| drstd + u32 |scale|,   dshift = |scale| dmean + |mean| dscale + dmean dscale + u32 |mean scale| + u32 |shift|
    d(running_mean) = 2 u32 |(1 - m) rm| + m dmean + u32 |m mean| + u32 |new|        (fl(1 - m), two products, the add)
    d(running_var)  = 2 u32 |(1 - m) rv| + m f dvar + 3 u32 |m f var| + u32 |new|,  f = n / max(n - 1, 1)   (fl(f), two products)
bn_relu:  d = u32 |z scale| + u32 |pre| + u32 |out| (residual) + u |out|.
bn_bwd:   dpre = u32 (|z scale| + |pre|).  The mask is discontinuous: an element with |pre64| < 2 dpre is UNDECIDED -- its dz is compared
    against both branches and its |da| (|da zhat|) is ADDED to the bound of sg (sgz).  The tests assert that undecided elements number at
    most max(1, 1e-4 numel) per case.  (z = 0 with shift = 0 has dpre = 0: decided, and masked.)
    d(sg)  = depth u32 (sum|g| + |sg before|) + sum_undecided |da|
    d(sgz) = (depth + 3) u32 sum|g zhat| + depth u32 |sgz before| + sum_undecided |da zhat|    (z - mean, the two products: 3)
    dz: zhat 2 roundings, fl(1 / R) and sg inv_n 2, zhat sgz inv_n 5 in all, the two subtractions and scale 3:
    d(dz) = |scale| (inv_n d(sg) + 2 u32 |sg inv_n| + |zhat| inv_n d(sgz) + 5 u32 |zhat sgz inv_n| + u32 |g - sg inv_n| + u32 |t|)
            + u32 |dz| + u |dz|,   t = g - sg inv_n - zhat sgz inv_n.
col2im:   d = 8 u32 sum|term| + u |out|.

`worst_ratio`, `unit_roundoff`, `f64` are rowstat_ref64's.  `nonfinite_ratio` is worst_ratio for planted NaNs: got must be NaN in exactly
the elements where the float64 contract is NaN and equal an infinite contract value (else inf), and inside its bound everywhere else.
"""
import math

import torch

from rowstat_ref64 import F64, U32, f64, unit_roundoff, worst_ratio  # noqa: F401  (re-exported)

MFMA = 2.0 ** -23
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def f32v(x):
    """the fp32 value of a Python float handed to a kernel as `float`"""
    return float(torch.tensor(x, dtype=torch.float32))


def nonfinite_ratio(got, ref, bound):
    g = f64(got)
    nan, inf = torch.isnan(ref), torch.isinf(ref)
    if not torch.equal(torch.isnan(g), nan) or not torch.equal(g[inf], ref[inf]):        # (an infinite contract value: that infinity)
        return math.inf
    z, nf = torch.zeros_like(ref), nan | inf
    return worst_ratio(torch.where(nf, z, g), torch.where(nf, z, ref), torch.where(nf, z, bound))


def relu64(v):
    return torch.where(v <= 0, torch.zeros_like(v), v)                 # NaN -> NaN, -0 and negatives -> +0


# ---- patch order (vr_patch_unfold's layout) ---------------------------------------------------------------------------------------------
def patch_perm(B, H, W, P):
    """int64 [B*H*W]: NHWC pixel -> its pixel slot in patch order"""
    pix = torch.arange(B * H * W)
    x, y, b = pix % W, (pix // W) % H, pix // (W * H)
    return ((b * (H // P) + y // P) * (W // P) + x // P) * (P * P) + (y % P) * P + x % P


def to_patch(t, B, H, W, P):
    """NHWC [B*H*W, C] -> patch order [B*gh*gw, P*P*C]"""
    C = t.shape[-1]
    o = torch.empty_like(t.reshape(B * H * W, C))
    o[patch_perm(B, H, W, P)] = t.reshape(B * H * W, C)
    return o.reshape(B * (H // P) * (W // P), P * P * C)


def from_patch(col, B, H, W, P):
    C = col.numel() // (B * H * W)
    return col.reshape(B * H * W, C)[patch_perm(B, H, W, P)]


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------
def _padded(a, B, H, W):
    return torch.nn.functional.pad(f64(a).reshape(B, H, W, -1), (0, 0, 1, 1, 1, 1))


def conv3x3_64(a, w, B, H, W, bias=None, relu=False, res=None, res_patch=0, out_patch=0):
    """-> (out [B*H*W, Cout] (or patch order), bound, same shape).  `bound` is for output unit roundoff 0: add u |out| with out_bound()."""
    Cout = w.shape[0]
    A, wt = _padded(a, B, H, W), f64(w).reshape(Cout, 9, -1)
    Cin = wt.shape[2]
    conv, mag = torch.zeros(B, H, W, Cout, dtype=F64), torch.zeros(B, H, W, Cout, dtype=F64)
    finite = bool(torch.isfinite(A).all() and torch.isfinite(wt).all())
    for tap in range(9):
        s = A[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, :]
        if finite:
            conv += s @ wt[:, tap].t()
            mag += s.abs() @ wt[:, tap].abs().t()
        else:               # planted NaN / inf: term by term, so that no BLAS shortcut around a zero decides where the NaNs go
            conv += (s[:, :, :, None, :] * wt[:, tap]).sum(-1)
            mag += (s[:, :, :, None, :].abs() * wt[:, tap].abs()).sum(-1)
    out, bd = conv.reshape(-1, Cout), 9 * Cin * MFMA * mag.reshape(-1, Cout)
    if bias is not None:
        out = out + f64(bias)
        bd = bd + U32 * out.abs()
    if relu:
        out = relu64(out)
    if res is not None:
        r = f64(res)
        out = out + (from_patch(r, B, H, W, res_patch) if res_patch else r.reshape(-1, Cout))
        bd = bd + U32 * out.abs()
    if out_patch:
        out, bd = to_patch(out, B, H, W, out_patch), to_patch(bd, B, H, W, out_patch)
    return out, bd


def out_bound(out, bd, u):
    """the factor 2 and the output rounding"""
    return 2 * (bd + u * out.abs())


def w_flip64(w4):
    """[Co, Ci, 3, 3] -> [Ci, (kh, kw, co)] = w[co, ci, 2 - kh, 2 - kw]"""
    return w4.flip(2, 3).permute(1, 2, 3, 0).reshape(w4.shape[1], 9 * w4.shape[0]).contiguous()


def conv1_64(img, w, op_dtype, bias=None, relu=False):
    """-> (out [B*Ho*Wo, Cout], bound at u = 0)"""
    B, _, H, W = img.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    I = torch.nn.functional.pad(f64(img.to(op_dtype)), (1, 2, 1, 2))        # (the extra right / bottom zeros are never a real tap's)
    wt = f64(w)[:, :27].reshape(Cout, 9, 3)
    out, mag = torch.zeros(B, Ho, Wo, Cout, dtype=F64), torch.zeros(B, Ho, Wo, Cout, dtype=F64)
    for tap in range(9):
        kh, kw = tap // 3, tap % 3
        s = I[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2].permute(0, 2, 3, 1)[:, :, :, None, :]     # [B, Ho, Wo, 1, 3]
        out += (s * wt[:, tap]).sum(-1)                                  # (term by term: NaNs go where the arithmetic puts them)
        mag += (s.abs() * wt[:, tap].abs()).sum(-1)
    out, bd = out.reshape(-1, Cout), 27 * MFMA * mag.reshape(-1, Cout)
    if bias is not None:
        out = out + f64(bias)
        bd = bd + U32 * out.abs()
    if relu:
        out = relu64(out)
    return out, bd


def wgrad_depth(B, H, W):
    tiles = B * ((H + 15) // 16) * ((W + 15) // 16)
    grid = min(tiles, 1024)
    return 256 * ((tiles + grid - 1) // grid) + grid


def wgrad64(a, dz, dw0, B, H, W):
    """-> (dw after [Cout, 9 Cin], bound)"""
    A, G = _padded(a, B, H, W), f64(dz).reshape(B * H * W, -1)
    Cin, Cout = A.shape[-1], G.shape[-1]
    dw, mag = torch.zeros(Cout, 9, Cin, dtype=F64), torch.zeros(Cout, 9, Cin, dtype=F64)
    for tap in range(9):
        s = A[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, :].reshape(B * H * W, Cin)
        dw[:, tap] = G.t() @ s
        mag[:, tap] = G.abs().t() @ s.abs()
    d0 = f64(dw0)
    return dw.reshape(Cout, -1) + d0, 2 * wgrad_depth(B, H, W) * U32 * (mag.reshape(Cout, -1) + d0.abs())


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------
def bn_path(R, C):
    """-> (rows_par, blocks, rows per thread) of vr_bn_stats / the reduction of vr_bn_bwd"""
    rows_par = 256 // (C // 8)
    blocks = min((R + 64 * rows_par - 1) // (64 * rows_par), 2048)
    return rows_par, blocks, (R + blocks * rows_par - 1) // (blocks * rows_par)


def bn_depth(R, C, before=False):
    """roundings of a column sum of R terms (added to a non-zero `before`): the launch's depth, but adding an exact zero does not round"""
    rows_par, blocks, chain = bn_path(R, C)
    return min(chain + rows_par + blocks, R if before else R - 1)


def bn_stats64(z, sum0=None, sumsq0=None):
    """-> dict(sum, sumsq [C] after the accumulation, and their bounds)"""
    Z = f64(z)
    R, C = Z.shape
    s0 = f64(sum0) if sum0 is not None else torch.zeros(C, dtype=F64)
    q0 = f64(sumsq0) if sumsq0 is not None else torch.zeros(C, dtype=F64)
    D = bn_depth(R, C, before=sum0 is not None)
    return dict(sum=Z.sum(0) + s0, sumsq=(Z * Z).sum(0) + q0, bsum=2 * D * U32 * (Z.abs().sum(0) + s0.abs()),
                bsumsq=2 * (D + 1) * U32 * ((Z * Z).sum(0) + q0.abs()))


def bn_finalize64(z, w, b, eps=BN_EPS, momentum=BN_MOMENTUM, rmean0=None, rvar0=None, unbiased_running=True):
    """BatchNorm2d's training statistics of z [R, C] -> dict of values and bounds (keys b<name>), `valid` [C] bool"""
    Z, w, b = f64(z), f64(w), f64(b)
    n, C = Z.shape
    eps, m = f32v(eps), f32v(momentum)
    D = bn_depth(n, C)
    mean = Z.sum(0) / n
    e2 = (Z * Z).sum(0) / n
    var = ((Z - mean) ** 2).sum(0) / n
    rstd = (var + eps) ** -0.5
    scale = w * rstd
    shift = b - mean * scale
    dmean = D * U32 * Z.abs().sum(0) / n + U32 * mean.abs()
    dvar = (D + 2) * U32 * e2 + 2 * mean.abs() * dmean + dmean ** 2 + U32 * mean ** 2 + U32 * var
    drstd = 0.5 * rstd ** 3 * dvar + 3 * U32 * rstd
    dscale = w.abs() * drstd + U32 * scale.abs()
    dshift = scale.abs() * dmean + mean.abs() * dscale + dmean * dscale + U32 * (mean * scale).abs() + U32 * shift.abs()
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, bmean=2 * dmean, brstd=2 * drstd, bscale=2 * dscale, bshift=2 * dshift,
               dvar=dvar, valid=dvar <= (var + eps) / 4, eps=eps)
    if rmean0 is not None:
        f = n / max(n - 1, 1) if unbiased_running else 1.0
        rm0, rv0 = f64(rmean0), f64(rvar0)
        out["rmean"] = (1 - m) * rm0 + m * mean
        out["rvar"] = (1 - m) * rv0 + m * var * f
        out["brmean"] = 2 * (2 * U32 * ((1 - m) * rm0).abs() + m * dmean + U32 * (m * mean).abs() + U32 * out["rmean"].abs())
        out["brvar"] = 2 * (2 * U32 * ((1 - m) * rv0).abs() + m * f * dvar + 3 * U32 * (m * f * var).abs() + U32 * out["rvar"].abs())
    return out


FINALIZE_KEYS = ("mean", "rstd", "scale", "shift")


def degenerate_ok(rstd, eps):
    """constant channels: finite, 0 < rstd <= eps^-1/2 (1 + 4 u32)"""
    r = f64(rstd)
    return bool(torch.isfinite(r).all() and (r > 0).all() and (r <= f32v(eps) ** -0.5 * (1 + 4 * U32)).all())


def bn_relu64(z, scale, shift, res=None, B=0, H=0, W=0, P=0):
    """-> (out, bound at u = 0); P > 0: out in patch order"""
    Z = f64(z)
    zs = Z * f64(scale)
    pre = zs + f64(shift)
    out = relu64(pre)
    bd = U32 * (zs.abs() + pre.abs())
    if res is not None:
        out = out + f64(res)
        bd = bd + U32 * out.abs()
    if P:
        out, bd = to_patch(out, B, H, W, P), to_patch(bd, B, H, W, P)
    return out, bd


def bn_bwd64(da, z, scale, shift, mean, rstd, sg0, sgz0, training, u, B=0, H=0, W=0, P=0, mask_ge=False, drop_sg_term=False):
    """-> dict(sg, sgz [C] after; dz, dz_alt [R, C] (dz_alt: the undecided elements on their other branch); bsg, bsgz, bdz; undecided count).
    da is in patch order when P > 0.  mask_ge / drop_sg_term: the injected errors of the host test (a wrong contract, never the default)."""
    Z = f64(z)
    R, C = Z.shape
    G = f64(da)
    G = from_patch(G, B, H, W, P) if P else G.reshape(R, C)
    sc, sh, mu, rs = f64(scale), f64(shift), f64(mean), f64(rstd)
    zs = Z * sc
    pre = zs + sh
    und = pre.abs() < 2 * U32 * (zs.abs() + pre.abs())
    keep = (pre >= 0) if mask_ge else (pre > 0)
    g = torch.where(keep, G, torch.zeros_like(G))
    zh = (Z - mu) * rs
    D = bn_depth(R, C, before=True)
    s0, q0 = f64(sg0), f64(sgz0)
    sg, sgz = g.sum(0) + s0, (g * zh).sum(0) + q0
    uG = torch.where(und, G.abs(), torch.zeros_like(G))
    dsg = D * U32 * (g.abs().sum(0) + s0.abs()) + uG.sum(0)
    dsgz = (D + 3) * U32 * (g * zh).abs().sum(0) + D * U32 * q0.abs() + (uG * zh.abs()).sum(0)
    inv_n = f32v(1.0 / R) if training else 0.0

    def dz_of(gg):
        t1 = 0.0 if drop_sg_term else sg * inv_n
        t = gg - t1 - zh * sgz * inv_n
        return sc * t, t, gg - sg * inv_n

    dz, t, gm = dz_of(g)
    dz_alt = dz_of(torch.where(und & ~keep, G, torch.where(und, torch.zeros_like(G), g)))[0]
    bdz = sc.abs() * (inv_n * dsg + 2 * U32 * (sg * inv_n).abs() + zh.abs() * inv_n * dsgz + 5 * U32 * (zh * sgz * inv_n).abs()
                      + U32 * gm.abs() + U32 * t.abs()) + (U32 + u) * torch.maximum(dz.abs(), dz_alt.abs())
    return dict(sg=sg, sgz=sgz, dz=dz, dz_alt=dz_alt, bsg=2 * dsg, bsgz=2 * dsgz, bdz=2 * bdz, undecided=int(und.sum()), numel=R * C)


def bwd_dz_ratio(got, ref):
    """worst_ratio of dz with the undecided elements allowed either branch"""
    g = f64(got)
    pick = torch.where((g - ref["dz"]).abs() <= (g - ref["dz_alt"]).abs(), ref["dz"], ref["dz_alt"])
    return worst_ratio(g, pick, ref["bdz"])


def undecided_cap(numel):
    return max(1, int(1e-4 * numel))


# ---- layout kernels ---------------------------------------------------------------------------------------------------------------------
def im2col_nhwc(a, B, H, W):
    """[B*H*W, C] -> [B*H*W, (kh, kw, c)], any dtype, exact"""
    C = a.shape[-1]
    A = torch.nn.functional.pad(a.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    return torch.cat([A[:, t // 3:t // 3 + H, t % 3:t % 3 + W, :] for t in range(9)], dim=-1).reshape(B * H * W, 9 * C)


def im2col_image(img, stride, ld, dtype):
    """fp32 NCHW [B, C, H, W] -> [B*Ho*Wo, ld] of dtype, k = (kh, kw, c), zeros in k >= 9 C"""
    B, C, H, W = img.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    I = torch.nn.functional.pad(img, (1, 2, 1, 2))
    col = torch.zeros(B, Ho, Wo, ld, dtype=torch.float32)
    for t in range(9):
        kh, kw = t // 3, t % 3
        col[..., t * C:(t + 1) * C] = I[:, :, kh:kh + stride * Ho:stride, kw:kw + stride * Wo:stride].permute(0, 2, 3, 1)
    return col.reshape(-1, ld).to(dtype)


def col2im64(dcol, B, H, W, u):
    """-> (dsrc [B*H*W, C] float64, bound)"""
    C = dcol.shape[-1] // 9
    D = f64(dcol).reshape(B, H, W, 9, C)
    P = torch.nn.functional.pad(D, (0, 0, 0, 0, 1, 1, 1, 1))             # [B, H + 2, W + 2, 9, C]
    out, mag = torch.zeros(B, H, W, C, dtype=F64), torch.zeros(B, H, W, C, dtype=F64)
    for t in range(9):
        kh, kw = t // 3, t % 3
        s = P[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W, t, :]            # dcol[(b, ih + 1 - kh, iw + 1 - kw)][(kh, kw, c)]
        out += s
        mag += s.abs()
    return out.reshape(-1, C), 2 * (8 * U32 * mag.reshape(-1, C) + u * out.reshape(-1, C).abs())


# ---- the inputs of the stem tests (shared by the host test and the GPU test) -------------------------------------------------------------
CONV_HW = [(1, 1), (16, 16), (15, 17), (17, 15), (33, 16), (16, 33)]
CONV_B = [1, 3]
CONV_CIN = [16, 24, 32]
CONV_COUT = [4, 12, 16, 20, 32]
PATCH_SHAPES = [(14, 14, 7), (28, 42, 7), (16, 32, 2)]
CONV1_HW = [(1, 1), (2, 3), (15, 16), (16, 17), (17, 63), (31, 64), (33, 65), (18, 129)]
CONV1_COUT = [4, 16, 20, 32]
BN_C = [8, 16, 24, 32, 256]
WGRAD_BIG = (257, 17, 17)                            # 1028 tiles > 1024 persistent workgroups


def bn_rows(C):
    rp = 256 // (C // 8)
    return [1, rp - 1, rp, rp + 1, 64 * rp, 64 * rp + 1, 4 * 64 * rp + 3]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def conv_inputs(B, H, W, Cin, Cout, dtype=torch.bfloat16):
    """-> a [B*H*W, Cin], w [Cout, 9 Cin] (dtype), bias fp32 [Cout], res [B*H*W, Cout] (dtype)"""
    g = _gen(B, H, W, Cin, Cout)
    a = torch.randn(B * H * W, Cin, generator=g).to(dtype)
    w = (torch.randn(Cout, 9 * Cin, generator=g) * (9 * Cin) ** -0.5).to(dtype)
    return a, w, 0.5 * torch.randn(Cout, generator=g), torch.randn(B * H * W, Cout, generator=g).to(dtype)


def isolate_batch(a, B, H, W):
    """image b gets the first row of image b + 1 in its last row and the last row of image b - 1 in its first row, scaled by 2^6: a halo
    row leaked from a neighbouring image is then 64 times a typical term, far outside the bound"""
    C = a.shape[-1]
    x = a.float().reshape(B, H, W, C).clone()
    src = x.clone()
    for b in range(B):
        if b + 1 < B:
            x[b, H - 1] = 64.0 * src[b + 1, 0]
        if b > 0:
            x[b, 0] = 64.0 * src[b - 1, H - 1]
    return x.reshape(-1, C).to(a.dtype)


def int_inputs(shape, lim, *key):
    """integers in [-lim, lim] as fp32"""
    return torch.randint(-lim, lim + 1, shape, generator=_gen(*key)).float()


def conv1_inputs(B, H, W, Cout, dtype=torch.bfloat16):
    g = _gen(B, H, W, Cout, 3)
    img = torch.randn(B, 3, H, W, generator=g)
    w = torch.zeros(Cout, 32)
    w[:, :27] = torch.randn(Cout, 27, generator=g) * 27 ** -0.5
    return img, w.to(dtype), 0.5 * torch.randn(Cout, generator=g)


def isolate_image(img):
    B, C, H, W = img.shape
    x = img.clone()
    for b in range(B):
        if b + 1 < B:
            x[b, :, H - 1] = 64.0 * img[b + 1, :, 0]
        if b > 0:
            x[b, :, 0] = 64.0 * img[b - 1, :, H - 1]
    return x


def bn_inputs(R, C, zdtype=torch.float32, constant=False):
    """z = offset[c] + std[c] randn with |offset| / std cycling through 0, 1, 3, 10, 30 (constant: channel 1 is exactly 3), weight, bias,
    running statistics, and non-zero accumulators"""
    g = _gen(R, C, 11)
    std = 0.5 + torch.rand(C, generator=g)
    ratio = torch.tensor([0.0, 1.0, -3.0, 10.0, -30.0])[torch.arange(C) % 5]
    z = ratio * std + std * torch.randn(R, C, generator=g)
    if constant:
        z[:, 1] = 3.0
    return dict(z=z.to(zdtype), w=1 + 0.2 * torch.randn(C, generator=g), b=0.3 * torch.randn(C, generator=g),
                rmean=torch.randn(C, generator=g), rvar=0.5 + torch.rand(C, generator=g),
                acc=torch.randn(2, C, generator=g), res=torch.randn(R, C, generator=g), da=torch.randn(R, C, generator=g))


def bn_handed(inp):
    """the fp32 (scale, shift, mean, rstd) a backward is handed: roundings of the float64 statistics of z"""
    f = bn_finalize64(inp["z"], inp["w"], inp["b"])
    return tuple(f[k].float() for k in ("scale", "shift", "mean", "rstd"))


# ---- the checks (shared: the host test hands them an fp32 emulation, the GPU test the kernels) --------------------------------------------
# `impl` has the entry points' Python signatures (vitres.kernels') on CPU tensors and returns CPU tensors.  Every function returns
# {quantity: worst error / bound}; the callers assert <= 1.  Exact statements return 0.0 or inf.
CONV_FORMS = ["plain", "res", "bias_relu", "bias_relu_res"]
PATCH_FORMS = ["res_patch", "bias_relu_patch", "bias_relu_patch_res"]
FORM_SHAPES = [(3, 15, 17), (1, 33, 16), (3, 16, 16), (1, 1, 1)]                # the residual / bias forms run on these (B, H, W)
FORM_COUT = [12, 32]


def exact(a, b):
    return 0.0 if a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) else math.inf


def check_conv3x3(impl, a, w, bias, res, B, H, W, out_dtype, form="plain", P=0, ratio=worst_ratio):
    """one launch of the conv3x3 family on the given operands -> ratio"""
    Cin, Cout = a.shape[-1], w.shape[0]
    u = unit_roundoff(out_dtype)
    if form == "plain":
        got, (ref, bd) = impl.conv3x3(a, w, B, H, W, Cin, Cout, out_dtype), conv3x3_64(a, w, B, H, W)
    elif form == "res":
        got, (ref, bd) = impl.conv3x3_res(a, w, res, B, H, W, Cin, Cout, out_dtype), conv3x3_64(a, w, B, H, W, res=res)
    elif form == "res_patch":
        rc = to_patch(res, B, H, W, P)
        got, (ref, bd) = impl.conv3x3_res_patch(a, w, rc, B, H, W, Cin, Cout, P, out_dtype), conv3x3_64(a, w, B, H, W, res=rc, res_patch=P)
    elif form in ("bias_relu", "bias_relu_res"):
        r = res if form.endswith("res") else None
        got = impl.conv3x3_bias_relu(a, w, bias, r, B, H, W, Cin, Cout, out_dtype)
        ref, bd = conv3x3_64(a, w, B, H, W, bias=bias, relu=True, res=r)
    elif form in ("bias_relu_patch", "bias_relu_patch_res"):
        r = res if form.endswith("res") else None
        got = impl.conv3x3_bias_relu_patch(a, w, bias, r, B, H, W, Cin, Cout, P, out_dtype)
        ref, bd = conv3x3_64(a, w, B, H, W, bias=bias, relu=True, res=r, out_patch=P)
    else:
        raise ValueError(form)
    assert got.dtype == out_dtype
    return ratio(got, ref, out_bound(ref, bd, u))


def run_conv3x3(impl, B, H, W, Cin, Cout, out_dtype, op_dtype=torch.bfloat16, form="plain", P=0, isolate=False):
    a, w, bias, res = conv_inputs(B, H, W, Cin, Cout, op_dtype)
    if isolate:
        a = isolate_batch(a, B, H, W)
    return check_conv3x3(impl, a, w, bias, res, B, H, W, out_dtype, form, P)


def dgrad64(dz, w4, B, H, W):
    """the transposed convolution: dx[b, y, x, ci] = sum_{co, kh, kw} dz[b, y + 1 - kh, x + 1 - kw, co] w4[co, ci, kh, kw] -> (dx, bound at u = 0)"""
    Co, Ci = w4.shape[0], w4.shape[1]
    G, w4 = _padded(dz, B, H, W), f64(w4)
    dx, mag = torch.zeros(B, H, W, Ci, dtype=F64), torch.zeros(B, H, W, Ci, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            s = G[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W, None, :]               # [B, H, W, 1, Co]
            wk = w4[:, :, kh, kw].t()                                             # [Ci, Co]
            dx += (s * wk).sum(-1)
            mag += (s.abs() * wk.abs()).sum(-1)
    return dx.reshape(-1, Ci), 9 * Co * MFMA * mag.reshape(-1, Ci)


def run_dgrad(impl, B, H, W, Ci, Co, out_dtype=torch.float32):
    """conv3x3(dz, conv_w_flip(w)) against the float64 transposed convolution, element by element; the flip itself bit for bit"""
    g = _gen(B, H, W, Ci, Co, 5)
    w4 = torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5
    dz = torch.randn(B * H * W, Co, generator=g).to(torch.bfloat16)
    wf = impl.conv_w_flip(w4, torch.bfloat16)
    got = impl.conv3x3(dz, wf, B, H, W, Co, Ci, out_dtype)
    ref, bd = dgrad64(dz, w4.to(torch.bfloat16), B, H, W)
    return dict(flip=exact(wf, w_flip64(w4).to(torch.bfloat16)), flip32=exact(impl.conv_w_flip(w4, torch.float32), w_flip64(w4)),
                dx=worst_ratio(got, ref, out_bound(ref, bd, unit_roundoff(out_dtype))))


def int_limit(nterms, lim=4):
    """largest |value| <= lim with nterms products below 2^24"""
    while lim > 1 and nterms * lim * lim >= 2 ** 24:
        lim -= 1
    assert nterms * lim * lim < 2 ** 24
    return lim


def run_conv3x3_int(impl, B, H, W, Cin, Cout):
    """integer operands: every partial sum is an integer below 2^24, the fp32 result equals the float64 one"""
    lim = int_limit(9 * Cin)
    a, w = int_inputs((B * H * W, Cin), lim, B, H, W, Cin).to(torch.bfloat16), int_inputs((Cout, 9 * Cin), lim, Cout, Cin).to(torch.bfloat16)
    ref, _ = conv3x3_64(a, w, B, H, W)
    assert float(ref.abs().max()) < 2 ** 24
    return exact(impl.conv3x3(a, w, B, H, W, Cin, Cout, torch.float32), ref.float())


def onehot_pixels(H, W):
    """corner, edges, the tile seam x = 15 / 16, an interior pixel -- those that exist"""
    cand = [(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H // 2, 15), (H // 2, 16), (15, W // 2), (16, W // 2), (H // 2, W // 2)]
    return sorted(set((y, x) for y, x in cand if 0 <= y < H and 0 <= x < W))


def run_conv3x3_onehot(impl, B, H, W, Cin, Cout):
    """a single non-zero (pixel, channel) returns the weights' taps at exactly its 9 neighbours and 0 elsewhere (the contract has no
    rounding: one product per output)"""
    _, w, _, _ = conv_inputs(B, H, W, Cin, Cout)
    worst = 0.0
    for n, (y, x) in enumerate(onehot_pixels(H, W)):
        a = torch.zeros(B, H, W, Cin)
        b, ci = n % B, (5 * n + Cin - 1) % Cin
        a[b, y, x, ci] = 2.0
        a = a.reshape(-1, Cin).to(torch.bfloat16)
        ref, _ = conv3x3_64(a, w, B, H, W)
        assert int((ref != 0).any(-1).sum()) <= 9
        worst = max(worst, exact(impl.conv3x3(a, w, B, H, W, Cin, Cout, torch.float32), ref.float()))
    return worst


def run_conv1(impl, B, H, W, Cout, out_dtype, op_dtype=torch.bfloat16, bias=False, relu=False, isolate=False):
    img, w, bs = conv1_inputs(B, H, W, Cout, op_dtype)
    if isolate:
        img = isolate_image(img)
    got = impl.conv1_direct(img, w, bs if bias else None, relu, out_dtype)
    ref, bd = conv1_64(img, w, op_dtype, bs if bias else None, relu)
    return worst_ratio(got, ref, out_bound(ref, bd, unit_roundoff(out_dtype)))


def run_conv1_int(impl, B, H, W, Cout):
    img = int_inputs((B, 3, H, W), 4, B, H, W)
    w = torch.zeros(Cout, 32)
    w[:, :27] = int_inputs((Cout, 27), 4, Cout)
    w = w.to(torch.bfloat16)
    ref, _ = conv1_64(img, w, torch.bfloat16)
    return exact(impl.conv1_direct(img, w, None, False, torch.float32), ref.float())


def run_conv1_onehot(impl, B, H, W, Cout):
    _, w, _ = conv1_inputs(B, H, W, Cout)
    worst = 0.0
    cand = [(0, 0), (H - 1, W - 1), (H // 2, 62), (H // 2, 63), (H // 2, 64), (15, W // 2), (16, W // 2), (H // 2, W // 2)]
    for n, (y, x) in enumerate(sorted(set((y, x) for y, x in cand if 0 <= y < H and 0 <= x < W))):
        img = torch.zeros(B, 3, H, W)
        img[n % B, n % 3, y, x] = 2.0
        ref, _ = conv1_64(img, w, torch.bfloat16)
        assert int((ref != 0).any(-1).sum()) <= 4                       # stride 2: at most 2 x 2 outputs see a pixel
        worst = max(worst, exact(impl.conv1_direct(img, w, None, False, torch.float32), ref.float()))
    return worst


def wgrad_inputs(B, H, W, C, integer=False):
    if integer:
        lim = int_limit(B * H * W)
        return (int_inputs((B * H * W, C), lim, B, H, W, C, 1).to(torch.bfloat16), int_inputs((B * H * W, C), lim, B, H, W, C, 2).to(torch.bfloat16),
                int_inputs((C, 9 * C), 4, C, 3))
    g = _gen(B, H, W, C, 9)
    return (torch.randn(B * H * W, C, generator=g).to(torch.bfloat16), torch.randn(B * H * W, C, generator=g).to(torch.bfloat16),
            torch.randn(C, 9 * C, generator=g))


def run_wgrad(impl, B, H, W, C, integer=False):
    a, dz, dw0 = wgrad_inputs(B, H, W, C, integer)
    got = impl.conv3x3_wgrad(a, dz, dw0.clone(), B, H, W, C, C)
    ref, bd = wgrad64(a, dz, dw0, B, H, W)
    if integer:
        assert float(bd.max()) / (2 * wgrad_depth(B, H, W) * U32) < 2 ** 24          # sum|dz a| + |dw0|: every partial sum is exact
        return exact(got, ref.float())
    return worst_ratio(got, ref, bd)


def run_bn_forward(impl, R, C, zdtype=torch.float32, constant=False, update_running=True, momentum=BN_MOMENTUM):
    """bn_stats into non-zero accumulators, then bn_stats -> bn_finalize against BatchNorm2d's statistics of z"""
    inp = bn_inputs(R, C, zdtype, constant)
    z, r = inp["z"], {}
    s, q = impl.bn_stats(z, inp["acc"][0].clone(), inp["acc"][1].clone())
    st = bn_stats64(z, inp["acc"][0], inp["acc"][1])
    r["sum+"], r["sumsq+"] = worst_ratio(s, st["sum"], st["bsum"]), worst_ratio(q, st["sumsq"], st["bsumsq"])
    s, q = impl.bn_stats(z, torch.zeros(C), torch.zeros(C))
    nbt0 = torch.tensor(41, dtype=torch.int64)
    scale, shift, mean, rstd, rm, rv, nbt = impl.bn_finalize(s, q, R, inp["w"], inp["b"], BN_EPS, momentum, inp["rmean"].clone(), inp["rvar"].clone(),
                                                             nbt0.clone(), update_running)
    f = bn_finalize64(z, inp["w"], inp["b"], BN_EPS, momentum, inp["rmean"], inp["rvar"])
    const = torch.zeros(C, dtype=torch.bool)                              # the channels whose variance is exactly 0
    const[1] = constant
    const[:] |= R == 1
    assert bool(torch.equal(f["var"] == 0, const))
    assert bool(f["valid"][~const].all()), "the first-order rstd bound needs dvar <= (var + eps) / 4 on every random-input channel"
    got = dict(mean=mean, rstd=rstd, scale=scale, shift=shift, rmean=rm, rvar=rv)
    if bool(const.any()):
        assert degenerate_ok(rstd[const], BN_EPS) and bool(torch.isfinite(torch.stack([scale[const], shift[const]])).all())
    for k in FINALIZE_KEYS + (("rmean", "rvar") if update_running else ()):
        sel = torch.ones(C, dtype=torch.bool) if k in ("mean", "rmean", "rvar") else ~const
        r[k] = worst_ratio(got[k][sel], f[k][sel], f["b" + k][sel])
    if update_running:
        r["nbt"] = 0.0 if int(nbt) == 42 else math.inf
    else:
        r["untouched"] = max(exact(rm, inp["rmean"]), exact(rv, inp["rvar"]), 0.0 if int(nbt) == 41 else math.inf)
    return r


def run_bn_relu(impl, R, C, zdtype, out_dtype, with_res, B=0, H=0, W=0, P=0):
    inp = bn_inputs(R, C, zdtype)
    scale, shift, _, _ = bn_handed(inp)
    res = inp["res"].to(out_dtype) if with_res else None
    if P:
        got = impl.bn_relu_patch(inp["z"], scale, shift, res, B, H, W, P, out_dtype)
    else:
        got = impl.bn_relu(inp["z"], scale, shift, res, out_dtype)
    ref, bd = bn_relu64(inp["z"], scale, shift, res, B, H, W, P)
    return worst_ratio(got, ref, out_bound(ref, bd, unit_roundoff(out_dtype)))


def bn_bwd_case(R, C, zdtype, da_dtype, training, B=0, H=0, W=0, P=0, **inject):
    """-> (inputs, float64 contract) of one backward case"""
    inp = bn_inputs(R, C, zdtype)
    handed = bn_handed(inp)
    da = inp["da"].to(da_dtype)
    if P:
        da = to_patch(da, B, H, W, P)
    ref = bn_bwd64(da, inp["z"], *handed, inp["acc"][0], inp["acc"][1], training, unit_roundoff(da_dtype), B, H, W, P, **inject)
    return (da, inp["z"], handed, inp["acc"]), ref


def run_bn_bwd(impl, R, C, zdtype, da_dtype, training, B=0, H=0, W=0, P=0):
    (da, z, handed, acc), ref = bn_bwd_case(R, C, zdtype, da_dtype, training, B, H, W, P)
    assert ref["undecided"] <= undecided_cap(ref["numel"]), (ref["undecided"], ref["numel"])
    if P:
        dz, sg, sgz = impl.bn_bwd_patch(da, z, *handed, acc[0].clone(), acc[1].clone(), training, B, H, W, P)
    else:
        dz, sg, sgz = impl.bn_bwd(da, z, *handed, acc[0].clone(), acc[1].clone(), training)
    assert dz.dtype == da.dtype
    return dict(sg=worst_ratio(sg, ref["sg"], ref["bsg"]), sgz=worst_ratio(sgz, ref["sgz"], ref["bsgz"]), dz=bwd_dz_ratio(dz, ref))


def bn_zero_probe(C=16, R=40):
    """exact inputs with pre-activations that are exactly 0: z in {-2 .. 2}, scale = 1, shift = 0, mean = 0, rstd = 1, da = 1 + (r mod 3).  z = 0 has
    pre = 0 with an error bound of 0: decided, and masked (the mask is strict)"""
    z = int_inputs((R, C), 2, R, C, 77)
    z[::3] = 0.0
    da = (1 + torch.arange(R) % 3).float()[:, None].expand(R, C).contiguous()
    return da, z, (torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C))


def run_bn_zero_probe(impl, training=True, **inject):
    da, z, handed = bn_zero_probe()
    R, C = z.shape
    ref = bn_bwd64(da, z, *handed, torch.zeros(C), torch.zeros(C), training, 0.0, **inject)
    assert ref["undecided"] == 0
    dz, sg, sgz = impl.bn_bwd(da, z, *handed, torch.zeros(C), torch.zeros(C), training)
    return dict(sg=exact(sg, ref["sg"].float()), sgz=exact(sgz, ref["sgz"].float()), dz=worst_ratio(dz, ref["dz"], ref["bdz"]))


def run_layouts(impl, B, H, W, C, dtype):
    """the permutation / cast kernels, bit for bit, and col2im inside its bound"""
    g = _gen(B, H, W, C, 13)
    a = torch.randn(B * H * W, C, generator=g).to(dtype)
    r = dict(im2col=exact(impl.im2col3x3(a, B, H, W, C), im2col_nhwc(a, B, H, W)))
    dcol = torch.randn(B * H * W, 9 * C, generator=g).to(dtype)
    ref, bd = col2im64(dcol, B, H, W, unit_roundoff(dtype))
    r["col2im"] = worst_ratio(impl.col2im3x3(dcol, B, H, W, C), ref, bd)
    return r


def run_unfold(impl, B, H, W, P, C, dtype):
    a = torch.randn(B * H * W, C, generator=_gen(B, H, W, P, C)).to(dtype)
    col = impl.patch_unfold(a, B, H // P, W // P, P, C)
    return dict(unfold=exact(col, to_patch(a, B, H, W, P)), fold=exact(impl.patch_fold(col, B, H // P, W // P, P, C), a))


def run_im2col_image(impl, B, H, W, C, stride, ld, dtype):
    img = torch.randn(B, C, H, W, generator=_gen(B, H, W, C, stride, ld))
    return exact(impl.im2col3x3_image(img, stride, ld, dtype), im2col_image(img, stride, ld, dtype))


# ---- the cases (one list for the emulation on the host and the kernels on the GPU) ------------------------------------------------------
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def conv_cases(Cin):
    """keyword sets of run_conv3x3: every (H, W), B, Cout in fp32 and bf16; fp16 operands; the residual / bias / patch forms; isolation"""
    for H, W in CONV_HW:
        for B in CONV_B:
            for Cout in CONV_COUT:
                for dt in (F32, BF):
                    yield dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, out_dtype=dt)
        for Cout in FORM_COUT:
            yield dict(B=3, H=H, W=W, Cin=Cin, Cout=Cout, out_dtype=F16, op_dtype=F16)
        yield dict(B=3, H=H, W=W, Cin=Cin, Cout=32, out_dtype=F32, isolate=True)
        yield dict(B=3, H=H, W=W, Cin=Cin, Cout=20, out_dtype=BF, isolate=True, form="bias_relu_res")
    for B, H, W in FORM_SHAPES:
        for Cout in FORM_COUT:
            for form in CONV_FORMS[1:]:
                for dt, op in ((F32, BF), (BF, BF), (F16, F16)):
                    yield dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, out_dtype=dt, op_dtype=op, form=form)
    for H, W, P in PATCH_SHAPES:
        for B in (1, 3):
            for form in PATCH_FORMS:
                for dt, op in ((F32, BF), (BF, BF), (F16, F16)):
                    yield dict(B=B, H=H, W=W, Cin=Cin, Cout=Cin, out_dtype=dt, op_dtype=op, form=form, P=P)


def dgrad_cases():
    for H, W in CONV_HW:
        for Ci, Co in ((16, 16), (24, 32), (32, 24), (12, 32), (20, 16)):         # (Co is the contraction here: 16 / 24 / 32)
            yield dict(B=3, H=H, W=W, Ci=Ci, Co=Co)


def conv1_cases(Cout):
    for i, (H, W) in enumerate(CONV1_HW):
        for bias in (False, True):
            for relu in (False, True):
                for dt, op in ((F32, BF), (BF, BF), (F16, F16)):
                    yield dict(B=1 + 2 * (i % 2), H=H, W=W, Cout=Cout, out_dtype=dt, op_dtype=op, bias=bias, relu=relu)
        yield dict(B=3, H=H, W=W, Cout=Cout, out_dtype=F32, bias=True, relu=True, isolate=True)


def wgrad_cases(C):
    for H, W in CONV_HW:
        yield dict(B=3, H=H, W=W, C=C)
        yield dict(B=3, H=H, W=W, C=C, integer=True)


def bn_forward_cases(C):
    for i, R in enumerate(bn_rows(C)):
        for zd in (F32, BF):
            yield dict(R=R, C=C, zdtype=zd, update_running=(i % 3 != 1), momentum=(0.1, 0.25)[i % 2])
    yield dict(R=bn_rows(C)[3], C=C, constant=True)
    yield dict(R=bn_rows(C)[-1], C=C, constant=True, zdtype=BF)


BN_DTYPES = [(F32, F32), (F32, BF), (BF, BF)]          # (z, da / out): the combinations the entry points accept


def bn_relu_cases(C):
    for R in bn_rows(C):
        for zd, od in BN_DTYPES:
            for with_res in (False, True):
                yield dict(R=R, C=C, zdtype=zd, out_dtype=od, with_res=with_res)


def bn_bwd_cases(C):
    for R in bn_rows(C):
        for zd, dd in BN_DTYPES:
            for training in (True, False):
                yield dict(R=R, C=C, zdtype=zd, da_dtype=dd, training=training)


def bn_patch_cases():
    for H, W, P in PATCH_SHAPES:
        for C in (24, 32):
            for zd, od in BN_DTYPES:
                yield dict(R=2 * H * W, C=C, zdtype=zd, B=2, H=H, W=W, P=P), od


def layout_cases():
    for H, W in CONV_HW:
        for C in (8, 24, 32):
            for dt in (F32, BF):
                yield dict(B=3, H=H, W=W, C=C, dtype=dt)


def image_cases():
    """both strides, ld 27 and 32 (ld = 32 in 16 bits with 3 channels is the row kernel), a generic channel count"""
    for H, W in CONV1_HW:
        for stride in (1, 2):
            for ld in (27, 32):
                for dt in (F32, BF, F16):
                    yield dict(B=2, H=H, W=W, C=3, stride=stride, ld=ld, dtype=dt)
        yield dict(B=2, H=H, W=W, C=5, stride=2, ld=48, dtype=BF)


def worst_of(r):
    return max(r.values()) if isinstance(r, dict) else r
