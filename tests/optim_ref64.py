"""Contracts of the step tail of csrc/optim.hip -- the AdamW pass over the flat arena (vr_adamw_flat, _dev, _dev_capped, _clip) and the
gradient-norm launches in front of it (vr_grad_sumsq, vr_clip_finish and their gated forms) -- in float64 numpy on the CPU; per-element
bounds derived below from the operation count; the launch arithmetic of adamw_launch and sumsq_launch; inputs, hyper-parameter sets and
case lists shared by tests/test_optim_ref_host.py (CPU) and tests/test_gpu_optim.py (device).

AdamW contract.  Float64 arithmetic on the fp32 inputs and on the hyper-parameters AS THE fp32 VALUES of vr_adamw_group (the rounding of
lr, 1 - beta1^t, ... to fp32 happens on the host and is the caller's, not the kernel's):
    gr   = g * grad_scale [* coef]                                 coef: the clip coefficient of vr_adamw_flat_clip
    x    = p * (1 - lr * wd)
    m'   = b1 m + (1 - b1) gr
    v'   = b2 v + (1 - b2) gr^2
    p'   = x - (lr / bias_c1) * m' / (sqrt(v') / sqrt_bias_c2 + eps)
    ema' = d ema + (1 - d) p'                                       d: the fp32 argument; 1 - d evaluated on that fp32 value
    shadow = round-to-nearest-even bf16 of the DEVICE's own p' bits: exact, not bounded (a NaN p' gives a NaN; payloads are not compared)
A group byte of 255, and for the _dev forms a group whose bias_c1 is 0, leave every bit of p, m, v, shadow and ema as it was.
test_optim_ref_host.py ties this to torch.optim.AdamW in float64 (five steps, two groups, 1e-12 relative).

EMA weights.  The kernel evaluates 1 - d on the fp32 value of d, so its two weights sum to exactly 1.  timm's ModelEmaV2 (the reference,
main.py:357-363) computes `1. - decay` in double; run in fp32 tensors that weight is the fp32 rounding of the double 1 - d, while d
itself is rounded to fp32 separately.  At d = 0.99996 fp32(d) = 0.999960005..., 1 - fp32(d) = 3.99947e-5 and fp32(1 - 0.99996) = 4.0e-5:
the per-step weights of the new parameters differ by 1.3e-4 relative, and the reference's two weights do not sum to 1.  Recorded, not
changed: the contract here is the kernel's statement in include/vitres_hip.h.

Bounds.  u = 2^-24, g(k) = k u / (1 - k u) (k roundings that multiply), every fp32 +, -, *, /, sqrt is correctly rounded (hipcc's default for
HIP: no fast-math, IEEE divide and sqrt) and optim.hip is built with the default contraction, so `a * b + c` may be ONE rounding
(fma) or two.  Every count below is for the uncontracted form, which has the most roundings; a contraction removes one and never adds any,
so both forms fit.  eg = roundings in gr: 1 (g * grad_scale), 2 with a clip coefficient other than 1.  D = 2^-149, one denormal quantum,
is added to every bound for a result that underflows.
    gr^ = gr (1 + t), |t| <= g(eg).
    m'^ = fl(fl(b1 m) + fl(fl(1 - b1) gr^)): the first term carries its product and the sum, the second fl(1 - b1), its product, the sum and gr^:
          dm <= g(2) |b1 m| + g(3 + eg) |(1 - b1) gr| + D                     (nothing cancels in the bound: the terms enter by magnitude)
    v'^ = fl(fl(b2 v) + fl(fl(fl(1 - b2) gr^) gr^)): all terms >= 0 (v >= 0), so the error is relative to v': the second term carries fl(1 - b2), two
          products, the sum and gr^ twice, the first only two roundings:
          dv <= g(4 + 2 eg) v' + D
    denom^ = fl(fl(sqrt(v'^) / sqrt_bias_c2) + eps): sqrt halves the relative error of v'^ and adds one rounding, the division one more:
          (3 + eg) + 1 = 4 + eg on sqrt(v') / sqrt_bias_c2; both summands >= 0, the sum rounds once: 5 + eg relative on denom.
    step^ = fl(fl(lr / bias_c1) * fl(m'^ / denom^)): three more roundings (two quotients, one product) on top of denom's, and m'^ itself:
          dstep <= g(8 + eg) |step| + (1 + g(8 + eg)) (lr / bias_c1) / denom * dm
    x^ = fl(p * fl(1 - fl(lr wd))): fl(lr wd) is off by u lr wd absolute, which moves the factor by u lr wd / |1 - lr wd| relative; the
          subtraction and the product round once each:
          dx <= (g(2) + u lr wd / |1 - lr wd|) |x|                                (= 3 u |x| at most for lr wd <= 1/2)
    p'^ = fl(x^ - step^): dp <= dx + dstep + u (|p'| + dx + dstep) + D
    ema'^ = fl(fl(d ema) + fl(fl(1 - d) p'^)): dema <= g(2) |d ema| + g(3) |(1 - d) p'| + (1 + g(3)) |1 - d| dp + D
Non-finite inputs.  The contract is evaluated with IEEE semantics: a NaN or inf in g gives the non-finite m', v', p', ema' the formula gives
(inf / inf = NaN in p'), and ratio() wants the same class (NaN, +inf, -inf) from the device at such elements.

vr_grad_sumsq contract.  partials[b] for b < active = the float64 sum of g^2 over the groups of eight i = b * 256 + thread + k * active * 256
whose byte is not 255; for b >= active EXACTLY +0.0.  Path: every thread keeps eight chains acc = fma(g, g, acc), one rounding per term,
L = ceil(n8 / (active * 256)) terms at most; then a tree of 3 (in the thread) + 6 (the wave's butterfly) + 2 (across the four waves)
additions.  All terms >= 0, so on each partial
          dpart <= g(L + 11) part + D.

vr_clip_finish contract.  norm is within one fp32 ulp of fp32(grad_scale * sqrt(sum of the partials in float64)) (the device adds the
partials in double in its own order, then rounds once to fp32: the two roundings can land on neighbouring fp32 values); coef, skip and
skipped are then EXACT functions of the device's own norm bits, fp32 arithmetic throughout:
    bad = norm is inf or NaN;  coef = bad ? 0 : fminf(1, max_norm / (norm + 1e-6f));  skip = bad;  skipped += bad.
The gated forms at gate != 0 give the same bits; at gate 0 they leave every byte of the partial sums / the state as it was."""
import math

import numpy as np

U = 2.0 ** -24
D = 2.0 ** -149
VR_OK, VR_EINVAL, VR_EALIGN, VR_EUNSUPPORTED = 0, -1, -2, -3
MAX_GROUPS = 16
DEFAULT_CAP = 8192                # adamw_launch: workgroups of the default grid
CANARY32 = 0x7fd57fd5             # one NaN bit pattern: guard zones and the regions a kernel must leave alone (tests/glue_ref64.py)
CANARY16 = 0x7fd5
GUARD = 8                         # elements in front of every guarded view: the arrays sit at an 8-element offset of their allocation
FIELDS = ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_c1", "sqrt_bias_c2", "grad_scale")
LR, B1, B2, EPS, WD, BC1, SBC2, GS = range(8)


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- launch paths, restated from adamw_launch and sumsq_launch -----------------------------------------------------------------------------------
def adamw_path(n, max_blocks=0):
    """-> (workgroups, grid-stride passes, threads live in the last pass)"""
    n8 = n // 8
    blocks = min((n8 + 255) // 256, max_blocks if max_blocks > 0 else DEFAULT_CAP)
    per = blocks * 256
    passes = (n8 + per - 1) // per
    return blocks, passes, n8 - (passes - 1) * per


def sumsq_path(n, n_partials, max_blocks=0):
    """-> (workgroups that have work, workgroups that write 0, terms of the longest chain)"""
    n8 = n // 8
    active = min((n8 + 255) // 256, n_partials)
    if max_blocks > 0:
        active = min(active, max_blocks)
    return active, n_partials - active, (n8 + active * 256 - 1) // (active * 256)


# the smallest sizes that reach each path: (n, max_blocks)
ADAMW_CASES = [(8, 0), (2040, 0), (2048, 0), (2056, 0), (4096, 2), (4104, 2), (8200, 2)]
ADAMW_BIG = 8 * (8192 * 256 + 257)                     # 16 779 272: a second pass of 257 threads under the default cap
BIG_SAMPLE = 2 ** 18                                   # float64 bounds of the big case on a strided sample of at most this many elements
SUMSQ_CASES = [(8, 1, 0), (8, 5, 0), (2048, 1, 0), (2056, 2, 0), (2056, 1, 0), (8 * 256 * 3 + 8, 4, 2), (8 * 256 * 300, 1, 0)]


# ---- hyper-parameter sets ------------------------------------------------------------------------------------------------------------------------
T_LIST = [1, 2, 10, 100000]
GROUP_SETS = ["two", "sixteen"]
GRAD_SCALES = [1.0, 0.125]
COEFS = [None, 0.37]
EMA_DECAYS = [None, 0.99, 0.99996]                     # the last is the reference's default (--model-ema-decay)


def bias_corrections(b1, b2, t):
    return 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)


def group_rows(kind):
    """(lr, weight_decay) per group: two groups as engine.param_groups_weight_decay makes them (decay / no decay) with different learning
    rates, or sixteen -- VR_ADAMW_MAX_GROUPS -- all different, every other one without decay"""
    if kind == "two":
        return [(1e-3, 0.05), (3e-4, 0.0)]
    return [(1e-3 * 0.83 ** i, 0.0 if i % 2 else 0.01 * (i + 1)) for i in range(MAX_GROUPS)]


def groups_f64(kind, t, grad_scale, betas=(0.9, 0.999), eps=1e-8):
    """[G, 8] float64 in the field order of vr_adamw_group, before any rounding (FlatAdamW._group_structs computes these doubles)"""
    bc1, sbc2 = bias_corrections(betas[0], betas[1], t)
    return np.array([[lr, betas[0], betas[1], eps, wd, bc1, sbc2, grad_scale] for lr, wd in group_rows(kind)], dtype=np.float64)


def groups_f32(kind, t, grad_scale):
    """the structs the kernel gets: every field rounded to fp32 once"""
    return groups_f64(kind, t, grad_scale).astype(np.float32)


def hyper_sets(coefs=COEFS):
    """every (t, group set, grad_scale, coef, ema_decay)"""
    return [(t, ks, gs, c, d) for t in T_LIST for ks in GROUP_SETS for gs in GRAD_SCALES for c in coefs for d in EMA_DECAYS]


def hyper_name(h):
    return "t=%d %s gs=%g coef=%s ema=%s" % h


def group_bytes(n, n_groups, holes=()):
    """one byte per eight elements, the groups interleaved every group of eight; holes: (lo8, hi8) stretches of 255"""
    gid = (np.arange(n // 8) % n_groups).astype(np.uint8)
    for lo, hi in holes:
        gid[lo:hi] = 255
    return gid


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ["typ", "tiny", "cold", "cancel", "zero", "big"]


def family_of(n):
    """index into FAMILIES per element: consecutive elements cycle through the six, shifted by one every 128 elements, so every family
    meets every group byte and every lane position, and one group of eight (n = 8) already holds all six"""
    j = np.arange(n)
    return (j + j // 128) % len(FAMILIES)


def adamw_inputs(n, seed):
    """-> dict of fp32 arrays p, g, m, v, ema.  The six families share one arena (the update is element-wise): family_of(n) says which
    element is which.  p holds exact zeros at every 7th element: there the update alone decides the result, and a bound relative to |p|
    cannot hide it.
      typ     g, m ~ 1e-3, v ~ 1e-6            tiny    the same at 1e-12 (v ~ 1e-24): eps decides the denominator
      cold    m = v = 0 (the first step)       cancel  b1 m = -(1 - b1) g up to 1e-3 relative: m' is what the roundings leave
      zero    g = 0                            big     g ~ 1e3 (an unscaled loss), m, v as typ"""
    r = np.random.default_rng(seed)
    fam = family_of(n)
    p = r.standard_normal(n) * 0.02
    p[::7] = 0.0
    ema = p + r.standard_normal(n) * 1e-3
    g = r.standard_normal(n) * 1e-3
    m = r.standard_normal(n) * 1e-3
    v = (r.standard_normal(n) * 1e-3) ** 2 + 1e-9
    tiny = fam == 1
    g[tiny] *= 1e-9
    m[tiny] *= 1e-9
    v[tiny] *= 1e-18
    cold = fam == 2
    m[cold] = 0.0
    v[cold] = 0.0
    cancel = fam == 3
    g32 = g.astype(np.float32).astype(np.float64)
    m[cancel] = -(1.0 - 0.9) / 0.9 * g32[cancel] * (1.0 + 1e-3 * r.standard_normal(int(cancel.sum())))
    g[fam == 4] = 0.0
    g[fam == 5] *= 1e6
    out = {k: a.astype(np.float32) for k, a in (("p", p), ("g", g), ("m", m), ("v", v), ("ema", ema))}
    assert (out["v"] >= 0).all() and (out["p"][::7] == 0).all()
    return out


SUMSQ_FAMILIES = ["randn", "ramp", "one"]


def sumsq_inputs(kind, n, seed=5):
    """randn * 3e-3; a geometric ramp from 1e-6 to 1e2 (fourteen decades of g^2 in one chain); one element of 1.0 among 1e-4s, placed in
    lane 0's first chain (element 0): every later term of that chain is 1e-8 against an accumulator of 1.  No square underflows."""
    if kind == "randn":
        g = np.random.default_rng(seed).standard_normal(n) * 3e-3
    elif kind == "ramp":
        g = 1e-6 * 1e8 ** (np.arange(n) / max(n - 1, 1))
        g[1::2] *= -1.0
    else:
        g = np.full(n, 1e-4)
        g[0] = 1.0
    return g.astype(np.float32)


# ---- canaries and integer views (numpy) ----------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def canary32(n):
    return np.full(n, CANARY32, dtype=np.uint32).view(np.float32)


def bf16_rne(x):
    """fp32 -> the 16 bits of its round-to-nearest-even bfloat16 (uint16); NaN -> a NaN"""
    u = bits(x.astype(np.float32)).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7fc0), r)


def shadow_mismatches(shadow_bits, p_new):
    """elements whose shadow (uint16) is not the bf16 of p_new (fp32, the device's own bits); two NaNs agree whatever their payload"""
    want = bf16_rne(p_new)
    nan16 = (shadow_bits & 0x7fff) > 0x7f80
    return np.where(np.isnan(p_new), ~nan16, shadow_bits != want)


def ratio(got, ref, bound, where=None):
    """worst |got - ref| / bound over `where`.  A non-finite reference wants the same class from the device (NaN / +inf / -inf); anything
    else non-finite, or an error against a zero bound, gives inf."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(err == 0, 0.0, err / bound)
    same_class = (np.isnan(ref) & np.isnan(got)) | (np.isinf(ref) & (got == ref))
    r = np.where(same_class, 0.0, np.where(np.isfinite(ref) & np.isfinite(got), r, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    if where is not None:
        r = r[where]
    return float(r.max()) if r.size else 0.0


WORST = {}                        # (kernel, output) -> worst ratio seen, printed last by both suites


def record(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


# ---- the AdamW contract and its bounds -----------------------------------------------------------------------------------------------------------
def live_elements(gid, groups, dev):
    """bool per element: updated at all (byte != 255, and for the _dev forms bias_c1 != 0)"""
    ge = np.repeat(gid.astype(np.int64), 8)
    live = ge != 255
    if dev:
        live &= np.asarray(groups, dtype=np.float64)[np.where(live, ge, 0), BC1] != 0
    return live


def adamw_contract(a, gid, groups, coef=None, d=None, dev=False):
    """a: dict of arrays p, g, m, v (and ema when d is given); gid: one byte per eight elements; groups: [G, 8] (fp32 as the kernel gets
    them, or float64 for the tie to torch); coef: None or the fp32 clip coefficient; d: None or the fp32 ema_decay.
    -> (ref, bound, live): float64 dicts over p, m, v (, ema).  Elements that are not live keep their input and have bound 0: the callers
    compare those by bits."""
    H = np.asarray(groups, dtype=np.float64)
    ge = np.repeat(gid.astype(np.int64), 8)
    live = live_elements(gid, H, dev)
    h = H[np.where(live, ge, 0)]
    p, g, m, v = (np.asarray(a[k], dtype=np.float64) for k in "pgmv")
    eg = 1 if coef is None or float(coef) == 1.0 else 2
    with np.errstate(all="ignore"):
        gr = g * h[:, GS] * (1.0 if coef is None else float(np.float32(coef)))
        lw = h[:, LR] * h[:, WD]
        x = p * (1.0 - lw)
        t1, t2 = h[:, B1] * m, (1.0 - h[:, B1]) * gr
        m1 = t1 + t2
        v1 = h[:, B2] * v + (1.0 - h[:, B2]) * gr * gr
        denom = np.sqrt(v1) / h[:, SBC2] + h[:, EPS]
        s = h[:, LR] / h[:, BC1]
        step = s * (m1 / denom)
        p1 = x - step
        dm = gamma(2) * np.abs(t1) + gamma(3 + eg) * np.abs(t2) + D
        dv = gamma(4 + 2 * eg) * v1 + D
        dstep = gamma(8 + eg) * np.abs(step) + (1.0 + gamma(8 + eg)) * np.abs(s / denom) * dm
        dx = (gamma(2) + U * np.abs(lw) / np.abs(1.0 - lw)) * np.abs(x)
        dp = dx + dstep + U * (np.abs(p1) + dx + dstep) + D
        ref = {"p": np.where(live, p1, p), "m": np.where(live, m1, m), "v": np.where(live, v1, v)}
        bound = {"p": np.where(live, dp, 0.0), "m": np.where(live, dm, 0.0), "v": np.where(live, dv, 0.0)}
        if d is not None:
            e, dd = np.asarray(a["ema"], dtype=np.float64), float(np.float32(d))
            e1 = dd * e + (1.0 - dd) * p1
            de = gamma(2) * np.abs(dd * e) + gamma(3) * np.abs((1.0 - dd) * p1) + (1.0 + gamma(3)) * abs(1.0 - dd) * dp + D
            ref["ema"], bound["ema"] = np.where(live, e1, e), np.where(live, de, 0.0)
    return ref, bound, live


def adamw_verdict(before, got, gid, groups, coef=None, d=None, dev=False, where=None):
    """before / got: dicts of the arrays in front of and behind one launch: p, g, m, v fp32, `ema` fp32 when d is given, `shadow` (uint16
    bits) when the launch wrote one.  -> {output: worst error / bound over `where`} for p, m, v (, ema), plus two exact verdicts that are 0
    or inf: "shadow" (live elements hold the bf16 of the device's own p') and "untouched" (every bit of every output of an element that
    is not live is as before)."""
    ref, bound, live = adamw_contract(before, gid, groups, coef, d, dev)
    sel = np.ones(live.size, dtype=bool) if where is None else where
    out = {k: ratio(got[k], ref[k], bound[k], live & sel) for k in ref}
    moved = np.zeros(live.size, dtype=bool)
    for k in list(ref) + (["shadow"] if "shadow" in got else []) + ([] if d is not None or "ema" not in got else ["ema"]):
        moved |= bits(got[k]) != bits(before[k])
    out["untouched"] = math.inf if (moved & ~live & sel).any() else 0.0
    if "shadow" in got:
        out["shadow"] = math.inf if (shadow_mismatches(got["shadow"], got["p"]) & live & sel).any() else 0.0
    return out


# ---- the gradient-norm contracts -----------------------------------------------------------------------------------------------------------------
def sumsq_contract(g, gid, n_partials, max_blocks=0):
    """-> (partials float64 [n_partials], bound, active).  Slots >= active are exactly +0.0 (bound 0)."""
    n8 = g.size // 8
    active, _, chain = sumsq_path(g.size, n_partials, max_blocks)
    sq = (np.asarray(g, dtype=np.float64) ** 2).reshape(n8, 8).sum(1) * (gid != 255)
    owner = (np.arange(n8) % (active * 256)) // 256
    part = np.zeros(n_partials)
    np.add.at(part, owner, sq)
    bound = np.where(np.arange(n_partials) < active, gamma(chain + 11) * part + D, 0.0)
    return part, bound, active


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def norm_ref(partials, grad_scale):
    """the float64 value the device rounds: grad_scale * sqrt(sum); the device's norm is within one fp32 ulp of its fp32 rounding"""
    with np.errstate(all="ignore"):
        return float(np.float64(np.float32(grad_scale)) * np.sqrt(np.asarray(partials, dtype=np.float64).sum()))


def norm_matches(norm, partials, grad_scale):
    want = norm_ref(partials, grad_scale)
    if math.isnan(want):
        return math.isnan(float(norm))
    with np.errstate(over="ignore"):
        w32 = np.float32(want)
    if np.isinf(w32):
        return float(norm) == float(w32)
    return abs(float(norm) - float(w32)) <= ulp32(w32)             # (an infinite norm fails here)


def clip_outputs(norm, max_norm, skipped_before):
    """-> (coef fp32, skip, skipped): the exact functions of the device's own norm (fp32) the contract states"""
    norm, one = np.float32(norm), np.float32(1.0)
    if not np.isfinite(norm):
        return np.float32(0.0), 1, skipped_before + 1
    with np.errstate(all="ignore"):
        q = np.float32(max_norm) / (norm + np.float32(1e-6))
    return (one if not q < one else q), 0, skipped_before             # fminf(1, q): q when q < 1, else 1


def norm_bound_rel(n, n_partials, max_blocks=0):
    """relative bound of the device's norm against the float64 norm of the same gradient: every partial is within G = g(L + 11) of its own
    sum and all terms are >= 0, so the total is too, and the square root maps 1 -+ G to within 1 - sqrt(1 - G) of 1 (G / 2 to first
    order); the sum and the root in double add a few 2^-53 (2^-48 covers 2048 * 8 partials), the one rounding to fp32 adds u."""
    chain = sumsq_path(n, n_partials, max_blocks)[2]
    return (1.0 - math.sqrt(1.0 - gamma(chain + 11))) * (1.0 + U) + U + 2.0 ** -48
