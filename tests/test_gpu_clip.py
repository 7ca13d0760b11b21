"""Gradient-norm clipping on the device (FlatAdamW(max_norm=...): vr_grad_sumsq -> vr_clip_finish -> vr_adamw_flat_clip), eager and
inside the captured train step.  The reference for every case is torch itself on the same gradients --
torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW, what the reference's loss_scaler(..., clip_grad=max_norm) calls."""
import math
import subprocess

import pytest
import torch

import optim_ref64
import recipe
import vitres
import vitres_oracle as O
from vitres import _lib, engine
from vitres.losses import SoftTargetCrossEntropy
from vitres.optim import NORM_PARTIALS, FlatAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build(seed=100, dtype=torch.bfloat16):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30, single_arch=False,
              hybrid_arch=False)
    nd = recipe.MICRO_DEFS[0]
    prod = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                               num_classes=recipe.MICRO_CLASSES, network_def=nd, drop_path_rate=0.0, drop_block_rate=None, **kw)
    orc = O.OracleViTSR(nd, img_size=recipe.MICRO_IMG, num_classes=recipe.MICRO_CLASSES, supernet=True, patch_output=True, **kw)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in orc.state_dict().items()], seed)
    prod.load_state_dict(sd)
    prod = prod.to(DEV)
    prod.set_compute_dtype(dtype)
    prod.train()
    prod.set_epoch(31)
    prod.load_state_dict(sd)
    return prod


def rel(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


def groups(model):
    return engine.param_groups_weight_decay(model, 0.05)


def torch_norm(model):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))


# ---- 1. the norm kernels --------------------------------------------------------------------------------------------
def device_norm(g, gid, cuts=(), cap=0):
    """vr_grad_sumsq over [0, n) split at `cuts` (one slice of the partial sums per range) + vr_clip_finish; returns
    (norm, coef, skip) as the kernels left them, max_norm = inf and grad_scale = 1.  cap: the launches' workgroup cap."""
    L = _lib.lib()
    n = g.numel()
    state = torch.tensor([float("inf"), 1.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    edges = [0] + list(cuts) + [n]
    counts = [min(((hi - lo) // 8 + 255) // 256, NORM_PARTIALS) for lo, hi in zip(edges, edges[1:])]
    partials = torch.full((sum(counts),), float("nan"), dtype=torch.float32, device=DEV)     # (never zeroed by the caller)
    stream = torch.cuda.current_stream().cuda_stream
    first = 0
    for (lo, hi), cnt in zip(zip(edges, edges[1:]), counts):
        _lib.check(L.vr_grad_sumsq(g.data_ptr() + 4 * lo, gid.data_ptr() + lo // 8, hi - lo, partials.data_ptr() + 4 * first, cnt, cap,
                                   stream), "vr_grad_sumsq")
        first += cnt
    _lib.check(L.vr_clip_finish(partials.data_ptr(), first, state.data_ptr(), stream), "vr_clip_finish")
    torch.cuda.synchronize()
    return state[2].clone(), float(state[3]), int(state.view(torch.int32)[4])


def arena_like(n, seed, holes=False):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    g = torch.randn(n, generator=gen, device=DEV, dtype=torch.float32) * 3e-3
    gid = (torch.arange(n // 8, device=DEV) % 2).to(torch.uint8)
    if holes:                                                     # stretches that are not parameters: padding / frozen
        n8 = n // 8
        for lo8, hi8 in ((0, 5), (n8 // 3, n8 // 3 + 1000), (n8 - 77, n8)):
            gid[lo8:hi8] = 255
            g[lo8 * 8:hi8 * 8] = 1e30                              # (1e30^2 overflows fp32: counted once, the norm is inf)
    return g, gid


def expected_norm(g, gid):
    keep = (gid != 255).repeat_interleave(8)
    return float(torch.sqrt((g.double() ** 2 * keep).sum()))


@pytest.mark.parametrize("n,holes", [(40 * 2 ** 20 + 8, False), (1024, False), (8, False), (3_000_008, False), (5_000_000, True),
                                     (144 * 10 ** 6, False)],
                         ids=["40M", "below-one-workgroup", "one-group", "3M", "5M-holes", "144M"])
def test_norm_matches_float64(n, holes):
    """sqrt(sum of squares) against torch in float64 to the bound derived in tests/optim_ref64.py from the launch's own path: an fp32
    chain of ceil(n8 / (active * 256)) fused terms plus the 11-level tree per partial sum, halved by the square root, plus one fp32
    rounding of the result; the partial sums are added in double.  (It was a flat 1e-5, which every one of these bounds is below.)"""
    g, gid = arena_like(n, 11, holes)
    want = expected_norm(g, gid)
    got, coef, skip = device_norm(g, gid)
    err = abs(float(got) - want) / want
    bound = optim_ref64.norm_bound_rel(n, min((n // 8 + 255) // 256, NORM_PARTIALS))
    print("n=%d holes=%s norm=%.9g float64=%.9g rel.err=%.3g bound=%.3g" % (n, holes, float(got), want, err, bound))
    assert skip == 0 and coef == 1.0                              # max_norm = inf: measured, not clipped
    assert bound < 1e-5 and err <= bound, (float(got), want, bound)
    again, _, _ = device_norm(g, gid)                             # replay stability: the same bits
    assert torch.equal(again, got)
    if n >= 1024:                                                 # split invariance: three ranges, three slices of partial sums
        a, b = (n // 3) // 8 * 8, (2 * n // 3) // 8 * 8 + 8
        # (capped like the early launches of the captured step: 256 workgroups keep a chain at 144 M / 3 / (2048 * 256) = 92 terms)
        split, _, _ = device_norm(g, gid, cuts=(a, b), cap=256)
        # (every partial sum of every range is within its own range's bound and all are >= 0: the total is within the largest)
        bound = max(optim_ref64.norm_bound_rel(hi - lo, min(((hi - lo) // 8 + 255) // 256, NORM_PARTIALS), 256)
                    for lo, hi in ((0, a), (a, b), (b, n)))
        assert bound < 1e-5 and abs(float(split) - want) / want <= bound, (float(split), want, bound)


def test_finish_applies_torchs_formula_and_flags_non_finite_norms():
    g, gid = arena_like(4096, 3)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    partials = torch.empty(2, dtype=torch.float32, device=DEV)
    want = expected_norm(g, gid)
    state = torch.tensor([0.25 * want, 0.5, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
    for bad in (False, True, False):
        if bad:
            g[17] = float("inf")
        _lib.check(L.vr_grad_sumsq(g.data_ptr(), gid.data_ptr(), 4096, partials.data_ptr(), 2, 0, stream), "vr_grad_sumsq")
        _lib.check(L.vr_clip_finish(partials.data_ptr(), 2, state.data_ptr(), stream), "vr_clip_finish")
        torch.cuda.synchronize()
        norm, coef = float(state[2]), float(state[3])
        skip, skipped = (int(v) for v in state.view(torch.int32)[4:6])
        if bad:
            assert not math.isfinite(norm) and coef == 0.0 and skip == 1 and skipped == 1
            g[17] = 0.0
        else:
            n_ = 0.5 * expected_norm(g, gid)                       # grad_scale = 0.5: the norm of what the optimizer uses
            assert abs(norm - n_) < 1e-5 * n_ and skip == 0
            assert abs(coef - min(1.0, 0.25 * want / (n_ + 1e-6))) < 1e-6
    assert int(state.view(torch.int32)[5]) == 1                   # the count is a running one


# ---- 2. eager trajectory ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ema", [None, 0.99])
def test_clipped_flat_adamw_matches_torch_clip_and_adamw(ema):
    """The pattern of test_flat_adamw_matches_torch_adamw with clipping: torch clip_grad_norm_ + torch.optim.AdamW against
    FlatAdamW(max_norm=...) on identical gradients (the backward's, times a per-step factor that puts the norm on either side of
    max_norm), and a third run with doubled gradients and grad_scale = 0.5."""
    crit = SoftTargetCrossEntropy()
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    models = [build() for _ in range(3)]
    ref_opt = torch.optim.AdamW(groups(models[0]), lr=2e-3, betas=(0.9, 0.999), eps=1e-8)
    opt = FlatAdamW(models[1], groups(models[1]), lr=2e-3, betas=(0.9, 0.999), eps=1e-8, ema_decay=ema, max_norm=1.0)
    opt2 = FlatAdamW(models[2], groups(models[2]), lr=2e-3, betas=(0.9, 0.999), eps=1e-8, ema_decay=ema, max_norm=1.0)
    opt2.grad_scale = 0.5
    ema_ref = {n: p.detach().clone() for n, p in models[0].named_parameters()}
    factors = [4.0, 0.25, 3.0, 0.125]
    max_norm, norms = None, []
    for it, f in enumerate(factors):
        for m, o in ((models[1], opt), (models[2], opt2)):
            torch.manual_seed(300 + it)
            o.zero_grad(set_to_none=True)
            out = m(x, patch_output_type="seq")
            (crit(out[0], t) + crit(out[1], pt)).backward()
        g1, g2 = models[1]._arena["gcur"], models[2]._arena["gcur"]
        g1.mul_(f)
        g2.copy_(g1 * 2.0)                                         # identical gradients, doubled (exact in fp32)
        for p_r, p_f in zip(models[0].parameters(), models[1].parameters()):
            p_r.grad = p_f.grad.detach().clone()
        if max_norm is None:
            max_norm = torch_norm(models[0]) / factors[0]          # the first backward's own norm: step 0 is 4x above it
            opt.max_norm = opt2.max_norm = max_norm
        tn = torch.nn.utils.clip_grad_norm_(models[0].parameters(), max_norm)
        ref_opt.step()
        opt.step()
        opt2.step()
        norms.append(float(tn))
        for o in (opt, opt2):
            assert abs(float(o.grad_norm()) - float(tn)) < 1e-5 * float(tn), (it, float(o.grad_norm()), float(tn))
        if it == 1:
            for o in (opt, opt2, ref_opt):
                for grp in o.param_groups:
                    grp["lr"] = 1e-3                               # scheduler-style lr change
        for n, p in models[0].named_parameters():
            ema_ref[n] = 0.99 * ema_ref[n] + 0.01 * p.detach() if ema else ema_ref[n]
    print("max_norm %.6g, norms %s" % (max_norm, norms))
    assert sum(n > max_norm for n in norms) >= 2 and sum(n < max_norm for n in norms) >= 1
    assert opt.skipped_steps() == 0 and opt2.skipped_steps() == 0
    p_ref = dict(models[0].named_parameters())
    for m, o in ((models[1], opt), (models[2], opt2)):
        a = m._arena
        assert a.get("shadow_ok")
        assert torch.equal(a["shadow"].float(), a["flat"].bfloat16().float())
        for n, p in m.named_parameters():
            assert rel(p, p_ref[n]) < 2e-6, n
        if ema:
            esd = o.ema_state_dict()
            for n in ema_ref:
                assert rel(esd[n], ema_ref[n]) < 2e-5, n
        assert o.state_dict()["step"] == 4
    # measure only: inf clips nothing and still reports the norm
    opt.max_norm = float("inf")
    before = models[1]._arena["flat"].clone()
    opt.step()
    assert float(opt._clip["state"][3]) == 1.0 and not torch.equal(before, models[1]._arena["flat"])


# ---- 3. inside the captured step -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_clipping_inside_the_graph_equals_clipped_step_after_the_graph(dtype, overlap):
    """GraphedTrainStep(optimizer=opt) with opt.max_norm set (early sums of squares on the side stream, finish, one full-width
    AdamW) against graph replay + eager opt.step() with the same max_norm; max_norm goes to inf and back between replays.
    Tolerances and their reason: test_optimizer_inside_the_graph_equals_step_after_the_graph (atomics order of the weight
    gradients differs run to run, Adam amplifies it).  The norms of the two runs are functions of the same batch and of
    parameters that agree to that tolerance: they are held to it too (bf16: to the bound on the losses)."""
    crit = SoftTargetCrossEntropy()
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    runs, max_norm = [], None
    for in_graph in (False, True):
        prod = build(dtype=dtype)
        opt = FlatAdamW(prod, groups(prod), lr=2e-3, ema_decay=0.99, max_norm=1.0)
        if dtype == torch.bfloat16:
            opt.own_shadow()
        g = engine.GraphedTrainStep(prod, crit, x, t, pt, "seq", optimizer=opt if in_graph else None, opt_overlap=overlap,
                                    opt_overlap_blocks=8)
        assert (g.optimizer is not None) == in_graph
        if max_norm is None:                                       # a probe replay (gradients only): half the first step's norm
            torch.manual_seed(900)
            g(x, t, pt, epoch=31, train_iter=0, arch_sample=None)
            max_norm = 0.5 * torch_norm(prod)
        losses, norms, coefs = [], [], []
        for it in range(4):
            torch.manual_seed(900 + it)
            opt.max_norm = float("inf") if it == 1 else max_norm
            if it == 2:
                for grp in opt.param_groups:
                    grp["lr"] = 5e-4
            if in_graph:
                opt.prepare_step()
                losses.append(g(x, t, pt, epoch=31, train_iter=it, arch_sample=None).item())
            else:
                losses.append(g(x, t, pt, epoch=31, train_iter=it, arch_sample=None).item())
                opt.step()
            norms.append(float(opt.grad_norm()))
            coefs.append(float(opt._clip["state"][3]))
        torch.cuda.synchronize()
        print("in_graph=%s max_norm=%.6g norms=%s coefs=%s" % (in_graph, max_norm, norms, coefs))
        assert norms[0] > max_norm and coefs[0] < 1.0              # clipping is active on the first step
        assert coefs[1] == 1.0                                     # inf: the replay followed the host's max_norm ...
        assert all(abs(c - min(1.0, max_norm / (n + 1e-6))) < 1e-6 for c, n in zip(coefs[2:], norms[2:]))     # ... and back
        assert opt.skipped_steps() == 0
        runs.append((losses, prod._arena["flat"].clone(), opt._flat_state["v"].clone(), opt._flat_state["ema"].clone(), opt._step,
                     prod._arena["shadow"].clone() if dtype == torch.bfloat16 else None, norms))
    (l0, p0, v0, e0, s0, sh0, n0), (l1, p1, v1, e1, s1, sh1, n1) = runs
    assert s0 == s1 == 4
    tol = 2e-3
    f32 = dtype == torch.float32
    assert max(abs(a - b) / abs(a) for a, b in zip(l0, l1)) < (1e-5 if f32 else 2e-2)
    assert max(abs(a - b) / abs(a) for a, b in zip(n0, n1)) < (tol if f32 else 2e-2)
    assert rel(p1, p0) < tol and rel(e1, e0) < tol and rel(v1, v0) < (1e-5 if f32 else 5e-2)
    if sh0 is not None:
        assert torch.equal(sh1.float(), p1.bfloat16().float())


# ---- 4. off is off ---------------------------------------------------------------------------------------------------------
def _demangle(names):
    if not any(n.startswith("_Z") for n in names):
        return names
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, timeout=60).stdout.splitlines()
        return out if len(out) == len(names) else names
    except (OSError, subprocess.SubprocessError):
        return names


class _LaunchLog:
    """The library behind a proxy that notes the name of every entry point called: what a capture launches, call by call."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("vr_"):
            return fn

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


def _captured_step(monkeypatch, **opt_kw):
    """One captured step with the optimizer inside: (entry points called while it was built and captured, names of the kernels a
    profiler saw in its replays, optimizer, step, batch)."""
    from torch.profiler import ProfilerActivity, profile
    crit = SoftTargetCrossEntropy()
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    prod = build()
    opt = FlatAdamW(prod, groups(prod), lr=2e-3, ema_decay=0.99, **opt_kw)
    opt.own_shadow()
    torch.manual_seed(77)      # (the warm-up steps and the capture draw the same sub-networks every time)
    calls = []
    real = _lib.lib()
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "lib", lambda: _LaunchLog(real, calls))
        g = engine.GraphedTrainStep(prod, crit, x, t, pt, "seq", optimizer=opt, opt_overlap=1, opt_overlap_blocks=8)
    torch.manual_seed(1)
    opt.prepare_step()
    g(x, t, pt, epoch=31, train_iter=0, arch_sample=None)
    torch.cuda.synchronize()
    # The tracer delivers its records late: a session can miss the last kernels of what ran inside it and receive those of launches
    # before it (seen here: a session without the 2 us clip_finish_kernel; a first session holding kernels of the eager warm-up
    # steps).  So the NAMES are taken as a set over several replays, after a session that takes delivery of the stale records, and
    # the exact launch COUNTS come from the call log above.
    for n_replays in (1, 4):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n_replays):
                g.graph.replay()                                   # the captured step alone (no upload, no copy in front)
            torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return calls, set(_demangle(sorted({e.name for e in ev}))), opt, g, (x, t, pt)


def test_max_norm_none_captures_todays_kernels_and_cannot_be_switched_on_later(monkeypatch):
    from collections import Counter
    calls_plain, plain, _, _, _ = _captured_step(monkeypatch)
    calls_off, off, opt, g, (x, t, pt) = _captured_step(monkeypatch, max_norm=None)
    calls_on, on, _, _, _ = _captured_step(monkeypatch, max_norm=1.0)
    clip_kernels = ("sumsq_kernel", "clip_finish_kernel")
    has = lambda names, s: any(s in n for n in names)             # noqa: E731
    # kernel names of the replayed graph
    assert len(plain) > 10, sorted(plain)[:5]
    assert off == plain, (sorted(off - plain), sorted(plain - off))
    assert not any(has(off, k) for k in clip_kernels)
    assert all(has(on, k) for k in clip_kernels), sorted(n for n in on if "anonymous" in n)
    adamw = lambda names: {n for n in names if "adamw_kernel" in n}      # noqa: E731
    assert len(adamw(off)) == 1 and len(adamw(on)) == 1 and adamw(off) != adamw(on)          # <true, false> / <true, true>
    assert on - adamw(on) - {n for n in on if any(k in n for k in clip_kernels)} == off - adamw(off)
    # launch for launch
    assert len(calls_plain) > 100
    assert calls_off == calls_plain, (Counter(calls_off) - Counter(calls_plain), Counter(calls_plain) - Counter(calls_off))
    assert opt._clip is None                                      # nothing was allocated either
    assert Counter(calls_off)["vr_adamw_flat_dev_capped"] == 2    # (the early range + the rest)
    assert Counter(calls_on) - Counter(calls_off) == Counter({"vr_grad_sumsq": 2, "vr_clip_finish": 1, "vr_adamw_flat_clip": 1})
    assert Counter(calls_off) - Counter(calls_on) == Counter({"vr_adamw_flat_dev_capped": 2})
    opt.max_norm = 1.0                                            # the graph holds no clipping launch: it cannot follow
    with pytest.raises(RuntimeError, match="max_norm"):
        opt.prepare_step()
    with pytest.raises(RuntimeError, match="max_norm"):
        g(x, t, pt, epoch=31, train_iter=1, arch_sample=None)
    opt.max_norm = None
    opt.prepare_step()
    g(x, t, pt, epoch=31, train_iter=1, arch_sample=None)
    torch.cuda.synchronize()


# ---- 5. a non-finite step --------------------------------------------------------------------------------------------------
def test_non_finite_step_is_skipped_and_the_next_one_trains():
    crit = SoftTargetCrossEntropy()
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    prod = build()
    opt = FlatAdamW(prod, groups(prod), lr=2e-3, ema_decay=0.99, max_norm=float("inf"))
    opt.own_shadow()
    g = engine.GraphedTrainStep(prod, crit, x, t, pt, "seq", optimizer=opt, opt_overlap=1, opt_overlap_blocks=8)

    def snapshot():
        torch.cuda.synchronize()
        st = opt._flat_state
        return [v.clone() for v in (prod._arena["flat"], st["m"], st["v"], st["ema"], prod._arena["shadow"])]

    def replay(it, targets):
        torch.manual_seed(900 + it)
        opt.prepare_step()
        g(x, targets, pt, epoch=31, train_iter=it, arch_sample=None)

    replay(0, t)
    before = snapshot()
    assert opt.skipped_steps() == 0 and all(bool(torch.isfinite(v.float()).all()) for v in before)
    bad = t.clone()
    bad[0, 0] = float("inf")                                      # ordinary data: one soft-target entry
    replay(1, bad)
    after = snapshot()
    assert opt.skipped_steps() == 1 and not math.isfinite(float(opt.grad_norm()))
    for a, b in zip(before, after):                               # parameters, both moments, EMA, shadow: the same bits
        assert torch.equal(a, b)
    replay(2, t)
    again = snapshot()
    assert opt.skipped_steps() == 1 and math.isfinite(float(opt.grad_norm()))
    assert all(bool(torch.isfinite(v.float()).all()) for v in again)
    assert not torch.equal(again[0], after[0]) and not torch.equal(again[1], after[1])       # it updated again
    assert opt._step == 3                                         # the host count includes the skipped step (documented)


# ---- 6. train_step ---------------------------------------------------------------------------------------------------------
def test_train_step_clips_in_the_optimizer_for_flat_adamw_and_with_torch_otherwise(monkeypatch):
    crit = SoftTargetCrossEntropy()
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    flat_model, twin = build(), build()
    opt = FlatAdamW(flat_model, groups(flat_model), lr=2e-3)
    ref_opt = torch.optim.AdamW(groups(twin), lr=2e-3, betas=(0.9, 0.999), eps=1e-8)
    torch.manual_seed(40)                                         # a probe backward: max_norm = half the first step's norm
    out = flat_model(x, patch_output_type="seq")
    (crit(out[0], t) + crit(out[1], pt)).backward()
    max_norm = 0.5 * torch_norm(flat_model)
    real = torch.nn.utils.clip_grad_norm_
    calls, given = [0], [None]

    def counting(parameters, max_norm_, *a, **k):
        calls[0] += 1
        parameters = list(parameters)
        if given[0] is not None:                                  # the twin gets the gradients the FlatAdamW step used
            for p, gr in zip(parameters, given[0]):
                p.grad.copy_(gr)
        return real(parameters, max_norm_, *a, **k)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", counting)
    for it in range(3):
        given[0] = None
        torch.manual_seed(40 + it)
        engine.train_step(flat_model, crit, opt, x, t, pt, "seq", epoch=31, train_iter=it, max_norm=max_norm)
        assert calls[0] == it                                     # FlatAdamW: torch's clip is never called
        assert opt.max_norm == max_norm
        given[0] = [p.grad.detach().clone() for p in flat_model.parameters()]
        torch.manual_seed(40 + it)
        engine.train_step(twin, crit, ref_opt, x, t, pt, "seq", epoch=31, train_iter=it, max_norm=max_norm)
        assert calls[0] == it + 1                                 # any other optimizer: the torch call
        if it == 0:
            assert float(opt.grad_norm()) > max_norm              # clipping is active
    p_ref = dict(twin.named_parameters())
    for n, p in flat_model.named_parameters():
        assert rel(p, p_ref[n]) < 2e-6, n


def test_one_rank_step_with_sync_then_clipped_step_equals_the_plain_path():
    """One rank: step_with_sync (a GradSync of world 1 exchanges nothing) followed by the clipped opt.step() walks the path of
    replay + clipped opt.step()."""
    crit = SoftTargetCrossEntropy()
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    out = []
    for synced in (False, True):
        prod = build(dtype=torch.float32)
        opt = FlatAdamW(prod, groups(prod), lr=2e-3, max_norm=0.01)
        g = engine.GraphedTrainStep(prod, crit, x, t, pt, "seq")
        sync = engine.GradSync(prod)
        for it in range(2):
            torch.manual_seed(900 + it)
            if synced:
                g.step_with_sync(sync, x, t, pt, epoch=31, train_iter=it, arch_sample=None)
            else:
                g(x, t, pt, epoch=31, train_iter=it, arch_sample=None)
            opt.step()
        torch.cuda.synchronize()
        out.append((prod._arena["flat"].clone(), float(opt.grad_norm())))
    assert rel(out[1][0], out[0][0]) < 2e-3 and abs(out[1][1] - out[0][1]) < 2e-3 * out[0][1]
