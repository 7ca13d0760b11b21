"""Gradient accumulation over micro-batches (accum_steps): the accumulate / gated entry points against torch on the same buffers,
loss_and_grad(accumulate=True) for every parameter, the averaged FlatAdamW update, and ONE captured graph serving every micro-step
of an update window (engine.GraphedTrainStep(accum_steps=k)).  Micro networks of tests/golden/recipe.py, micro-batch 8.
(The file's name sorts it behind the other files that open profiler sessions: theirs then run as they did before this file existed.)"""
import math
from collections import Counter

import pytest
import torch

import recipe
import vitres
from vitres import _lib, engine
from vitres import kernels as K
from vitres.losses import SoftTargetCrossEntropy
from vitres.optim import FlatAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_BAND = 5e-4          # the project's fp32 gradient band: whole-tensor relative L2


def build(et=0, dtype=torch.bfloat16, dpr=0.0, seed=None):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30, single_arch=False,
              hybrid_arch=False)
    prod = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                               num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[et], drop_path_rate=dpr,
                               drop_block_rate=None, **kw)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in prod.state_dict().items()], 100 + et if seed is None else seed)
    prod.load_state_dict(sd)
    prod = prod.to(DEV)
    prod.set_compute_dtype(dtype)
    prod.train()
    prod.set_epoch(31)
    prod.load_state_dict(sd)
    return prod


_MB = {}


def micro_batches(n):
    """The first n micro-batches (8 images each), made once and shared."""
    for i in range(n):
        if i not in _MB:
            x, t, pt, _ = recipe.inputs(7 + i, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
            _MB[i] = (x.to(DEV), t.to(DEV), pt.to(DEV))
    return [_MB[i] for i in range(n)]


def rel(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def groups(model):
    return engine.param_groups_weight_decay(model, 0.05)


def torch_norm(model):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))


def stream():
    return torch.cuda.current_stream().cuda_stream


def gate_word(v):
    return torch.tensor([v, 12345], dtype=torch.int32, device=DEV)[0:1]


# ---- 1. entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,B,C,src_ld", [(24, 1, 588, 592), (8, 9, 6, 54), (16, 9, 3, 32), (32, 49, 5, 245), (1, 1, 4099, 4099),
                                          (1, 1, 1_200_003, 1_200_003)],
                         ids=["padded-rows", "co-9-ci6", "conv1-ld32", "7x7-ci5", "flat-add", "grid-stride"])
def test_relayout_add_adds_onto_what_is_there(A, B, C, src_ld):
    """dst[a, c, b] += src[a, b, c] onto a destination holding non-zero data: an fp32 sum of two terms, exact up to one rounding."""
    gen = torch.Generator(device=DEV).manual_seed(A * 1000 + C)
    src = torch.randn(A, src_ld, generator=gen, device=DEV)
    dst = torch.randn(A, B * C, generator=gen, device=DEV)
    want = dst + src[:, :B * C].reshape(A, B, C).permute(0, 2, 1).reshape(A, B * C)
    K.relayout_add(src, dst, A, B, C, src_ld=src_ld)
    torch.cuda.synchronize()
    assert torch.allclose(dst, want, rtol=1e-6, atol=0.0)
    with pytest.raises(ValueError):
        K.relayout_add(src.bfloat16(), dst, A, B, C, src_ld=src_ld)           # fp32 only


def test_gated_clear_follows_its_gate():
    n = 300_001
    gen = torch.Generator(device=DEV).manual_seed(3)
    buf = torch.randn(n, generator=gen, device=DEV) + 3.0
    before = buf.clone()
    ranges = [(3, 1000), (5000, 75_001), (200_000, n)]            # odd starts, lengths that are no multiple of a workgroup's span
    K.zero_ranges(buf, ranges, gate=gate_word(0))
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    K.zero_ranges(buf, ranges, gate=gate_word(1))
    torch.cuda.synchronize()
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    for lo, hi in ranges:
        keep[lo:hi] = False
        assert not bool(buf[lo:hi].any())
    assert torch.equal(buf[keep], before[keep])
    K.zero_ranges(buf, [(0, n)], gate=gate_word(0))
    assert torch.equal(buf[keep], before[keep])
    K.zero_ranges(buf, [(0, n)], gate=gate_word(7))               # any non-zero word opens the gate
    torch.cuda.synchronize()
    assert not bool(buf.any())


def test_gated_norm_launches_follow_their_gate():
    L = _lib.lib()
    n = 3_000_008
    gen = torch.Generator(device=DEV).manual_seed(11)
    g = torch.randn(n, generator=gen, device=DEV) * 3e-3
    gid = (torch.arange(n // 8, device=DEV) % 2).to(torch.uint8)
    gid[5:9] = 255
    cnt = 777
    state0 = torch.tensor([0.01, 0.5, -1.0, -2.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    state0.view(torch.int32)[4:8] = torch.tensor([1, 3, 41, 42], dtype=torch.int32, device=DEV)
    sentinel = torch.full((cnt + 5,), float("nan"), dtype=torch.float32, device=DEV)

    def run(gate, cap):
        partials, state = sentinel.clone(), state0.clone()
        if gate is None:
            _lib.check(L.vr_grad_sumsq(g.data_ptr(), gid.data_ptr(), n, partials.data_ptr(), cnt, cap, stream()), "vr_grad_sumsq")
            _lib.check(L.vr_clip_finish(partials.data_ptr(), cnt, state.data_ptr(), stream()), "vr_clip_finish")
        else:
            w = gate_word(gate)
            _lib.check(L.vr_grad_sumsq_gated(g.data_ptr(), gid.data_ptr(), n, partials.data_ptr(), cnt, cap, w.data_ptr(), stream()),
                       "vr_grad_sumsq_gated")
            if gate == 0:
                partials[:cnt] = 1.0                               # (something finite for the finish to leave alone)
            _lib.check(L.vr_clip_finish_gated(partials.data_ptr(), cnt, state.data_ptr(), w.data_ptr(), stream()),
                       "vr_clip_finish_gated")
        torch.cuda.synchronize()
        return partials.view(torch.int32), state.view(torch.int32)
    for cap in (0, 64):
        ref_p, ref_s = run(None, cap)
        on_p, on_s = run(1, cap)
        assert torch.equal(on_p, ref_p) and torch.equal(on_s, ref_s)          # gate 1: the ungated result, bit for bit
        assert ref_s[4].item() == 0 and ref_s[5].item() == 3 and ref_s[6:].tolist() == [41, 42]
        w = gate_word(0)
        partials, state = sentinel.clone(), state0.clone()
        _lib.check(L.vr_grad_sumsq_gated(g.data_ptr(), gid.data_ptr(), n, partials.data_ptr(), cnt, cap, w.data_ptr(), stream()),
                   "vr_grad_sumsq_gated")
        _lib.check(L.vr_clip_finish_gated(ref_p.view(torch.float32).data_ptr(), cnt, state.data_ptr(), w.data_ptr(), stream()),
                   "vr_clip_finish_gated")
        torch.cuda.synchronize()
        assert torch.equal(partials.view(torch.int32), sentinel.view(torch.int32))           # its slice of the partial sums untouched
        assert torch.equal(state.view(torch.int32), state0.view(torch.int32))                # all 8 dwords, `skipped` included
    # a non-finite sum behind an open gate counts, behind a closed one it does not
    g[17] = float("inf")
    _, s_on = run(1, 0)
    _, s_off = run(0, 0)
    assert s_on[4].item() == 1 and s_on[5].item() == 4 and s_off[5].item() == 3


# ---- 2. every parameter accumulates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("et", [0, 4, 5])
def test_every_parameter_accumulates(et, dtype):
    """g1, g2 from two fresh loss_and_grad calls on two micro-batches; the same two calls with accumulate=True on the second leave
    g1 + g2 in EVERY parameter.  Same kernels in both runs: only the fp32 summation order differs, while a store where an add belongs
    (or a second clear) loses a whole term.  Seeds as in tests/test_accum_host.py, which checks on the emulation that every tensor has
    a non-zero gradient in each micro-batch; asserted here again."""
    prod = build(et, dtype, dpr=0.2)
    mb = micro_batches(2)

    def run(i, accumulate=False):
        torch.manual_seed(500 + i)
        prod.drop_path_generator(seed=900 + i)
        return prod.loss_and_grad(*mb[i], "seq", accumulate=accumulate)
    single = []
    for i in range(2):
        prod.zero_grad(set_to_none=True)
        run(i)
        single.append({n: p.grad.clone() for n, p in prod.named_parameters() if p.requires_grad})
    prod.zero_grad(set_to_none=True)
    run(0)
    run(1, accumulate=True)
    torch.cuda.synchronize()
    worst = (0.0, None)
    for n, p in prod.named_parameters():
        if not p.requires_grad:
            continue
        g1, g2 = single[0][n], single[1][n]
        assert float(g1.abs().max()) > 0 and float(g2.abs().max()) > 0, n
        err = rel_l2(p.grad, g1.double() + g2.double())
        worst = max(worst, (err, n))
        assert err <= GRAD_BAND, (n, err)
    print("embed type %d %s: worst relative L2 %.3g (%s)" % (et, dtype, worst[0], worst[1]))
    with pytest.raises(RuntimeError, match="fresh gradients"):
        prod.loss_and_grad(*mb[0], "seq")


# ---- 3. the averaged update ----------------------------------------------------------------------------------------------------
def _accumulate_two(prod):
    mb = micro_batches(2)
    prod.zero_grad(set_to_none=True)
    for i in range(2):
        torch.manual_seed(500 + i)
        prod.loss_and_grad(*mb[i], "seq", accumulate=i > 0)
    return prod._arena["gcur"]


def test_the_update_uses_the_mean_over_the_window():
    """k = 2, eager: grad_norm() is the norm of (g1 + g2) / 2; with max_norm at half of it the step equals that of a twin whose arena
    holds (g1 + g2) / 2 and whose accum_steps is 1.  (The first Adam step does not see the gradient's scale: the norm and the clipped
    step are what prove the 1 / k.)"""
    prod = build()
    opt = FlatAdamW(prod, groups(prod), lr=2e-3, ema_decay=0.99, max_norm=float("inf"), accum_steps=2)
    opt.own_shadow()
    G = _accumulate_two(prod).clone()
    want = 0.5 * torch_norm(prod)
    opt.step()
    assert opt._step == 1
    assert abs(float(opt.grad_norm()) - want) < 1e-5 * want, (float(opt.grad_norm()), want)
    # the clipped step against the twin
    a, b = build(), build()
    oa = FlatAdamW(a, groups(a), lr=2e-3, ema_decay=0.99, max_norm=0.5 * want, accum_steps=2)
    ob = FlatAdamW(b, groups(b), lr=2e-3, ema_decay=0.99, max_norm=0.5 * want)
    oa.own_shadow()
    ob.own_shadow()
    _accumulate_two(a).copy_(G)                                   # (identical sums in both: the atomics' order is not under test)
    b.zero_grad(set_to_none=True)
    torch.manual_seed(500)
    b.loss_and_grad(*micro_batches(1)[0], "seq")
    b._arena["gcur"].copy_(G * 0.5)                               # the mean, halved exactly
    oa.step()
    ob.step()
    torch.cuda.synchronize()
    assert abs(float(oa.grad_norm()) - want) < 1e-5 * want and abs(float(ob.grad_norm()) - want) < 1e-5 * want
    assert 0.49 < float(oa._clip["state"][3]) < 0.51              # clipping is active
    tol = 2e-3
    sa, sb = oa._flat_state, ob._flat_state
    assert rel(a._arena["flat"], b._arena["flat"]) < tol and rel(sa["ema"], sb["ema"]) < tol and rel(sa["m"], sb["m"]) < tol
    assert rel(sa["v"], sb["v"]) < 5e-2
    assert rel(a._arena["shadow"].float(), b._arena["shadow"].float()) < tol + 2.0 ** -8
    assert torch.equal(a._arena["shadow"].float(), a._arena["flat"].bfloat16().float())


def test_train_step_accumulates_and_steps_on_the_last_micro_step():
    """The autograd path: engine.train_step(accum_steps=2, micro_step=0 / 1) with a FlatAdamW leaves the window's sum in the arena
    and takes one update, on its mean."""
    crit = SoftTargetCrossEntropy()
    prod, twin = build(dtype=torch.float32), build(dtype=torch.float32)       # (fp32: both paths form the logit gradients in fp32)
    opt = FlatAdamW(prod, groups(prod), lr=2e-3, max_norm=float("inf"))
    G = _accumulate_two(twin)
    want = 0.5 * torch_norm(twin)
    before = opt._bind()["flat"].clone()
    mb = micro_batches(2)
    for i in range(2):
        torch.manual_seed(500 + i)
        engine.train_step(prod, crit, opt, mb[i][0], mb[i][1], mb[i][2], "seq", epoch=31, train_iter=0, max_norm=float("inf"),
                          accum_steps=2, micro_step=i)
        assert opt._step == i                                     # 0 after the first micro-step, 1 after the window
        if i == 0:
            assert torch.equal(prod._arena["flat"], before)
    assert opt.accum_steps == 2
    assert rel_l2(prod._arena["gcur"], G) <= GRAD_BAND
    assert abs(float(opt.grad_norm()) - want) < 1e-4 * want
    assert not torch.equal(prod._arena["flat"], before)


# ---- 4. one graph, gated ---------------------------------------------------------------------------------------------------------
def _snapshot(prod, opt):
    torch.cuda.synchronize()
    st = opt._flat_state
    return [v.clone() for v in (prod._arena["flat"], st["m"], st["v"], st["ema"], prod._arena["shadow"])]


def test_one_captured_graph_serves_the_whole_window(monkeypatch):
    crit = SoftTargetCrossEntropy()
    mb = micro_batches(6)
    # eager reference: three micro-batches accumulated, one step on their mean
    ref = build()
    ropt = FlatAdamW(ref, groups(ref), lr=2e-3, ema_decay=0.99, max_norm=float("inf"), accum_steps=3)
    ropt.own_shadow()
    ref.zero_grad(set_to_none=True)
    for i in range(3):
        torch.manual_seed(900 + i)
        ref.loss_and_grad(*mb[i], "seq", accumulate=i > 0)
    max_norm = 0.5 * torch_norm(ref) / 3                          # half the norm of the window's mean: clipping is active
    ropt.max_norm = max_norm
    ropt.step()
    # the graph
    prod = build()
    opt = FlatAdamW(prod, groups(prod), lr=2e-3, ema_decay=0.99, max_norm=max_norm)
    opt.own_shadow()
    captures = [0]
    real_enter = torch.cuda.graph.__enter__

    def counting(self):
        captures[0] += 1
        return real_enter(self)
    monkeypatch.setattr(torch.cuda.graph, "__enter__", counting)
    g = engine.GraphedTrainStep(prod, crit, *mb[0], "seq", optimizer=opt, opt_overlap=1, opt_overlap_blocks=8, accum_steps=3)
    monkeypatch.setattr(torch.cuda.graph, "__enter__", real_enter)
    assert captures[0] == 1 and len(g.more_graphs) == 0 and g.accum_steps == 3 and opt.accum_steps == 3
    arena4 = None
    for it in range(6):
        pos = it % 3
        assert g.micro_step == pos
        before, skipped, step = _snapshot(prod, opt), opt.skipped_steps(), opt._step
        torch.manual_seed(900 + it)
        opt.prepare_step(apply=(g.micro_step == g.accum_steps - 1))
        g(*mb[it], epoch=31, train_iter=it // 3, arch_sample=None)
        after = _snapshot(prod, opt)
        if pos < 2:                                               # a non-final replay changes nothing but the gradient arena
            assert all(torch.equal(a, b) for a, b in zip(before, after)), it
            assert opt.skipped_steps() == skipped and opt._step == step
        else:
            assert opt._step == step + 1 and not torch.equal(before[0], after[0])
        if it == 2:
            assert float(opt._clip["state"][3]) < 1.0             # clipped
            assert rel(after[0], ref._arena["flat"]) < 2e-3 and rel(after[3], ropt._flat_state["ema"]) < 2e-3
            assert abs(float(opt.grad_norm()) - float(ropt.grad_norm())) < 2e-2 * float(ropt.grad_norm())
            assert torch.equal(after[4].float(), after[0].bfloat16().float())
        if it == 3:
            arena4 = prod._arena["gcur"].clone()
    assert g.micro_step == 0 and opt._step == 2 and opt.skipped_steps() == 0
    # after replay 4 the arena held micro-batch 4's gradients alone (the second window cleared): the same parameters, eagerly
    ref._arena["flat"].copy_(before[0])                           # (`before` of replay 6 = the parameters replays 4 - 6 ran on)
    ref.invalidate_shadow()
    ref.zero_grad(set_to_none=True)
    torch.manual_seed(900 + 3)
    ref.loss_and_grad(*mb[3], "seq")
    off = ref._arena["offsets"]
    for p, (o, n) in zip(ref._arena["params"], off):
        if p.requires_grad:
            assert rel_l2(arena4[o:o + n], ref._arena["gcur"][o:o + n]) <= GRAD_BAND


def test_a_window_without_a_plan_buffer_stages_the_control_words_alone():
    """accum_steps = 2 on the plain network (no supernet, no DropPath): nothing of a plan reaches the graph, the static device buffer
    holds {clear, apply} and nothing else.  One window of the captured step against loss_and_grad(accumulate=...) x 2 + step() on an
    identically filled twin: the quantities and bands of test_one_captured_graph_serves_the_whole_window at it == 2."""
    crit = SoftTargetCrossEntropy()
    mb = micro_batches(2)

    def plain():
        m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output", img_size=recipe.MICRO_IMG, num_classes=recipe.MICRO_CLASSES,
                                network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0)
        m.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 100))
        m = m.to(DEV)
        m.set_compute_dtype(torch.bfloat16)
        m.train()
        opt = FlatAdamW(m, groups(m), lr=2e-3, ema_decay=0.99, accum_steps=2)
        opt.own_shadow()
        return m, opt
    ref, ropt = plain()
    ref.zero_grad(set_to_none=True)
    for i in range(2):
        ref.loss_and_grad(*mb[i], "seq", accumulate=i > 0)
    ropt.step()
    prod, opt = plain()
    g = engine.GraphedTrainStep(prod, crit, *mb[0], "seq", optimizer=opt, accum_steps=2)
    assert g.keep_static is None and g._ctl_all.numel() == 2
    start = _snapshot(prod, opt)
    for i in range(2):
        assert g.micro_step == i
        opt.prepare_step(apply=(g.micro_step == g.accum_steps - 1))
        g(*mb[i], epoch=31, train_iter=0, arch_sample=None)
        after = _snapshot(prod, opt)
        if i == 0:                                                # the non-final replay changes nothing but the gradient arena
            assert all(torch.equal(a, b) for a, b in zip(start, after))
    assert g.micro_step == 0 and opt._step == 1 and not torch.equal(start[0], after[0])
    print("parameters %.3g, EMA %.3g (band 2e-3)" % (rel(after[0], ref._arena["flat"]), rel(after[3], ropt._flat_state["ema"])))
    assert rel(after[0], ref._arena["flat"]) < 2e-3 and rel(after[3], ropt._flat_state["ema"]) < 2e-3
    assert torch.equal(after[4].float(), after[0].bfloat16().float())


class _LaunchLog:
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


def _capture(monkeypatch, max_norm, **kw):
    from torch.profiler import ProfilerActivity, profile
    crit = SoftTargetCrossEntropy()
    mb = micro_batches(1)[0]
    prod = build()
    opt = FlatAdamW(prod, groups(prod), lr=2e-3, ema_decay=0.99, max_norm=max_norm)
    opt.own_shadow()
    torch.manual_seed(77)
    calls, real = [], _lib.lib()
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "lib", lambda: _LaunchLog(real, calls))
        g = engine.GraphedTrainStep(prod, crit, *mb, "seq", optimizer=opt, opt_overlap=1, opt_overlap_blocks=8, **kw)
    torch.manual_seed(1)
    opt.prepare_step(apply=(g.micro_step == g.accum_steps - 1))
    g(*mb, epoch=31, train_iter=0, arch_sample=None)
    torch.cuda.synchronize()
    # The tracer delivers its records late: a session can miss kernels of what ran inside it (seen here: one without the side stream's
    # kernels) and receive those of launches before it.  The launches before it are this function's own eager warm-up steps, the same
    # for every capture compared, so the names are the union over several sessions; the exact launches come from the call log.
    names = set()
    for n_replays in (1, 4, 4, 4):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n_replays):
                g.graph.replay()
            torch.cuda.synchronize()
        names |= {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return calls, names, g


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["plain", "clip"])
def test_one_micro_step_captures_todays_kernels(monkeypatch, max_norm):
    calls_plain, names_plain, _ = _capture(monkeypatch, max_norm)
    calls_one, names_one, g = _capture(monkeypatch, max_norm, accum_steps=1)
    assert len(calls_plain) > 100 and calls_one == calls_plain, Counter(calls_one) - Counter(calls_plain)
    assert names_one == names_plain, (sorted(names_one - names_plain), sorted(names_plain - names_one))
    assert not any("gated" in n or "relayout_add" in n for n in names_one | set(calls_one))
    assert g._ctl_all is None and g.micro_step == 0
    # and the gated entry points are what a window of several captures instead
    calls_k, names_k, _ = _capture(monkeypatch, max_norm, accum_steps=2)
    diff = Counter(calls_k) - Counter(calls_plain)
    assert diff["vr_zero_ranges_gated"] == 1 and diff["vr_relayout_add"] >= 1
    assert Counter(calls_plain)["vr_grad_sumsq"] == diff["vr_grad_sumsq_gated"] == (2 if max_norm else 0)
    assert Counter(calls_plain)["vr_clip_finish"] == diff["vr_clip_finish_gated"] == (1 if max_norm else 0)
    assert Counter(calls_k)["vr_grad_sumsq"] == 0 and Counter(calls_k)["vr_clip_finish"] == 0


# ---- 5. a non-finite micro-step ---------------------------------------------------------------------------------------------------
def test_a_non_finite_micro_step_skips_the_window_once():
    crit = SoftTargetCrossEntropy()
    mb = micro_batches(2)
    prod = build()
    opt = FlatAdamW(prod, groups(prod), lr=2e-3, ema_decay=0.99, max_norm=float("inf"))
    opt.own_shadow()
    g = engine.GraphedTrainStep(prod, crit, *mb[0], "seq", optimizer=opt, opt_overlap=1, opt_overlap_blocks=8, accum_steps=2)

    def window(w, bad_first=False):
        for j in range(2):
            x, t, pt = mb[j]
            if bad_first and j == 0:
                t = t.clone()
                t[0, 0] = float("inf")                            # ordinary data: one soft-target entry
            torch.manual_seed(900 + 2 * w + j)
            opt.prepare_step(apply=(g.micro_step == 1))
            g(x, t, pt, epoch=31, train_iter=w, arch_sample=None)
    window(0)
    before = _snapshot(prod, opt)
    assert opt.skipped_steps() == 0 and all(bool(torch.isfinite(v.float()).all()) for v in before)
    window(1, bad_first=True)
    after = _snapshot(prod, opt)
    assert opt.skipped_steps() == 1 and not math.isfinite(float(opt.grad_norm()))           # once per window, not per micro-step
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    window(2)
    again = _snapshot(prod, opt)
    assert opt.skipped_steps() == 1 and math.isfinite(float(opt.grad_norm()))
    assert all(bool(torch.isfinite(v.float()).all()) for v in again)
    assert not torch.equal(again[0], after[0]) and not torch.equal(again[1], after[1])      # the clean window updated


# ---- 6. it trains ----------------------------------------------------------------------------------------------------------------------
def test_bf16_graphed_accumulation_trains():
    """bf16, two micro-batches of 8 per update (the halves of one batch of 16 with hard targets), 30 updates, optimizer in the graph:
    the loss falls below 0.6 x its start, the band of test_bf16_step_trains_like_the_fp32_step."""
    crit = SoftTargetCrossEntropy()
    x, _, _, labels = recipe.inputs(21, 16, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
    x = x.to(DEV)
    t = torch.nn.functional.one_hot(labels, recipe.MICRO_CLASSES).float().to(DEV)
    prod = build(seed=100)
    with torch.no_grad():
        n_patch = prod(x[:8], patch_output_type="seq")[1].shape[1]
    pt = t[:, None, :].repeat(1, n_patch, 1).contiguous()
    halves = [(x[:8].contiguous(), t[:8].contiguous(), pt[:8].contiguous()), (x[8:].contiguous(), t[8:].contiguous(), pt[8:].contiguous())]
    opt = FlatAdamW(prod, groups(prod), lr=1e-3)
    opt.own_shadow()
    prod.drop_path_generator(seed=5)
    g = engine.GraphedTrainStep(prod, crit, *halves[0], "seq", optimizer=opt, accum_steps=2)
    losses = []
    for it in range(60):
        torch.manual_seed(4000 + it)
        opt.prepare_step(apply=(g.micro_step == 1))
        losses.append(g(*halves[it % 2], epoch=31, train_iter=it // 2, arch_sample="multi").clone())
    traj = torch.stack(losses).cpu().double().view(30, 2).mean(1)             # per update: the mean of its two micro-batch losses
    msg = "bf16, k = 2: %.4f -> %.4f over %d updates" % (traj[0], traj[-1], opt._step)
    print(msg)
    assert opt._step == 30 and bool(torch.isfinite(traj).all())
    assert traj[-1] < 0.6 * traj[0], msg


# ---- 7. no exchange off-window -----------------------------------------------------------------------------------------------------------
class _CountingSync(engine.GradSync):
    def __init__(self, model):
        super().__init__(model)
        self.calls = []

    def all_reduce_range(self, lo, hi):
        self.calls.append(("all_reduce_range", lo, hi))
        return super().all_reduce_range(lo, hi)

    def finish(self, works, average=True):
        works = list(works)
        self.calls.append(("finish", len(works), average))
        return super().finish(works, average=average)

    def all_reduce_grads(self, average=True):
        self.calls.append(("all_reduce_grads", average))
        return super().all_reduce_grads(average=average)


@pytest.mark.parametrize("split", [False, True], ids=["whole", "split"])
def test_step_with_sync_exchanges_only_on_the_final_micro_step(split):
    crit = SoftTargetCrossEntropy()
    mb = micro_batches(2)
    seqs = {}
    for k in (1, 2):
        prod = build(dtype=torch.float32)
        g = engine.GraphedTrainStep(prod, crit, *mb[0], "seq", split_for_sync=split, accum_steps=k)
        assert bool(g.more_graphs) == split
        sync = _CountingSync(prod)
        per_call = []
        for it in range(2 * k):
            torch.manual_seed(900 + it)
            final = g.micro_step == k - 1
            g.step_with_sync(sync, *mb[it % 2], average=False, epoch=31, train_iter=it // k, arch_sample=None)
            per_call.append((final, list(sync.calls)))
            sync.calls.clear()
        torch.cuda.synchronize()
        seqs[k] = per_call
    today = seqs[1][0][1]
    assert today and all(c == today for _, c in seqs[1])          # k = 1: every step exchanges, as today
    assert [f for f, _ in seqs[2]] == [False, True, False, True]
    for final, calls in seqs[2]:
        assert calls == (today if final else []), (final, calls)
