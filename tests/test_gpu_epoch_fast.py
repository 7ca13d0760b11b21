"""engine.train_one_epoch(..., fast=engine.FastPath()): the epoch loop on the captured step (GraphedTrainStep with the FlatAdamW update,
clipping and accumulation inside its graph) against the eager loop and against hand-driven replays.  Micro supernet, 8 samples,
example_per_arch 2."""
import copy
import math

import pytest
import torch

import recipe
import vitres
from vitres import checkpoint, engine
from vitres.losses import SoftTargetCrossEntropy
from vitres.optim import FlatAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"
CRIT = SoftTargetCrossEntropy()
QUIET = type("L", (), {"info": staticmethod(lambda s: None)})


def build(dtype=torch.bfloat16, dpr=0.0, et=0):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[et], drop_path_rate=dpr, **kw)
    m.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 100 + et))
    return m.to(DEV).set_compute_dtype(dtype)


def optim(model, **kw):
    return FlatAdamW(model, engine.param_groups_weight_decay(model, 0.05), lr=2e-3, **kw)


_MB = {}


def batches(n, first=0, size=8):
    """Loader of n batches (images, soft targets) on the device, made once; PATCH[targets.data_ptr()] holds the patch targets."""
    out = []
    for i in range(first, first + n):
        if (i, size) not in _MB:
            x, t, pt, _ = recipe.inputs(40 + i, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
            _MB[(i, size)] = (x[:size].to(DEV), t[:size].to(DEV), pt[:size].to(DEV))
        out.append(_MB[(i, size)])
    return out


class Mix:
    """patch_mixup_fn stub: draws from the CPU RNG as a mixup does, returns 'seq' patch targets, logs the previous step's keep tables."""

    def __init__(self, model, data):
        self.model, self.keeps = model, []
        self.patch = {t.data_ptr(): pt for _, t, pt in data}

    def log(self):
        k = self.model.last_keeps
        self.keeps.append(None if k is None else torch.stack(list(k)).clone())

    def __call__(self, x, t):
        torch.rand(3)
        self.log()
        return x, t, self.patch[t.data_ptr()], "seq"


def epoch(model, opt, data, ep, fast, **kw):
    mix = Mix(model, data)
    stats = engine.train_one_epoch(model, CRIT, [(x, t) for x, t, _ in data], opt, DEV, ep, patch_mixup_fn=mix, print_freq=0,
                                   logger=QUIET, fast=fast, **kw)
    mix.log()
    torch.cuda.synchronize()
    return stats, mix.keeps


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


def same_keeps(a, b):
    return len(a) == len(b) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_same_trajectory_as_the_eager_loop(dtype):
    """Two epochs (30: rewiring in set_epoch, and 31) of three batches, arch_sample='multi', a learning-rate change between them.
    Bands: those of test_optimizer_inside_the_graph_equals_step_after_the_graph (the same two paths)."""
    data = batches(3)
    runs = []
    for use_fast in (False, True):
        torch.manual_seed(2024)
        m = build(dtype)
        opt = optim(m, ema_decay=0.99)
        fp = engine.FastPath() if use_fast else None
        m.train()
        out, keeps, steps = [], [], []
        for ep, lr in ((30, 2e-3), (31, 5e-4)):
            for grp in opt.param_groups:
                grp["lr"] = lr
            m.set_epoch(ep)
            s, k = epoch(m, opt, data, ep, fp, arch_sample="multi")
            out.append(s)
            keeps.append(k[1:])                                   # (entry 0: before the epoch's first step)
            if fp is not None:
                steps.append(list(fp.steps))
        runs.append((out, keeps, m._arena["flat"].clone(), opt._flat_state["ema"].clone(), opt._step, steps))
    (s0, k0, p0, e0, n0, _), (s1, k1, p1, e1, n1, steps) = runs
    assert n0 == n1 == 6
    assert len(steps[0]) == 1 and len(steps[1]) == 1 and steps[0][0] is steps[1][0]      # the second epoch reuses the captured step
    for a, b in zip(k0, k1):
        assert len(a) == 3 and same_keeps(a, b)
    assert not torch.equal(k0[1][0], k0[1][1])                    # (the stub's draws move the tables from step to step)
    for a, b in zip(s0, s1):
        assert list(a) == list(b) == ["loss", "lr"] and a["lr"] == b["lr"]
        print("loss eager %r fast %r" % (a["loss"], b["loss"]))
        assert abs(a["loss"] - b["loss"]) < (1e-5 if dtype == torch.float32 else 2e-2) * abs(a["loss"])
    assert s0[0]["lr"] == 2e-3 and s0[1]["lr"] == 5e-4
    print("parameters rel", rel(p1, p0), "ema rel", rel(e1, e0))
    assert rel(p1, p0) < 2e-3 and rel(e1, e0) < 2e-3


def test_accumulation_and_clipping_follow_the_eager_loop():
    data = batches(5)                                             # two windows of two; the fifth batch is a dropped trailing window
    runs = []
    for use_fast in (False, True):
        torch.manual_seed(7)
        m = build(torch.float32)
        opt = optim(m)
        m.train()
        m.set_epoch(31)
        fp = engine.FastPath() if use_fast else None
        s, _ = epoch(m, opt, data, 31, fp, arch_sample="multi", accum_steps=2, max_norm=1.0)
        runs.append((s, m, opt, fp, float(opt.grad_norm())))
    (s0, m0, o0, _, n0), (s1, m1, o1, fp, n1) = runs
    assert o0._step == o1._step == 2 and o1.max_norm == 1.0 and o1.accum_steps == 2
    print("grad norm eager %r fast %r" % (n0, n1))
    assert abs(n1 - n0) < 1e-4 * n0
    assert abs(s1["loss"] - s0["loss"]) < 1e-5 * abs(s0["loss"]) and s1["lr"] == s0["lr"]
    assert rel(m1._arena["flat"], m0._arena["flat"]) < 2e-3
    step = fp.steps[0]
    assert step.micro_step == 0 and step.accum_steps == 2 and step.optimizer is o1
    # an inf in one micro-batch's input: the window is skipped once, nothing on the device moves; the loop's finite check exits
    before = [m1._arena["flat"].clone(), o1._flat_state["m"].clone(), o1._flat_state["v"].clone()]
    x, t, pt = data[0]
    bad = x.clone()
    bad[0, 0, 0, 0] = float("inf")
    poisoned = [(bad, t, pt), data[1]]
    with pytest.raises(SystemExit):
        epoch(m1, o1, poisoned, 31, fp, arch_sample="multi", accum_steps=2, max_norm=1.0, sync_every=100)
    torch.cuda.synchronize()
    assert o1.skipped_steps() == 1 and fp.steps[0] is step
    after = [m1._arena["flat"], o1._flat_state["m"], o1._flat_state["v"]]
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_recapture_rules():
    m = build(torch.bfloat16)
    opt = optim(m)
    m.train()
    m.set_epoch(31)
    fp = engine.FastPath()
    run = lambda size, **kw: epoch(m, opt, batches(2, size=size), 31, fp, arch_sample="multi", **kw)   # noqa: E731
    run(8)
    s8, = fp.steps
    run(4)                                                        # a second batch size adds a second captured step
    assert len(fp.steps) == 2 and fp.steps[0] is s8
    s4 = fp.steps[1]
    run(8)                                                        # reused, now the most recent
    assert fp.steps == [s4, s8]
    run(8, max_norm=1.0)                                          # a third key evicts the least recently used
    assert len(fp.steps) == 2 and fp.steps[0] is s8 and s4 not in fp.steps
    s8c = fp.steps[1]
    assert math.isfinite(float(opt.grad_norm()))
    run(8)                                                        # clipping off again: the plain step, nothing raises
    assert fp.steps == [s8c, s8] and opt.max_norm is None
    run(4)                                                        # evicts the clipping step ...
    run(8, max_norm=1.0)                                          # ... and on again re-captures
    assert s8c not in fp.steps and s8 not in fp.steps and len(fp.steps) == 2
    run(8, max_norm=0)                                            # on -> off with no plain step left: re-captured, not raised
    assert len(fp.steps) == 2 and fp.steps[1].optimizer is opt and opt._graph_clip is False
    n = opt._step
    m.set_compute_dtype(torch.float32)                            # another compute dtype re-captures
    bf16_steps = list(fp.steps)
    run(8)
    assert fp.steps[1] not in bf16_steps and opt._step == n + 2


def test_drop_path_stream_and_resume():
    data = batches(3)

    def fresh():
        torch.manual_seed(11)
        m = build(torch.float32, dpr=0.2)
        m.train()
        m.set_epoch(31)
        return m, optim(m)
    m, opt = fresh()
    fp = engine.FastPath()
    s1, _ = epoch(m, opt, data, 31, fp, arch_sample="multi")
    state = m.drop_path_rng_state().clone()
    ck = copy.deepcopy(checkpoint.checkpoint_dict(m, opt, None, 31))
    rng = torch.random.get_rng_state()
    s2, _ = epoch(m, opt, data, 32, fp, arch_sample="multi")
    # the same number of hand-driven replays
    h, hopt = fresh()
    g = engine.GraphedTrainStep(h, CRIT, *data[0], "seq", optimizer=hopt)
    for it, (x, t, pt) in enumerate(data):
        hopt.prepare_step()
        g(x, t, pt, epoch=31, train_iter=it, arch_sample="multi")
    torch.cuda.synchronize()
    assert torch.equal(h.drop_path_rng_state(), state)
    # a checkpoint taken between the epochs resumes to the same losses (fp32 band of the same path run twice: atomics order)
    r, ropt = fresh()
    assert checkpoint.resume(ck, r, ropt) == 32
    torch.random.set_rng_state(rng)
    r2, _ = epoch(r, ropt, data, 32, engine.FastPath(), arch_sample="multi")
    print("epoch 32 loss %r resumed %r" % (s2["loss"], r2["loss"]))
    assert abs(r2["loss"] - s2["loss"]) < 1e-5 * abs(s2["loss"]) and s1["loss"] != s2["loss"]


class Ema:
    def __init__(self):
        self.updates = 0

    def update(self, model):
        self.updates += 1


def test_model_ema_and_the_optimizer_ema_are_updated():
    data = batches(4)
    runs = []
    for use_fast in (False, True):
        torch.manual_seed(5)
        m = build(torch.bfloat16)
        opt = optim(m, ema_decay=0.9)
        m.train()
        m.set_epoch(31)
        ema = Ema()
        epoch(m, opt, data, 31, engine.FastPath() if use_fast else None, arch_sample="multi", accum_steps=2, model_ema=ema)
        assert ema.updates == 2                                   # once per update, not per micro-batch
        runs.append((opt._flat_state["ema"].clone(), m._arena["flat"].clone()))
    assert not torch.equal(runs[1][0], runs[1][1])
    assert rel(runs[1][0], runs[0][0]) < 2e-3


def test_one_rank_with_grad_sync_runs_the_in_graph_form():
    m = build(torch.bfloat16)
    opt = optim(m)
    m.train()
    m.set_epoch(31)
    fp = engine.FastPath()
    sync = engine.GradSync(m)
    assert sync.world == 1
    s, _ = epoch(m, opt, batches(2), 31, fp, arch_sample="multi", grad_sync=sync)
    assert fp.steps[0].optimizer is opt and not fp.steps[0].more_graphs and opt._step == 2 and math.isfinite(s["loss"])


def test_fp32_training_after_a_bf16_arena_reads_fp32_weights():
    """set_compute_dtype(float32) on a model whose arena was made in bf16 (the re-capture case above): the fp32 backward must read
    the fp32 weights, not the transposed bf16 shadows a bf16 arena keeps for its fused data gradients.  Against a model that was
    fp32 from the start, same state and draws: loss 1e-5, whole-arena gradient within the project's fp32 band (relative L2 5e-4)."""
    x, t, pt = batches(1)[0]
    out = []
    for first in (torch.bfloat16, torch.float32):
        m = build(first)
        m.train()
        m.set_epoch(31)
        if first == torch.bfloat16:
            torch.manual_seed(3)
            m.zero_grad(set_to_none=True)
            m.loss_and_grad(x, t, pt, "seq")                      # (makes the arena, in bf16)
            assert m._arena["tmap"]
            m.set_compute_dtype(torch.float32)
        torch.manual_seed(3)
        m.zero_grad(set_to_none=True)
        loss = m.loss_and_grad(x, t, pt, "seq")
        torch.cuda.synchronize()
        out.append((float(loss), m._arena["gcur"].clone()))
    (la, ga), (lb, gb) = out
    print("loss %r %r gradient rel l2 %r" % (la, lb, float((ga - gb).double().norm() / gb.double().norm())))
    assert abs(la - lb) < 1e-5 * abs(lb)
    assert float((ga - gb).double().norm() / gb.double().norm()) <= 5e-4


def _two_ranks(backend):
    """Two ranks of tests/epoch_fast_worker.py under torch.distributed.run (127.0.0.1 rendezvous)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VITRES_DIST_BACKEND=backend)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(here, "epoch_fast_worker.py")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("FAST ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("FAST "):])


def _check_two_ranks(d, backend):
    """Eager loop against fast= on two ranks, bf16, accum_steps 2, max_norm 1.0.  Bands: those of the bf16 cases of
    test_one_captured_graph_serves_the_whole_window (parameters / EMA 2e-3, gradient norm 2e-2) and of the trajectory test (loss 2e-2)."""
    print(d)
    assert d["backend"] == backend and d["world"] == 2
    assert d["split"] == [1, True, 1, 0]                          # one captured step, optimizer outside it, backward in two graphs
    assert d["steps"] == [2, 2] and d["skipped"] == [0, 0] and d["lr"][0] == d["lr"][1]
    assert d["grad_scale_after"] == 1.0                           # the 1 / world of the update does not stick to the optimizer
    assert abs(d["loss"][1] - d["loss"][0]) < 2e-2 * abs(d["loss"][0])
    assert abs(d["norm"][1] - d["norm"][0]) < 2e-2 * d["norm"][0]
    assert d["param_rel"] < 2e-3 and d["ema_rel"] < 2e-3 and d["moved"]
    assert d["shadow_in_step"] and d["ranks_agree"]


def test_two_ranks_over_rccl():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _check_two_ranks(_two_ranks("nccl"), "nccl")


def test_two_ranks_sharing_one_gpu_over_gloo():
    """The several-rank form where one GPU is visible: both ranks on GPU 0, the exchange over gloo (a functional check)."""
    _check_two_ranks(_two_ranks("gloo"), "gloo")
