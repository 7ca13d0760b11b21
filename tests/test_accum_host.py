"""Host side of gradient accumulation over micro-batches (accum_steps): validation, the 1/k factor the optimizer carries, the
no-update upload of a non-final micro-step, the window bookkeeping, the seed rule, and engine.train_one_epoch(accum_steps=2) against a
hand-written loop on the kernel emulation.  The kernels themselves and the captured step are checked in tests/test_gpu_grad_accum.py."""
import math
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import recipe  # noqa: E402

import emu_accum  # noqa: E402
import vitres  # noqa: E402
import vitres_oracle as O  # noqa: E402
from vitres import _lib, engine, optim  # noqa: E402
from vitres.optim import FlatAdamW  # noqa: E402

ENTRY_POINTS = ("vr_relayout_add", "vr_zero_ranges_gated", "vr_grad_sumsq_gated", "vr_clip_finish_gated")


def micro(et=0, mode="multi", dpr=0.0):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30,
              single_arch=(mode == "single"), hybrid_arch=(mode == "hybrid"))
    return vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                               num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[et], drop_path_rate=dpr,
                               drop_block_rate=None, **kw)


def filled(et=0, mode="multi", dpr=0.0, seed=100):
    m = micro(et, mode, dpr)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)
    m.load_state_dict(sd)
    m.set_compute_dtype(torch.float32)
    m.train()
    m.set_epoch(31)
    m.load_state_dict(sd)
    return m


def flat(m, **kw):
    return FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=1e-3, **kw)


def test_header_declares_and_symbol_table_lists_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    declared = set(re.findall(r"^int\s+(vr_\w+)\s*\(", hdr, flags=re.M))
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.SYMBOLS, name
        assert hasattr(_lib.lib(), name)
    # the gated forms take the ungated argument list plus one gate pointer in front of the stream; the old ones are unchanged
    for name in ("vr_zero_ranges", "vr_grad_sumsq", "vr_clip_finish"):
        assert len(_lib.SYMBOLS[name + "_gated"]) == len(_lib.SYMBOLS[name]) + 1
    assert len(_lib.SYMBOLS["vr_zero_ranges"]) == 3 and len(_lib.SYMBOLS["vr_grad_sumsq"]) == 7
    assert len(_lib.SYMBOLS["vr_clip_finish"]) == 4 and len(_lib.SYMBOLS["vr_relayout"]) == 10


def test_accum_steps_is_validated():
    m = micro()
    assert flat(m).accum_steps == 1
    assert flat(m, accum_steps=4).accum_steps == 4
    for bad in (0, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            flat(m, accum_steps=bad)
    opt = flat(m)
    opt.accum_steps = 0                                           # a plain attribute: checked where it is used
    with pytest.raises(ValueError):
        opt._group_structs(1)
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError):
            engine._check_accum(bad)
    with pytest.raises(ValueError):
        engine._check_accum(2, micro_step=2)
    with pytest.raises(ValueError):
        engine.train_one_epoch(m, None, [], None, "cpu", 0, accum_steps=0)


def test_group_structs_and_clip_upload_carry_grad_scale_over_k():
    m = micro()
    opt = flat(m, max_norm=1.5, accum_steps=4)
    opt.grad_scale = 0.5
    arr = opt._group_structs(1)
    assert all(arr[i].grad_scale == 0.125 for i in range(len(opt.param_groups)))
    c = opt._clip_upload(torch.device("cpu"))
    assert c["state"][:2].tolist() == [1.5, 0.125]                # max_norm, the factor vr_clip_finish scales the norm by
    opt.accum_steps = 1
    assert opt._group_structs(1)[0].grad_scale == 0.5             # k = 1: today's value
    assert opt._clip_upload(torch.device("cpu"))["state"][1].item() == 0.5


def test_prepare_step_without_apply_leaves_the_count_and_uploads_zeros():
    m = micro()
    opt = flat(m, max_norm=1.0, accum_steps=2)
    opt.prepare_step()
    assert opt._step == 1 and float(opt._hp_dev.abs().sum()) > 0
    state = opt._clip["state"].clone()
    opt.max_norm = 3.0
    opt.prepare_step(apply=False)
    assert opt._step == 1                                         # the count follows optimizer updates
    assert torch.equal(opt._hp_dev, torch.zeros_like(opt._hp_dev))          # bias_c1 == 0 in every group: "no update this replay"
    assert torch.equal(opt._clip["state"], state)                 # nothing of the clip state is touched either
    opt.prepare_step(apply=True)
    assert opt._step == 2 and float(opt._hp_dev.abs().sum()) > 0 and opt._clip["state"][0].item() == 3.0
    assert opt._hp_dev[7].item() == 0.5                           # grad_scale / accum_steps of group 0
    # the bias corrections are those of update 2
    assert abs(opt._hp_dev[5].item() - (1 - 0.9 ** 2)) < 1e-7


def test_window_bookkeeping_wraps():
    pos, seen = 0, []
    for _ in range(7):
        clear, apply, nxt = engine._window(pos, 3)
        seen.append((pos, clear, apply))
        pos = nxt
    assert seen == [(0, True, False), (1, False, False), (2, False, True)] * 2 + [(0, True, False)]
    assert engine._window(0, 1) == (True, True, 0)                # k = 1: every step clears and applies


class Crit(torch.nn.Module):
    def forward(self, x, t):
        return O.soft_target_ce(x, t)


class Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


def batches(n):
    out = []
    for it in range(n):
        x, t, _, _ = recipe.inputs(300 + it, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
        out.append((x, t))
    return out


@pytest.mark.parametrize("n_batches", [4, 5], ids=["whole-windows", "trailing-window"])
def test_emulated_epoch_with_two_micro_steps_equals_a_hand_written_loop(monkeypatch, n_batches):
    """train_one_epoch(accum_steps=2) in 'single' mode against the loop written out: zero_grad per window, two backwards of loss / 2,
    one optimizer step, the seed epoch * 10000 + UPDATE index for both micro-steps.  The fifth batch of the second case is dropped."""
    emu_accum.install(monkeypatch)
    crit, loader = Crit(), batches(n_batches)
    seeds = []
    real_seed = torch.manual_seed

    def noting(s):
        seeds.append(int(s))
        return real_seed(s)
    # the loop under test
    prod = filled(mode="single")
    opt = torch.optim.AdamW(engine.param_groups_weight_decay(prod, 0.05), lr=1e-3)
    log = Log()
    torch.manual_seed(4321)
    monkeypatch.setattr(torch, "manual_seed", noting)
    stats = engine.train_one_epoch(prod, crit, loader, opt, "cpu", 31, None, max_norm=None, print_freq=0, arch_sample="single",
                                   logger=log, accum_steps=2)
    monkeypatch.setattr(torch, "manual_seed", real_seed)
    assert seeds == [310000, 310000, 310001, 310001]              # the optimizer update's index, shared by a window
    dropped = [s for s in log.lines if "trailing" in s]
    assert len(dropped) == (1 if n_batches == 5 else 0)
    # written out
    twin = filled(mode="single")
    topt = torch.optim.AdamW(engine.param_groups_weight_decay(twin, 0.05), lr=1e-3)
    torch.manual_seed(4321)
    losses = []
    for u in range(2):
        topt.zero_grad(set_to_none=True)
        for j in range(2):
            x, t = loader[2 * u + j]
            rng = torch.random.get_rng_state()
            torch.manual_seed(31 * 10000 + u)
            loss = crit(twin(x)[0], t)
            torch.random.set_rng_state(rng)
            (loss / 2).backward()
            losses.append(loss.item())
        topt.step()
    assert stats["loss"] == pytest.approx(sum(losses) / 4, rel=1e-12)        # every micro-batch's own loss is metered
    assert all(math.isfinite(v) for v in losses)
    sd, tsd = prod.state_dict(), twin.state_dict()
    assert recipe.checksum(sd) == recipe.checksum(tsd)
    for k in sd:
        assert torch.equal(sd[k], tsd[k]), k
    assert not torch.equal(sd["cls_head.weight"], filled(mode="single").state_dict()["cls_head.weight"])     # (it did train)


def test_emulated_epoch_at_one_micro_step_is_the_old_loop(monkeypatch):
    """accum_steps=1 (the default) and an explicit 1 walk the same path: the same losses, the same parameters."""
    emu_accum.install(monkeypatch)
    out = []
    for kw in ({}, {"accum_steps": 1}):
        prod = filled()
        opt = torch.optim.AdamW(engine.param_groups_weight_decay(prod, 0.05), lr=1e-3)
        torch.manual_seed(77)
        stats = engine.train_one_epoch(prod, Crit(), batches(3), opt, "cpu", 31, None, max_norm=None, print_freq=0,
                                       arch_sample="multi", logger=Log(), **kw)
        out.append((stats, prod.state_dict()))
    assert out[0][0] == out[1][0]
    assert all(torch.equal(out[0][1][k], out[1][1][k]) for k in out[0][1])


@pytest.mark.parametrize("et", [0, 4, 5])
def test_emulated_loss_and_grad_accumulates_every_parameter(monkeypatch, et):
    """The host routing of loss_and_grad(accumulate=True) on the emulation: every parameter's accumulated gradient is g1 + g2 (the
    writers that go through a temporary add, BatchNorm's sums do not pollute dz), and the seeds of tests/test_gpu_grad_accum.py give every
    parameter tensor a non-zero gradient in each micro-batch."""
    emu_accum.install(monkeypatch)
    prod = filled(et, dpr=0.2, seed=100 + et)
    mb = []
    for s in (7, 8):
        x, t, pt, _ = recipe.inputs(s, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
        mb.append((x, t, pt))

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
    l0 = run(0, accumulate=True)                                  # nothing there yet: behaves as a fresh call
    l1 = run(1, accumulate=True)
    assert l0.item() != l1.item()
    for n, p in prod.named_parameters():
        if not p.requires_grad:
            continue
        g1, g2 = single[0][n], single[1][n]
        assert float(g1.abs().max()) > 0 and float(g2.abs().max()) > 0, n
        want = g1.double() + g2.double()
        err = float((p.grad.double() - want).norm() / want.norm())
        assert err < 1e-6, (n, err)
    with pytest.raises(RuntimeError, match="fresh gradients"):
        prod.loss_and_grad(*mb[0], "seq")                         # without the flag the old rule stands
