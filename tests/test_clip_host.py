"""Host side of the on-device gradient-norm clipping (FlatAdamW(max_norm=...), vr_grad_sumsq / vr_clip_finish /
vr_adamw_flat_clip): the C ABI is declared and listed, the argument is validated, it survives the optimizer's state dict, and
switching it off costs nothing.  No kernel is launched here; tests/test_gpu_clip.py holds the numerical checks."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import recipe  # noqa: E402

import vitres  # noqa: E402
from vitres import _lib, engine, optim  # noqa: E402
from vitres.optim import FlatAdamW  # noqa: E402

ENTRY_POINTS = ("vr_grad_sumsq", "vr_clip_finish", "vr_adamw_flat_clip")


def micro():
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    return vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                               num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], **kw)


def flat(m, **kw):
    return FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=1e-3, **kw)


def test_header_declares_and_symbol_table_lists_the_clip_entry_points():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    declared = set(re.findall(r"^int\s+(vr_\w+)\s*\(", hdr, flags=re.M))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(_lib.lib(), name)
    assert "typedef struct vr_clip_state" in hdr
    # the ctypes mirror of vr_clip_state: 8 dwords, the count of skipped steps is dword 5 (FlatAdamW.skipped_steps reads it there)
    assert ctypes.sizeof(optim._ClipState) == 32 and optim._ClipState.skipped.offset == 20 and optim._ClipState.norm.offset == 8
    # the existing entry points kept their signatures
    assert len(_lib.SYMBOLS["vr_adamw_flat"]) == 12 and len(_lib.SYMBOLS["vr_adamw_flat_dev_capped"]) == 13


def test_max_norm_constructs_and_is_validated():
    m = micro()
    opt = flat(m, max_norm=1.0)
    assert opt.max_norm == 1.0 and opt.clip_enabled()
    assert flat(m, max_norm=float("inf")).clip_enabled()          # measure only
    for off in (None, 0, 0.0):
        assert not flat(m, max_norm=off).clip_enabled()
    for bad in (-1.0, float("nan"), -float("inf")):
        with pytest.raises(ValueError):
            flat(m, max_norm=bad)
    opt.max_norm = -2.0                                           # a plain attribute: checked where it is used
    with pytest.raises(ValueError):
        opt.clip_enabled()
    with pytest.raises(ValueError):
        opt.state_dict()


def test_max_norm_survives_the_state_dict_round_trip():
    torch.manual_seed(4)
    m = micro()
    opt = flat(m, max_norm=0.75)
    sd = opt.state_dict()
    assert sd["max_norm"] == 0.75
    assert {"step", "exp_avg", "exp_avg_sq", "ema", "param_groups"} <= set(sd)           # the layout is the old one plus the key
    opt2 = flat(m)
    assert opt2.max_norm is None
    opt2.load_state_dict(sd)
    assert opt2.max_norm == 0.75 and opt2.clip_enabled()
    off = flat(m).state_dict()
    assert off["max_norm"] is None
    opt2.load_state_dict(off)
    assert opt2.max_norm is None and not opt2.clip_enabled()
    del sd["max_norm"]                                            # a flat state dict written before the key existed
    opt3 = flat(m, max_norm=2.0)
    opt3.load_state_dict(sd)
    assert opt3.max_norm == 2.0


def test_torch_layout_state_dict_without_the_key_still_loads():
    torch.manual_seed(5)
    m = micro()
    ref = torch.optim.AdamW(engine.param_groups_weight_decay(m, 0.05), lr=1e-3)
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g) * 1e-2
        ref.step()
    for p in m.parameters():
        p.grad = None
    opt = flat(m, max_norm=3.0)
    opt.load_state_dict(ref.state_dict())
    assert opt._step == 2 and opt.max_norm == 3.0                 # the constructor's value stays
    back = opt.torch_state_dict()
    assert set(back) == {"state", "param_groups"}                 # what a checkpoint stores is unchanged
    torch.optim.AdamW(engine.param_groups_weight_decay(m, 0.05), lr=1e-3).load_state_dict(back)


def test_no_clip_state_is_allocated_while_max_norm_is_off():
    m = micro()
    opt = flat(m)
    opt.prepare_step()                                            # (CPU: fills the hyper-parameter block, launches nothing)
    assert opt._clip is None and opt.skipped_steps() == 0
    assert opt._hp_dev.numel() == optim.MAX_GROUPS * 8
    with pytest.raises(RuntimeError):
        opt.grad_norm()
    on = flat(m, max_norm=1.0)
    on.prepare_step()
    assert on._clip is not None and on._clip["state"].numel() == 8
    assert on._clip["state"][:2].tolist() == [1.0, 1.0]           # max_norm, grad_scale: what the finish kernel reads
    assert float(on.grad_norm()) == 0.0 and on.skipped_steps() == 0


def test_prepare_step_raises_when_max_norm_no_longer_matches_the_captured_graph():
    m = micro()
    opt = flat(m)
    opt._graph_clip = False                                       # what GraphedTrainStep records at capture
    opt.prepare_step()
    opt.max_norm = 1.0
    with pytest.raises(RuntimeError, match="max_norm"):
        opt.prepare_step()
    opt.max_norm = None
    opt._graph_clip = True
    with pytest.raises(RuntimeError, match="max_norm"):
        opt.prepare_step()
    opt.max_norm = float("inf")                                   # on <-> inf is the switch a captured graph follows
    opt.prepare_step()
