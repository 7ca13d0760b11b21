"""train_one_epoch(..., fast=FastPath()) refuses what the captured step does not serve, by name and before anything is launched (CPU).
That fast=None is the loop it was is shown by the suites that run it (tests/test_host_emulated.py, tests/test_accum_host.py)."""
import pytest
import torch

import recipe
import vitres
from vitres import engine
from vitres import kernels as K
from vitres.losses import SoftTargetCrossEntropy
from vitres.optim import FlatAdamW


class NoLoader:
    def __iter__(self):
        raise AssertionError("the loader was read before the arguments were checked")


@pytest.fixture
def setup(monkeypatch):
    def launched(*a, **kw):
        raise AssertionError("a kernel wrapper asked for a device pointer before the arguments were checked")
    monkeypatch.setattr(K, "_p", launched)
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0,
                            num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    return m, FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=1e-3)


def run(m, opt, device="cuda", **kw):
    return engine.train_one_epoch(m, SoftTargetCrossEntropy(), NoLoader(), opt, device, 31, fast=engine.FastPath(), **kw)


def test_optimizer_must_be_a_flat_adamw_of_this_model(setup):
    m, opt = setup
    with pytest.raises(ValueError, match="^optimizer"):
        run(m, torch.optim.AdamW(m.parameters(), lr=1e-3))
    other = vitres.create_model("flexible_vit_sr_patch14_224_patch_output", img_size=recipe.MICRO_IMG,
                                num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0])
    with pytest.raises(ValueError, match="^optimizer"):
        run(m, FlatAdamW(other, other.parameters(), lr=1e-3))


def test_loss_scaler_is_refused(setup):
    m, opt = setup
    with pytest.raises(ValueError, match="^loss_scaler"):
        run(m, opt, loss_scaler=lambda *a, **kw: None)


def test_teacher_is_refused(setup):
    m, opt = setup
    with pytest.raises(ValueError, match="^teacher_model"):
        run(m, opt, teacher_model=torch.nn.Identity())


def test_tensors_must_be_on_the_gpu(setup):
    m, opt = setup
    with pytest.raises(ValueError, match="^device"):
        run(m, opt, device="cpu")
    with pytest.raises(ValueError, match="^model"):               # a CUDA device named, the parameters still on the host
        run(m, opt, device="cuda")


def test_one_fast_path_serves_one_optimizer_and_criterion(setup):
    m, opt = setup
    fp = engine.FastPath()
    crit = SoftTargetCrossEntropy()
    with pytest.raises(ValueError, match="^device"):              # (records the pair, then stops at the CPU device)
        engine.train_one_epoch(m, crit, NoLoader(), opt, "cpu", 31, fast=fp)
    with pytest.raises(ValueError, match="^optimizer"):
        engine.train_one_epoch(m, crit, NoLoader(), FlatAdamW(m, m.parameters(), lr=1e-3), "cpu", 31, fast=fp)
    with pytest.raises(ValueError, match="^criterion"):
        engine.train_one_epoch(m, SoftTargetCrossEntropy(), NoLoader(), opt, "cpu", 31, fast=fp)


def test_fast_path_starts_empty():
    assert engine.FastPath().steps == [] and engine.FastPath.MAX_STEPS == 2
