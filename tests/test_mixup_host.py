"""vitres.mixup.Mixup without a GPU: the order of its numpy draws against timm 0.3.2's, written out here call by call; the two
rounding rules of 1 - lam; what it refuses; the entry points' argument checks (which return before any launch); and the eager
train_one_epoch with the kernel wrapper replaced by tests/mixup_ref.py's emulation, against timm's statements on the same draws."""
import os
import re

import numpy as np
import pytest
import torch

import emu_kernels
import mixup_ref
import recipe
import vitres
import vitres_oracle as O
from vitres import _lib, engine, kernels as K
from vitres.mixup import Mixup, param_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P = 0x10000                                                       # a fake, 16-byte aligned device address: nothing is launched
H, W = 24, 40


# ---- draw order --------------------------------------------------------------------------------------------------------------------
def replay_box(lam, minmax, correct_lam):
    """timm's cutmix_bbox_and_lam on an H x W image, numpy call by numpy call."""
    if minmax is not None:
        cut_h = np.random.randint(int(H * minmax[0]), int(H * minmax[1]))
        cut_w = np.random.randint(int(W * minmax[0]), int(W * minmax[1]))
        yl = np.random.randint(0, H - cut_h)
        xl = np.random.randint(0, W - cut_w)
        yu, xu = yl + cut_h, xl + cut_w
    else:
        ratio = np.sqrt(1 - lam)
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy = np.random.randint(0, H)
        cx = np.random.randint(0, W)
        yl, yu = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
        xl, xu = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
    if correct_lam or minmax is not None:
        lam = 1. - (yu - yl) * (xu - xl) / float(H * W)
    return (int(yl), int(yu), int(xl), int(xu)), lam


def replay_batch(mixup_alpha, cutmix_alpha, minmax, prob, switch_prob, correct_lam):
    if minmax is not None:
        cutmix_alpha = 1.0
    lam, cut, box = 1., False, None
    if np.random.rand() < prob:
        if mixup_alpha > 0. and cutmix_alpha > 0.:
            cut = bool(np.random.rand() < switch_prob)
            lam = np.random.beta(cutmix_alpha, cutmix_alpha) if cut else np.random.beta(mixup_alpha, mixup_alpha)
        elif mixup_alpha > 0.:
            lam = np.random.beta(mixup_alpha, mixup_alpha)
        else:
            cut = True
            lam = np.random.beta(cutmix_alpha, cutmix_alpha)
        lam = float(lam)
    if lam != 1. and cut:
        box, lam = replay_box(lam, minmax, correct_lam)
    return lam, cut, box


def replay_elem(n, mixup_alpha, cutmix_alpha, minmax, prob, switch_prob, correct_lam):
    if minmax is not None:
        cutmix_alpha = 1.0
    cut = np.zeros(n, dtype=bool)
    if mixup_alpha > 0. and cutmix_alpha > 0.:
        cut = np.random.rand(n) < switch_prob
        lam_cut = np.random.beta(cutmix_alpha, cutmix_alpha, size=n)
        lam_mix = np.random.beta(mixup_alpha, mixup_alpha, size=n)              # both arrays are always drawn
        lam_mix = np.where(cut, lam_cut, lam_mix)
    elif mixup_alpha > 0.:
        lam_mix = np.random.beta(mixup_alpha, mixup_alpha, size=n)
    else:
        cut = np.ones(n, dtype=bool)
        lam_mix = np.random.beta(cutmix_alpha, cutmix_alpha, size=n)
    lam = np.where(np.random.rand(n) < prob, lam_mix.astype(np.float32), np.ones(n, dtype=np.float32))
    assert lam.dtype == np.float32
    boxes = [None] * n
    for i in range(n):                                            # boxes afterwards, in sample order, only for cutmix with lam != 1
        if lam[i] != 1. and cut[i]:
            boxes[i], lam[i] = replay_box(lam[i], minmax, correct_lam)
    return lam, cut, boxes


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


BATCH_CONFIGS = {
    "both": dict(mixup_alpha=0.8, cutmix_alpha=1.0),
    "mixup_only": dict(mixup_alpha=0.8, cutmix_alpha=0.),
    "cutmix_only": dict(mixup_alpha=0., cutmix_alpha=1.0),
    "minmax": dict(mixup_alpha=0.8, cutmix_alpha=0., cutmix_minmax=(0.2, 0.7)),
    "prob_half": dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5),
    "uncorrected": dict(mixup_alpha=0.8, cutmix_alpha=1.0, correct_lam=False, switch_prob=0.8),
}


def _cfg(kw):
    return (kw.get("mixup_alpha", 1.), kw.get("cutmix_alpha", 0.), kw.get("cutmix_minmax"), kw.get("prob", 1.0),
            kw.get("switch_prob", 0.5), kw.get("correct_lam", True))


@pytest.mark.parametrize("name", sorted(BATCH_CONFIGS))
def test_batch_mode_draws_in_timms_order(name):
    kw = BATCH_CONFIGS[name]
    seen = set()
    for seed in range(12):
        np.random.seed(seed)
        d = Mixup(num_classes=10, **kw).draw(8, (H, W))
        after = np.random.get_state()
        np.random.seed(seed)
        lam, cut, box = replay_batch(*_cfg(kw))
        assert same_state(after, np.random.get_state()), (name, seed)
        assert d["mode"] == 'batch' and isinstance(d["lam"], float) and d["lam"] == lam and d["cutmix"] == cut and d["box"] == box
        if box is not None:
            assert 0 <= box[0] <= box[1] <= H and 0 <= box[2] <= box[3] <= W
        seen.add("identity" if lam == 1. and box is None else "cutmix" if cut else "blend")
    want = {"both": {"cutmix", "blend"}, "mixup_only": {"blend"}, "cutmix_only": {"cutmix"}, "minmax": {"cutmix", "blend"},
            "prob_half": {"cutmix", "blend", "identity"}, "uncorrected": {"cutmix", "blend"}}[name]
    assert seen == want, seen                                     # the seeds reach every branch the configuration has


@pytest.mark.parametrize("mode", ["elem", "pair"])
@pytest.mark.parametrize("name", ["both", "mixup_only", "cutmix_only", "minmax", "prob_half", "uncorrected"])
def test_elem_and_pair_modes_draw_in_timms_order(mode, name):
    kw = BATCH_CONFIGS[name]
    B = 8
    n = B if mode == "elem" else B // 2
    for seed in range(4):
        np.random.seed(100 + seed)
        d = Mixup(num_classes=10, mode=mode, **kw).draw(B, (H, W))
        after = np.random.get_state()
        np.random.seed(100 + seed)
        lam, cut, boxes = replay_elem(n, *_cfg(kw))
        assert same_state(after, np.random.get_state()), (mode, name, seed)
        assert d["mode"] == mode and d["lam"].dtype == np.float32 and d["lam"].shape == (n,)
        assert np.array_equal(d["lam"], lam) and np.array_equal(d["cutmix"], cut) and d["box"] == boxes
        rows = param_table(d, B)
        assert rows.shape == (B,)
        if mode == "pair":                                        # sample B-1-i gets sample i's parameters
            assert all(rows[i] == rows[B - 1 - i] for i in range(B))
        assert np.array_equal(rows["lam"][:n], lam)
        assert np.array_equal(rows["cutmix"][:n] != 0, np.array([b is not None for b in boxes]))


def test_a_skipped_batch_draws_once_and_changes_nothing():
    np.random.seed(3)
    d = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0., num_classes=10).draw(8, (H, W))
    after = np.random.get_state()
    np.random.seed(3)
    np.random.rand()
    assert same_state(after, np.random.get_state())
    assert d == dict(mode='batch', lam=1., cutmix=False, box=None)
    rows = param_table(d, 8)
    assert (rows["lam"] == 1).all() and (rows["oml"] == 0).all() and (rows["cutmix"] == 0).all()


# ---- rounding ------------------------------------------------------------------------------------------------------------------------
LAM = 0.6            # fp32(1. - 0.6) = 0.4 but fp32(1) - fp32(0.6) = 0.39999998: found by a search over np.random.beta(.8, .8) draws


def test_each_mode_rounds_one_minus_lam_its_own_way(monkeypatch):
    by_double, by_fp32 = np.float32(1. - LAM), np.float32(1) - np.float32(LAM)
    assert by_double != by_fp32 and by_double == np.float32(0.4) and by_fp32 == np.nextafter(np.float32(0.4), np.float32(0))
    calls = mixup_ref.install(monkeypatch)
    x, _, _, y = recipe.inputs(5, 4, 8, 10, 1)
    mixer = Mixup(num_classes=10)
    draws = {"batch": dict(mode='batch', lam=LAM, cutmix=False, box=None),
             "elem": dict(mode='elem', lam=np.full(4, LAM, dtype=np.float32), cutmix=np.zeros(4, dtype=bool), box=[None] * 4),
             "pair": dict(mode='pair', lam=np.full(2, LAM, dtype=np.float32), cutmix=np.zeros(2, dtype=bool), box=[None] * 2)}
    for mode, want in (("batch", by_double), ("elem", by_fp32), ("pair", by_fp32)):
        got_x, got_t = mixer(x, y, draw=draws[mode])
        rows = calls[-1]["params"]
        assert (rows["lam"] == np.float32(LAM)).all() and (rows["oml"] == want).all(), mode
        ref_x, ref_t = mixup_ref.mix(x, y, draws[mode], 10, 0.1)  # ... and that IS timm's arithmetic in that mode
        assert mixup_ref.bits_equal(got_x, ref_x) and mixup_ref.bits_equal(got_t, ref_t), mode
    # the smoothed one-hot values: doubles, rounded to fp32 on the way into the kernel
    assert calls[-1]["off"] == 0.1 / 10 and calls[-1]["on"] == 1. - 0.1 + 0.1 / 10


# ---- validation ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    declared = set(re.findall(r"^int\s+(vr_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.lib()
    for name in ("vr_mixup", "vr_mixup_u8"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.vr_version() >= 1003
    assert K.MIXUP_PARAM.itemsize == 32 and K.MIXUP_PARAM.names == tuple(n for n, _ in _lib.MixupParam._fields_)
    assert re.search(r"float lam, oml;\s*int32_t y0, y1, x0, x1;\s*int32_t cutmix;\s*int32_t pad;", hdr)


def _abi(u8, samples=P, out=P * 2, labels=P * 3, targets=P * 4, params=P * 5, B=4, C=3, H_=8, W_=16, K_=10, mean=True):
    lib = _lib.lib()
    args = (samples, out, labels, targets, params, B, C, H_, W_, K_, 0.9, 0.01)
    if not u8:
        return lib.vr_mixup(*args, None)
    m, s = K.norm_constants(MEAN + (0.5,), STD + (0.25,))
    return lib.vr_mixup_u8(*args, m if mean else None, s, None)


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
def test_entry_points_validate_before_any_launch(u8):
    for name in ("samples", "out", "labels", "targets", "params"):
        assert _abi(u8, **{name: None}) == EINVAL, name
    assert _abi(u8, B=0) == EINVAL and _abi(u8, H_=-1) == EINVAL and _abi(u8, K_=0) == EINVAL
    assert _abi(u8, W_=18) == EUNSUPPORTED                        # W % 4
    assert _abi(u8, B=3) == EUNSUPPORTED                          # an odd batch has a sample that is its own partner
    assert _abi(u8, out=P) == EUNSUPPORTED                        # samples == out
    assert _abi(u8, out=P * 2 + 4) == EALIGN and _abi(u8, params=P * 5 + 2) == EALIGN
    assert _abi(u8, B=0, W_=18) == EINVAL and _abi(u8, B=3, out=P * 2 + 4) == EUNSUPPORTED       # EINVAL, EUNSUPPORTED, EALIGN
    if u8:
        assert _abi(u8, mean=False) == EINVAL and _abi(u8, C=5) == EUNSUPPORTED
        assert _abi(u8, samples=P + 2) == EALIGN                  # (bytes: 4-byte alignment is enough, P + 4 would be launched)
    else:
        assert _abi(u8, samples=P + 4) == EALIGN and _abi(u8, C=5, B=3) == EUNSUPPORTED


def test_box_check_is_the_host_wrappers():
    rows = np.zeros(4, dtype=K.MIXUP_PARAM)
    rows["lam"], rows["cutmix"] = 1, 1
    assert K.check_mixup_params(rows, 4, 8, 16) is not None       # the empty box is legal
    rows["y1"], rows["x1"] = 8, 16
    K.check_mixup_params(rows, 4, 8, 16)                          # ... and so is the whole image
    for field, value in (("y1", 9), ("x1", 17), ("y0", -1), ("x0", -1), ("y0", 9), ("x0", 17)):
        bad = rows.copy()
        bad[field][2] = value
        with pytest.raises(RuntimeError, match="VR_EINVAL.*sample 2"):
            K.check_mixup_params(bad, 4, 8, 16)
    with pytest.raises(ValueError, match="table"):
        K.check_mixup_params(rows[:3], 4, 8, 16)
    x = torch.zeros(4, 3, 8, 16)
    bad = rows.copy()
    bad["x1"][0] = 17
    with pytest.raises(RuntimeError, match="VR_EINVAL"):          # refused before the CPU tensor is
        K.mixup(x, torch.zeros(4, dtype=torch.int64), bad, 10, 0.9, 0.01)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):           # CPU tensors: there is no CPU path
        K.mixup(x, torch.zeros(4, dtype=torch.int64), rows, 10, 0.9, 0.01)
    with pytest.raises(TypeError):
        K.mixup(x.to(torch.uint8), torch.zeros(4, dtype=torch.int64), rows, 10, 0.9, 0.01)


def test_mixup_refuses_what_it_does_not_take(monkeypatch):
    y = torch.zeros(4, dtype=torch.int64)
    xf, u8 = torch.zeros(4, 3, 8, 8), torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="mode"):
        Mixup(mode="half")
    state = np.random.get_state()
    with pytest.raises(AssertionError, match="Batch size should be even when using this"):
        Mixup(num_classes=10)(xf[:3], y[:3])
    with pytest.raises(ValueError, match="input_norm"):
        Mixup(num_classes=10)(u8, y)                              # uint8 without a normaliser
    with pytest.raises(ValueError, match="twice"):
        Mixup(num_classes=10, input_norm=(MEAN, STD))(xf, y)
    assert same_state(state, np.random.get_state())               # refused before anything was drawn
    with pytest.raises(RuntimeError, match="CUDA/HIP"):           # CPU tensors have no path, as for SwitchTokenMix
        Mixup(num_classes=10)(xf, y)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        Mixup(num_classes=10, input_norm=(MEAN, STD))(u8, y)
    assert Mixup(input_norm=(MEAN, STD)).normalizes and not Mixup().normalizes
    assert Mixup(cutmix_minmax=(0.2, 0.8)).cutmix_alpha == 1.0
    mixup_ref.install(monkeypatch)
    mixer = Mixup(num_classes=10)
    for kw in (dict(out=torch.empty(4, 3, 8, 4)), dict(out=torch.empty(4, 3, 8, 8, dtype=torch.float64)),
               dict(targets_out=torch.empty(4, 11)), dict(targets_out=torch.empty(4, 10, dtype=torch.float16)),
               dict(out=torch.empty(4, 3, 8, 16)[..., ::2])):
        with pytest.raises(ValueError, match="out"):
            mixer(xf, y, **kw)
    out, t_out = torch.full((4, 3, 8, 8), 9.), torch.full((4, 10), 9.)
    keep = xf.clone()
    got = mixer(xf + 1, y, out=out, targets_out=t_out)
    assert got[0] is out and got[1] is t_out and not bool((out == 9.).any()) and not bool((t_out == 9.).any())
    assert torch.equal(xf, keep)


# ---- the engine, on the emulation ------------------------------------------------------------------------------------------------------
class Crit(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, t):
        loss = O.soft_target_ce(x, t)
        self.seen.append(float(loss.detach()))
        return loss


class Quiet:
    info = staticmethod(lambda s: None)


def micro():
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0,
                            drop_block_rate=None, **kw)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 100)
    m.load_state_dict(sd)
    m.set_compute_dtype(torch.float32)
    m.train()
    m.set_epoch(31)
    m.load_state_dict(sd)
    return m


def label_batches(n):
    out = []
    for it in range(n):
        x, _, _, y = recipe.inputs(500 + it, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
        out.append((x, y))
    return out


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_eager_epoch_with_mixup_equals_timms_statements_on_the_same_seed(monkeypatch, mode):
    emu_kernels.install(monkeypatch)
    calls = mixup_ref.install(monkeypatch)
    runs = []
    for use_ref in (False, True):
        m = micro()
        opt = torch.optim.AdamW(engine.param_groups_weight_decay(m, 0.05), lr=1e-3)
        mixer = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=recipe.MICRO_CLASSES)
        crit = Crit()
        torch.manual_seed(77)
        np.random.seed(2)
        stats = engine.train_one_epoch(m, crit, label_batches(3), opt, "cpu", 31, None, max_norm=None, print_freq=0,
                                       arch_sample="multi", logger=Quiet, mixup_fn=mixup_ref.RefMixup(mixer) if use_ref else mixer)
        runs.append((stats, crit.seen, m.state_dict(), np.random.get_state()))
    assert len(calls) == 3                                        # the class went through vitres.kernels.mixup, the reference not
    kinds = {bool(c["params"]["cutmix"].any()) for c in calls}
    assert mode != "batch" or kinds == {True, False}              # the seed mixes both ways within the epoch
    (sa, la, pa, ga), (sb, lb, pb, gb) = runs
    assert len(la) == 3 and la == lb and sa == sb
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    assert same_state(ga, gb)


def test_uint8_batches_still_need_a_normalising_mix():
    m = micro()
    u8 = torch.zeros(2, 3, recipe.MICRO_IMG, recipe.MICRO_IMG, dtype=torch.uint8)
    loader = [(u8, torch.zeros(2, dtype=torch.int64))]
    crit = torch.nn.CrossEntropyLoss()
    for mix in (lambda x, t: (x, t), Mixup(num_classes=recipe.MICRO_CLASSES)):
        with pytest.raises(TypeError, match="DevicePrefetchLoader.*SwitchTokenMix.*Mixup.*input_norm="):
            engine.train_one_epoch(m, crit, loader, None, "cpu", 0, mixup_fn=mix, print_freq=0)
    # a normalising Mixup passes the guard: the batch reaches the mix (which, on CPU tensors, has no kernel to run)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        engine.train_one_epoch(m, crit, loader, None, "cpu", 0, print_freq=0,
                               mixup_fn=Mixup(num_classes=recipe.MICRO_CLASSES, input_norm=(MEAN, STD)))
