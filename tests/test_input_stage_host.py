"""The uint8 input side without a GPU: the two entry points' declarations and argument validation (which returns before any
launch), the normalisation constants, SwitchTokenMix's dtype rules, and DevicePrefetchLoader / ResidentU8Batches with the
normaliser replaced by tests/emu_input.py; the look-ahead contract for every loader of vitres.data that has it (the crop and JPEG
loaders on the emulated entries of tests/emu_ragged.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import emu_input
import emu_jpeg
import emu_ragged
from vitres import _lib, data, engine, kernels as K
from vitres.resized_crop import ResizeCenterCrop
from vitres.token_mixup import SwitchTokenMix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P = 0x10000                                                       # a fake, 16-byte aligned device address: nothing is launched


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    declared = set(re.findall(r"^int\s+(vr_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.lib()
    for name in ("vr_normalize_u8", "vr_token_mix_u8"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.vr_version() >= 1002


def _norm(inp=P, out=P * 2, B=2, C=3, H=8, W=16, mean=True, std=True):
    m, s = K.norm_constants(MEAN + (0.5,), STD + (0.25,))
    return _lib.lib().vr_normalize_u8(inp, out, B, C, H, W, m if mean else None, s if std else None, None)


def test_normalize_u8_validates_before_any_launch():
    assert _norm(inp=None) == EINVAL and _norm(out=None) == EINVAL and _norm(mean=False) == EINVAL and _norm(std=False) == EINVAL
    assert _norm(B=0) == EINVAL and _norm(H=-1) == EINVAL
    assert _norm(W=18) == EUNSUPPORTED and _norm(W=6) == EUNSUPPORTED
    assert _norm(C=5) == EUNSUPPORTED
    assert _norm(out=P * 2 + 4) == EALIGN and _norm(out=P * 2 + 8) == EALIGN
    assert _norm(inp=P + 1) == EALIGN
    assert _norm(C=5, out=P * 2 + 4) == EUNSUPPORTED              # the existing order: EINVAL, EUNSUPPORTED, EALIGN
    assert _norm(B=0, W=18) == EINVAL


def _mix(samples=P, out=P * 2, labels=P * 3, partner=P * 4, targets=P * 5, patch_targets=P * 6, B=4, C=3, H=8, W=16, K_=10, pl=4,
         half=2, mean=True):
    m, s = K.norm_constants(MEAN + (0.5,), STD + (0.25,))
    return _lib.lib().vr_token_mix_u8(samples, out, labels, partner, targets, patch_targets, B, C, H, W, K_, pl, half, 0, 1, 0, 1,
                                      0.5, 0.5, 0.5, 0.5, 0.9, 0.01, m if mean else None, s, None)


def test_token_mix_u8_validates_before_any_launch():
    for name in ("samples", "out", "labels", "partner", "targets", "patch_targets"):
        assert _mix(**{name: None}) == EINVAL, name
    assert _mix(mean=False) == EINVAL
    assert _mix(half=5) == EINVAL and _mix(half=-1) == EINVAL and _mix(K_=0) == EINVAL
    assert _mix(W=18) == EUNSUPPORTED                             # W % 4
    assert _mix(C=5) == EUNSUPPORTED
    assert _mix(H=6) == EUNSUPPORTED                              # H % patch_len
    assert _mix(out=P * 2 + 4) == EALIGN
    assert _mix(samples=P + 2) == EALIGN
    assert _mix(half=5, C=5, out=P * 2 + 4) == EINVAL and _mix(C=5, out=P * 2 + 4) == EUNSUPPORTED


def test_input_norm_constants_are_timms():
    """x * 255 in Python doubles, then rounded to fp32: torch.tensor([x * 255 for x in mean])."""
    m, s = K.norm_constants(MEAN, STD)
    assert isinstance(m, ctypes.Array) and len(m) == len(s) == 3
    for got, x in zip(list(m) + list(s), MEAN + STD):
        assert np.float32(got) == np.float32(x * 255) and got == float(torch.tensor([x * 255])[0])
    mix = SwitchTokenMix(4, num_classes=10, input_norm=(MEAN, STD))
    assert [np.float32(v) for v in mix.input_norm[0]] == [np.float32(x * 255) for x in MEAN]
    assert [np.float32(v) for v in mix.input_norm[1]] == [np.float32(x * 255) for x in STD]
    assert mix.normalizes and not SwitchTokenMix(4).normalizes
    assert K.IMAGENET_DEFAULT_MEAN == MEAN and K.IMAGENET_DEFAULT_STD == STD
    with pytest.raises(ValueError):
        K.norm_constants((0.5,) * 5, (0.5,) * 5)
    with pytest.raises(ValueError):
        K.norm_constants(MEAN, STD[:2])


def test_switch_token_mix_dtype_rules():
    u8 = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    y = torch.zeros(4, dtype=torch.int64)
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="input_norm"):
        SwitchTokenMix(4, num_classes=10)(u8, y)                  # uint8 without a normaliser
    with pytest.raises(ValueError, match="twice"):
        SwitchTokenMix(4, num_classes=10, input_norm=(MEAN, STD))(u8.float(), y)
    assert torch.equal(torch.random.get_rng_state(), state)       # refused before anything was drawn
    with pytest.raises(RuntimeError, match="GPU"):                # fp32 without input_norm: as before (CPU tensors have no path)
        SwitchTokenMix(4, num_classes=10)(u8.float(), y)
    with pytest.raises(RuntimeError, match="GPU"):
        SwitchTokenMix(4, num_classes=10, input_norm=(MEAN, STD))(u8, y)


def test_uint8_reaching_a_model_or_the_loop_raises_type_error():
    import recipe
    import vitres
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0],
                            num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    u8 = torch.zeros(2, 3, recipe.MICRO_IMG, recipe.MICRO_IMG, dtype=torch.uint8)
    from vitres.nets import vit_sr_supernet
    old = vit_sr_supernet._REQUIRE_CUDA
    vit_sr_supernet._REQUIRE_CUDA = False
    try:
        m.eval()
        with pytest.raises(TypeError, match="DevicePrefetchLoader"):
            m(u8)
        m.train()
        with pytest.raises(TypeError, match="input_norm="):
            m.loss_and_grad(u8, torch.zeros(2, recipe.MICRO_CLASSES))
    finally:
        vit_sr_supernet._REQUIRE_CUDA = old
    crit = torch.nn.CrossEntropyLoss()
    loader = [(u8, torch.zeros(2, dtype=torch.int64))]
    for mix in (None, lambda x, t: (x, t, None, "seq"), SwitchTokenMix(1, num_classes=recipe.MICRO_CLASSES)):
        with pytest.raises(TypeError, match="DevicePrefetchLoader.*input_norm="):
            engine.train_one_epoch(m, crit, loader, None, "cpu", 0, patch_mixup_fn=mix, print_freq=0)


class Loader(list):
    sampler, dataset = "the sampler", "the dataset"


def u8_set(n, seed=0, shape=(3, 4, 8)):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n,) + shape, dtype=torch.uint8, generator=g), torch.arange(n)


def look_ahead_cases():
    """[(name, three host batches of two images under 64 pixels a side, loader -> the look-ahead loader over it)]: every loader of
    vitres.data that copies one batch ahead, the crop loader on padded and on ragged input, the JPEG loader padded and ragged."""
    x, y = u8_set(6)
    rs = np.random.RandomState(1)
    decoded = [[(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), k) for k, (h, w) in enumerate(sizes)]
               for sizes in ([(21, 30), (33, 18)], [(40, 25), (19, 44)], [(17, 17), (16, 23)])]
    names = ["37x53.420.q85", "48x40.444.q30r2", "31x64.422.q95rr", "17x23.gray.q100opt", "fallback.png", "9x17.420.q30r2"]
    records = emu_jpeg.golden_records(np.load(os.path.join(ROOT, "tests", "golden", "f22_jpeg_pil.npz")))
    files = [(next(r for r in records if r[0] == n)[2], k % 5) for k, n in enumerate(names)]
    jpegs = [data.jpeg_collate(files[i:i + 2]) for i in range(0, 6, 2)]

    def crop(loader):
        return data.DeviceCropLoader(loader, ResizeCenterCrop(16, crop_pct=0.8, interpolation="bilinear"), "cpu")
    return [("prefetch", [(x[i:i + 2], y[i:i + 2]) for i in range(0, 6, 2)], lambda l: data.DevicePrefetchLoader(l, "cpu", MEAN, STD)),
            ("crop", [data.pad_collate_u8(b) for b in decoded], crop),
            ("crop, ragged", [data.ragged_collate_u8(b) for b in decoded], crop),
            ("jpeg", jpegs, lambda l: data.DeviceJpegLoader(l, "cpu")),
            ("jpeg, ragged", jpegs, lambda l: data.DeviceJpegLoader(l, "cpu", ragged=True))]


def test_device_prefetch_loader(monkeypatch):
    calls = emu_input.install(monkeypatch)
    emu_ragged.install(monkeypatch)
    for name, batches, wrap in look_ahead_cases():                # __len__, .sampler and .dataset are the wrapped loader's
        over = wrap(Loader(batches))
        assert len(over) == 3 and over.sampler == "the sampler" and over.dataset == "the dataset", name
        assert len(list(over)) == 3 and len(list(over)) == 3, name                 # re-iterable
    del calls[:]
    x, y = u8_set(14)
    loader = Loader((x[i:i + 4], y[i:i + 4]) for i in range(0, 14, 4))           # 4, 4, 4, 2
    pre = data.DevicePrefetchLoader(loader, "cpu", MEAN, STD)
    assert len(pre) == 4 and pre.sampler == "the sampler" and pre.dataset == "the dataset"
    ref = emu_input.normalize_u8_reference(x, MEAN, STD)
    for _ in range(2):                                            # re-iterable
        got = list(pre)
        assert [tuple(b.shape) for b, _ in got] == [(4, 3, 4, 8)] * 3 + [(2, 3, 4, 8)]
        assert torch.equal(torch.cat([b for b, _ in got]), ref) and torch.equal(torch.cat([t for _, t in got]), y)
        assert all(b.dtype == torch.float32 for b, _ in got)
    assert len(calls) == 8
    raw = list(data.DevicePrefetchLoader(loader, "cpu", MEAN, STD, normalize=False))
    assert len(calls) == 8 and all(b.dtype == torch.uint8 for b, _ in raw)
    assert torch.equal(torch.cat([b for b, _ in raw]), x)
    assert list(data.DevicePrefetchLoader(Loader(), "cpu", MEAN, STD)) == []
    with pytest.raises(TypeError, match="uint8"):
        list(data.DevicePrefetchLoader(Loader([(x[:4].float(), y[:4])]), "cpu", MEAN, STD))


def test_prefetch_runs_one_batch_ahead(monkeypatch):
    emu_input.install(monkeypatch)
    emu_ragged.install(monkeypatch)
    for name, batches, wrap in look_ahead_cases():
        taken = []

        def gen():
            for i, batch in enumerate(batches):
                taken.append(i)
                yield batch
        it = iter(wrap(gen()))
        next(it)
        assert taken == [0, 1], name                              # batch 1 was fetched (and its copy issued) before batch 0 was yielded
        next(it)
        assert taken == [0, 1, 2], name
        next(it)
        with pytest.raises(StopIteration):
            next(it)
        assert taken == [0, 1, 2], name


def test_resident_u8_batches(monkeypatch):
    calls = emu_input.install(monkeypatch)
    x, y = u8_set(20, seed=3)
    res = data.ResidentU8Batches(x, y, 8, MEAN, STD)
    assert len(res) == 3 and len(data.ResidentU8Batches(x[:16], y[:16], 8, MEAN, STD)) == 2
    ref = emu_input.normalize_u8_reference(x, MEAN, STD)
    for _ in range(2):                                            # re-iterable, same batches
        seen = []
        for i, (b, t) in enumerate(res):
            assert tuple(b.shape) == ((8, 3, 4, 8) if i < 2 else (4, 3, 4, 8))      # short last batch
            assert torch.equal(b, ref[8 * i:8 * i + b.shape[0]]) and torch.equal(t, y[8 * i:8 * i + b.shape[0]])
            seen.append(b)
        assert len(seen) == 3
    # two alternating buffers, never a fresh one: batch i and i + 2 share storage, i and i + 1 do not
    ptrs = [out.data_ptr() for _, out, _ in calls]
    assert len(ptrs) == 6 and all(out is not None for _, out, _ in calls)
    assert len(set(ptrs)) == 2 and all(ptrs[i] != ptrs[i + 1] and ptrs[i] == ptrs[i + 2] for i in range(4))
    assert {p for p in ptrs} == {b.data_ptr() for b in res._bufs}
    # a batch stays intact while the next one is produced
    it = iter(res)
    b0, _ = next(it)
    keep = b0.clone()
    next(it)
    assert torch.equal(b0, keep)
    with pytest.raises(TypeError):
        data.ResidentU8Batches(x.float(), y, 8, MEAN, STD)
    with pytest.raises(ValueError):
        data.ResidentU8Batches(x, y[:3], 8, MEAN, STD)
    small = data.ResidentU8Batches(x[:3], y[:3], 8, MEAN, STD)    # a set smaller than one batch
    (b, t), = list(small)
    assert tuple(b.shape) == (3, 3, 4, 8) and torch.equal(b, ref[:3])
