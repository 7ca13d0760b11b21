"""CPU checks of the device crop-and-resize stage: the numpy emulation tests/emu_resample.py against PIL itself (where PIL is
importable) and against PIL's committed outputs (always); the box draws of vitres.resized_crop against a hand-restated loop; the
evaluation transform's integer arithmetic; pad_collate_u8; the host-side box check and the ABI's struct and symbols."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import emu_resample as E
from vitres import _lib, data
from vitres import kernels as K
from vitres.resized_crop import RandomResizedCrop, ResizeCenterCrop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f20_resample_pil.npz")


def _random_case(rng, i):
    """(src [1,1,Hs,Ws], box, So_h, So_w, filter): scales from 1/4 to 8, one-pixel boxes, boxes flush with every canvas edge."""
    Hs, Ws = (rng.randint(80, 130), rng.randint(80, 130)) if i % 8 == 0 else (rng.randint(1, 70), rng.randint(1, 70))
    w, h = rng.randint(1, Ws), rng.randint(1, Hs)
    if i % 7 == 0:
        w = 1
    if i % 11 == 0:
        h = 1
    x0, y0 = rng.randint(0, Ws - w), rng.randint(0, Hs - h)
    edge = i % 5
    if edge == 1:
        x0 = 0
    elif edge == 2:
        y0 = 0
    elif edge == 3:
        x0 = Ws - w
    elif edge == 4:
        y0 = Hs - h
    So_h, So_w = rng.choice([4, 8, 16, 20]), rng.choice([4, 8, 16, 24])
    ow, oh = So_w + rng.choice([0, 0, 3, 9]), So_h + rng.choice([0, 0, 5])
    wx, wy = rng.randint(0, ow - So_w), rng.randint(0, oh - So_h)
    src = np.random.RandomState(i).randint(0, 256, (1, 1, Hs, Ws)).astype(np.uint8)
    if i % 3 == 0:
        src = ((src > 127) * 255).astype(np.uint8)             # black / white: the cubic's overshoot reaches both clamps
    return src, [(x0, y0, w, h, ow, oh, wx, wy, i & 1)], So_h, So_w, rng.choice([E.BILINEAR, E.BICUBIC])


def test_emulation_equals_pil_on_random_draws():
    pytest.importorskip("PIL")
    rng = random.Random(1)
    scales = []
    for i in range(300):
        src, box, So_h, So_w, filt = _random_case(rng, i)
        scales.append(box[0][2] / box[0][4])
        assert np.array_equal(E.resample_u8(src, box, So_h, So_w, filt), E.pil_resample_u8(src, box, So_h, So_w, filt)), (i, box, filt)
    assert min(scales) < 0.5 and max(scales) > 3 and sum(1 for s in scales if s > 3) >= 10


def test_emulation_equals_the_committed_pil_outputs():
    g = np.load(GOLDEN)
    names = sorted({k.split(".")[0] for k in g.files})
    assert len(names) == 18
    for name in names:
        So_h, So_w, filt = (int(v) for v in g[name + ".meta"])
        got = E.resample_u8(g[name + ".src"], g[name + ".boxes"], So_h, So_w, filt)
        assert np.array_equal(got, g[name + ".out"]), name


def test_committed_outputs_are_what_pil_gives_today():
    pytest.importorskip("PIL")
    g = np.load(GOLDEN)
    for name in ("down_bicubic", "wide_bilinear", "edges", "bands"):
        So_h, So_w, filt = (int(v) for v in g[name + ".meta"])
        assert np.array_equal(E.pil_resample_u8(g[name + ".src"], g[name + ".boxes"], So_h, So_w, filt), g[name + ".out"]), name


def test_padding_of_the_golden_canvases_never_leaks():
    """The `edges` canvases are 255 outside the 41 x 57 image: a box flush with an image edge gives the same bytes when the padding
    is something else -- the supports are clipped to the crop, not to the canvas."""
    g = np.load(GOLDEN)
    src, boxes = g["edges.src"].copy(), g["edges.boxes"]
    src[:, :, 41:, :] = 0
    src[:, :, :, 57:] = 0
    got = E.resample_u8(src, boxes, 16, 16, 3)
    assert np.array_equal(got[:4], g["edges.out"][:4]) and not np.array_equal(got[4:], g["edges.out"][4:])


# ---- the draws ------------------------------------------------------------------------------------------------------------------------
def _restated_draw(sizes, size, scale, ratio, hflip, rnd, gen):
    """timm 0.3.2 RandomResizedCropAndInterpolation.get_params then torchvision RandomHorizontalFlip, sample by sample."""
    rows, fallbacks = [], 0
    for height, width in sizes:
        area = height * width
        for _ in range(10):
            target_area = rnd.uniform(scale[0], scale[1]) * area
            aspect = math.exp(rnd.uniform(math.log(ratio[0]), math.log(ratio[1])))
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if w <= width and h <= height:
                i = rnd.randint(0, height - h)
                j = rnd.randint(0, width - w)
                break
        else:
            fallbacks += 1
            in_ratio = width / height
            if in_ratio < min(ratio):
                w, h = width, int(round(width / min(ratio)))
            elif in_ratio > max(ratio):
                h, w = height, int(round(height * max(ratio)))
            else:
                w, h = width, height
            i, j = (height - h) // 2, (width - w) // 2
        flip = int(bool(torch.rand(1, generator=gen) < hflip))
        rows.append((j, i, w, h, size, size, 0, 0, flip, 0, 0, 0))
    return np.asarray(rows, dtype=np.int32), fallbacks


@pytest.mark.parametrize("seed,sizes,scale", [
    (0, [(375, 500), (500, 375), (224, 224), (333, 500), (64, 48)] * 4, (0.08, 1.0)),
    (3, [(40, 400), (400, 40), (100, 100), (30, 300)] * 3, (0.9, 1.0)),          # narrow images, large areas: the fallback branch
])
def test_random_resized_crop_draws_follow_timm_and_torchvision(seed, sizes, scale):
    tf = RandomResizedCrop(224, scale=scale, rng=random.Random(seed), generator=torch.Generator().manual_seed(seed))
    got = tf.draw(np.asarray(sizes))
    want, fallbacks = _restated_draw(sizes, 224, scale, (3 / 4, 4 / 3), 0.5, random.Random(seed), torch.Generator().manual_seed(seed))
    assert got.dtype == np.int32 and got.shape == (len(sizes), 12) and np.array_equal(got, want)
    assert (fallbacks > 0) == (seed == 3), fallbacks
    assert 0 < got[:, 8].sum() < len(sizes)                                         # both flip values occur
    for (h, w), row in zip(sizes, got):
        assert row[2] >= 1 and row[3] >= 1 and 0 <= row[0] and row[0] + row[2] <= w and 0 <= row[1] and row[1] + row[3] <= h
    K.check_resample_boxes(got, len(sizes), max(h for h, _ in sizes), max(w for _, w in sizes), 224)


def test_random_resized_crop_uses_the_module_generators_by_default_and_refuses_random_interpolation():
    random.seed(11)
    torch.manual_seed(12)
    a = RandomResizedCrop(32, interpolation="bilinear").draw([(50, 60), (70, 40)])
    random.seed(11)
    torch.manual_seed(12)
    b = RandomResizedCrop(32, interpolation="bilinear").draw(torch.tensor([[50, 60], [70, 40]], dtype=torch.int32))
    assert np.array_equal(a, b) and RandomResizedCrop(32, interpolation="bilinear").filter == 2 and RandomResizedCrop(32).filter == 3
    state = torch.get_rng_state()
    RandomResizedCrop(32, hflip=0).draw([(50, 60)])                                  # no flip transform, no torch draw
    assert torch.equal(state, torch.get_rng_state())
    with pytest.raises(NotImplementedError):
        RandomResizedCrop(32, interpolation="random")
    with pytest.raises(ValueError):
        RandomResizedCrop(32, interpolation="lanczos")


def test_resize_center_crop_arithmetic():
    tf = ResizeCenterCrop()                                                          # 224, crop_pct 224 / 256, bicubic
    assert tf.scale_size == 256 and tf.filter == 3
    got = tf.draw([(375, 500), (500, 375), (224, 224)])                              # (h, w)
    #                x0 y0   w    h   ow   oh  wx  wy flip
    assert got[:, :9].tolist() == [[0, 0, 500, 375, 341, 256, 58, 16, 0],            # int(256 * 500 / 375) = 341; round(58.5) = 58 (even)
                                   [0, 0, 375, 500, 256, 341, 16, 58, 0],
                                   [0, 0, 224, 224, 256, 256, 16, 16, 0]]
    assert tf.resized(256, 300) == (256, 300) and tf.resized(300, 256) == (300, 256)  # short side already there: torchvision returns img
    assert ResizeCenterCrop(224, crop_pct=0.9).scale_size == 248                     # int(248.88...)
    with pytest.raises(ValueError):
        ResizeCenterCrop(224, crop_pct=1.2)


# ---- collation and the host side of the wrapper ---------------------------------------------------------------------------------------
def test_pad_collate_u8_shapes_and_padding():
    rs = np.random.RandomState(0)
    imgs = [rs.randint(1, 256, (h, w, 3)).astype(np.uint8) for h, w in ((5, 7), (9, 6), (8, 8))]
    canvas, sizes, labels = data.pad_collate_u8([(imgs[0], 3), (imgs[1], 0), (imgs[2], 7)])
    assert canvas.dtype == torch.uint8 and tuple(canvas.shape) == (3, 3, 12, 8)      # maxima (9, 8) rounded up to multiples of 4
    assert sizes.dtype == torch.int32 and sizes.tolist() == [[5, 7], [9, 6], [8, 8]]
    assert labels.dtype == torch.int64 and labels.tolist() == [3, 0, 7]
    for b, img in enumerate(imgs):
        h, w = img.shape[:2]
        assert np.array_equal(canvas[b, :, :h, :w].numpy(), img.transpose(2, 0, 1))
        assert not canvas[b, :, h:, :].any() and not canvas[b, :, :, w:].any()
    with pytest.raises(TypeError):
        data.pad_collate_u8([(imgs[0].astype(np.float32), 0)])
    with pytest.raises(ValueError):
        data.pad_collate_u8([])


def test_box_table_check():
    ok = [(0, 0, 16, 12, 8, 8, 0, 0, 1), (3, 2, 13, 10, 12, 9, 4, 1, 0)]
    table = K.check_resample_boxes(ok, 2, 12, 16, 8)
    assert table.dtype == np.int32 and table.shape == (2, 12) and table[:, :9].tolist() == [list(r) for r in ok]
    assert not table[:, 9:].any()
    for bad in ((0, 0, 17, 12, 8, 8, 0, 0, 0), (0, 1, 16, 12, 8, 8, 0, 0, 0), (-1, 0, 4, 4, 8, 8, 0, 0, 0), (0, 0, 0, 4, 8, 8, 0, 0, 0),
                (0, 0, 4, 4, 7, 8, 0, 0, 0), (0, 0, 4, 4, 12, 9, 5, 0, 0), (0, 0, 4, 4, 12, 9, 0, 2, 0), (0, 0, 4, 4, 12, 9, -1, 0, 0)):
        with pytest.raises(RuntimeError, match="VR_EINVAL"):
            K.check_resample_boxes([ok[0], bad], 2, 12, 16, 8)
    with pytest.raises(ValueError):
        K.check_resample_boxes(ok, 3, 12, 16, 8)


def test_abi_struct_symbols_and_band_rule():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    assert re.search(r"int32_t x0, y0, w, h;.*\n\s*int32_t ow, oh;.*\n\s*int32_t wx, wy;.*\n\s*int32_t flip;.*\n\s*int32_t reserved\[3\];\s*}\s*"
                     r"vr_resample_box;", hdr)
    assert ctypes.sizeof(_lib.ResampleBox) == 48
    assert [n for n, _ in _lib.ResampleBox._fields_][:9] == list(K.RESAMPLE_BOX_FIELDS)
    lib = _lib.lib()
    assert lib.vr_version() >= 1006
    assert lib.vr_resample_ws_bytes(128, 224, 224) == 0
    # the band rule needs no device: the tallest band, up to 32 rows, that fits the LDS budget at the launch's worst scale
    assert K.resample_band_rows(3, 256, 320, 224, "bicubic") == 32
    assert K.resample_band_rows(3, 64, 64, (48, 16), 3) == 32
    assert 1 <= K.resample_band_rows(3, 1024, 1024, 224, 3) < 32
    assert K.resample_band_rows(3, 8, 8, 8, 2) == 8                                  # never taller than the output
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.resample_band_rows(1, 16, 8192, 16, 3)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.resample_band_rows(3, 16, 16, (8, 6), 3)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):
        K.resample_band_rows(5, 16, 16, 8, 3)
    with pytest.raises(RuntimeError):                                                # no CPU path
        K.resample_u8(torch.zeros((1, 3, 16, 16), dtype=torch.uint8), [(0, 0, 16, 16, 8, 8, 0, 0, 0)], 8, 3)
