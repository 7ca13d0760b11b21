"""vr_resample_u8 on the GPU: crop + resize (+ window, + mirror) of uint8 canvases, bit for bit against PIL's own outputs committed in
tests/golden/f20_resample_pil.npz (written by tests/golden/make_resample_golden.py; PIL is not needed here) and against the numpy
emulation tests/emu_resample.py -- on the smallest shapes that reach every path: down- and up-scaling, both filters, 25-tap supports,
one-pixel boxes, boxes flush with the image's and the canvas's edges inside a canvas padded with 255, mirrored and plain samples in
one launch, the centre-crop window, several row bands, a refused launch, graph replay with rewritten boxes, and the loader chain."""
import os
import random

import numpy as np
import pytest
import torch

import emu_resample as E
from vitres import data
from vitres import kernels as K
from vitres.resized_crop import RandomResizedCrop, ResizeCenterCrop

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f20_resample_pil.npz")
_CASES = {}

CASES = ["down_bicubic", "down_bilinear", "up_bicubic", "up_bilinear", "wide_bicubic", "wide_bilinear", "thin", "edges",
         "edges_bilinear", "flip", "window", "window_full", "b3_c1", "b3_c3", "bands", "real"]


def case(name):
    """(src, boxes, (So_h, So_w), filter, PIL's output, the emulation's output), loaded / computed once and never written."""
    if name not in _CASES:
        g = np.load(GOLDEN)
        src, boxes, (So_h, So_w, filt) = g[name + ".src"], g[name + ".boxes"], (int(v) for v in g[name + ".meta"])
        _CASES[name] = (src, boxes, (So_h, So_w), filt, g[name + ".out"], E.resample_u8(src, boxes, So_h, So_w, filt))
    return _CASES[name]


def run(src, boxes, size, filt, **kw):
    return K.resample_u8(torch.from_numpy(src).to(DEV), boxes, size, filt, **kw).cpu()


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_pil_and_the_emulation(name):
    src, boxes, size, filt, pil, emu = case(name)
    got = run(src, boxes, size, filt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == pil.shape
    assert torch.equal(got, torch.from_numpy(pil)), "differs from PIL in %d bytes" % int((got.numpy() != pil).sum())
    assert torch.equal(got, torch.from_numpy(emu))


def test_mirrored_and_plain_samples_in_one_launch():
    src, boxes, size, filt, pil, _ = case("flip")
    assert boxes[0, 8] == 0 and boxes[1, 8] == 1 and np.array_equal(boxes[0, :8], boxes[1, :8])
    got = run(src, boxes, size, filt)
    assert torch.equal(got[1], got[0].flip(-1)) and torch.equal(got, torch.from_numpy(pil))


def test_window_is_the_full_resize_cropped():
    """The centre-crop form computes only the window; it must be the bytes of the full resize at that place."""
    src, boxes, size, filt, pil, _ = case("window")
    fsrc, fboxes, fsize, ffilt, _, _ = case("window_full")
    assert np.array_equal(src, fsrc) and filt == ffilt and np.array_equal(boxes[0, :6], fboxes[0, :6])
    wx, wy = int(boxes[0, 6]), int(boxes[0, 7])
    assert wx > 0 and wy > 0
    full = run(fsrc, fboxes, fsize, ffilt)
    win = run(src, boxes, size, filt)
    assert torch.equal(win, full[:, :, wy:wy + size[0], wx:wx + size[1]]) and torch.equal(win, torch.from_numpy(pil))


def test_bands_case_spans_row_bands_with_a_boundary_in_mid_image():
    src, boxes, (So_h, So_w), filt, pil, _ = case("bands")
    band = K.resample_band_rows(src.shape[1], src.shape[2], src.shape[3], (So_h, So_w), filt)
    assert band >= 1 and -(-So_h // band) >= 2, band                               # at least two bands: a boundary inside the image
    assert torch.equal(run(src, boxes, (So_h, So_w), filt), torch.from_numpy(pil))


def test_out_argument_and_three_boxes():
    src, boxes, size, filt, pil, _ = case("b3_c3")
    assert len({tuple(b) for b in boxes.tolist()}) == 3
    out = torch.full(pil.shape, 7, dtype=torch.uint8, device=DEV)
    ret = K.resample_u8(torch.from_numpy(src).to(DEV), boxes, size, filt, out=out)
    assert ret is out and torch.equal(out.cpu(), torch.from_numpy(pil))


def test_a_launch_whose_worst_scale_does_not_fit_is_refused():
    """A 16 x 8192 canvas to 16 x 16: the widest possible support needs 2049 taps per output column -- more LDS than the budget even
    for a one-row band.  The wrapper raises VR_EUNSUPPORTED and writes nothing."""
    src = torch.zeros((1, 1, 16, 8192), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 1, 16, 16), 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.resample_u8(src, [(0, 0, 8192, 16, 16, 16, 0, 0, 0)], 16, "bicubic", out=out)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.resample_band_rows(1, 16, 8192, 16, "bicubic")
    torch.cuda.synchronize()
    assert bool((out == 9).all())


def test_argument_rejections():
    src = torch.zeros((2, 3, 16, 16), dtype=torch.uint8, device=DEV)
    ok = [(0, 0, 16, 16, 8, 8, 0, 0, 0)] * 2
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                           # box outside the canvas
        K.resample_u8(src, [(1, 0, 16, 16, 8, 8, 0, 0, 0)] * 2, 8, 3)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                           # window outside (ow, oh)
        K.resample_u8(src, [(0, 0, 16, 16, 8, 8, 1, 0, 0)] * 2, 8, 3)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                           # w = 0
        K.resample_u8(src, [(0, 0, 0, 16, 8, 8, 0, 0, 0)] * 2, 8, 3)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):                     # So_w % 4
        K.resample_u8(src, [(0, 0, 16, 16, 6, 8, 0, 0, 0)] * 2, (8, 6), 3)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                           # C = 5
        K.resample_u8(torch.zeros((2, 5, 16, 16), dtype=torch.uint8, device=DEV), ok, 8, 3)
    with pytest.raises(RuntimeError, match="VR_EALIGN"):                           # a source one byte past a dword
        K.resample_u8(torch.zeros(2 * 3 * 16 * 16 + 1, dtype=torch.uint8, device=DEV)[1:].view(2, 3, 16, 16), ok, 8, 3)
    with pytest.raises(ValueError):
        K.resample_u8(src, ok, 8, "lanczos")
    with pytest.raises(TypeError):
        K.resample_u8(src.float(), ok, 8, 3)


def test_captured_launch_follows_boxes_rewritten_in_place():
    src, boxes_a, size, filt, pil_a, emu_a = case("graph_a")
    src_b, boxes_b, size_b, filt_b, pil_b, emu_b = case("graph_b")
    assert np.array_equal(src, src_b) and size == size_b and filt == filt_b and not np.array_equal(pil_a, pil_b)
    B, _, Hs, Ws = src.shape
    table = torch.from_numpy(K.check_resample_boxes(boxes_a, B, Hs, Ws, size)).to(DEV)
    next_table = torch.from_numpy(K.check_resample_boxes(boxes_b, B, Hs, Ws, size)).to(DEV)
    dsrc = torch.from_numpy(src).to(DEV)
    out = torch.zeros(pil_a.shape, dtype=torch.uint8, device=DEV)
    K.resample_u8(dsrc, table, size, filt, out=out)                                # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.resample_u8(dsrc, table, size, filt, out=out)
    out.zero_()
    graph.replay()
    assert torch.equal(out.cpu(), torch.from_numpy(pil_a)) and np.array_equal(pil_a, emu_a)
    table.copy_(next_table)
    graph.replay()
    assert torch.equal(out.cpu(), torch.from_numpy(pil_b)) and np.array_equal(pil_b, emu_b)


def _images(seed, sizes):
    rs = np.random.RandomState(seed)
    return [(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), i % 5) for i, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("kind", ["train", "eval"])
def test_crop_loader_into_prefetch_loader_is_the_emulations_crop_normalised(kind):
    """pad_collate_u8 -> DeviceCropLoader -> DevicePrefetchLoader: two batches of images of different sizes; every yielded batch is
    vr_normalize_u8 of the emulation's crop of the same canvases by the same draws."""
    S = 16
    batches = [_images(20, [(21, 30), (33, 18), (17, 17)]), _images(21, [(40, 25), (19, 44), (16, 23)])]
    collated = [data.pad_collate_u8(b) for b in batches]
    if kind == "train":
        make = lambda: RandomResizedCrop(S, rng=random.Random(5), generator=torch.Generator().manual_seed(6))   # noqa: E731
    else:
        make = lambda: ResizeCenterCrop(S, crop_pct=0.8, interpolation="bilinear")                               # noqa: E731
    ref_tf, tf = make(), make()
    loader = data.DevicePrefetchLoader(data.DeviceCropLoader(collated, tf, DEV), DEV)
    seen = 0
    for (x, labels), (canvas, sizes, want_labels) in zip(loader, collated):
        boxes = ref_tf.draw(sizes)
        crop = E.resample_u8(canvas.numpy(), boxes, S, S, tf.filter)
        want = K.normalize_u8(torch.from_numpy(crop).to(DEV), K.IMAGENET_DEFAULT_MEAN, K.IMAGENET_DEFAULT_STD)
        assert x.dtype == torch.float32 and tuple(x.shape) == (3, 3, S, S) and torch.equal(x, want)
        assert torch.equal(labels.cpu(), want_labels)
        seen += 1
    assert seen == 2 and len(loader) == 2
