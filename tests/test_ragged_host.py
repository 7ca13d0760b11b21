"""CPU checks of the ragged route (vr_ragged_plane, vr_jpeg_reconstruct_ragged_u8, vr_resample_ragged_u8): the numpy emulation
tests/emu_ragged.py against PIL's committed outputs (tests/golden/f23_ragged_pil.npz, always) and against PIL itself (where it is
importable); ragged_collate_u8's layout; the host checks of plane and box tables field by field; the ABI and the workspace rule;
the loader chains on the emulated entries against the padded chains; and the refusal of the padded plan that made the route
necessary."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import emu_jpeg as EJ
import emu_ragged as E
import emu_resample as ER
from vitres import _lib, data
from vitres import kernels as K
from vitres.resized_crop import RandomResizedCrop, ResizeCenterCrop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["wide_bicubic", "wide_bilinear", "tall", "both", "mixed", "mixed_bilinear", "eval_window", "graph_a", "graph_b"]
F20 = np.load(os.path.join(ROOT, "tests", "golden", "f20_resample_pil.npz"))
F22 = np.load(os.path.join(ROOT, "tests", "golden", "f22_jpeg_pil.npz"))


def layout(images, seed=0):
    """the tests' layout of a case: different extra pitches, gaps between samples, everything that is no pixel filled with 255"""
    rs = np.random.RandomState(seed)
    return E.pack(images, extra_pitch=[4 * int(rs.randint(0, 4)) for _ in images], gap=40, fill=255, lead=32)


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_emulation_equals_the_committed_pil_outputs(name):
    images, boxes, (So_h, So_w), filt, pil = E.golden_case(name)
    flat, planes = layout(images)
    got = E.resample_ragged_u8(flat, planes, boxes, images[0].shape[0], So_h, So_w, filt)
    assert np.array_equal(got, pil), "differs from PIL in %d bytes" % int((got != pil).sum())
    # no byte that is not a pixel reaches an output: the same planes with another fill give the same bytes
    flat0, _ = E.pack(images, extra_pitch=[int(p["pitch"]) - (img.shape[2] + 3) // 4 * 4 for p, img in zip(planes, images)], gap=40,
                      fill=0, lead=32)
    assert np.array_equal(E.resample_ragged_u8(flat0, planes, boxes, images[0].shape[0], So_h, So_w, filt), pil)


def test_the_fixture_holds_the_shapes_it_is_for():
    shapes = {n: [im.shape for im in E.golden_case(n)[0]] for n in CASES}
    assert shapes["wide_bicubic"] == [(1, 16, 8192)] and shapes["tall"] == [(1, 8192, 16)]
    assert shapes["mixed"] == [(3, 5, 7), (3, 40, 1800), (3, 1500, 12), (3, 64, 64)]
    images, boxes, size, filt, _ = E.golden_case("both")
    assert size == (8, 8) and images[0].shape == (3, 301, 1999) and [1, 1] in boxes[:, 2:4].tolist()
    assert (boxes[0, :4] == [0, 0, 1999, 301]).all()
    _, boxes, _, _, _ = E.golden_case("mixed")
    assert set(boxes[:, 8].tolist()) == {0, 1}
    # the evaluation transform's own box of a 96 x 2048 image
    images, boxes, size, filt, _ = E.golden_case("eval_window")
    tf = ResizeCenterCrop(32)
    assert np.asarray(tf.draw(np.array([[96, 2048]])))[:, :9].tolist() == [boxes[0].tolist()] and size == (32, 32) and K.RESAMPLE_FILTERS[tf.filter] == filt
    assert boxes[0, 4] == 768 and 0 < boxes[0, 6] < 768 - 32
    streams, pixels, _, _, _, _ = E.golden_jpeg_big()
    assert [p.shape for p in pixels] == [(48, 4100, 3), (33, 70, 3), (20, 37, 3), (25, 31, 3)]
    assert os.path.getsize(E.GOLDEN) < 512 * 1024


def test_committed_outputs_are_what_pil_gives_today():
    pytest.importorskip("PIL")
    for name in ("mixed", "eval_window", "tall"):
        images, boxes, (So_h, So_w), filt, pil = E.golden_case(name)
        for b, img in enumerate(images):
            assert np.array_equal(ER.pil_resample_u8(img[None], boxes[b:b + 1], So_h, So_w, filt)[0], pil[b])


def test_emulation_equals_pil_on_random_draws():
    pytest.importorskip("PIL")
    rng = random.Random(11)
    for i in range(6):
        B, C = rng.randint(1, 3), rng.choice((1, 3))
        rs = np.random.RandomState(100 + i)
        images = []
        for _ in range(B):
            h, w = rng.choice(((rng.randint(1, 40), rng.randint(500, 3000)), (rng.randint(500, 3000), rng.randint(1, 40)),
                               (rng.randint(3, 90), rng.randint(3, 90))))
            images.append(rs.randint(0, 256, (C, h, w)).astype(np.uint8))
        So_h, So_w = rng.choice(((8, 8), (16, 12), (4, 20)))
        filt = rng.choice((2, 3))
        boxes = []
        for img in images:
            _, h, w = img.shape
            bw, bh = rng.randint(1, w), rng.randint(1, h)
            ow, oh = So_w + rng.randint(0, 5), So_h + rng.randint(0, 5)
            boxes.append((rng.randint(0, w - bw), rng.randint(0, h - bh), bw, bh, ow, oh, rng.randint(0, ow - So_w),
                          rng.randint(0, oh - So_h), rng.randint(0, 1)))
        flat, planes = layout(images, seed=i)
        got = E.resample_ragged_u8(flat, planes, boxes, C, So_h, So_w, filt)
        for b, img in enumerate(images):
            assert np.array_equal(got[b], ER.pil_resample_u8(img[None], [boxes[b]], So_h, So_w, filt)[0]), (i, b, boxes[b])


def test_emulation_follows_pils_pass_order_at_its_threshold():
    """PIL resizes an image more than 100 times as tall as wide vertically first: 1200 x 12 goes horizontal first, 1201 x 12 not"""
    pytest.importorskip("PIL")
    img = np.random.RandomState(5).randint(0, 256, (1, 1310, 16)).astype(np.uint8)
    flat, planes = layout([img])
    for h in (1200, 1201, 1300):
        for box in ((2, 7, 12, h, 16, 16, 0, 0, 1), (2, 7, 12, h, 20, 24, 3, 5, 0)):
            got = E.resample_ragged_u8(flat, planes, [box], 1, 16, 16, 3)
            assert np.array_equal(got, ER.pil_resample_u8(img[None], [box], 16, 16, 3)), box
    box = (2, 7, 12, 1201, 16, 16, 0, 0, 0)
    assert not np.array_equal(E.resample_plane(img[0], box, 16, 16, 3), ER.resample_plane(img[0], box, 16, 16, 3))


@pytest.mark.parametrize("name", ["down_bicubic", "thin", "edges", "flip", "window", "b3_c3", "bands"])
def test_repacked_padded_cases_equal_their_committed_outputs(name):
    src, boxes, (So_h, So_w, filt) = F20[name + ".src"], F20[name + ".boxes"], (int(v) for v in F20[name + ".meta"])
    flat, planes = E.repack_padded(src)
    assert np.array_equal(E.resample_ragged_u8(flat, planes, boxes, src.shape[1], So_h, So_w, filt), F20[name + ".out"])


def _collate_big():
    streams, pixels, boxes, size, filt, crops = E.golden_jpeg_big()
    return data.jpeg_collate([(s, k) for k, s in enumerate(streams)]), pixels, boxes, size, filt, crops


def test_emulated_reconstruct_of_the_big_streams_is_pil_and_keeps_the_gaps():
    (blob, descs, qtabs, sizes, _), pixels, _, _, _, _ = _collate_big()
    assert descs[:, 0].tolist() == [0, 0, 0, 1] and sizes.tolist() == [list(p.shape[:2]) for p in pixels]
    images = [np.ascontiguousarray(p.transpose(2, 0, 1)) for p in pixels]
    want, planes = layout(images)
    poisoned = np.where(E.pixel_mask(planes, [im.shape for im in images], want.size), 0x5A, 255).astype(np.uint8)
    got = E.reconstruct_ragged_u8(blob.numpy(), descs.numpy(), qtabs.numpy(), poisoned, planes)
    inside = np.zeros(want.size, dtype=bool)
    for p in planes:
        inside[int(p["off"]):int(p["off"]) + 3 * int(p["rows"]) * int(p["pitch"])] = True
    pix = E.pixel_mask(planes, [im.shape for im in images], want.size)
    assert np.array_equal(got[pix], want[pix])                            # PIL's pixels
    assert not got[inside & ~pix].any()                                   # pad columns are zero
    assert (got[~inside] == 255).all()                                    # gaps keep their bytes


def test_emulated_reconstruct_of_committed_streams_equals_their_canvases():
    records = [r for r in EJ.golden_records(F22) if r[1] == 0][::16]
    blob, descs, qtabs, sizes, _ = data.jpeg_collate([(r[2], k) for k, r in enumerate(records)])
    planes, nbytes = K.ragged_layout(sizes.numpy(), 3)
    got = E.reconstruct_ragged_u8(blob.numpy(), descs.numpy(), qtabs.numpy(), np.zeros(nbytes, dtype=np.uint8), planes)
    for r, p in zip(records, planes):
        h, w = r[3].shape[:2]
        assert np.array_equal(E.view(got, p, 3)[:, :h, :w], r[3].transpose(2, 0, 1)), r[0]


# ---- collation and the host side of the wrappers -------------------------------------------------------------------------------------------
def test_ragged_collate_u8_layout_and_padding():
    rs = np.random.RandomState(0)
    imgs = [rs.randint(1, 256, (h, w, 3)).astype(np.uint8) for h, w in ((5, 7), (9, 6), (1, 1), (8, 8))]
    flat, planes, sizes, labels = data.ragged_collate_u8([(img, k + 3) for k, img in enumerate(imgs)])
    assert flat.dtype == torch.uint8 and flat.dim() == 1 and planes.dtype == torch.int32 and tuple(planes.shape) == (4, 8)
    assert sizes.dtype == torch.int32 and sizes.tolist() == [[5, 7], [9, 6], [1, 1], [8, 8]]
    assert labels.dtype == torch.int64 and labels.tolist() == [3, 4, 5, 6]
    rec = planes.numpy().view(K.RAGGED_PLANE_DTYPE).reshape(-1)
    assert rec["pitch"].tolist() == [8, 8, 4, 8] and rec["rows"].tolist() == [5, 9, 1, 8]
    assert rec["off"].tolist() == [0, 128, 352, 368] and flat.numel() == 368 + 192 and not (rec["off"] % 16).any()
    pix = E.pixel_mask(rec, [(3,) + img.shape[:2] for img in imgs], flat.numel())
    assert not flat.numpy()[~pix].any() and pix.sum() == sum(img.size for img in imgs)
    for img, p in zip(imgs, rec):
        assert np.array_equal(E.view(flat.numpy(), p, 3)[:, :, :img.shape[1]], img.transpose(2, 0, 1))
    assert np.array_equal(K.check_ragged_planes(rec, 3, flat.numel(), sizes.numpy()), planes.numpy())
    assert rec["reserved"].tolist() == [[3, 0]] * 4                       # the collate's note of the channel count
    # the emulation's own layout rule gives the same table
    mine = E.pack([img.transpose(2, 0, 1) for img in imgs])[1]
    assert all(np.array_equal(mine[k], rec[k]) for k in ("off", "pitch", "rows", "ws_off"))
    with pytest.raises(TypeError):
        data.ragged_collate_u8([(imgs[0].astype(np.float32), 0)])
    with pytest.raises(ValueError):
        data.ragged_collate_u8([])
    # one channel
    flat1, planes1, _, _ = data.ragged_collate_u8([(imgs[0][:, :, :1], 0)])
    assert flat1.numel() == 48 and planes1.tolist() == [[0, 0, 8, 5, 0, 0, 1, 0]]


@pytest.mark.parametrize("field,value", [("off", -16), ("off", 8), ("off", 1 << 40), ("pitch", 0), ("pitch", 6), ("pitch", 8196),
                                         ("pitch", 4), ("rows", 0), ("rows", 8193), ("rows", 8), ("rows", 10)])
def test_check_ragged_planes_rejects(field, value):
    sizes = np.array([[5, 7], [9, 6], [8, 8]])
    planes, nbytes = K.ragged_layout(sizes, 3)
    assert K.check_ragged_planes(planes, 3, nbytes, sizes).shape == (3, 8)
    bad = planes.copy()
    bad[field][1] = value                                                 # (rows 8 < the image's 9; rows 10 runs into sample 2)
    with pytest.raises(RuntimeError, match="VR_EINVAL.*sample"):
        K.check_ragged_planes(bad, 3, nbytes, sizes)
    # what the device can see of it, it refuses too; a plane too small for its image or overlapping another only the host can know
    host_only = (field, value) in (("pitch", 4), ("rows", 8), ("rows", 10))
    assert E.plane_ok(bad[1], 3, nbytes, 8192, 8192) == host_only


def test_check_ragged_planes_shapes_and_ends():
    sizes = np.array([[5, 7], [9, 6]])
    planes, nbytes = K.ragged_layout(sizes, 3)
    as_ints = planes.view(np.int32).reshape(2, 8)
    assert np.array_equal(K.check_ragged_planes(as_ints, 3, nbytes), as_ints)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                              # the last plane runs past the declared size
        K.check_ragged_planes(planes, 3, nbytes - 16)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                              # four channels need more than three do
        K.check_ragged_planes(planes, 4, nbytes)
    with pytest.raises(ValueError):
        K.check_ragged_planes(as_ints[:, :7], 3, nbytes)
    with pytest.raises(ValueError):
        K.check_ragged_planes(planes, 3, nbytes, sizes[:1])
    with pytest.raises(ValueError):
        K.ragged_layout(np.array([[0, 4]]))


def test_box_check_is_against_the_samples_own_plane():
    planes, _ = K.ragged_layout(np.array([[12, 16], [40, 8]]), 3)
    ok = [(0, 0, 16, 12, 8, 8, 0, 0, 1), (1, 2, 7, 38, 12, 9, 4, 1, 0)]
    table = K.check_ragged_boxes(ok, planes, 8)
    assert table.dtype == np.int32 and table.shape == (2, 12) and table[:, :9].tolist() == [list(r) for r in ok]
    K.check_ragged_boxes([ok[0], (0, 0, 8, 40, 8, 8, 0, 0, 0)], planes, 8)                 # 40 rows: fine for sample 1 ...
    with pytest.raises(RuntimeError, match="VR_EINVAL.*sample 0"):                         # ... and outside sample 0's 12
        K.check_ragged_boxes([(0, 0, 8, 40, 8, 8, 0, 0, 0), ok[1]], planes, 8)
    for bad in ((0, 0, 9, 12, 8, 8, 0, 0, 0), (2, 0, 7, 4, 8, 8, 0, 0, 0), (0, 37, 4, 4, 8, 8, 0, 0, 0), (-1, 0, 4, 4, 8, 8, 0, 0, 0),
                (0, 0, 0, 4, 8, 8, 0, 0, 0), (0, 0, 4, 4, 7, 8, 0, 0, 0), (0, 0, 4, 4, 12, 9, 5, 0, 0), (0, 0, 4, 4, 12, 9, 0, 2, 0)):
        with pytest.raises(RuntimeError, match="VR_EINVAL.*sample 1"):
            K.check_ragged_boxes([ok[0], bad], planes, 8)
    with pytest.raises(ValueError):
        K.check_ragged_boxes(ok[:1], planes, 8)


def test_abi_struct_symbols_and_workspace_rule():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    assert re.search(r"int64_t off;.*\n\s*int32_t pitch;.*\n\s*int32_t rows;.*\n\s*int64_t ws_off;.*\n\s*int32_t reserved\[2\];\s*}\s*"
                     r"vr_ragged_plane;", hdr)
    assert ctypes.sizeof(_lib.RaggedPlane) == 32 == K.RAGGED_PLANE_DTYPE.itemsize == E.PLANE.itemsize and K.RAGGED_PLANE_INTS == 8
    assert [n for n, _ in _lib.RaggedPlane._fields_] == list(K.RAGGED_PLANE_DTYPE.names) == list(E.PLANE.names)
    assert [K.RAGGED_PLANE_DTYPE.fields[n][1] for n in K.RAGGED_PLANE_DTYPE.names] == [0, 8, 12, 16, 24]
    assert "static_assert(sizeof(vr_ragged_plane) == 32" in open(os.path.join(ROOT, "vit-search_amd", "csrc", "ragged.h")).read()
    lib = _lib.lib()
    for name in ("vr_jpeg_reconstruct_ragged_u8", "vr_resample_ragged_u8", "vr_resample_ragged_ws_bytes"):
        assert hasattr(lib, name)
    # the workspace follows the SUM of the heights: 127 images of 375 rows and one of 2848, not 128 x 2848
    rows = 127 * 375 + 2848
    assert lib.vr_resample_ragged_ws_bytes(3, rows, 224) == 3 * rows * 224 == K.resample_ragged_ws_bytes(3, rows, 224)
    assert lib.vr_resample_ragged_ws_bytes(1, 1, 4) == 16 and lib.vr_resample_ragged_ws_bytes(3, 0, 224) == 0
    planes, _ = K.ragged_layout(np.array([[5, 7], [9, 6], [8, 8]]), 3)
    assert K.ragged_ws_offsets(planes, 3, 16, [5, 2, 8]) == 3 * 15 * 16 and planes["ws_off"].tolist() == [0, 240, 336]
    assert K.ragged_ws_offsets(planes, 3, 16) == 3 * 22 * 16 + 0 and planes["ws_off"].tolist() == [0, 240, 672]
    assert K.ragged_bounds(planes) == (9, 8)
    with pytest.raises(RuntimeError):                                                # no CPU path
        K.resample_ragged_u8(torch.zeros(1024, dtype=torch.uint8), planes[:1], [(0, 0, 7, 5, 8, 8, 0, 0, 0)], 3, 8, 3)


def test_the_padded_plan_still_refuses_the_wide_case():
    """16 x 8192 -> 16: the launch vr_resample_u8 refuses and the ragged entry exists for (the plan alone: no device needed)."""
    assert _lib.lib().vr_resample_band_rows(1, 16, 8192, 16, 16, 3) == -3
    assert _lib.lib().vr_resample_band_rows(1, 16, 8192, 16, 16, 2) == -3
    assert _lib.lib().vr_resample_band_rows(3, 48, 4100, 16, 16, 3) == -3                  # jpeg_big's canvas


# ---- the loader chains on the emulated entries -------------------------------------------------------------------------------------------
def _transform(kind, S):
    if kind == "train":
        return RandomResizedCrop(S, rng=random.Random(5), generator=torch.Generator().manual_seed(6))
    return ResizeCenterCrop(S, crop_pct=0.8, interpolation="bilinear")


@pytest.mark.parametrize("kind", ["train", "eval"])
def test_ragged_collate_chain_equals_the_padded_chain_on_the_emulated_entries(kind, monkeypatch):
    E.install(monkeypatch)
    rs = np.random.RandomState(3)
    batches = [[(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), i % 5) for i, (h, w) in enumerate(sizes)]
               for sizes in ([(21, 30), (33, 18), (17, 17)], [(40, 25), (19, 44), (16, 23)])]
    padded = [data.pad_collate_u8(b) for b in batches]
    ragged = [data.ragged_collate_u8(b) for b in batches]
    want = list(data.DeviceCropLoader(padded, _transform(kind, 16), "cpu"))
    got = list(data.DeviceCropLoader(ragged, _transform(kind, 16), "cpu"))
    assert len(got) == len(want) == 2
    for (x, y), (wx, wy) in zip(got, want):
        assert x.dtype == torch.uint8 and tuple(x.shape) == (3, 3, 16, 16) and torch.equal(x, wx) and torch.equal(y, wy)


@pytest.mark.parametrize("kind", ["train", "eval"])
def test_ragged_jpeg_chain_equals_the_padded_chain_on_the_emulated_entries(kind, monkeypatch):
    E.install(monkeypatch)
    names = ["37x53.420.q85", "48x40.444.q30r2", "31x64.422.q95rr", "17x23.gray.q100opt", "fallback.png", "9x17.420.q30r2"]
    records = [next(r for r in EJ.golden_records(F22) if r[0] == n) for n in names]
    files = [(r[2], k % 5) for k, r in enumerate(records)]
    collated = [data.jpeg_collate(files[:3]), data.jpeg_collate(files[3:])]
    want = list(data.DeviceCropLoader(data.DeviceJpegLoader(collated, "cpu"), _transform(kind, 16), "cpu"))
    jl = data.DeviceJpegLoader(collated, "cpu", ragged=True)
    first = next(iter(jl))
    assert isinstance(first[0], data.RaggedCanvas) and first[0].channels == 3 and first[1].tolist() == [[37, 53], [48, 40], [31, 64]]
    assert np.array_equal(first[0].plane(0, (37, 53)).numpy(), records[0][3].transpose(2, 0, 1))
    got = list(data.DeviceCropLoader(data.DeviceJpegLoader(collated, "cpu", ragged=True), _transform(kind, 16), "cpu"))
    assert len(got) == len(want) == 2
    for (x, y), (wx, wy) in zip(got, want):
        assert tuple(x.shape) == (3, 3, 16, 16) and torch.equal(x, wx) and torch.equal(y, wy)


def test_big_images_go_through_the_ragged_chain_where_the_padded_chain_is_refused(monkeypatch):
    E.install(monkeypatch)
    collated, pixels, boxes, size, filt, crops = _collate_big()

    S = size[0]

    class Fixed:                                                          # the fixture's boxes in a transform's place
        size, filter = S, "bicubic"

        def draw(self, sizes):
            assert np.asarray(sizes).tolist() == [list(p.shape[:2]) for p in pixels]
            return boxes
    assert filt == 3
    (x, y), = data.DeviceCropLoader(data.DeviceJpegLoader([collated], "cpu", ragged=True), Fixed(), "cpu")
    assert np.array_equal(x.numpy(), crops) and y.tolist() == [0, 1, 2, 3]
    (x, y), = data.DeviceCropLoader([data.ragged_collate_u8([(p, k) for k, p in enumerate(pixels)])], Fixed(), "cpu")
    assert np.array_equal(x.numpy(), crops)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        list(data.DeviceCropLoader(data.DeviceJpegLoader([collated], "cpu"), Fixed(), "cpu"))
