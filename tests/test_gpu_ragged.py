"""The ragged route on the GPU (vr_jpeg_reconstruct_ragged_u8, vr_resample_ragged_u8 and their loaders): bit for bit against PIL's
own outputs committed in tests/golden/f23_ragged_pil.npz (tests/golden/make_ragged_golden.py; PIL is not needed here) and against
the numpy emulation tests/emu_ragged.py, on the smallest shapes at which each thing can go wrong: 8192-wide and 8192-tall boxes (the
launch the padded entry refuses; coefficient tables that take several sweeps), boxes flush with the image's edges and a one-pixel
box, four shapes and both pass orders in one launch with 255 in every byte that is no pixel, the centre-crop window, encoded files
of which one is 48 x 4100; every case of f20_resample_pil.npz repacked as ragged planes, all streams of f22_jpeg_pil.npz; out= and a
reused workspace, a captured launch pair under rewritten tables, invalid plane records inside an allocation larger than declared,
every return code, and the loader chains against the padded ones."""
import os
import random

import numpy as np
import pytest
import torch

import emu_jpeg as EJ
import emu_ragged as E
from vitres import _lib, data
from vitres import kernels as K
from vitres.rand_augment import RandAugment
from vitres.resized_crop import RandomResizedCrop, ResizeCenterCrop

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5
HERE = os.path.dirname(os.path.abspath(__file__))
F20 = np.load(os.path.join(HERE, "golden", "f20_resample_pil.npz"))
F22 = np.load(os.path.join(HERE, "golden", "f22_jpeg_pil.npz"))
CASES = ["wide_bicubic", "wide_bilinear", "tall", "both", "mixed", "mixed_bilinear", "eval_window", "graph_a", "graph_b"]
F20_CASES = ["down_bicubic", "down_bilinear", "up_bicubic", "up_bilinear", "wide_bicubic", "wide_bilinear", "thin", "edges",
             "edges_bilinear", "flip", "window", "window_full", "b3_c1", "b3_c3", "bands", "graph_a", "graph_b", "real"]
_CASES = {}


def layout(images, seed=0):
    """different extra pitches, gaps between the samples, 255 in every byte that is no pixel"""
    rs = np.random.RandomState(seed)
    return E.pack(images, extra_pitch=[4 * int(rs.randint(0, 4)) for _ in images], gap=40, fill=255, lead=32)


def case(name):
    """(flat, planes, boxes, C, size, filter, PIL's output, the emulation's output), made once and never written"""
    if name not in _CASES:
        images, boxes, size, filt, pil = E.golden_case(name)
        flat, planes = layout(images)
        C = images[0].shape[0]
        _CASES[name] = (flat, planes, boxes, C, size, filt, pil, E.resample_ragged_u8(flat, planes, boxes, C, size[0], size[1], filt))
    return _CASES[name]


def run(flat, planes, boxes, C, size, filt, **kw):
    return K.resample_ragged_u8(torch.from_numpy(flat).to(DEV), planes, boxes, C, size, filt, **kw).cpu()


@pytest.mark.parametrize("name", CASES)
def test_kernels_equal_pil_and_the_emulation(name):
    flat, planes, boxes, C, size, filt, pil, emu = case(name)
    got = run(flat, planes, boxes, C, size, filt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == pil.shape
    assert torch.equal(got, torch.from_numpy(pil)), "differs from PIL in %d bytes" % int((got.numpy() != pil).sum())
    assert torch.equal(got, torch.from_numpy(emu))


def test_the_wide_case_is_the_launch_the_padded_entry_refuses():
    flat, planes, boxes, C, size, filt, pil, _ = case("wide_bicubic")
    canvas = torch.from_numpy(E.view(flat, planes[0], C)[None, :, :, :8192].copy()).to(DEV)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.resample_u8(canvas, boxes, size, filt)
    assert torch.equal(run(flat, planes, boxes, C, size, filt), torch.from_numpy(pil))


def test_mixed_takes_both_pass_orders_and_no_gap_byte_reaches_an_output():
    """sample 2 (1500 x 12, more than 100 times as tall as wide) is the crop PIL resizes vertically first; with 0 instead of 255 in
    every byte that is no pixel the outputs are the same bytes"""
    flat, planes, boxes, C, size, filt, pil, _ = case("mixed")
    h, w = boxes[:, 3], boxes[:, 2]
    assert (h > 100 * w).tolist() == [False, False, True, False] and len({int(p["pitch"]) for p in planes}) == 4
    images = E.golden_case("mixed")[0]
    zeros = flat.copy()
    zeros[~E.pixel_mask(planes, [im.shape for im in images], flat.size)] = 0
    assert (flat != zeros).sum() > 1000
    assert torch.equal(run(zeros, planes, boxes, C, size, filt), torch.from_numpy(pil))
    assert torch.equal(run(flat, planes, boxes, C, size, filt), torch.from_numpy(pil))


@pytest.mark.parametrize("name", F20_CASES)
def test_padded_cases_repacked_as_ragged_planes_equal_their_committed_outputs(name):
    src, boxes, (So_h, So_w, filt) = F20[name + ".src"], F20[name + ".boxes"], (int(v) for v in F20[name + ".meta"])
    flat, planes = E.repack_padded(src)
    got = run(flat, planes, boxes, src.shape[1], (So_h, So_w), filt)
    assert torch.equal(got, torch.from_numpy(F20[name + ".out"]))


def test_out_argument_and_workspace_reuse_across_a_larger_batch():
    small, big = case("graph_a"), case("mixed")
    need = [K.ragged_ws_offsets(E.table(c[1]).copy(), c[3], c[4][1], c[2][:, 3]) for c in (small, big)]
    assert need[1] > need[0]
    ws = torch.full((need[1] + 64,), POISON, dtype=torch.uint8, device=DEV)
    for c in (small, big, small):
        flat, planes, boxes, C, size, filt, pil, _ = c
        out = torch.full(pil.shape, 7, dtype=torch.uint8, device=DEV)
        ret = K.resample_ragged_u8(torch.from_numpy(flat).to(DEV), planes, boxes, C, size, filt, out=out, workspace=ws)
        assert ret is out and torch.equal(out.cpu(), torch.from_numpy(pil))
    assert bool((ws[-64:] == POISON).all())
    with pytest.raises(ValueError, match="workspace"):
        run(*big[:6], workspace=ws[:need[1] - 16])


# ---- reconstruction ------------------------------------------------------------------------------------------------------------------------
def _reconstruct(collated, planes, nbytes, fill=POISON, **kw):
    blob, descs, qtabs = (t.to(DEV) for t in collated[:3])
    dst = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    got = K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, planes, dst=dst, **kw)
    assert got is dst
    return dst.cpu().numpy()


def _check_planes(got, planes, pixels, fill):
    shapes = [(3,) + p.shape[:2] for p in pixels]
    pix = E.pixel_mask(planes, shapes, got.size)
    inside = np.zeros(got.size, dtype=bool)
    for p, img in zip(planes, pixels):
        off, rows, pitch = int(p["off"]), int(p["rows"]), int(p["pitch"])
        inside[off:off + 3 * rows * pitch] = True
        h, w = img.shape[:2]
        assert np.array_equal(E.view(got, p, 3)[:, :h, :w], img.transpose(2, 0, 1))
    assert not got[inside & ~pix].any(), "pad columns are zero"
    assert (got[~inside] == fill).all(), "bytes between the planes keep their values"


def test_all_committed_streams_through_the_ragged_reconstruct_equal_pil():
    records = [r for r in EJ.golden_records(F22) if r[1] == 0]
    assert len(records) == 208
    collated = data.jpeg_collate([(r[2], k) for k, r in enumerate(records)])
    planes, nbytes = K.ragged_layout(collated[3].numpy(), 3)
    got = _reconstruct(collated, planes, nbytes)
    _check_planes(got, planes, [r[3] for r in records], POISON)
    # ... and equal the padded reconstruct's bytes inside every image's plane
    Hs, Ws = ((int(v) + 3) // 4 * 4 for v in collated[3].numpy().max(axis=0))
    canvas = K.jpeg_reconstruct_u8(*(t.to(DEV) for t in collated[:3]), Hs, Ws).cpu().numpy()
    for b, p in enumerate(planes):
        rows, pitch = int(p["rows"]), int(p["pitch"])
        assert np.array_equal(E.view(got, p, 3), canvas[b, :, :rows, :pitch])


def _big():
    streams, pixels, boxes, size, filt, crops = E.golden_jpeg_big()
    return data.jpeg_collate([(s, k) for k, s in enumerate(streams)]), pixels, boxes, size, filt, crops


def test_big_streams_canvases_then_crops_equal_pil_and_the_gaps_survive():
    collated, pixels, boxes, size, filt, crops = _big()
    assert collated[1][:, 0].tolist() == [0, 0, 0, 1]                      # three coefficient records and a raw one
    want, planes = layout([np.ascontiguousarray(p.transpose(2, 0, 1)) for p in pixels])
    got = _reconstruct(collated, planes, want.size, fill=255)
    _check_planes(got, planes, pixels, 255)
    emu = E.reconstruct_ragged_u8(collated[0].numpy(), collated[1].numpy(), collated[2].numpy(), np.full(want.size, 255, np.uint8), planes)
    assert np.array_equal(got, emu)
    out = run(got, planes, boxes, 3, size, filt)
    assert torch.equal(out, torch.from_numpy(crops))
    canvas = K.jpeg_reconstruct_u8(*(t.to(DEV) for t in collated[:3]), 48, 4100)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.resample_u8(canvas, boxes, size, filt)


def test_a_captured_launch_pair_follows_planes_and_boxes_rewritten_in_place():
    collated, pixels, boxes_a, size, filt, crops_a = _big()
    images = [np.ascontiguousarray(p.transpose(2, 0, 1)) for p in pixels]
    _, planes_a = layout(images, seed=1)
    _, planes_b = E.pack(images, extra_pitch=[8, 0, 12, 4], gap=16, fill=0, lead=4096)
    nbytes = max(int((pl["off"] + 3 * pl["rows"].astype(np.int64) * pl["pitch"]).max()) for pl in (planes_a, planes_b))
    boxes_b = boxes_a.copy()
    boxes_b[:, 8] ^= 1
    boxes_b[0, :4] = (1000, 3, 3000, 40)
    bounds = (max(K.ragged_bounds(planes_a)[0], K.ragged_bounds(planes_b)[0]), max(K.ragged_bounds(planes_a)[1],
                                                                                  K.ragged_bounds(planes_b)[1]))
    tables = []
    for planes, boxes in ((planes_a, boxes_a), (planes_b, boxes_b)):
        planes = planes.copy()
        need = K.ragged_ws_offsets(planes, 3, size[1])                       # over the planes' rows: holds for any box
        tables.append((torch.from_numpy(K.check_ragged_planes(planes, 3, nbytes, collated[3].numpy())).to(DEV),
                       torch.from_numpy(K.check_ragged_boxes(boxes, planes, size)).to(DEV), need, planes))
    blob, descs, qtabs = (t.to(DEV) for t in collated[:3])
    dplanes, dboxes = tables[0][0].clone(), tables[0][1].clone()
    dst = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    jws = torch.empty(K.jpeg_ws_bytes(blob.numel()), dtype=torch.uint8, device=DEV)
    rws = torch.empty(max(t[2] for t in tables), dtype=torch.uint8, device=DEV)
    out = torch.zeros(crops_a.shape, dtype=torch.uint8, device=DEV)

    def pair():
        K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, dplanes, dst=dst, workspace=jws, bounds=bounds)
        K.resample_ragged_u8(dst, dplanes, dboxes, 3, size, filt, out=out, workspace=rws, bounds=bounds)
    pair()                                                                # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair()
    out.zero_()
    graph.replay()
    assert torch.equal(out.cpu(), torch.from_numpy(crops_a))
    dplanes.copy_(tables[1][0])
    dboxes.copy_(tables[1][1])
    graph.replay()
    flat_b, _ = E.pack(images, extra_pitch=[8, 0, 12, 4], gap=16, fill=0, lead=4096)
    want_b = E.resample_ragged_u8(flat_b, tables[1][3], boxes_b, 3, size[0], size[1], filt)
    assert not np.array_equal(want_b, crops_a) and torch.equal(out.cpu(), torch.from_numpy(want_b))


def test_a_captured_resample_follows_boxes_rewritten_in_place():
    flat, planes, boxes_a, C, size, filt, pil_a, _ = case("graph_a")
    flat_b, _, boxes_b, _, _, _, pil_b, _ = case("graph_b")
    assert np.array_equal(flat, flat_b) and not np.array_equal(pil_a, pil_b)
    planes = planes.copy()
    need = K.ragged_ws_offsets(planes, C, size[1])
    dplanes = torch.from_numpy(K.check_ragged_planes(planes, C, flat.size)).to(DEV)
    dboxes = torch.from_numpy(K.check_ragged_boxes(boxes_a, planes, size)).to(DEV)
    nxt = torch.from_numpy(K.check_ragged_boxes(boxes_b, planes, size)).to(DEV)
    src, ws = torch.from_numpy(flat).to(DEV), torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.zeros(pil_a.shape, dtype=torch.uint8, device=DEV)
    kw = dict(out=out, workspace=ws, bounds=K.ragged_bounds(planes))
    K.resample_ragged_u8(src, dplanes, dboxes, C, size, filt, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.resample_ragged_u8(src, dplanes, dboxes, C, size, filt, **kw)
    out.zero_()
    graph.replay()
    assert torch.equal(out.cpu(), torch.from_numpy(pil_a))
    dboxes.copy_(nxt)
    graph.replay()
    assert torch.equal(out.cpu(), torch.from_numpy(pil_b))


# ---- invalid plane records: the allocation is larger than the declared size, so nothing can leave it even if a check were wrong -------------
SLACK = 1 << 16


@pytest.mark.parametrize("field,value", [("pitch", "narrow"), ("rows", "short"), ("pitch", "odd"), ("off", "misaligned"),
                                         ("off", "past")])
def test_an_invalid_plane_record_in_the_reconstruct_writes_nothing_for_its_sample(field, value):
    collated, pixels, _, _, _, _ = _big()
    images = [np.ascontiguousarray(p.transpose(2, 0, 1)) for p in pixels]
    want, planes = layout(images)
    declared, victim = want.size, 1                                        # (33 x 70: pitch 72 or more)
    bad = planes.copy()
    h, w = pixels[victim].shape[:2]
    bad[field][victim] = {"narrow": 68, "short": h - 1, "odd": int(planes["pitch"][victim]) + 2,
                          "misaligned": int(planes["off"][victim]) + 4, "past": declared - 64}[value]
    with pytest.raises(RuntimeError, match="VR_EINVAL"):
        K.check_ragged_planes(bad, 3, declared, collated[3].numpy())
    blob, descs, qtabs = (t.to(DEV) for t in collated[:3])
    dst = torch.full((declared + SLACK,), POISON, dtype=torch.uint8, device=DEV)
    table = torch.from_numpy(np.ascontiguousarray(bad).view(np.int32).reshape(4, 8)).to(DEV)   # a device table: the caller's to check
    K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, table, dst=dst, dst_bytes=declared, bounds=(64, 4128))
    got = dst.cpu().numpy()
    assert (got[declared:] == POISON).all(), "the canaries past the declared size"
    good = [b for b in range(4) if b != victim]
    _check_planes(got[:declared], planes[good], [pixels[b] for b in good], POISON)   # neighbours are PIL's; all else keeps the poison
    assert np.array_equal(got, E.reconstruct_ragged_u8(collated[0].numpy(), collated[1].numpy(), collated[2].numpy(),
                                                       np.full(declared + SLACK, POISON, np.uint8), bad, nbytes=declared,
                                                       bounds=(64, 4128)))


@pytest.mark.parametrize("field,value", [("pitch", "odd"), ("off", "misaligned"), ("off", "past"), ("rows", "beyond"),
                                         ("ws_off", "past")])
def test_an_invalid_plane_record_in_the_resample_zeroes_its_sample(field, value):
    flat, planes, boxes, C, size, filt, pil, _ = case("mixed")
    declared, victim = flat.size, 3
    good = planes.copy()
    need = K.ragged_ws_offsets(good, C, size[1], boxes[:, 3])
    bad = good.copy()
    bad[field][victim] = {"odd": int(planes["pitch"][victim]) + 2, "misaligned": int(planes["off"][victim]) + 4,
                          "past": declared - 64 if field == "off" else need, "beyond": 8000}[value]
    if field != "ws_off":
        with pytest.raises(RuntimeError, match="VR_EINVAL"):
            K.check_ragged_planes(bad, C, declared)
    src = torch.full((declared + SLACK,), POISON, dtype=torch.uint8, device=DEV)
    src[:declared] = torch.from_numpy(flat)
    ws = torch.full((need + SLACK,), POISON, dtype=torch.uint8, device=DEV)
    out = torch.full((pil.shape[0] + 1,) + pil.shape[1:], POISON, dtype=torch.uint8, device=DEV)
    table = torch.from_numpy(np.ascontiguousarray(bad).view(np.int32).reshape(4, 8)).to(DEV)
    dboxes = torch.from_numpy(K.check_ragged_boxes(boxes, good, size)).to(DEV)
    L = _lib.lib()
    rc = L.vr_resample_ragged_u8(src.data_ptr(), declared, table.data_ptr(), dboxes.data_ptr(), out.data_ptr(), 4, C, 1500, 1816,
                                 size[0], size[1], filt, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = out.cpu().numpy()
    want = pil.copy()
    want[victim] = 0
    assert np.array_equal(got[:4], want) and (got[4] == POISON).all()
    assert bool((ws[need:] == POISON).all()) and bool((src[declared:] == POISON).all())


def test_argument_errors():
    flat, planes, boxes, C, size, filt, pil, _ = case("graph_a")
    planes = planes.copy()
    need = K.ragged_ws_offsets(planes, C, size[1], boxes[:, 3])
    src = torch.from_numpy(flat).to(DEV)
    dplanes = torch.from_numpy(K.check_ragged_planes(planes, C, flat.size)).to(DEV)
    dboxes = torch.from_numpy(K.check_ragged_boxes(boxes, planes, size)).to(DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty(pil.shape[0] * C * 16 * 20 + 16, dtype=torch.uint8, device=DEV)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    Hs, Ws = K.ragged_bounds(planes)

    def call(src_p=src.data_ptr(), n=flat.size, pl=dplanes.data_ptr(), bx=dboxes.data_ptr(), o=out.data_ptr(), B=2, C=C, Hs=Hs, Ws=Ws,
             So_h=16, So_w=16, filt=filt, w=ws.data_ptr(), wb=need):
        return L.vr_resample_ragged_u8(src_p, n, pl, bx, o, B, C, Hs, Ws, So_h, So_w, filt, w, wb, stream)
    assert call(src_p=None) == -1 and call(pl=None) == -1 and call(bx=None) == -1 and call(o=None) == -1 and call(w=None) == -1
    assert call(n=0) == -1 and call(B=0) == -1 and call(Hs=0) == -1 and call(So_h=0) == -1 and call(So_w=0) == -1
    assert call(C=0) == -1 and call(C=5) == -1 and call(filt=1) == -1 and call(filt=4) == -1
    assert call(wb=0) == -1 and call(wb=C * 16 - 1) == -1                           # smaller than one row of one sample
    assert call(o=src.data_ptr()) == -1 and call(w=src.data_ptr()) == -1 and call(w=out.data_ptr()) == -1
    assert call(So_w=18) == -3 and call(B=65536) == -3 and call(Ws=Ws + 2) == -3
    assert call(src_p=src.data_ptr() + 4) == -2 and call(w=ws.data_ptr() + 4, wb=need - 4) == -2 and call(o=out.data_ptr() + 2) == -2
    assert call(pl=dplanes.data_ptr() + 4) == -2 and call(bx=dboxes.data_ptr() + 2) == -2
    assert call() == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.resample_ragged_u8(src, planes, np.concatenate([boxes[:, :4], [[18, 16, 0, 0, 0]] * 2], axis=1), C, (16, 18), filt)
    with pytest.raises(ValueError):
        K.resample_ragged_u8(src, planes, boxes, C, size, "lanczos")
    with pytest.raises(ValueError):
        K.resample_ragged_u8(src, dplanes, boxes, C, size, filt)                      # a device table with a host table
    with pytest.raises(TypeError):
        K.resample_ragged_u8(src.view(1, -1), planes, boxes, C, size, filt)

    collated, pixels, _, _, _, _ = _big()
    jplanes, nbytes = K.ragged_layout(collated[3].numpy(), 3)
    blob, descs, qtabs = (t.to(DEV) for t in collated[:3])
    n = blob.numel()
    dst = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
    jws = torch.empty(K.jpeg_ws_bytes(n), dtype=torch.uint8, device=DEV)
    jt = torch.from_numpy(K.check_ragged_planes(jplanes, 3, nbytes, collated[3].numpy())).to(DEV)

    def jcall(blob_p=blob.data_ptr(), n=n, d=descs.data_ptr(), q=qtabs.data_ptr(), o=dst.data_ptr(), ob=nbytes, pl=jt.data_ptr(), B=4,
              Hs=48, Ws=4100, w=jws.data_ptr(), wb=jws.numel()):
        return L.vr_jpeg_reconstruct_ragged_u8(blob_p, n, d, q, o, ob, pl, B, Hs, Ws, w, wb, stream)
    assert jcall(blob_p=None) == -1 and jcall(d=None) == -1 and jcall(q=None) == -1 and jcall(o=None) == -1 and jcall(pl=None) == -1
    assert jcall(n=0) == -1 and jcall(ob=0) == -1 and jcall(B=0) == -1 and jcall(Hs=0) == -1 and jcall(Ws=0) == -1
    assert jcall(w=None) == -1 and jcall(wb=jws.numel() - 16) == -1 and jcall(w=blob.data_ptr()) == -1 and jcall(w=dst.data_ptr()) == -1
    assert jcall(o=blob.data_ptr()) == -1
    assert jcall(Ws=4102) == -3 and jcall(Hs=8196) == -3 and jcall(Ws=8196) == -3 and jcall(B=65536) == -3
    assert jcall(o=dst.data_ptr() + 4) == -2 and jcall(pl=jt.data_ptr() + 4) == -2 and jcall(blob_p=blob.data_ptr() + 8) == -2
    assert jcall() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, jt, dst=dst)                 # a device table without bounds
    with pytest.raises(ValueError):
        K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, jplanes[:3], dst=dst)


# ---- the loader chains ---------------------------------------------------------------------------------------------------------------------
NAMES_E2E = ["37x53.420.q85", "48x40.444.q30r2", "31x64.422.q95rr", "17x23.gray.q100opt",
             "48x40.420.q95rr", "fallback.progressive", "37x53.422.q100opt", "31x64.444.q85"]


def _transform(kind, S):
    if kind == "train":
        return RandomResizedCrop(S, rng=random.Random(5), generator=torch.Generator().manual_seed(6))
    return ResizeCenterCrop(S, crop_pct=0.8, interpolation="bilinear")


@pytest.mark.parametrize("kind", ["eval", "train"])
def test_ragged_loader_chains_equal_the_padded_chain(kind):
    """DataLoader(jpeg_collate) -> DeviceJpegLoader(ragged=True) -> DeviceCropLoader (+ RandAugment in training), and
    ragged_collate_u8 -> DeviceCropLoader, against the padded forms of both: two batches of four files, the same seeds."""
    S = 16
    records = [next(r for r in EJ.golden_records(F22) if r[0] == n) for n in NAMES_E2E]
    files = [(r[2], k % 5) for k, r in enumerate(records)]
    loader = torch.utils.data.DataLoader(files, batch_size=4, collate_fn=data.jpeg_collate, pin_memory=True)
    decoded = [[(r[3], k % 5) for k, r in list(enumerate(records))[lo:lo + 4]] for lo in (0, 4)]
    padded = [data.pad_collate_u8(b) for b in decoded]
    ragged = [data.ragged_collate_u8(b) for b in decoded]
    aug = (lambda: RandAugment("rand-m9-mstd0.5-inc1", size=S, rng=random.Random(7), np_rng=np.random.RandomState(8))) \
        if kind == "train" else (lambda: None)
    want = [(x.cpu(), y.cpu()) for x, y in data.DeviceCropLoader(padded, _transform(kind, S), DEV, augment=aug())]
    jl = data.DeviceJpegLoader(loader, DEV, ragged=True)
    assert len(jl) == 2 and jl.dataset is files and jl.sampler is loader.sampler
    chains = {"jpeg": data.DeviceCropLoader(jl, _transform(kind, S), DEV, augment=aug()),
              "collate": data.DeviceCropLoader(ragged, _transform(kind, S), DEV, augment=aug())}
    for name, chain in chains.items():
        got = [(x.cpu(), y.cpu()) for x, y in chain]
        assert len(got) == len(want) == 2, name
        for (x, y), (wx, wy) in zip(got, want):
            assert x.dtype == torch.uint8 and tuple(x.shape) == (4, 3, S, S) and torch.equal(x, wx) and torch.equal(y, wy), name
    for (canvas, sizes, _), batch in zip(data.DeviceJpegLoader(loader, DEV, ragged=True), decoded):
        assert isinstance(canvas, data.RaggedCanvas)
        for b, (img, _) in enumerate(batch):
            assert np.array_equal(canvas.plane(b, img.shape[:2]).cpu().numpy(), img.transpose(2, 0, 1))


def test_big_images_pass_the_ragged_chains_where_the_padded_chain_raises():
    collated, pixels, boxes, size, filt, crops = _big()
    S = size[0]

    class Fixed:                                                          # the fixture's boxes in a transform's place
        size, filter = S, "bicubic"

        def draw(self, sizes):
            return boxes
    (x, y), = data.DeviceCropLoader(data.DeviceJpegLoader([collated], DEV, ragged=True), Fixed(), DEV)
    assert torch.equal(x.cpu(), torch.from_numpy(crops)) and y.tolist() == [0, 1, 2, 3]
    (x, y), = data.DeviceCropLoader([data.ragged_collate_u8([(p, k) for k, p in enumerate(pixels)])], Fixed(), DEV)
    assert torch.equal(x.cpu(), torch.from_numpy(crops))
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        list(data.DeviceCropLoader(data.DeviceJpegLoader([collated], DEV), Fixed(), DEV))
