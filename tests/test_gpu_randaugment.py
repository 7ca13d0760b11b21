"""vr_rand_augment_u8 on the GPU: timm's RandAugment ops on uint8 batches, bit for bit against PIL's own outputs committed in
tests/golden/f21_randaugment_pil.npz (written by tests/golden/make_randaugment_golden.py; PIL is not needed here) and against the
numpy emulation tests/emu_randaugment.py -- on B <= 4 and 16 / 32 / 48 pixel images that reach every op kind and branch: the table
ops at the ends of their arguments, autocontrast and equalize on both sides of their identity conditions, the blends at the ends of
timm's factor range and a 64-factor sweep over both clip ends, contrast at a mean of k + 0.5, the smoothing filter's border, affine
maps in both filters in one launch (all fill, no fill, H != W), statistics ops after an affine layer, up to four layers, a captured
launch that follows its table, argument rejections, and the loader chain; one 68 x 64 case has more pixel quads than the workgroup
has lanes."""
import os
import random

import numpy as np
import pytest
import torch

import emu_randaugment as E
from vitres import data
from vitres import kernels as K
from vitres.rand_augment import RandAugment
from vitres.resized_crop import RandomResizedCrop

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f21_randaugment_pil.npz"))
_CASES = {}
BLENDS = (E.BRIGHTNESS, E.COLOR, E.CONTRAST, E.SHARPNESS)


def records(table):
    return E.fill_records(K.ra_table(*np.asarray(table["op"]).shape), table)


def case(name):
    """(src, host op table, fill, PIL's output, the emulation's output), loaded / computed once and never written."""
    if name not in _CASES:
        src, table, fill, pil = E.golden_case(G, name)
        _CASES[name] = (src, records(table), fill, pil, E.rand_augment_u8(src, table, fill))
    return _CASES[name]


def run(src, table, fill, **kw):
    return K.rand_augment_u8(torch.from_numpy(src).to(DEV), table, fill, **kw).cpu()


@pytest.mark.parametrize("name", E.golden_names(G))
def test_kernel_equals_pil_and_the_emulation(name):
    src, table, fill, pil, emu = case(name)
    got = run(src, table, fill)
    assert got.dtype == torch.uint8 and tuple(got.shape) == pil.shape
    assert torch.equal(got, torch.from_numpy(pil)), "differs from PIL in %d bytes" % int((got.numpy() != pil).sum())
    assert torch.equal(got, torch.from_numpy(emu))


def test_table_ops_at_the_ends_of_their_arguments():
    src, table, fill, pil, _ = case("lut_a")
    assert table["op"][:, 0].tolist() == [E.INVERT, E.POSTERIZE, E.POSTERIZE, E.POSTERIZE] and table["iarg"][1:3, 0].tolist() == [0, 7]
    got = run(src, table, fill).numpy()
    assert np.array_equal(got[0], 255 - src[0]) and (got[1] == 0).all() and np.array_equal(got[2], src[2] & 0xFE)
    src, table, fill, pil, _ = case("lut_b")
    assert table["iarg"][:2, 0].tolist() == [0, 256]
    got = run(src, table, fill).numpy()
    assert np.array_equal(got[0], 255 - src[0]) and np.array_equal(got[1], src[1]) and np.array_equal(got, pil)


def test_autocontrast_constant_channel_and_stretch():
    src, table, fill, pil, _ = case("autocontrast")
    got = run(src, table, fill).numpy()
    assert (src[1, 1] == 77).all() and (got[1, 1] == 77).all()
    assert (src[0].min(), src[0].max()) == (40, 200) and (got[0].min(), got[0].max()) == (0, 255) and np.array_equal(got, pil)


def test_equalize_on_both_sides_of_step_zero():
    src, table, fill, pil, _ = case("equalize16")
    steps = [[E.equalize_step(np.bincount(src[b, c].ravel(), minlength=256)) for c in range(3)] for b in range(3)]
    assert steps == [[0] * 3, [0] * 3, [1] * 3]
    got = run(src, table, fill).numpy()
    assert np.array_equal(got[:2], src[:2]) and not np.array_equal(got[2], src[2]) and np.array_equal(got, pil)
    src, table, fill, pil, _ = case("equalize32")
    steps = [E.equalize_step(np.bincount(src[b, c].ravel(), minlength=256)) for b in range(3) for c in range(3)]
    assert steps[:8] == [(1024 - int(np.bincount(src[b, c].ravel())[-1])) // 255 for b in range(3) for c in range(3)][:8]
    assert min(steps[:8]) > 0 and steps[8] == 0
    got = run(src, table, fill).numpy()
    assert np.array_equal(got, pil) and (got[2, 2] == 9).all() and (got[1] == 255).any()


@pytest.mark.parametrize("which", range(4))
def test_blend_factor_sweep(which):
    """64 factors from 0.1 to 1.9, four per launch, on an image that holds 0 and 255 side by side"""
    src, factors, want = G["sweep.src"], G["sweep.factors"], G["sweep.out"][which]
    fill = tuple(int(v) for v in G["sweep.fill"])
    assert src.min() == 0 and src.max() == 255 and (want == 0).any() and (want == 255).any()
    dsrc = torch.from_numpy(np.repeat(src, 4, axis=0)).to(DEV)
    for lo in range(0, 64, 4):
        table = K.ra_table(4, 1)
        table["op"], table["factor"][:, 0] = BLENDS[which], factors[lo:lo + 4]
        got = K.rand_augment_u8(dsrc, table, fill).cpu().numpy()
        assert np.array_equal(got, want[lo:lo + 4]), (BLENDS[which], factors[lo:lo + 4])


def test_contrast_where_the_grey_mean_is_half_way():
    src, table, fill, pil, _ = case("contrast_half")
    means = [float(E.grey(src[b]).sum()) / 1024 for b in range(3)]
    k = int(means[0])
    assert means[0] == k + 0.5 and all(abs(m - (k + 0.5)) <= 1e-3 for m in means)
    assert [E.contrast_mean(src[b]) for b in range(3)] == [k + 1, k, k + 1]
    assert torch.equal(run(src, table, fill), torch.from_numpy(pil))


def test_sharpness_copies_the_border():
    src, table, fill, pil, _ = case("degenerate")                                   # factor 0: the smoothed image itself
    assert table["op"][3, 0] == E.SHARPNESS and table["factor"][3, 0] == 0
    got = run(src, table, fill).numpy()[3]
    assert np.array_equal(got[:, 0], src[3][:, 0]) and np.array_equal(got[:, -1], src[3][:, -1])
    assert np.array_equal(got[:, :, 0], src[3][:, :, 0]) and np.array_equal(got[:, :, -1], src[3][:, :, -1])
    assert not np.array_equal(got[:, 1:-1, 1:-1], src[3][:, 1:-1, 1:-1]) and np.array_equal(got, pil[3])
    src, table, fill, pil, _ = case("blend_1.9")                                    # and with a factor: the border is the source's
    got = run(src, table, fill).numpy()[3]
    assert np.array_equal(got[:, 0], src[3][:, 0]) and np.array_equal(got[:, :, -1], src[3][:, :, -1])


def test_affine_all_fill_none_fill_and_both_filters_in_one_launch():
    src, table, fill, pil, _ = case("affine_fill")
    assert table["filter"][:, 0].tolist() == [3, 2, 3, 2]
    got = run(src, table, fill).numpy()
    f = np.array(fill, dtype=np.uint8).reshape(3, 1, 1)
    assert (got[0] == f).all() and (got[1] == f).all() and np.array_equal(got, pil)
    for name in ("affine_shear", "affine_translate", "affine_rotate"):
        assert set(case(name)[1]["filter"][:, 0].tolist()) == {2, 3}
    for name, hw in (("affine_wide", (16, 32)), ("affine_tall", (48, 32))):
        assert case(name)[0].shape[2:] == hw


def test_trips_case_has_more_quads_than_lanes():
    src, table, fill, pil, _ = case("trips")
    assert src.shape[2] * src.shape[3] // 4 > 1024 and set(table["op"].ravel().tolist()) == {E.AFFINE, E.SHARPNESS, E.CONTRAST}
    assert torch.equal(run(src, table, fill), torch.from_numpy(pil))


def test_recipe_size_against_the_emulation():
    """224 x 224, the recipes' size (a dozen trips of every loop), tables of the recipes' config: against the emulation the vectors pin"""
    rs = np.random.RandomState(5)
    y, x = np.mgrid[0:224, 0:224]
    src = np.stack([np.clip(128 + 140 * np.sin(f * x + p) * np.cos(g * y) + rs.normal(0, 9, (224, 224)), 0, 255).astype(np.uint8)
                    for f, g, p in rs.uniform(0.01, 0.2, (12, 3))]).reshape(4, 3, 224, 224)
    ra = RandAugment("rand-m9-mstd0.5-inc1", size=224, interpolation="random", rng=random.Random(2), np_rng=np.random.RandomState(3))
    table = ra.draw(4)
    table[0, 0] = table[0, 1]                                                      # (whatever was drawn: sample 0 runs two affine layers)
    table[0]["op"], table[0]["filter"] = E.AFFINE, (2, 3)
    table[0, 0]["m"], table[0, 1]["m"] = (1, 0.27, 0, 0, 1, 0), (0.9, -0.3, 40.5, 0.3, 0.9, -20.25)
    assert (table["op"] != 0).sum() >= 4
    assert torch.equal(run(src, table, ra.fill), torch.from_numpy(E.rand_augment_u8(src, table, ra.fill)))


def test_identity_records_copy_the_source():
    src, table, fill, pil, _ = case("identity2")
    assert (table["op"] == 0).all() and np.array_equal(pil, src)
    assert torch.equal(run(src, table, fill), torch.from_numpy(src))
    one = K.ra_table(2, 1)
    assert torch.equal(run(src, one, fill), torch.from_numpy(src))
    big = np.random.RandomState(0).randint(0, 256, (3, 3, 36, 20)).astype(np.uint8)    # a plane that is no multiple of 16 bytes
    assert torch.equal(run(big, K.ra_table(3, 4), fill), torch.from_numpy(big))


def test_bad_device_records_apply_nothing():
    """The device table is the caller's to check; a record outside the contract is skipped, the rest of the chain runs."""
    src, table, fill, pil, _ = case("lut_a")
    t = K.ra_table(4, 2)
    t["op"][:, 0] = (99, E.POSTERIZE, E.SOLARIZE, E.AFFINE)
    t["iarg"][:, 0] = (0, 9, -3, 0)
    t["filter"][:, 0] = (0, 0, 0, 7)
    t["op"][:, 1] = E.INVERT
    dev = torch.from_numpy(np.ascontiguousarray(t).view(np.int32).reshape(4, 2, 16)).to(DEV)
    got = K.rand_augment_u8(torch.from_numpy(src).to(DEV), dev, fill).cpu().numpy()
    assert np.array_equal(got, 255 - src)


def test_out_argument_and_different_ops_per_sample():
    src, table, fill, pil, _ = case("mixed")
    assert len({tuple(r) for r in table["op"].tolist()}) == 4
    out = torch.full(pil.shape, 7, dtype=torch.uint8, device=DEV)
    ret = K.rand_augment_u8(torch.from_numpy(src).to(DEV), table, fill, out=out)
    assert ret is out and torch.equal(out.cpu(), torch.from_numpy(pil))


def test_argument_rejections_leave_out_unwritten():
    src = torch.zeros((2, 3, 16, 16), dtype=torch.uint8, device=DEV)
    out = torch.full((2, 3, 16, 16), 9, dtype=torch.uint8, device=DEV)
    ok = K.ra_table(2, 2)
    ok["op"] = E.INVERT
    bad = ok.copy()
    bad["op"][1, 1] = 12
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                             # an unknown op in the host table
        K.rand_augment_u8(src, bad, (0, 0, 0), out=out)
    bad = ok.copy()
    bad["op"][0, 0], bad["iarg"][0, 0] = E.POSTERIZE, 9
    with pytest.raises(RuntimeError, match="VR_EINVAL"):
        K.rand_augment_u8(src, bad, (0, 0, 0), out=out)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                             # src == out
        K.rand_augment_u8(src, ok, (0, 0, 0), out=src)
    five = torch.zeros((2, 5, 16), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                             # five layers
        K.rand_augment_u8(src, five, (0, 0, 0), out=out)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):                       # W % 4
        K.rand_augment_u8(torch.zeros((2, 3, 16, 18), dtype=torch.uint8, device=DEV), ok, (0, 0, 0))
    with pytest.raises(RuntimeError, match="VR_EALIGN"):                             # a source one byte past a dword
        K.rand_augment_u8(torch.zeros(2 * 3 * 16 * 16 + 1, dtype=torch.uint8, device=DEV)[1:].view(2, 3, 16, 16), ok, (0, 0, 0), out=out)
    with pytest.raises(TypeError):
        K.rand_augment_u8(src.float(), ok, (0, 0, 0))
    with pytest.raises(TypeError):                                                   # one channel
        K.rand_augment_u8(src[:, :1], ok[:, :1], (0, 0, 0))
    with pytest.raises(ValueError):
        K.rand_augment_u8(src, ok, (0, 0, 256), out=out)
    with pytest.raises(ValueError):
        K.rand_augment_u8(src, ok, (0, 0, 0), out=out[:1])
    L = K._lib.lib()
    assert L.vr_rand_augment_ws_bytes(2, 16, 16, 1) == 0 and L.vr_rand_augment_ws_bytes(2, 16, 16, 2) == 2 * 3 * 16 * 16
    table = torch.from_numpy(K.check_ra_table(ok, 2)).to(DEV)
    rc = L.vr_rand_augment_u8(src.data_ptr(), table.data_ptr(), out.data_ptr(), 2, 16, 16, 2, 0, None, 0, None)
    assert rc == -1                                                                  # two layers need the workspace
    torch.cuda.synchronize()
    assert bool((out == 9).all())


def test_captured_launch_follows_a_table_rewritten_in_place():
    src, table_a, fill, pil_a, emu_a = case("graph_a")
    src_b, table_b, _, pil_b, emu_b = case("graph_b")
    assert np.array_equal(src, src_b) and not np.array_equal(pil_a, pil_b)
    B = src.shape[0]
    table = torch.from_numpy(K.check_ra_table(table_a, B)).to(DEV)
    next_table = torch.from_numpy(K.check_ra_table(table_b, B)).to(DEV)
    dsrc = torch.from_numpy(src).to(DEV)
    out = torch.zeros(pil_a.shape, dtype=torch.uint8, device=DEV)
    K.rand_augment_u8(dsrc, table, fill, out=out)                                   # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.rand_augment_u8(dsrc, table, fill, out=out)
    out.zero_()
    graph.replay()
    assert torch.equal(out.cpu(), torch.from_numpy(pil_a)) and np.array_equal(pil_a, emu_a)
    table.copy_(next_table)
    graph.replay()
    assert torch.equal(out.cpu(), torch.from_numpy(pil_b)) and np.array_equal(pil_b, emu_b)


def _images(seed, sizes):
    rs = np.random.RandomState(seed)
    return [(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), i % 5) for i, (h, w) in enumerate(sizes)]


def test_crop_loader_with_augment_into_prefetch_loader_is_the_emulations_chain():
    """pad_collate_u8 -> DeviceCropLoader(augment=) -> DevicePrefetchLoader: every yielded batch is vr_normalize_u8 of the emulation's
    RandAugment of the device's crop by the same draws (the crop itself is pinned by tests/test_gpu_resample.py)."""
    S = 16
    batches = [_images(20, [(21, 30), (33, 18), (17, 17), (25, 40)]), _images(21, [(40, 25), (19, 44), (16, 23), (30, 30)])]
    collated = [data.pad_collate_u8(b) for b in batches]
    make_tf = lambda: RandomResizedCrop(S, rng=random.Random(5), generator=torch.Generator().manual_seed(6))              # noqa: E731
    make_ra = lambda: RandAugment("rand-m9-mstd0.5-inc1", size=S, rng=random.Random(7), np_rng=np.random.RandomState(8))  # noqa: E731
    ref_tf, ref_ra = make_tf(), make_ra()
    loader = data.DevicePrefetchLoader(data.DeviceCropLoader(collated, make_tf(), DEV, augment=make_ra()), DEV)
    seen, applied = 0, 0
    for (x, labels), (canvas, sizes, want_labels) in zip(loader, collated):
        crop = K.resample_u8(canvas.to(DEV), ref_tf.draw(sizes), S, ref_tf.filter).cpu().numpy()
        table = ref_ra.draw(4)
        applied += int((table["op"] != 0).sum())
        aug = E.rand_augment_u8(crop, table, ref_ra.fill)
        want = K.normalize_u8(torch.from_numpy(aug).to(DEV), K.IMAGENET_DEFAULT_MEAN, K.IMAGENET_DEFAULT_STD)
        assert x.dtype == torch.float32 and tuple(x.shape) == (4, 3, S, S) and torch.equal(x, want)
        assert torch.equal(labels.cpu(), want_labels)
        seen += 1
    assert seen == 2 and len(loader) == 2 and applied >= 4
