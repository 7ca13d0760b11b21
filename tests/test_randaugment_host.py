"""CPU checks of the device RandAugment stage: the numpy emulation tests/emu_randaugment.py against PIL's committed outputs (always)
and against PIL itself on a wider random sweep (where PIL is importable); the draws of vitres.rand_augment.RandAugment against timm
0.3.2's statements restated by hand; Image.rotate's matrix; the host-side record check; DeviceCropLoader(augment=None) unchanged."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest
import torch

import emu_randaugment as E
from vitres import _lib, data
from vitres import kernels as K
from vitres.rand_augment import RAND_INCREASING_TRANSFORMS, RAND_TRANSFORMS, RandAugment, parse_config, rotate_matrix
from vitres.resized_crop import RandomResizedCrop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f21_randaugment_pil.npz")
G = np.load(GOLDEN)
BLENDS = (E.BRIGHTNESS, E.COLOR, E.CONTRAST, E.SHARPNESS)


def test_op_codes_and_record_layout_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    for name, code in K.RA_OPS.items():
        assert "VR_RA_%s = %d" % (name.upper(), code) in hdr
        assert getattr(E, name.upper()) == code
    assert ctypes.sizeof(_lib.RaOp) == 64 == K.RA_DTYPE.itemsize
    for f in ("op", "filter", "iarg", "factor", "m"):
        assert getattr(_lib.RaOp, f).offset == K.RA_DTYPE.fields[f][1]
    assert "vr_rand_augment_ws_bytes" in _lib.OTHER_SYMBOLS and "size_t vr_rand_augment_ws_bytes(" in hdr


@pytest.mark.parametrize("name", E.golden_names(G))
def test_emulation_equals_pils_committed_output(name):
    src, table, fill, pil = E.golden_case(G, name)
    assert np.array_equal(E.rand_augment_u8(src, table, fill), pil)
    recs = E.fill_records(K.ra_table(*table["op"].shape), table)                  # the structured table gives the same
    assert np.array_equal(E.rand_augment_u8(src, recs, K.ra_fill(fill)), pil)


def test_emulation_equals_pils_committed_factor_sweep():
    src, factors, out = G["sweep.src"], G["sweep.factors"], G["sweep.out"]
    assert len(factors) == 64 and factors.min() < 1 < factors.max() and src.min() == 0 and src.max() == 255
    for i, op in enumerate(BLENDS):
        for j, f in enumerate(factors):
            assert np.array_equal(E.apply_op(src[0], op, 0, 0, f, None, (0, 0, 0)), out[i, j]), (op, f)
        assert (out[i] == 0).any() and (out[i] == 255).any()                     # both clip ends are reached


def test_golden_cases_take_the_branches_they_are_named_for():
    src = G["equalize16.src"]
    steps = [[E.equalize_step(np.bincount(src[b, c].ravel(), minlength=256)) for c in range(3)] for b in range(3)]
    assert steps == [[0] * 3, [0] * 3, [1] * 3]                                   # 256 pixels: step == 0 unless the last bin holds one
    assert np.array_equal(G["equalize16.out"][:2], src[:2]) and not np.array_equal(G["equalize16.out"][2], src[2])
    for name in ("equalize32", "equalize48"):
        src = G[name + ".src"]
        steps = [E.equalize_step(np.bincount(src[b, c].ravel(), minlength=256)) for b in range(src.shape[0]) for c in range(3)]
        assert max(steps) > 0 and not np.array_equal(G[name + ".out"], src)
    assert E.equalize_step(np.bincount(G["equalize32.src"][2, 2].ravel(), minlength=256)) == 0        # the one-valued channel
    ac, out = G["autocontrast.src"], G["autocontrast.out"]
    assert (ac[1, 1] == 77).all() and (out[1, 1] == 77).all()                                         # constant: untouched
    assert ac[0].min() == 40 and ac[0].max() == 200 and out[0].min() == 0 and out[0].max() == 255    # stretched
    half = G["contrast_half.src"]
    means = [float(E.grey(half[b]).sum()) / (32 * 32) for b in range(3)]
    k = int(means[0])
    assert means[0] == k + 0.5 and all(abs(m - (k + 0.5)) <= 1e-3 for m in means)
    assert [E.contrast_mean(half[b]) for b in range(3)] == [k + 1, k, k + 1]
    deg, dsrc = G["degenerate.out"], G["degenerate.src"]
    assert (deg[0] == 0).all() and (deg[1, 0] == deg[1, 1]).all() and len(np.unique(deg[2])) == 1
    s = deg[3]                                                                                        # SMOOTH: the border is the source's
    assert np.array_equal(s[:, 0], dsrc[3][:, 0]) and np.array_equal(s[:, -1], dsrc[3][:, -1])
    assert np.array_equal(s[:, :, 0], dsrc[3][:, :, 0]) and np.array_equal(s[:, :, -1], dsrc[3][:, :, -1])
    assert not np.array_equal(s[:, 1:-1, 1:-1], dsrc[3][:, 1:-1, 1:-1])
    fill = G["affine_fill.fill"].reshape(3, 1, 1)
    af = G["affine_fill.out"]
    assert (af[0] == fill).all() and (af[1] == fill).all()
    fsrc = G["affine_fill.src"]
    assert all(not ((af[b] == fill).all(axis=0) & ~(fsrc[b] == fill).all(axis=0)).any() for b in (2, 3))
    assert set(G["affine_shear.ops"][:, 0, 1].tolist()) == {2, 3}


def test_emulation_equals_pil_on_random_records():
    """A wider sweep than the committed vectors: random sizes, ops and arguments through PIL itself."""
    pytest.importorskip("PIL")
    import make_randaugment_golden as M
    rng = random.Random(3)
    for i in range(120):
        H, W = rng.choice([5, 8, 13, 16, 21]), rng.choice([4, 8, 12, 20])
        src = (M.noise if i % 2 else M.smooth_noise)(100 + i, 1, H, W)
        recs = []
        for _ in range(2):
            op = rng.randrange(12)
            if op == E.AFFINE:
                kind = rng.randrange(4)
                filt = rng.choice([2, 3])
                r = (M.rotation(rng.uniform(-40, 40), W, H, filt), M.shear_x(rng.uniform(-0.4, 0.4), filt),
                     M.shear_y(rng.uniform(-0.4, 0.4), filt), M.translate_x(rng.uniform(-0.6, 0.6), W, filt))[kind]
            else:
                iarg = {E.POSTERIZE: rng.randint(0, 8), E.SOLARIZE: rng.randint(0, 256), E.SOLARIZE_ADD: rng.randint(0, 255)}.get(op, 0)
                r = M.rec(op, iarg=iarg, factor=rng.uniform(0.0, 2.2))
            recs.append(r)
        want = M.pil_case(src, [recs], M.FILL)
        table = dict(op=np.array([[r["op"] for r in recs]]), filter=np.array([[r["filt"] for r in recs]]),
                     iarg=np.array([[r["iarg"] for r in recs]]), factor=np.array([[r["factor"] for r in recs]]),
                     m=np.array([[r["m"] for r in recs]]))
        assert np.array_equal(E.rand_augment_u8(src, table, M.FILL), want), (i, recs)


# ---- the draws -----------------------------------------------------------------------------------------------------------------------
class Recorder:
    """a random.Random that logs what is asked of it"""

    def __init__(self, seed):
        self.r, self.log = random.Random(seed), []

    def random(self):
        self.log.append("random")
        return self.r.random()

    def gauss(self, mu, sigma):
        self.log.append("gauss")
        return self.r.gauss(mu, sigma)

    def choice(self, seq):
        self.log.append("choice")
        return self.r.choice(seq)


def test_config_strings():
    assert parse_config("rand-m9-mstd0.5-inc1") == (9, 2, 0.5, True)
    assert parse_config("rand-m7-n3") == (7, 3, 0.0, False)
    assert parse_config("rand") == (10.0, 2, 0.0, False)
    with pytest.raises(NotImplementedError):
        RandAugment("rand-m9-w0")
    with pytest.raises(ValueError):
        RandAugment("rand-m9-q1")
    with pytest.raises(ValueError):
        RandAugment("augmix-m9")
    with pytest.raises(ValueError):
        RandAugment("rand-m9-n5")
    ra = RandAugment()
    assert ra.layers == 2 and ra.fill == (124, 116, 104) and ra.ops == RAND_INCREASING_TRANSFORMS and ra.size == (224, 224)
    assert RandAugment("rand-m9").ops == RAND_TRANSFORMS and len(RAND_TRANSFORMS) == len(RAND_INCREASING_TRANSFORMS) == 15
    assert RandAugment("rand-n3-m4").draw(5).shape == (5, 3)


def test_a_fixed_seed_gives_a_fixed_table_and_the_histogram_covers_all_ops():
    make = lambda: RandAugment(size=32, rng=random.Random(1), np_rng=np.random.RandomState(2))        # noqa: E731
    a, b = make().draw(64), make().draw(64)
    assert a.dtype == K.RA_DTYPE and a.shape == (64, 2) and a.tobytes() == b.tobytes()
    assert make().draw(63).tobytes() != a[1:].tobytes()
    K.check_ra_table(a, 64, 2)
    # which of the 15 ops were chosen is what np_rng gave; about half of the records are identity
    chosen = np.random.RandomState(2).choice(15, 2 * 64 * 8)
    assert set(chosen.tolist()) == set(range(15))
    big = RandAugment(size=32, rng=random.Random(1), np_rng=np.random.RandomState(2)).draw(64 * 8)
    kinds = np.bincount(big["op"].ravel(), minlength=12)
    assert (kinds > 0).all() and 0.4 < kinds[0] / big.size < 0.6
    assert set(big["filter"][big["op"] == E.AFFINE].tolist()) == {3}


def _expected_draw(seed, np_seed, B, config, size, interpolation):
    """timm's RandAugment.__call__ + AugmentOp.__call__ + the level functions, written out once more, as (name, argument) lists"""
    m, n, mstd, inc = parse_config(config)
    names = RAND_INCREASING_TRANSFORMS if inc else RAND_TRANSFORMS
    r, nr, out = random.Random(seed), np.random.RandomState(np_seed), []
    for _ in range(B):
        row = []
        for i in nr.choice(15, n):
            name = names[i]
            if r.random() > 0.5:
                row.append(None)
                continue
            level = min(10., max(0, r.gauss(m, mstd) if mstd > 0 else m)) / 10.
            neg = lambda v: -v if r.random() > 0.5 else v                                              # noqa: E731
            if name in ("AutoContrast", "Equalize", "Invert"):
                arg = ()
            elif name == "Rotate":
                arg = neg(level * 30.)
            elif name in ("ShearX", "ShearY"):
                arg = neg(level * 0.3)
            elif name in ("TranslateXRel", "TranslateYRel"):
                arg = neg(level * 0.45)
            elif name.endswith("Increasing") and name[0] in "CBS" and not name.startswith("Solarize"):
                arg = 1.0 + neg(level * .9)
            elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
                arg = level * 1.8 + 0.1
            elif name == "Posterize":
                arg = int(level * 4)
            elif name == "PosterizeIncreasing":
                arg = 4 - int(level * 4)
            elif name == "Solarize":
                arg = int(level * 256)
            elif name == "SolarizeIncreasing":
                arg = 256 - int(level * 256)
            else:
                assert name == "SolarizeAdd"
                arg = int(level * 110)
            filt = None
            if name in ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"):
                filt = r.choice((2, 3)) if interpolation == "random" else {"bilinear": 2, "bicubic": 3}[interpolation]
            row.append((name, arg, filt))
        out.append(row)
    return out


@pytest.mark.parametrize("config,interpolation", [("rand-m9-mstd0.5-inc1", "bicubic"), ("rand-m9-mstd0.5", "random"),
                                                  ("rand-m6-n3-mstd0", "bilinear"), ("rand-m10-n4-mstd2-inc1", "random")])
def test_draws_follow_timms_statements(config, interpolation):
    H, W, B = 24, 32, 200
    table = RandAugment(config, size=(H, W), interpolation=interpolation, rng=random.Random(11), np_rng=np.random.RandomState(12)).draw(B)
    want = _expected_draw(11, 12, B, config, (H, W), interpolation)
    seen = set()
    for b in range(B):
        for k, w in enumerate(want[b]):
            rec = table[b, k]
            if w is None:
                assert rec["op"] == E.IDENTITY
                continue
            name, arg, filt = w
            seen.add(name)
            base = name.replace("Increasing", "")
            if base in ("AutoContrast", "Equalize", "Invert"):
                assert rec["op"] == K.RA_OPS[base.lower()]
            elif base in ("Color", "Contrast", "Brightness", "Sharpness"):
                assert rec["op"] == K.RA_OPS[base.lower()] and rec["factor"] == np.float32(arg)
            elif base == "Posterize":
                assert (rec["op"], rec["iarg"]) == (E.POSTERIZE, arg) and 0 <= arg <= 4
            elif base == "Solarize":
                assert (rec["op"], rec["iarg"]) == (E.SOLARIZE, arg)
            elif base == "SolarizeAdd":
                assert (rec["op"], rec["iarg"]) == (E.SOLARIZE_ADD, arg)
            else:
                m = {"ShearX": (1, arg, 0, 0, 1, 0), "ShearY": (1, 0, 0, arg, 1, 0), "TranslateXRel": (1, 0, arg * W, 0, 1, 0),
                     "TranslateYRel": (1, 0, 0, 0, 1, arg * H)}.get(base) or rotate_matrix(arg, W, H)
                if m is None:
                    assert rec["op"] == E.IDENTITY
                else:
                    assert rec["op"] == E.AFFINE and rec["filter"] == filt and rec["m"].tolist() == [float(v) for v in m]
    assert len(seen) == 15
    if interpolation == "random":
        assert set(table["filter"][table["op"] == E.AFFINE].tolist()) == {2, 3}


def test_random_is_consumed_in_the_stated_order():
    for name, extra in (("Invert", []), ("Rotate", ["random"]), ("ShearX", ["random"]), ("TranslateYRel", ["random"]),
                        ("ColorIncreasing", ["random"]), ("Color", []), ("PosterizeIncreasing", []), ("SolarizeAdd", [])):
        for interpolation in ("bicubic", "random"):
            rec = Recorder(5)
            ra = RandAugment("rand-m9-mstd0.5-inc1", size=16, interpolation=interpolation, rng=rec)
            table = K.ra_table(1, 1)
            ra.level_to_record(name, 9.0, rec, table[0, 0:1])
            affine = name in ("Rotate", "ShearX", "TranslateYRel")
            assert rec.log == extra + (["choice"] if affine and interpolation == "random" else []), (name, interpolation, rec.log)
    # a whole draw: per sample the op choice (numpy), then per op the coin, the magnitude, the sign where the op has one, the filter
    signed = {"Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "ColorIncreasing", "ContrastIncreasing",
              "BrightnessIncreasing", "SharpnessIncreasing"}
    for config, interpolation in (("rand-m9-mstd0.5-inc1", "random"), ("rand-m9-mstd0.5-inc1", "bicubic"), ("rand-m9-mstd0-inc1", "random")):
        rec = Recorder(6)
        table = RandAugment(config, size=16, interpolation=interpolation, rng=rec, np_rng=np.random.RandomState(0)).draw(40)
        nr, want = np.random.RandomState(0), []
        for b in range(40):
            for k, i in enumerate(nr.choice(15, 2)):
                name = RAND_INCREASING_TRANSFORMS[i]
                want.append("random")
                if table[b, k]["op"] == E.IDENTITY:                               # (at magnitude 9 no applied op comes out as identity)
                    continue
                want += ["gauss"] if "mstd0.5" in config else []
                want += ["random"] if name in signed else []
                want += ["choice"] if interpolation == "random" and table[b, k]["op"] == E.AFFINE else []
        assert rec.log == want and rec.log.count("random") > 80
        assert ("gauss" in rec.log) == ("mstd0.5" in config) and ("choice" in rec.log) == (interpolation == "random")


def test_level_functions_at_the_ends():
    def rec_of(config, name, level, seed=0):
        ra = RandAugment(config, size=(20, 40), rng=random.Random(seed))
        t = K.ra_table(1, 1)
        ra.level_to_record(name, level, ra.rng, t[0, 0:1])
        return t[0, 0]
    f32 = np.float32
    for name in ("Color", "Contrast", "Brightness", "Sharpness"):
        assert [rec_of("rand", name, lv)["factor"] for lv in (0, 9, 10)] == [f32(0.1), f32(0.9 * 1.8 + 0.1), f32(1.0 * 1.8 + 0.1)]
        inc = [float(rec_of("rand-inc1", name + "Increasing", lv, seed=s)["factor"]) for lv in (0, 9, 10) for s in range(6)]
        assert set(inc[:6]) == {1.0} and set(inc[6:12]) == {float(f32(1 + 0.9 * .9)), float(f32(1 - 0.9 * .9))}
        assert set(inc[12:]) == {float(f32(1.9)), float(f32(1.0 - 0.9))}
    assert [int(rec_of("rand", "Posterize", lv)["iarg"]) for lv in (0, 9, 10)] == [0, 3, 4]
    assert [int(rec_of("rand-inc1", "PosterizeIncreasing", lv)["iarg"]) for lv in (0, 9, 10)] == [4, 1, 0]
    assert [int(rec_of("rand", "Solarize", lv)["iarg"]) for lv in (0, 9, 10)] == [0, 230, 256]
    assert [int(rec_of("rand-inc1", "SolarizeIncreasing", lv)["iarg"]) for lv in (0, 9, 10)] == [256, 26, 0]
    assert [int(rec_of("rand", "SolarizeAdd", lv)["iarg"]) for lv in (0, 9, 10)] == [0, 99, 110]
    assert {abs(rec_of("rand", "ShearX", 10, seed=s)["m"][1]) for s in range(4)} == {0.3}
    assert {rec_of("rand", "ShearY", 9, seed=s)["m"][3] for s in range(8)} == {0.9 * 0.3, -(0.9 * 0.3)}
    assert {rec_of("rand", "TranslateXRel", 10, seed=s)["m"][2] for s in range(8)} == {0.45 * 40, -0.45 * 40}
    assert {rec_of("rand", "TranslateYRel", 10, seed=s)["m"][5] for s in range(8)} == {0.45 * 20, -0.45 * 20}
    assert rec_of("rand", "Rotate", 0)["op"] == E.IDENTITY and rec_of("rand", "ShearX", 0)["op"] == E.AFFINE
    got = {tuple(rec_of("rand", "Rotate", 10, seed=s)["m"]) for s in range(8)}
    assert got == {rotate_matrix(30.0, 40, 20), rotate_matrix(-30.0, 40, 20)}


def test_rotate_matrix_is_image_rotates():
    pytest.importorskip("PIL")
    from PIL import Image
    assert rotate_matrix(0.0, 16, 16) is None and rotate_matrix(360.0, 16, 16) is None
    for bad in (90.0, 180.0, -90.0):
        with pytest.raises(NotImplementedError):
            rotate_matrix(bad, 16, 16)
    rs = np.random.RandomState(0)
    for (H, W) in ((16, 16), (20, 36), (33, 17)):
        img = Image.fromarray(rs.randint(0, 256, (H, W, 3)).astype(np.uint8), "RGB")
        for angle in (30.0, -30.0, 27.3, -0.4, 1e-3, -13.7):
            for filt in (2, 3):
                via = img.transform(img.size, Image.AFFINE, rotate_matrix(angle, W, H), resample=filt, fillcolor=(124, 116, 104))
                assert np.array_equal(np.asarray(via), np.asarray(img.rotate(angle, resample=filt, fillcolor=(124, 116, 104))))


def test_check_ra_table_rejections():
    ok = K.ra_table(2, 2)
    ok[0, 0]["op"], ok[0, 0]["filter"], ok[0, 0]["m"] = E.AFFINE, 3, (1, 0, 0, 0, 1, 0)
    ok[1, 1]["op"], ok[1, 1]["iarg"] = E.POSTERIZE, 8
    ints = K.check_ra_table(ok, 2, 2)
    assert ints.dtype == np.int32 and ints.shape == (2, 2, 16) and ints.flags.c_contiguous
    assert ints[0, 0, 0] == E.AFFINE and ints[0, 0, 1] == 3 and ints[1, 1, 2] == 8
    assert ints[0, 0, 4:6].view(np.float64)[0] == 1.0

    def bad(**kw):
        t = ok.copy()
        for f, v in kw.items():
            t[1, 0][f] = v
        with pytest.raises(RuntimeError, match="VR_EINVAL.*sample 1, layer 0"):
            K.check_ra_table(t, 2, 2)
    bad(op=12)
    bad(op=-1)
    bad(op=E.AFFINE, filter=0)
    bad(op=E.AFFINE, filter=3, m=(1, 0, np.nan, 0, 1, 0))
    bad(op=E.AFFINE, filter=2, m=(1, 0, 0, 0, np.inf, 0))
    bad(op=E.POSTERIZE, iarg=9)
    bad(op=E.POSTERIZE, iarg=-1)
    bad(op=E.SOLARIZE, iarg=257)
    bad(op=E.SOLARIZE_ADD, iarg=256)
    bad(op=E.CONTRAST, factor=np.nan)
    bad(op=E.BRIGHTNESS, factor=np.inf)
    with pytest.raises(ValueError):
        K.check_ra_table(ok, 3, 2)
    with pytest.raises(ValueError):
        K.check_ra_table(ok, 2, 1)
    with pytest.raises(ValueError):
        K.check_ra_table(np.zeros((2, 2, 16), np.int32), 2, 2)
    with pytest.raises(ValueError):
        K.check_ra_table(K.ra_table(2, 5), 2)
    for f in ((1, 2), (1, 2, 256), (1.5, 2, 3), (-1, 0, 0)):
        with pytest.raises(ValueError):
            K.ra_fill(f)
    assert K.ra_fill((124, 116, 104)) == 124 | 116 << 8 | 104 << 16 and E.fill_rgb(K.ra_fill((1, 2, 3))) == (1, 2, 3)


def test_crop_loader_without_augment_is_unchanged(monkeypatch):
    """augment=None: the same boxes, the same single resample_u8 call, nothing else; the augment's table is drawn after the boxes."""
    assert list(inspect.signature(data.DeviceCropLoader.__init__).parameters) == ["self", "loader", "transform", "device", "augment"]
    assert inspect.signature(data.DeviceCropLoader.__init__).parameters["augment"].default is None
    calls = []
    monkeypatch.setattr(K, "resample_u8", lambda canvas, table, size, filt: calls.append(("resample", table.clone())) or canvas[:, :, :16, :16])
    monkeypatch.setattr(K, "rand_augment_u8", lambda u8, ops, fill: calls.append(("augment", ops.clone(), fill)) or u8)
    rs = np.random.RandomState(0)
    batches = [data.pad_collate_u8([(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), 1) for h, w in ((21, 30), (33, 18))])
               for _ in range(2)]
    tf = lambda: RandomResizedCrop(16, rng=random.Random(5), generator=torch.Generator().manual_seed(6))   # noqa: E731
    ref = tf()
    out = list(data.DeviceCropLoader(batches, tf(), "cpu"))
    assert [c[0] for c in calls] == ["resample", "resample"] and len(out) == 2
    for (kind, table), (canvas, sizes, labels) in zip(calls, batches):
        assert np.array_equal(table.numpy(), K.check_resample_boxes(ref.draw(sizes), 2, canvas.shape[2], canvas.shape[3], 16))
    del calls[:]
    ref, ref_aug = tf(), RandAugment(size=16, rng=random.Random(7), np_rng=np.random.RandomState(8))
    aug = RandAugment(size=16, rng=random.Random(7), np_rng=np.random.RandomState(8))
    out = list(data.DeviceCropLoader(batches, tf(), "cpu", augment=aug))
    assert [c[0] for c in calls] == ["resample", "augment"] * 2
    for i, (canvas, sizes, labels) in enumerate(batches):
        assert np.array_equal(calls[2 * i][1].numpy(), K.check_resample_boxes(ref.draw(sizes), 2, canvas.shape[2], canvas.shape[3], 16))
        assert np.array_equal(calls[2 * i + 1][1].numpy(), K.check_ra_table(ref_aug.draw(2), 2)) and calls[2 * i + 1][2] == (124, 116, 104)
    with pytest.raises(ValueError):
        data.DeviceCropLoader(batches, tf(), "cpu", augment=RandAugment(size=32))
