"""vr_mixup / vr_mixup_u8 and vitres.mixup.Mixup on the GPU against timm's statements restated in tests/mixup_ref.py, on hand-written
draws: every comparison is bit for bit (two rounded products and one rounded add per element; the uint8 normaliser is bit-exact
already).  Then the class on seeded draws, and train_one_epoch mixing uint8 batches straight into the captured step's static inputs."""
import numpy as np
import pytest
import torch

import mixup_ref as R
import recipe
import vitres
from vitres import engine
from vitres import kernels as K
from vitres.losses import SoftTargetCrossEntropy
from vitres.mixup import Mixup
from vitres.optim import FlatAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = K.IMAGENET_DEFAULT_MEAN, K.IMAGENET_DEFAULT_STD
QUIET = type("L", (), {"info": staticmethod(lambda s: None)})
CRIT = SoftTargetCrossEntropy()
SHAPES = {"2x8": (2, 3, 8, 8),                                    # the smallest: 4-pixel lanes, one workgroup
          "4x20": (4, 3, 20, 20),                                 # W % 16 != 0
          "6x32": (6, 3, 32, 32),                                 # 16-pixel lanes
          "4x48_off16": (4, 3, 48, 48),                           # a wide row whose uint8 pointer is 4 bytes off 16: the 4-pixel form
          "4x224": (4, 3, 224, 224)}
_DATA = {}


def data(shape):
    """Per shape, made once and never written: (uint8 batch, its normalised fp32 batch): 0 and 255 in every channel, a constant sample."""
    if shape not in _DATA:
        g = torch.Generator().manual_seed(7000 + shape[0] * shape[3])
        u = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        u[:, :, 0, 0] = 0
        u[:, :, -1, -1] = 255
        u[-1] = 77
        _DATA[shape] = (u, R.normalized(u, MEAN, STD))
    return _DATA[shape]


def labels_for(B, K_):
    """Sample 0 and its partner B-1 share a label, the other pairs (B > 2) do not."""
    y = (torch.arange(B) * 3 + 1) % K_
    y[B - 1] = y[0]
    return y


def canaried(shape, lead=64):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * lead,), -12345.0, device=DEV)
    return whole[lead:lead + n].view(shape), whole, lead, lead + n


def canary_intact(whole, lo, hi):
    return bool((whole[:lo] == -12345.0).all()) and bool((whole[hi:] == -12345.0).all())


def on_device_u8(u8, off16):
    """The batch on the device; off16: as a contiguous view 4 bytes past a 16-byte boundary."""
    if not off16:
        return u8.to(DEV)
    big = torch.zeros(u8.numel() + 64, dtype=torch.uint8, device=DEV)
    view = big[4:4 + u8.numel()].view(u8.shape)
    view.copy_(u8)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def check_case(shape, draw, K_=5, off16=False):
    """One draw on one shape: the fp32 form against timm's statements, then the uint8 form against the same reference and against
    vr_normalize_u8 followed by vr_mixup."""
    u8, xf = data(shape)
    y = labels_for(shape[0], K_)
    ref_x, ref_t = R.mix(xf, y, draw, K_, 0.1)
    x_dev, y_dev = xf.to(DEV), y.to(DEV)
    out, whole, lo, hi = canaried(shape)
    got_x, got_t = Mixup(num_classes=K_)(x_dev, y_dev, draw=draw, out=out)
    assert got_x.data_ptr() == out.data_ptr()
    assert R.bits_equal(got_x, ref_x), "fp32 samples differ from timm's statements"
    assert R.bits_equal(got_t, ref_t), "fp32 targets differ from timm's statements"
    assert canary_intact(whole, lo, hi) and torch.equal(x_dev.cpu(), xf), "wrote outside out, or into the input"
    x8 = on_device_u8(u8, off16)
    out8, whole8, lo8, hi8 = canaried(shape)
    got8_x, got8_t = Mixup(num_classes=K_, input_norm=(MEAN, STD))(x8, y_dev, draw=draw, out=out8)
    assert R.bits_equal(got8_x, ref_x), "uint8 samples differ from timm's statements on the normalised batch"
    assert R.bits_equal(got8_t, ref_t), "uint8 targets differ"
    assert canary_intact(whole8, lo8, hi8) and torch.equal(x8.cpu(), u8)
    two_x, two_t = Mixup(num_classes=K_)(K.normalize_u8(x8, MEAN, STD), y_dev, draw=draw)       # the two-pass path on the device
    assert torch.equal(got8_x.view(torch.int32), two_x.view(torch.int32)) and torch.equal(got8_t.view(torch.int32), two_t.view(torch.int32))


def boxes(S):
    """Pixel boxes (y0, y1, x0, x1) on an S x S image whose edges fall every way a 4- or 16-pixel lane can meet them."""
    wide = S >= 32
    out = {"empty": (2, 2, 3, 3), "empty_rows_only": (4, 4, 0, S), "empty_cols_only": (0, S, 5, 5), "whole": (0, S, 0, S),
           "one_pixel": (5, 6, 5, 6), "all_but_edge_columns": (0, S, 1, S - 1),
           "inside_one_lane": (1, 4, 17, 23) if wide else (1, 4, 5, 7),
           "straddles_a_lane_boundary": (2, 7, 14, 18) if S >= 20 else (2, 7, 3, 5),
           "spans_lanes": (1, S - 1, 3, S - 3),
           "top": (0, 2, 2, 7), "bottom": (S - 2, S, 1, 6), "left": (3, 6, 0, 3), "right": (2, 5, S - 3, S),
           "top_left_pixel": (0, 1, 0, 1), "bottom_right_pixel": (S - 1, S, S - 1, S)}
    if wide:
        out["lane_aligned"] = (3, 9, 16, 32)
        out["one_off_lane_aligned"] = (3, 9, 15, 33 if S > 32 else 32)
    assert all(0 <= a <= b <= S and 0 <= c <= d <= S for a, b, c, d in out.values())
    return out


def cut_lam(box, S):
    return 1. - (box[1] - box[0]) * (box[3] - box[2]) / float(S * S)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_batch_wide_boxes_are_bit_exact(name):
    shape = SHAPES[name]
    S = shape[2]
    for bname, box in boxes(S).items():
        try:
            check_case(shape, dict(mode='batch', lam=cut_lam(box, S), cutmix=True, box=box), off16=name.endswith("off16"))
        except AssertionError as e:
            raise AssertionError("%s %s %s: %s" % (name, bname, box, e))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_per_sample_boxes_are_bit_exact(name):
    """elem-mode tables: every sample of a launch its own box (B boxes per table, all the boxes over a few tables)."""
    shape = SHAPES[name]
    B, S = shape[0], shape[2]
    todo = list(boxes(S).items())
    while len(todo) % B:
        todo.append(todo[len(todo) % 3])
    for k in range(0, len(todo), B):
        chunk = todo[k:k + B]
        d = dict(mode='elem', lam=np.array([cut_lam(b, S) for _, b in chunk], dtype=np.float32), cutmix=np.ones(B, dtype=bool),
                 box=[b for _, b in chunk])
        try:
            check_case(shape, d, off16=name.endswith("off16"))
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (name, [n for n, _ in chunk], e))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_blends_and_mixed_tables_are_bit_exact(name):
    """Batch-wide blends (lam = 0.6 is where the two roundings of 1 - lam part), the untouched batch, and elem / pair tables that
    hold cutmix, blend and identity samples in one launch."""
    shape = SHAPES[name]
    B, S = shape[0], shape[2]
    off16 = name.endswith("off16")
    bx = boxes(S)
    assert np.float32(0.99999999) == 1 and np.float32(1. - 0.99999999) != 0      # timm blends this one: its lam != 1. is on the double
    for lam in (0.6, 0.37, 0., 0.9999999, 0.99999999):
        check_case(shape, dict(mode='batch', lam=lam, cutmix=False, box=None), off16=off16)
    check_case(shape, dict(mode='batch', lam=1., cutmix=False, box=None), off16=off16)
    check_case(shape, dict(mode='batch', lam=1., cutmix=True, box=None), off16=off16)          # Beta returned exactly 1: no box drawn
    kinds = [("cut", bx["straddles_a_lane_boundary"]), ("blend", 0.6), ("same", 1.), ("cut", bx["one_pixel"]), ("blend", 0.37),
             ("cut", bx["empty"])]
    for mode, n in (("elem", B), ("pair", B // 2)):
        for shift in range(3):
            pick = [kinds[(i + shift) % len(kinds)] for i in range(n)]
            d = dict(mode=mode, lam=np.array([cut_lam(v, S) if k == "cut" else v for k, v in pick], dtype=np.float32),
                     cutmix=np.array([k == "cut" for k, _ in pick]), box=[v if k == "cut" else None for k, v in pick])
            check_case(shape, d, off16=off16)
            if mode == "pair":
                rows = vitres.mixup.param_table(d, B)
                assert all(rows[i] == rows[B - 1 - i] for i in range(B))


@pytest.mark.parametrize("K_", [5, 1000])
def test_targets(K_):
    """Smoothed one-hots blended per sample: a pair with equal labels and pairs with different ones, K below and above one
    workgroup's 256 lanes; labels at both ends of the class range."""
    shape = SHAPES["4x20"]
    for lams in ([0.6, 0.25, 1., 0.], [1., 1., 1., 1.], [0.5, 0.5, 0.5, 0.5]):
        d = dict(mode='elem', lam=np.array(lams, dtype=np.float32), cutmix=np.zeros(4, dtype=bool), box=[None] * 4)
        check_case(shape, d, K_=K_)
    check_case(shape, dict(mode='batch', lam=0.6, cutmix=False, box=None), K_=K_)
    _, xf = data(shape)
    y = torch.tensor([0, K_ - 1, K_ - 1, 2])
    d = dict(mode='pair', lam=np.array([0.3, 0.8], dtype=np.float32), cutmix=np.zeros(2, dtype=bool), box=[None] * 2)
    canary, whole, lo, hi = canaried((4, K_))
    _, t = Mixup(num_classes=K_, label_smoothing=0.1)(xf.to(DEV), y.to(DEV), draw=d, targets_out=canary)
    assert R.bits_equal(t, R.mix(xf, y, d, K_, 0.1)[1]) and canary_intact(whole, lo, hi)
    assert abs(float(t.sum()) - 4.) < 1e-4
    _, t0 = Mixup(num_classes=K_, label_smoothing=0.)(xf.to(DEV), y.to(DEV), draw=d)
    assert R.bits_equal(t0, R.mix(xf, y, d, K_, 0.)[1])


def test_untouched_samples_keep_their_bits_and_never_see_the_partner():
    """fp32 inputs: -0.0 survives lam == 1 (x * 1 + xj * 0 would make it +0.0), and an inf in the partner of a lam == 1 sample stays
    out of it (inf * 0 would be NaN)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 8, 8, generator=g)
    x[:, :, 0, :5] = -0.0
    x[3, 1, 4, 4] = float("inf")                                  # sample 3 is sample 0's partner
    x[1, 0, 2, 2] = float("-inf")                                 # sample 1 is sample 2's
    y = torch.tensor([1, 2, 3, 4])
    assert bool((x.view(torch.int32) == -2 ** 31).any())
    d = dict(mode='elem', lam=np.array([1., 0.37, 1., 0.6], dtype=np.float32), cutmix=np.zeros(4, dtype=bool), box=[None] * 4)
    got, t = Mixup(num_classes=5)(x.to(DEV), y.to(DEV), draw=d)
    ref_x, ref_t = R.mix(x, y, d, 5, 0.1)
    assert R.bits_equal(got, ref_x) and R.bits_equal(t, ref_t)
    assert R.bits_equal(got[0], x[0]) and R.bits_equal(got[2], x[2])
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all())
    assert not bool(torch.isnan(got).any())
    # the whole batch untouched (batch mode, the probability draw missed), and a cutmix with -0.0 on both sides of the box edge
    for d in (dict(mode='batch', lam=1., cutmix=False, box=None), dict(mode='batch', lam=0.5, cutmix=True, box=(0, 4, 2, 7))):
        got, _ = Mixup(num_classes=5)(x.to(DEV), y.to(DEV), draw=d)
        assert R.bits_equal(got, R.mix(x, y, d, 5, 0.1)[0])
    assert R.bits_equal(Mixup(num_classes=5)(x.to(DEV), y.to(DEV), draw=dict(mode='batch', lam=1., cutmix=False, box=None))[0], x)


def test_rejections_leave_out_as_it_was():
    rows = np.zeros(4, dtype=K.MIXUP_PARAM)
    rows["lam"], rows["oml"] = 0.5, 0.5
    x = data(SHAPES["4x20"])[1].to(DEV)
    y = torch.tensor([1, 2, 3, 4], device=DEV)

    def refused(code, x_, y_, rows_, out_, kind=RuntimeError):
        t_out = torch.full((x_.shape[0], 5), 9.0, device=DEV)
        with pytest.raises(kind, match=code):
            K.mixup(x_, y_, rows_, 5, 0.9, 0.02, out=out_, targets_out=t_out)
        torch.cuda.synchronize()
        assert bool((t_out == 9.0).all())

    out = torch.full((3, 3, 20, 20), 9.0, device=DEV)             # an odd batch
    refused("VR_EUNSUPPORTED", x[:3], y[:3], rows[:3], out)
    assert bool((out == 9.0).all())
    x6 = torch.zeros(4, 3, 8, 6, device=DEV)                      # W % 4
    out = torch.full((4, 3, 8, 6), 9.0, device=DEV)
    refused("VR_EUNSUPPORTED", x6, y, rows, out)
    assert bool((out == 9.0).all())
    keep = x.clone()                                              # samples == out
    refused("VR_EUNSUPPORTED", x, y, rows, x)
    assert torch.equal(x, keep)
    whole = torch.full((x.numel() + 8,), 9.0, device=DEV)         # out 4 bytes off a 16-byte boundary
    refused("VR_EALIGN", x, y, rows, whole[1:1 + x.numel()].view(x.shape))
    assert bool((whole == 9.0).all())
    out = torch.full(tuple(x.shape), 9.0, device=DEV)             # a box past the image
    for field, value in (("y1", 21), ("x1", 21), ("x0", -1)):
        bad = rows.copy()
        bad["cutmix"] = 1
        bad[field][3] = value
        refused("VR_EINVAL", x, y, bad, out)
    u8 = data(SHAPES["4x20"])[0].to(DEV)
    norm = K.norm_constants(MEAN, STD)
    for x_, rows_, code in ((u8[:3], rows[:3], "VR_EUNSUPPORTED"), (u8, rows[:2], "table")):
        with pytest.raises((RuntimeError, ValueError), match=code):
            K.mixup(x_, y[:x_.shape[0]], rows_, 5, 0.9, 0.02, norm=norm, out=out[:x_.shape[0]])
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())


@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_seeded_class_equals_timms_statements_on_the_same_draws(mode):
    shape, K_ = SHAPES["6x32"], 10
    B, S = shape[0], shape[2]
    u8, xf = data(shape)
    y = labels_for(B, K_)
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=K_)
    kinds = set()
    for seed in range(4):
        np.random.seed(seed)
        d = Mixup(**kw).draw(B, (S, S))
        after = np.random.randint(0, 1 << 30)
        ref_x, ref_t = R.mix(xf, y, d, K_, 0.1)
        kinds |= {"cut" if b is not None else "blend" for b in (d["box"] if mode != "batch" else [d["box"]])}
        outs = [torch.full(shape, 9.0, device=DEV), torch.full((B, K_), 9.0, device=DEV)]
        for norm, x, bufs in ((None, xf, None), ((MEAN, STD), u8, None), (None, xf, outs), ((MEAN, STD), u8, outs)):
            np.random.seed(seed)
            extra = {} if bufs is None else dict(out=bufs[0], targets_out=bufs[1])
            got_x, got_t = Mixup(input_norm=norm, **kw)(x.to(DEV), y.to(DEV), **extra)
            assert np.random.randint(0, 1 << 30) == after         # drew exactly what draw() draws
            assert R.bits_equal(got_x, ref_x) and R.bits_equal(got_t, ref_t), (mode, seed, norm is not None)
            if bufs is not None:
                assert got_x.data_ptr() == bufs[0].data_ptr() and got_t.data_ptr() == bufs[1].data_ptr()
    assert kinds == {"cut", "blend"}                              # the seeds reach both mixes


# ---- training, end to end -------------------------------------------------------------------------------------------------------
class RecordingMixup(Mixup):
    """A Mixup that remembers, per call, its draw and return values and -- before the next call and after the epoch -- the captured
    step's static inputs as the step that consumed the mix left them."""

    def __init__(self, fast, *a, **kw):
        super().__init__(*a, **kw)
        self.fast, self.calls, self._open = fast, [], None

    def draw(self, batch, hw=(224, 224)):
        self._d = super().draw(batch, hw)
        return self._d

    def __call__(self, x, target, **kw):
        self.close()
        ret = super().__call__(x, target, **kw)
        self._open = dict(d=self._d, into=kw.get("out") is not None and kw.get("targets_out") is not None,
                          ptrs=[r.data_ptr() for r in ret], mixed=[r.clone() for r in ret])
        return ret

    def close(self):
        c, self._open = self._open, None
        if c is None:
            return
        torch.cuda.synchronize()
        if self.fast is not None:
            step = self.fast.steps[-1]
            assert step.pt is None
            c["static"] = [step.x.clone(), step.t.clone()]
            c["static_ptrs"] = [step.x.data_ptr(), step.t.data_ptr()]
        self.calls.append(c)


def supernet(dtype):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0, **kw)
    m.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 100))
    return m.to(DEV).set_compute_dtype(dtype)


_TRAIN = []


def train_data():
    if not _TRAIN:
        S = recipe.MICRO_IMG
        for i in range(4):
            g = torch.Generator().manual_seed(9000 + i)
            u8 = torch.randint(0, 256, (8, 3, S, S), dtype=torch.uint8, generator=g)
            _TRAIN.append((u8, R.normalized(u8, MEAN, STD), (torch.arange(8) * (i + 1) + i) % recipe.MICRO_CLASSES))
    return _TRAIN


def run_epoch(dtype, use_fast, use_u8):
    torch.manual_seed(2024)
    np.random.seed(2024)
    m = supernet(dtype)
    opt = FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=2e-3)
    m.train()
    m.set_epoch(31)
    fp = engine.FastPath() if use_fast else None
    mix = RecordingMixup(fp, mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=recipe.MICRO_CLASSES,
                         input_norm=(MEAN, STD) if use_u8 else None)
    loader = [((u8 if use_u8 else xf).to(DEV), y.to(DEV)) for u8, xf, y in train_data()]
    stats = engine.train_one_epoch(m, CRIT, loader, opt, DEV, 31, mixup_fn=mix, print_freq=0, logger=QUIET, fast=fp,
                                   arch_sample="multi")
    mix.close()
    torch.cuda.synchronize()
    return stats, mix.calls, m._arena["flat"].clone(), fp


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


@pytest.mark.parametrize("use_fast", [True, False], ids=["fast", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_training_on_uint8_batches_through_mixup_follows_the_fp32_run(dtype, use_fast):
    """uint8 batches through Mixup(input_norm=) against the torch-normalised fp32 batches through the plain Mixup, same seeds.  The mixed
    inputs are bit-identical (checked against timm's statements); the bands on the loss and the parameters are those
    test_training_on_uint8_batches_follows_the_fp32_run (tests/test_gpu_input_stage.py) uses for two runs of this step."""
    s8, c8, p8, fp8 = run_epoch(dtype, use_fast, True)
    sf, cf, pf, _ = run_epoch(dtype, use_fast, False)
    assert len(c8) == len(cf) == 4
    for i, (a, b, (u8, xf, y)) in enumerate(zip(c8, cf, train_data())):
        assert a["d"] == b["d"], i                                # the same draws
        want = R.mix(xf, y, a["d"], recipe.MICRO_CLASSES, 0.1)
        for run in (a, b):
            assert all(R.bits_equal(g, w) for g, w in zip(run["mixed"], want)), i
            if use_fast:                                          # what the captured step read
                assert all(R.bits_equal(g, w) for g, w in zip(run["static"], want)), i
                # from the second batch on the mix wrote into the step's own buffers: the replay issued no input copy
                assert run["into"] == (i > 0)
                assert (run["ptrs"] == run["static_ptrs"]) == (i > 0)
            else:
                assert not run["into"]
    if use_fast:
        assert len(fp8.steps) == 1
    print("loss u8 %r fp32 %r parameters rel %r" % (s8["loss"], sf["loss"], rel(p8, pf)))
    assert abs(s8["loss"] - sf["loss"]) < (1e-5 if dtype == torch.float32 else 2e-2) * abs(sf["loss"])
    assert rel(p8, pf) < 2e-3


@pytest.mark.parametrize("use_fast", [True, False], ids=["fast", "eager"])
def test_uint8_batch_with_a_mixup_that_does_not_normalise_raises(use_fast):
    m = supernet(torch.float32)
    opt = FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=2e-3)
    u8, _, y = train_data()[0]
    loader = [(u8.to(DEV), y.to(DEV))]
    for mix in (Mixup(num_classes=recipe.MICRO_CLASSES), lambda x, t: (x.float(), t)):
        with pytest.raises(TypeError, match="DevicePrefetchLoader.*Mixup.*input_norm="):
            engine.train_one_epoch(m, CRIT, loader, opt, DEV, 31, mixup_fn=mix, print_freq=0, logger=QUIET,
                                   fast=engine.FastPath() if use_fast else None)
