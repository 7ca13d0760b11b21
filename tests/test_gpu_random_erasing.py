"""Random erasing on the GPU: vr_random_erase against tests/erase_ref.py's float64 statement of the noise contract (derived bound), and
the three fused uint8 entries -- vr_normalize_u8_erase, vr_token_mix_u8_erase, vr_mixup_u8_erase -- bit for bit against the three
stages they fold together (vr_normalize_u8 -> vr_random_erase -> vr_token_mix / vr_mixup), on hand-set rectangles and on the smallest
shapes that reach every lane form.  Then one epoch on uint8 batches with the erase in the mix against the fp32 run whose batches were
erased beforehand.

The rectangles are all inside their images: that a rectangle outside the image addresses nothing outside the buffers follows from the
indexing code (csrc/mixup.hip: erase_meets / erase_lane only COMPARE a lane's pixel coordinates with a rectangle; every address is
formed from the launch's own B, C, H, W) and is not probed here."""
import random

import numpy as np
import pytest
import torch

import erase_ref
import mixup_ref as R
import recipe
import vitres
from vitres import engine
from vitres import kernels as K
from vitres.losses import SoftTargetCrossEntropy
from vitres.mixup import Mixup
from vitres.optim import FlatAdamW
from vitres.random_erasing import RandomErasing
from vitres.token_mixup import SwitchTokenMix

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN4, STD4 = K.IMAGENET_DEFAULT_MEAN + (0.5,), K.IMAGENET_DEFAULT_STD + (0.25,)
QUIET = type("L", (), {"info": staticmethod(lambda s: None)})
CRIT = SoftTargetCrossEntropy()
MODES = ("pixel", "rand", "const")
SEED, CALL = 2 ** 63 + 5, 2 ** 32 + 7                              # both halves of both 64-bit words in use
K_ = 5
# name: (shape, uint8 pointer 4 bytes past a 16-byte boundary, patch_len, box on the patch grid)
SHAPES = {"v16": ((4, 3, 8, 16), False, 4, (1, 3, 1, 3)),         # 16-pixel lanes
          "v4_width": ((4, 3, 6, 20), False, 2, (0, 1, 1, 2)),    # 4-pixel lanes: W % 16 != 0
          "v4_align": ((4, 3, 8, 32), True, 4, (1, 3, 1, 3)),     # 4-pixel lanes: the pointer
          "c1": ((2, 1, 4, 8), False, 4, (1, 3, 1, 3)),
          "c4": ((4, 4, 5, 12), False, 1, (0, 1, 0, 1))}
_DATA = {}


def norm_of(C):
    return MEAN4[:C], STD4[:C]


def data(shape):
    """Per shape, made once and never written: (uint8 batch, its normalised fp32 batch)."""
    if shape not in _DATA:
        g = torch.Generator().manual_seed(8000 + shape[0] * shape[3])
        u = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        u[:, :, 0, 0] = 0
        u[:, :, -1, -1] = 255
        _DATA[shape] = (u, R.normalized(u, *norm_of(shape[1])))
    return _DATA[shape]


def sample_rows(H, W):
    """Hand-set rectangle rows (R = 3) of one sample each."""
    E = (0, 0, 0, 0)
    return [[(2, 2, 3, 3), (1, 2, 5, 6), E],                      # an empty one, a single pixel
            [(0, H - 1, 0, W - 1), E, E],                         # all but the last row and column
            [(1, 3, 1, 7), (H - 2, H, W - 3, W), E],              # straddles quads; touches the last row and column
            [(0, 3, 0, 6), (1, 4, 2, 8), (2, H, 1, 5)]]           # three overlapping


def tables(shape):
    """Rectangle tables [B, 3, 4] that between them give every row to a sample (and, rotated, to another sample)."""
    B, _, H, W = shape
    rows = sample_rows(H, W)
    out = []
    for shift in range(0, 4, 1 if B < 4 else 2):
        out.append(np.array([rows[(b + shift) % 4] for b in range(B)], dtype=np.int32))
    for t in out:
        K.check_erase_rects(t, B, H, W)
    return out


def erase_for(table, mode, seed=SEED, call=CALL):
    return K.erase_args(table, mode, seed, call)


def canaried(shape, lead=64):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * lead,), -12345.0, device=DEV)
    return whole[lead:lead + n].view(shape), whole, lead, lead + n


def canary_intact(whole, lo, hi):
    return bool((whole[:lo] == -12345.0).all()) and bool((whole[hi:] == -12345.0).all())


def on_device_u8(u8, off16):
    if not off16:
        x = u8.to(DEV)
        assert x.data_ptr() % 16 == 0
        return x
    big = torch.zeros(u8.numel() + 64, dtype=torch.uint8, device=DEV)
    view = big[4:4 + u8.numel()].view(u8.shape)
    view.copy_(u8)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def inside_mask(table, shape):
    """bool [B, C, H, W]: the elements some rectangle of their sample covers."""
    m = torch.zeros(shape, dtype=torch.bool)
    for b in range(shape[0]):
        for y0, y1, x0, x1 in table[b]:
            m[b, :, y0:y1, x0:x1] = True
    return m


def staged(x8, table, mode, norm, seed=SEED, call=CALL):
    """Stages one and two on the device: vr_normalize_u8, then vr_random_erase in place, with canaries around the batch."""
    xf, whole, lo, hi = canaried(tuple(x8.shape))
    K.normalize_u8(x8, *norm, out=xf)
    K.random_erase(xf, erase_for(table, mode, seed, call))
    assert canary_intact(whole, lo, hi)
    return xf


# ---- 1: the normaliser -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_normalize_u8_erase_equals_normalize_then_erase(name, mode):
    shape, off16, _, _ = SHAPES[name]
    u8, xf = data(shape)
    norm = norm_of(shape[1])
    x8 = on_device_u8(u8, off16)
    plain = K.normalize_u8(x8, *norm)
    assert same_bits(plain.cpu(), xf)
    for table in tables(shape):
        out, whole, lo, hi = canaried(shape)
        got = K.normalize_u8_erase(x8, *norm, erase_for(table, mode), out=out)
        assert got.data_ptr() == out.data_ptr() and canary_intact(whole, lo, hi) and torch.equal(x8.cpu(), u8)
        assert same_bits(got, staged(x8, table, mode, norm)), "fused differs from normalise -> erase"
        m = inside_mask(table, shape).to(DEV)
        assert bool(torch.equal(bits(got)[~m], bits(plain)[~m])), "changed a pixel outside every rectangle"
        assert m.any() and not bool(torch.equal(bits(got)[m], bits(plain)[m]))


# ---- 2, 3: the mixes ---------------------------------------------------------------------------------------------------------------------
def token_draw(shape, box):
    B = shape[0]
    h = B // 2
    partner = torch.cat([torch.roll(torch.arange(h), 1), torch.roll(torch.arange(B - h), 1) + h])
    return dict(half=h, partner=partner, box=box, lam_patch=0.625, lam_img=0.37)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_token_mix_u8_erase_equals_the_three_stages(name, mode):
    shape, off16, pl, box = SHAPES[name]
    B, C = shape[:2]
    u8, _ = data(shape)
    norm = norm_of(C)
    x8 = on_device_u8(u8, off16)
    y = ((torch.arange(B) * 3 + 1) % K_).to(DEV)
    d = token_draw(shape, box)
    assert d["half"] >= 1 and B - d["half"] >= 1                  # a box half and an image half in every launch
    x0, t0, pt0, _ = SwitchTokenMix(pl, num_classes=K_, input_norm=norm)(x8, y, draw=d)        # the no-erase entry
    for table in tables(shape):
        ea = erase_for(table, mode)
        out, whole, lo, hi = canaried(shape)
        t_out, t_whole, t_lo, t_hi = canaried((B, K_))
        pt_out, pt_whole, pt_lo, pt_hi = canaried((B, pl * pl, K_))
        xs, t, pt, pot = SwitchTokenMix(pl, num_classes=K_, input_norm=norm)(x8, y, draw=dict(d, erase=ea), out=out, targets_out=t_out,
                                                                             patch_targets_out=pt_out)
        assert pot == "seq" and xs.data_ptr() == out.data_ptr() and torch.equal(x8.cpu(), u8)
        assert canary_intact(whole, lo, hi) and canary_intact(t_whole, t_lo, t_hi) and canary_intact(pt_whole, pt_lo, pt_hi)
        x3, t3, pt3, _ = SwitchTokenMix(pl, num_classes=K_)(staged(x8, table, mode, norm), y, draw=d)
        assert same_bits(xs, x3), "fused differs from normalise -> erase -> vr_token_mix"
        assert same_bits(t, t3) and same_bits(pt, pt3) and same_bits(t, t0) and same_bits(pt, pt0)
        m = inside_mask(table, shape)
        m = (m | m[d["partner"]]).to(DEV)                         # a pixel can only change under the own or the partner's rectangles
        assert bool(torch.equal(bits(xs)[~m], bits(x0)[~m])), "changed a pixel outside every rectangle"
        assert not same_bits(xs, x0)
        # the fp32 form of the class: a copy is erased, the caller's batch keeps its bits
        xf = K.normalize_u8(x8, *norm)
        keep = xf.clone()
        x4, t4, pt4, _ = SwitchTokenMix(pl, num_classes=K_)(xf, y, draw=dict(d, erase=ea))
        assert same_bits(x4, xs) and same_bits(t4, t) and same_bits(pt4, pt) and same_bits(xf, keep)


def mixup_draws(shape):
    """elem-mode draws whose samples are a cutmix, a blend, an untouched one (lam == 1) and a cutmix with another box."""
    B, _, H, W = shape
    kinds = [("cut", (1, 3, 2, 7)), ("blend", 0.6), ("same", 1.), ("cut", (0, H, W - 5, W))]
    out = []
    for shift in range(0, 4, 1 if B < 4 else 2):
        pick = [kinds[(i + shift) % 4] for i in range(B)]
        lam = [1. - (v[1] - v[0]) * (v[3] - v[2]) / float(H * W) if k == "cut" else v for k, v in pick]
        out.append(dict(mode='elem', lam=np.array(lam, dtype=np.float32), cutmix=np.array([k == "cut" for k, _ in pick]),
                        box=[v if k == "cut" else None for k, v in pick]))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mixup_u8_erase_equals_the_three_stages(name, mode):
    shape, off16, _, _ = SHAPES[name]
    B, C = shape[:2]
    u8, _ = data(shape)
    norm = norm_of(C)
    x8 = on_device_u8(u8, off16)
    y = ((torch.arange(B) * 3 + 1) % K_).to(DEV)
    flip = torch.arange(B - 1, -1, -1)
    copies = 0
    for d, table in zip(mixup_draws(shape), tables(shape)):
        ea = erase_for(table, mode)
        x0, t0 = Mixup(num_classes=K_, input_norm=norm)(x8, y, draw=d)                       # the no-erase entry
        out, whole, lo, hi = canaried(shape)
        t_out, t_whole, t_lo, t_hi = canaried((B, K_))
        xs, t = Mixup(num_classes=K_, input_norm=norm)(x8, y, draw=dict(d, erase=ea), out=out, targets_out=t_out)
        assert xs.data_ptr() == out.data_ptr() and torch.equal(x8.cpu(), u8)
        assert canary_intact(whole, lo, hi) and canary_intact(t_whole, t_lo, t_hi)
        x3, t3 = Mixup(num_classes=K_)(staged(x8, table, mode, norm), y, draw=d)
        assert same_bits(xs, x3), "fused differs from normalise -> erase -> vr_mixup"
        assert same_bits(t, t3) and same_bits(t, t0)
        m = inside_mask(table, shape)
        untouched = [i for i in range(B) if not d["cutmix"][i] and d["lam"][i] == 1.]
        for i in untouched:                                       # the lam == 1 copy carries the sample's own erase, nothing of the partner
            assert same_bits(xs[i], staged(x8, table, mode, norm)[i])
            assert bool(torch.equal(bits(xs[i])[~m[i].to(DEV)], bits(x0[i])[~m[i].to(DEV)]))
        copies += len(untouched)
        m = (m | m[flip]).to(DEV)
        assert bool(torch.equal(bits(xs)[~m], bits(x0)[~m])), "changed a pixel outside every rectangle"
        assert not same_bits(xs, x0)
        xf = K.normalize_u8(x8, *norm)
        keep = xf.clone()
        x4, t4 = Mixup(num_classes=K_)(xf, y, draw=dict(d, erase=ea))                        # the fp32 form: erases a copy
        assert same_bits(x4, xs) and same_bits(t4, t) and same_bits(xf, keep)
    assert copies >= 1


# ---- 4: the noise against the float64 contract ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_random_erase_meets_the_contract_within_the_derived_bound(name):
    shape, _, _, _ = SHAPES[name]
    B, C, H, W = shape
    _, xf = data(shape)
    worst = 0.
    for table in tables(shape):
        for mode in MODES:
            x, whole, lo, hi = canaried(shape)
            x.copy_(xf)
            assert K.random_erase(x, erase_for(table, mode)) is x and canary_intact(whole, lo, hi)
            got = x.cpu()
            want, inside, bound = erase_ref.erase(xf.numpy(), table, mode, SEED, CALL)
            inside_t = torch.from_numpy(inside)
            assert bool(torch.equal(bits(got)[~inside_t], bits(xf)[~inside_t])), "changed a pixel outside every rectangle"
            err = np.abs(got.numpy().astype(np.float64) - want)
            assert inside.any() and (err[~inside] == 0).all()
            if mode == "const":
                assert bool((bits(got)[inside_t] == 0).all())     # +0.0, not -0.0
                continue
            ratio = float((err[inside] / bound[inside]).max())
            worst = max(worst, ratio)
            assert (err <= bound).all(), "%s %s: %.3g of the bound (largest error %.3g)" % (name, mode, ratio, err.max())
            assert np.abs(got.numpy()[inside]).max() < 5.77
            if mode == "rand":
                for b in range(B):
                    owner = np.full((H, W), -1)
                    for r, (y0, y1, x0, x1) in enumerate(table[b]):
                        owner[y0:y1, x0:x1] = r                   # the later rectangle wins
                    for r in range(table.shape[1]):
                        sel = torch.from_numpy(owner == r)
                        for c in range(C):
                            vals = bits(got[b, c])[sel]
                            assert vals.numel() == 0 or bool((vals == vals[0]).all()), "a rectangle's colour varies"
                            if vals.numel():
                                colour, bd = erase_ref.rect_colours(SEED, CALL, b, r)
                                assert abs(float(got[b, c][sel][0]) - colour[c]) <= bd[c]
    print("%s: largest error / bound = %.3f" % (name, worst))


# ---- 5: one function of (seed, call, b, c, y, x) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pixel", "rand"])
def test_noise_does_not_depend_on_the_lane_form_and_follows_seed_and_call(mode):
    shape, _, pl, box = SHAPES["v4_align"]                        # W = 32: 16-pixel lanes on an aligned pointer, 4-pixel lanes off one
    B, C = shape[:2]
    u8, _ = data(shape)
    norm = norm_of(C)
    wide, narrow = on_device_u8(u8, False), on_device_u8(u8, True)
    y = ((torch.arange(B) * 3 + 1) % K_).to(DEV)
    table = tables(shape)[1]
    ea = erase_for(table, mode)
    m = inside_mask(table, shape).to(DEV)
    ref = K.normalize_u8_erase(wide, *norm, ea)
    assert same_bits(ref, K.normalize_u8_erase(narrow, *norm, ea)) and same_bits(ref, K.normalize_u8_erase(wide, *norm, ea))
    d = token_draw(shape, box)
    mix = SwitchTokenMix(pl, num_classes=K_, input_norm=norm)
    assert same_bits(mix(wide, y, draw=dict(d, erase=ea))[0], mix(narrow, y, draw=dict(d, erase=ea))[0])
    md = mixup_draws(shape)[0]
    mixup = Mixup(num_classes=K_, input_norm=norm)
    assert same_bits(mixup(wide, y, draw=dict(md, erase=ea))[0], mixup(narrow, y, draw=dict(md, erase=ea))[0])
    for other in (erase_for(table, mode, call=CALL + 1), erase_for(table, mode, seed=SEED + 1), erase_for(table, mode, seed=SEED ^ (1 << 40)),
                  erase_for(table, mode, call=CALL ^ (1 << 40))):
        got = K.normalize_u8_erase(wide, *norm, other)
        assert bool(torch.equal(bits(got)[~m], bits(ref)[~m]))
        changed = (bits(got)[m] != bits(ref)[m]).float().mean()
        assert float(changed) > 0.99, float(changed)              # every erased element moved (equal fp32 draws are ~2^-24 events)


def test_rejections_leave_the_buffers_as_they_were():
    shape = SHAPES["v16"][0]
    u8, xf = data(shape)
    x8, norm = u8.to(DEV), norm_of(3)
    table = tables(shape)[0]
    out = torch.full(shape, 9.0, device=DEV)
    bad = table.copy()
    bad[1, 0] = (0, 9, 0, 4)
    with pytest.raises(RuntimeError, match="VR_EINVAL.*sample 1"):
        K.normalize_u8_erase(x8, *norm, erase_for(bad, "pixel"), out=out)
    with pytest.raises(ValueError, match="table"):
        K.normalize_u8_erase(x8, *norm, erase_for(table[:3], "pixel"), out=out)
    x = xf.to(DEV)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):
        K.random_erase(x, erase_for(bad, "pixel"))
    whole = torch.full((x.numel() + 8,), 9.0, device=DEV)
    with pytest.raises(RuntimeError, match="VR_EALIGN"):
        K.random_erase(whole[1:1 + x.numel()].view(shape), erase_for(table, "pixel"))
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and bool((whole == 9.0).all()) and same_bits(x.cpu(), xf)


# ---- 6: training, end to end --------------------------------------------------------------------------------------------------------------
class RecordingMixup(Mixup):
    """A Mixup that remembers, per call, its draw, its erase arguments and return values and -- before the next call and after the
    epoch -- the captured step's static inputs as the step that consumed the mix left them."""

    def __init__(self, fast, *a, **kw):
        super().__init__(*a, **kw)
        self.fast, self.calls, self._open = fast, [], None

    def draw(self, batch, hw=(224, 224)):
        self._d = super().draw(batch, hw)
        return self._d

    def __call__(self, x, target, **kw):
        self.close()
        ret = super().__call__(x, target, **kw)
        self._open = dict(d=self._d, erase=self.last_erase, into=kw.get("out") is not None, mixed=[r.clone() for r in ret])
        return ret

    def close(self):
        c, self._open = self._open, None
        if c is None:
            return
        torch.cuda.synchronize()
        if self.fast is not None:
            step = self.fast.steps[-1]
            c["static"] = [step.x.clone(), step.t.clone()]
        self.calls.append(c)


def supernet(dtype):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0, **kw)
    m.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 100))
    return m.to(DEV).set_compute_dtype(dtype)


_TRAIN = []
NORM3 = norm_of(3)


def train_data():
    if not _TRAIN:
        S = recipe.MICRO_IMG
        for i in range(4):
            g = torch.Generator().manual_seed(9100 + i)
            _TRAIN.append((torch.randint(0, 256, (8, 3, S, S), dtype=torch.uint8, generator=g),
                           (torch.arange(8) * (i + 1) + i) % recipe.MICRO_CLASSES))
    return _TRAIN


def new_erasing():
    return RandomErasing(probability=1, seed=SEED, rng=random.Random(0))


def run_epoch(dtype, use_fast, use_u8):
    torch.manual_seed(2024)
    np.random.seed(2024)
    m = supernet(dtype)
    opt = FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=2e-3)
    m.train()
    m.set_epoch(31)
    fp = engine.FastPath() if use_fast else None
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=recipe.MICRO_CLASSES)
    if use_u8:
        mix = RecordingMixup(fp, input_norm=NORM3, erase=new_erasing(), **kw)
        loader = [(u8.to(DEV), y.to(DEV)) for u8, y in train_data()]
    else:                                                         # normalised and erased beforehand: the same tables, seed and calls
        mix, er, loader = RecordingMixup(fp, **kw), new_erasing(), []
        for u8, y in train_data():
            loader.append((er(K.normalize_u8(u8.to(DEV), *NORM3)), y.to(DEV)))
        assert er.call == 4
    stats = engine.train_one_epoch(m, CRIT, loader, opt, DEV, 31, mixup_fn=mix, print_freq=0, logger=QUIET, fast=fp, arch_sample="multi")
    mix.close()
    torch.cuda.synchronize()
    return stats, mix.calls, m._arena["flat"].clone(), fp


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


@pytest.mark.parametrize("use_fast", [True, False], ids=["fast", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_training_on_uint8_batches_with_erase_follows_the_pre_erased_fp32_run(dtype, use_fast):
    """The inputs of the two runs are bit-identical (checked per step against the three stages run here); the bands on the loss and the
    parameters are those of test_training_on_uint8_batches_through_mixup_follows_the_fp32_run (tests/test_gpu_mixup.py)."""
    s8, c8, p8, fp8 = run_epoch(dtype, use_fast, True)
    sf, cf, pf, _ = run_epoch(dtype, use_fast, False)
    assert len(c8) == len(cf) == 4
    for i, (a, b, (u8, y)) in enumerate(zip(c8, cf, train_data())):
        assert a["d"] == b["d"] and b["erase"] is None, i
        ea = a["erase"]
        assert (ea["seed"], ea["call"], ea["mode"]) == (SEED, i, "pixel") and bool((ea["rects"][:, 0, 0] < ea["rects"][:, 0, 1]).all())
        want = Mixup(num_classes=recipe.MICRO_CLASSES)(staged(u8.to(DEV), ea["rects"], "pixel", NORM3, SEED, i), y.to(DEV), draw=a["d"])
        for run in (a, b):
            assert all(same_bits(g, w) for g, w in zip(run["mixed"], want)), i
            if use_fast:                                          # what the captured step read
                assert all(same_bits(g, w) for g, w in zip(run["static"], want)), i
                assert run["into"] == (i > 0)                     # from the second batch on the mix wrote into the step's own buffers
    if use_fast:
        assert len(fp8.steps) == 1
    print("loss u8+erase %r pre-erased fp32 %r parameters rel %r" % (s8["loss"], sf["loss"], rel(p8, pf)))
    assert abs(s8["loss"] - sf["loss"]) < (1e-5 if dtype == torch.float32 else 2e-2) * abs(sf["loss"])
    assert rel(p8, pf) < 2e-3
