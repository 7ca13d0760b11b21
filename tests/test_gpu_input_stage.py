"""The uint8 input side on the GPU: vr_normalize_u8 and vr_token_mix_u8 against torch's CPU statement
`(u8.float() - mean) / std` and the oracle's SwitchTokenMix on it -- every comparison bit for bit -- then the loaders of
vitres.data and train_one_epoch mixing uint8 batches straight into the captured step's static inputs."""
import numpy as np
import pytest
import torch

import recipe
import vitres
import vitres_oracle as O
from vitres import data, engine, evo_eval
from vitres import kernels as K
from vitres.losses import SoftTargetCrossEntropy
from vitres.optim import FlatAdamW
from vitres.token_mixup import SwitchTokenMix

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = K.IMAGENET_DEFAULT_MEAN, K.IMAGENET_DEFAULT_STD
MEAN4, STD4 = MEAN + (0.5,), STD + (0.25,)
QUIET = type("L", (), {"info": staticmethod(lambda s: None)})
CRIT = SoftTargetCrossEntropy()
_U8 = {}


def u8_batch(shape, seed=0):
    """Seeded uint8 batch, made once per shape: 0 and 255 forced into every channel, the last sample constant."""
    if (shape, seed) not in _U8:
        g = torch.Generator().manual_seed(1000 + seed)
        u = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        u[:, :, 0, 0] = 0
        u[:, :, -1, -1] = 255
        u[-1] = 77
        _U8[(shape, seed)] = u
    return _U8[(shape, seed)]


def normalized(u8, mean=MEAN, std=STD):
    """timm's PrefetchLoader statement on the CPU, torch fp32."""
    C = u8.shape[1]
    m = torch.tensor([x * 255 for x in mean[:C]]).view(1, C, 1, 1)
    s = torch.tensor([x * 255 for x in std[:C]]).view(1, C, 1, 1)
    return (u8.float() - m) / s


def canaried(shape, lead=64):
    """A fp32 view of `shape` inside a larger buffer filled with a canary value, 16-byte aligned: (view, whole buffer, lo, hi)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * lead,), -12345.0, device=DEV)
    return whole[lead:lead + n].view(shape), whole, lead, lead + n


def canary_intact(whole, lo, hi):
    return bool((whole[:lo] == -12345.0).all()) and bool((whole[hi:] == -12345.0).all())


# ---- vr_normalize_u8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 56, 56),              # W % 16 != 0: the 4-pixel form
                                   (2, 3, 64, 64), (1, 3, 224, 224),      # the 16-pixel form
                                   (3, 1, 8, 16), (2, 4, 4, 32)])        # one and four channels
def test_normalize_u8_is_bit_exact(shape):
    u8 = u8_batch(shape)
    ref = normalized(u8, MEAN4, STD4)
    C = shape[1]
    x = u8.to(DEV)
    out, whole, lo, hi = canaried(shape)
    got = K.normalize_u8(x, MEAN4[:C], STD4[:C], out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), ref) and canary_intact(whole, lo, hi)
    assert torch.equal(K.normalize_u8(x, MEAN4[:C], STD4[:C]).cpu(), ref)       # the allocating form
    assert torch.equal(x.cpu(), u8)


def test_normalize_u8_wide_row_but_pointer_off_16_bytes():
    """W = 64 qualifies for the 16-pixel form, the pointer (4 bytes into its allocation) does not: the 4-pixel form must run."""
    u8 = u8_batch((2, 3, 64, 64))
    big = torch.zeros(u8.numel() + 64, dtype=torch.uint8, device=DEV)
    view = big[4:4 + u8.numel()].view(u8.shape)
    view.copy_(u8)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    out, whole, lo, hi = canaried(u8.shape)
    K.normalize_u8(view, MEAN, STD, out=out)
    assert torch.equal(out.cpu(), normalized(u8)) and canary_intact(whole, lo, hi)
    assert torch.equal(view.cpu(), u8)


def test_normalize_u8_rejects_what_it_does_not_take():
    x = u8_batch((2, 3, 8, 16)).to(DEV)
    with pytest.raises(TypeError):
        K.normalize_u8(x.float(), MEAN, STD)
    with pytest.raises(ValueError):
        K.normalize_u8(x, MEAN4, STD4)                            # four constants, three channels
    with pytest.raises(ValueError):
        K.normalize_u8(x, MEAN, STD, out=torch.empty(2, 3, 8, 16, dtype=torch.float16, device=DEV))
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.normalize_u8(torch.zeros(1, 3, 4, 6, dtype=torch.uint8, device=DEV), MEAN, STD)


# ---- vr_token_mix_u8 ---------------------------------------------------------------------------------------------------------------
def draws(B, pl):
    """Injected draws: (name, box, lam_img, partner) -- the boxes are in units of the pl x pl patch grid."""
    h = B // 2
    g = torch.Generator().manual_seed(B)
    shuffled = torch.cat([torch.randperm(h, generator=g), torch.randperm(B - h, generator=g) + h])
    fixed = torch.arange(B)                                       # a permutation of each half with a fixed point: its first sample
    for lo, n in ((0, h), (h, B - h)):
        if n > 1:
            fixed[lo + 1:lo + n] = torch.roll(torch.arange(lo + 1, lo + n), 1)
    cases = [("empty", (1, 1, 2, 2), 0.37, shuffled), ("whole", (0, pl, 0, pl), 0.37, shuffled)]
    for name, (y, x) in (("corner00", (0, 0)), ("corner01", (0, pl - 1)), ("corner10", (pl - 1, 0)), ("corner11", (pl - 1, pl - 1))):
        cases.append((name, (y, y + 1, x, x + 1), 0.37, shuffled))
    # edges inside a 4- and a 16-pixel vector at every shipped geometry (W / pl = 14 or 56 pixels per patch column)
    cases += [("mid", (1, 3, 1, 2), 0.0, shuffled), ("mid_wide", (0, 2, 1, 4), 1.0, fixed), ("mid_fixed", (2, 4, 0, 3), 0.37, fixed)]
    return cases


def oracle_mix(x, labels, pl, K_, od):
    """oracle.switch_token_mix; for half = 0 (B = 1), which its patch-level statements cannot reshape, its image-level statements
    (vitres_oracle.py: out = x * lam + x[perm] * (1 - lam), the targets likewise, every patch target the mixed target) alone."""
    if od["half"] > 0:
        return O.switch_token_mix(x, labels, pl, K_, 0.1, draw=od)[:3]
    lam, gb = od["lam_img"], od["perm_b"]
    y = O._smooth_one_hot(labels, K_, 0.1)
    tg = y * lam + y[gb] * (1. - lam)
    return x * lam + x[gb] * (1. - lam), tg, tg.reshape(x.shape[0], 1, -1).repeat(1, pl * pl, 1)


def run_mix_case(u8, labels, pl, K_, box, lam_img, partner):
    B = u8.shape[0]
    h = B // 2
    y0, y1, x0, x1 = box
    lam_patch = 1 - ((y1 - y0) * (x1 - x0) + 0.0) / (pl * pl)
    d = dict(half=h, partner=partner, box=box, lam_patch=float(lam_patch), lam_img=float(lam_img))
    od = dict(half=h, perm_a=partner[:h], perm_b=partner[h:] - h, box=box, lam_patch=float(lam_patch), lam_img=float(lam_img))
    xr, tr, ptr = oracle_mix(normalized(u8), labels, pl, K_, od)
    x = u8.to(DEV)
    out, whole, lo, hi = canaried(tuple(u8.shape))
    mix8 = SwitchTokenMix(pl, num_classes=K_, smoothing=0.1, input_norm=(MEAN, STD))
    xs, t, pt, pot = mix8(x, labels.to(DEV), out=out, draw=d)
    assert pot == "seq" and xs.data_ptr() == out.data_ptr()
    assert torch.equal(xs.cpu(), xr), "samples differ from the oracle"
    assert torch.equal(t.cpu(), tr) and torch.equal(pt.cpu(), ptr)
    assert canary_intact(whole, lo, hi) and torch.equal(x.cpu(), u8)
    # ... and from the two-pass path on the device: vr_normalize_u8, then vr_token_mix
    x2, t2, pt2, _ = SwitchTokenMix(pl, num_classes=K_, smoothing=0.1)(K.normalize_u8(x, MEAN, STD), labels.to(DEV), draw=d)
    assert torch.equal(xs, x2) and torch.equal(t, t2) and torch.equal(pt, pt2)


@pytest.mark.parametrize("shape", [(8, 3, 56, 56), (6, 3, 64, 64), (7, 3, 32, 32), (4, 3, 224, 224)],
                         ids=["8x56", "6x64", "7x32_odd", "4x224"])
def test_token_mix_u8_is_bit_exact(shape):
    pl, K_ = 4, 10
    u8 = u8_batch(shape, seed=1)
    labels = torch.arange(shape[0]) * 3 % K_
    for name, box, lam_img, partner in draws(shape[0], pl):
        try:
            run_mix_case(u8, labels, pl, K_, box, lam_img, partner)
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (shape, name, e))


def test_token_mix_u8_single_sample_and_misaligned_input():
    """B = 1: half = 0, the sample is its own image-level partner.  And the 4-pixel form on a wide row whose pointer is off 16 bytes."""
    u8 = u8_batch((1, 3, 32, 32), seed=2)
    run_mix_case(u8, torch.tensor([4]), 4, 10, (0, 2, 1, 3), 0.37, torch.tensor([0]))
    u8 = u8_batch((4, 3, 64, 64), seed=2)
    labels = torch.tensor([1, 2, 3, 4])
    partner = torch.tensor([1, 0, 3, 2])
    big = torch.zeros(u8.numel() + 64, dtype=torch.uint8, device=DEV)
    view = big[8:8 + u8.numel()].view(u8.shape)
    view.copy_(u8)
    d = dict(half=2, partner=partner, box=(1, 3, 1, 2), lam_patch=1 - 2 / 16, lam_img=0.37)
    od = dict(half=2, perm_a=partner[:2], perm_b=partner[2:] - 2, box=d["box"], lam_patch=d["lam_patch"], lam_img=0.37)
    xr, tr, ptr, _ = O.switch_token_mix(normalized(u8), labels, 4, 10, 0.1, draw=od)
    xs, t, pt, _ = SwitchTokenMix(4, num_classes=10, input_norm=(MEAN, STD))(view, labels.to(DEV), draw=d)
    assert view.data_ptr() % 16 == 8
    assert torch.equal(xs.cpu(), xr) and torch.equal(t.cpu(), tr) and torch.equal(pt.cpu(), ptr)


def test_seeded_uint8_path_draws_as_the_fp32_path_and_out_forms_write_the_same_bits():
    B, pl, K_ = 8, 4, 10
    u8 = u8_batch((B, 3, 56, 56), seed=3)
    y = (torch.arange(B) * 7 % K_).to(DEV)
    x8, xf = u8.to(DEV), normalized(u8).to(DEV)
    after = []
    res = []
    for norm, x in (((MEAN, STD), x8), (None, xf)):
        torch.manual_seed(41)
        np.random.seed(51)
        res.append(SwitchTokenMix(pl, num_classes=K_, input_norm=norm)(x, y))
        after.append((np.random.randint(0, 1 << 30), int(torch.randint(0, 1 << 30, (1,)))))
    assert after[0] == after[1]                                   # the next draw of each generator is the same
    torch.manual_seed(41)
    np.random.seed(51)
    od = O.token_mix_draw(B, pl)
    xr, tr, ptr, _ = O.switch_token_mix(normalized(u8), y.cpu(), pl, K_, 0.1, draw=od)
    for xs, t, pt, _ in res:
        assert torch.equal(xs.cpu(), xr) and torch.equal(t.cpu(), tr) and torch.equal(pt.cpu(), ptr)
    for norm, x in (((MEAN, STD), x8), (None, xf)):               # out= / targets_out= / patch_targets_out=
        torch.manual_seed(41)
        np.random.seed(51)
        bufs = [torch.full(s, 9.0, device=DEV) for s in ((B, 3, 56, 56), (B, K_), (B, pl * pl, K_))]
        got = SwitchTokenMix(pl, num_classes=K_, input_norm=norm)(x, y, out=bufs[0], targets_out=bufs[1], patch_targets_out=bufs[2])
        assert [g.data_ptr() for g in got[:3]] == [b.data_ptr() for b in bufs]
        assert torch.equal(bufs[0].cpu(), xr) and torch.equal(bufs[1].cpu(), tr) and torch.equal(bufs[2].cpu(), ptr)
    with pytest.raises(ValueError, match="targets_out"):
        SwitchTokenMix(pl, num_classes=K_)(xf, y, targets_out=torch.empty(B, K_ + 1, device=DEV))


# ---- vitres.data -------------------------------------------------------------------------------------------------------------------
def test_device_prefetch_loader_on_the_device():
    u8 = u8_batch((14, 3, 16, 32), seed=4)
    y = torch.arange(14)
    loader = [(u8[i:i + 4].pin_memory(), y[i:i + 4]) for i in range(0, 14, 4)]          # four batches, the last one short
    ref = normalized(u8)
    got = list(data.DevicePrefetchLoader(loader, DEV, MEAN, STD))
    assert [b.shape[0] for b, _ in got] == [4, 4, 4, 2] and all(b.is_cuda and t.is_cuda for b, t in got)
    assert torch.equal(torch.cat([b for b, _ in got]).cpu(), ref) and torch.equal(torch.cat([t for _, t in got]).cpu(), y)
    raw = list(data.DevicePrefetchLoader(loader, DEV, MEAN, STD, normalize=False))
    assert all(b.dtype == torch.uint8 and b.is_cuda for b, _ in raw)
    assert torch.equal(torch.cat([b for b, _ in raw]).cpu(), u8)


def supernet(dtype):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0, **kw)
    m.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 100))
    return m.to(DEV).set_compute_dtype(dtype)


def test_resident_u8_batches_feed_evaluate_and_score_candidate():
    """20 images, batch 8 (the last batch is short), against the same calls on the pre-normalised fp32 set: the inputs are
    bit-identical, so the counts are equal; the loss band (1e-6 relative) only covers the two launches not being the same launch."""
    m = supernet(torch.float32).eval()
    S = recipe.MICRO_IMG
    u8 = u8_batch((20, 3, S, S), seed=5)
    y = torch.arange(20) % recipe.MICRO_CLASSES
    x = normalized(u8).to(DEV)
    fp32 = [(x[i:i + 8], y[i:i + 8].to(DEV)) for i in range(0, 20, 8)]
    res = data.ResidentU8Batches(u8.to(DEV), y.to(DEV), 8, MEAN, STD)
    assert len(res) == 3
    for (a, ta), (b, tb) in zip(res, fp32):
        assert torch.equal(a, b) and torch.equal(ta, tb)
    nd = recipe.MICRO_CANDIDATES[1]
    want_eval = engine.evaluate(fp32, m, DEV, logger=QUIET)
    want_score = evo_eval.score_candidate(m, nd, fp32)
    for _ in range(2):                                            # iterating twice gives the same result
        got = engine.evaluate(res, m, DEV, logger=QUIET)
        print("evaluate", got, want_eval)
        assert got["acc1"] == want_eval["acc1"] and got["acc5"] == want_eval["acc5"]
        assert abs(got["loss"] - want_eval["loss"]) <= 1e-6 * abs(want_eval["loss"])
        assert evo_eval.score_candidate(m, nd, res) == want_score
    st_a, st_b = K.eval_state(DEV), K.eval_state(DEV)             # the hit counts themselves
    with torch.no_grad():
        for (a, ta), (b, tb) in zip(res, fp32):
            K.eval_metrics(m(a), ta, st_a)
            K.eval_metrics(m(b), tb, st_b)
    ra, rb = K.read_eval_state(st_a), K.read_eval_state(st_b)
    assert ra["rows"] == 20 and all(ra[k] == rb[k] for k in ("top1", "top5", "rows", "calls"))


# ---- training, end to end -------------------------------------------------------------------------------------------------------
class RecordingMix(SwitchTokenMix):
    """A SwitchTokenMix that remembers, per call, its draws and return values and -- before the next call and after the epoch --
    the captured step's static inputs and the model's keep tables as the step that consumed the mix left them."""

    def __init__(self, model, fast, *a, **kw):
        super().__init__(*a, **kw)
        self.model, self.fast, self.calls, self._open = model, fast, [], None

    def draw(self, batch):
        self._d = super().draw(batch)
        return self._d

    def __call__(self, samples, targets, **kw):
        self.close()
        ret = super().__call__(samples, targets, **kw)
        self._open = dict(d=self._d, ret=ret, into=kw.get("out") is not None, ptrs=[r.data_ptr() for r in ret[:3]],
                          mixed=[r.clone() for r in ret[:3]])
        return ret

    def close(self):
        c, self._open = self._open, None
        if c is None:
            return
        torch.cuda.synchronize()
        c["keeps"] = torch.stack(list(self.model.last_keeps)).clone()
        if self.fast is not None:
            step = self.fast.steps[-1]
            c["static"] = [step.x.clone(), step.t.clone(), step.pt.clone()]
            c["static_ptrs"] = [step.x.data_ptr(), step.t.data_ptr(), step.pt.data_ptr()]
        del c["ret"]
        self.calls.append(c)


def train_data():
    S = recipe.MICRO_IMG
    out = []
    for i in range(3):
        u8 = u8_batch((8, 3, S, S), seed=20 + i)
        out.append((u8, normalized(u8), (torch.arange(8) * (i + 1) + i) % recipe.MICRO_CLASSES))
    return out


def run_epoch(dtype, use_fast, use_u8):
    torch.manual_seed(2024)
    np.random.seed(2024)
    m = supernet(dtype)
    opt = FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=2e-3)
    m.train()
    m.set_epoch(31)
    fp = engine.FastPath() if use_fast else None
    mix = RecordingMix(m, fp, 1, num_classes=recipe.MICRO_CLASSES, input_norm=(MEAN, STD) if use_u8 else None)
    loader = [((u8 if use_u8 else xf).to(DEV), y.to(DEV)) for u8, xf, y in train_data()]
    stats = engine.train_one_epoch(m, CRIT, loader, opt, DEV, 31, patch_mixup_fn=mix, print_freq=0, logger=QUIET, fast=fp,
                                   arch_sample="multi")
    mix.close()
    torch.cuda.synchronize()
    return stats, mix.calls, m._arena["flat"].clone(), fp


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


@pytest.mark.parametrize("use_fast", [True, False], ids=["fast", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_training_on_uint8_batches_follows_the_fp32_run(dtype, use_fast):
    """uint8 batches through SwitchTokenMix(input_norm=) against the torch-normalised fp32 batches through the plain mix, same seeds.
    The mixed inputs are bit-identical (checked against the oracle); the bands on the loss and the parameters are those
    test_same_trajectory_as_the_eager_loop uses for two runs of this step (the weight-gradient atomics)."""
    s8, c8, p8, fp8 = run_epoch(dtype, use_fast, True)
    sf, cf, pf, _ = run_epoch(dtype, use_fast, False)
    assert len(c8) == len(cf) == 3
    for i, (a, b, (u8, xf, y)) in enumerate(zip(c8, cf, train_data())):
        d = a["d"]
        assert d["box"] == b["d"]["box"] and torch.equal(d["partner"], b["d"]["partner"]) and d["lam_img"] == b["d"]["lam_img"]
        od = dict(half=4, perm_a=d["partner"][:4], perm_b=d["partner"][4:] - 4, box=d["box"], lam_patch=d["lam_patch"],
                  lam_img=d["lam_img"])
        want = O.switch_token_mix(xf, y, 1, recipe.MICRO_CLASSES, 0.1, draw=od)[:3]
        for run in (a, b):
            assert all(torch.equal(g.cpu(), w) for g, w in zip(run["mixed"], want)), i
            if use_fast:                                          # what the captured step read
                assert all(torch.equal(g.cpu(), w) for g, w in zip(run["static"], want)), i
                # from the second batch on the mix wrote into the step's own buffers: the replay issued no input copy
                assert run["into"] == (i > 0)
                assert (run["ptrs"] == run["static_ptrs"]) == (i > 0)
        assert torch.equal(a["keeps"], b["keeps"]), i
    if use_fast:
        assert len(fp8.steps) == 1
    print("loss u8 %r fp32 %r parameters rel %r" % (s8["loss"], sf["loss"], rel(p8, pf)))
    assert abs(s8["loss"] - sf["loss"]) < (1e-5 if dtype == torch.float32 else 2e-2) * abs(sf["loss"])
    assert rel(p8, pf) < 2e-3


@pytest.mark.parametrize("use_fast", [True, False], ids=["fast", "eager"])
def test_uint8_batch_without_a_normalising_mix_raises(use_fast):
    m = supernet(torch.float32)
    opt = FlatAdamW(m, engine.param_groups_weight_decay(m, 0.05), lr=2e-3)
    u8, _, y = train_data()[0]
    loader = [(u8.to(DEV), y.to(DEV))]
    for mix in (None, SwitchTokenMix(1, num_classes=recipe.MICRO_CLASSES), lambda x, t: (x, t, None, "seq")):
        with pytest.raises(TypeError, match="DevicePrefetchLoader.*input_norm="):
            engine.train_one_epoch(m, CRIT, loader, opt, DEV, 31, patch_mixup_fn=mix, print_freq=0, logger=QUIET,
                                   fast=engine.FastPath() if use_fast else None)
    m.eval()
    with pytest.raises(TypeError, match="DevicePrefetchLoader"):
        m(u8.to(DEV))
