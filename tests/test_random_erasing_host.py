"""Random erasing without a GPU: the reference noise of tests/erase_ref.py (Philox known answers, moments), the order of
vitres.random_erasing.RandomErasing's draws against timm 0.3.2's statements written out here call by call, what the new entry points
refuse (before any launch), and the eager train_one_epoch with the erase wrappers replaced by tests/emu_erase.py's emulation: uint8
batches through Mixup / SwitchTokenMix(input_norm=, erase=) against normalise -> reference erase -> the plain emulated mix."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import emu_erase
import emu_kernels
import erase_ref
import mixup_ref
import recipe
import vitres
import vitres_oracle as O
from vitres import _lib, data, engine, kernels as K
from vitres.mixup import Mixup
from vitres.random_erasing import RandomErasing
from vitres.token_mixup import SwitchTokenMix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P = 0x10000                                                       # a fake, 16-byte aligned device address: nothing is launched


# ---- the reference noise ---------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    ones, pi = 0xFFFFFFFF, (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                               ((ones,) * 4, (ones, ones), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                               (pi, (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = erase_ref.philox4x32_10(np.array(counter, dtype=np.uint64), key)
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    both = erase_ref.philox4x32_10(np.array([(0, 0, 0, 0), pi], dtype=np.uint64), (0, 0))       # vectorised over counters
    assert tuple(int(v) for v in both[0]) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


@pytest.mark.parametrize("seed", [0, 0x1234, 2 ** 63 + 5])
def test_reference_noise_has_the_moments_of_a_normal(seed):
    z, bound = erase_ref.quad_noise(seed, 7, 3, np.arange(16384))
    z = z.ravel()
    n = z.size
    assert n == 65536
    mean, var, third = z.mean(), (z ** 2).mean(), (z ** 3).mean()
    print("seed %#x: mean %.2f var %.2f third %.2f standard errors" % (
        seed, mean * math.sqrt(n), (var - 1) / math.sqrt(2. / n), third / math.sqrt(15. / n)))
    assert abs(mean) < 4 / math.sqrt(n)                           # Var z = 1
    assert abs(var - 1) < 4 * math.sqrt(2. / n)                   # Var z^2 = 2
    assert abs(third) < 4 * math.sqrt(15. / n)                    # Var z^3 = 15
    assert np.abs(z).max() < 5.77 and erase_ref.Z_MAX < 5.77
    assert bound.max() < 2e-5 and bound.min() >= 0
    # another call, sample or domain is another stream
    for other in (erase_ref.quad_noise(seed, 8, 3, np.arange(64))[0], erase_ref.quad_noise(seed, 7, 4, np.arange(64))[0],
                  erase_ref.quad_noise(seed + 1, 7, 3, np.arange(64))[0]):
        assert not np.array_equal(other, z.reshape(-1, 4)[:64])
    assert not np.array_equal(erase_ref.rect_colours(seed, 7, 3, 0)[0], z[:4])


def test_reference_erase_applies_rectangles_in_order():
    x = np.arange(2 * 3 * 6 * 8, dtype=np.float32).reshape(2, 3, 6, 8)
    rects = np.array([[(1, 4, 1, 7), (2, 6, 5, 8), (0, 0, 0, 0)], [(0, 0, 3, 5), (3, 3, 0, 8), (5, 6, 7, 8)]], dtype=np.int32)
    for mode in ("const", "rand", "pixel"):
        out, inside, bound = erase_ref.erase(x, rects, mode, 11, 2)
        want = np.zeros(x.shape, dtype=bool)
        want[0, :, 1:4, 1:7] = want[0, :, 2:6, 5:8] = want[1, :, 5:6, 7:8] = True
        assert np.array_equal(inside, want) and np.array_equal(out[~inside], x[~inside].astype(np.float64))
        assert (bound[~inside] == 0).all()
        if mode == "const":
            assert (out[inside] == 0).all() and (bound == 0).all()
        elif mode == "rand":
            first, second = erase_ref.rect_colours(11, 2, 0, 0)[0], erase_ref.rect_colours(11, 2, 0, 1)[0]
            for c in range(3):
                assert (out[0, c, 1:2, 1:7] == first[c]).all() and (out[0, c, 2:6, 5:8] == second[c]).all()      # the later one wins
                assert (out[0, c, 2:4, 1:5] == first[c]).all()
        else:
            noise = erase_ref.pixel_noise(11, 2, 0, 3, 6, 8)[0]
            assert np.array_equal(out[0][inside[0]], noise[inside[0]])
            assert np.array_equal(noise[1, 2, 4:8], erase_ref.quad_noise(11, 2, 0, [(1 * 6 + 2) * 8 // 4 + 1])[0][0])


# ---- draw order ------------------------------------------------------------------------------------------------------------------------
def replay_sample(rnd, H, W, probability, min_count, max_count, min_area=0.02, max_area=1 / 3, min_aspect=0.3, attempts=None):
    """timm 0.3.2 RandomErasing._erase, statement by statement, minus the tensor assignment: the rectangles as (slot, y0, y1, x0, x1)."""
    log_aspect = (math.log(min_aspect), math.log(1 / min_aspect))
    found = []
    if rnd.random() > probability:
        return found
    area = H * W
    count = min_count if min_count == max_count else rnd.randint(min_count, max_count)
    for k in range(count):
        for attempt in range(10):
            target_area = rnd.uniform(min_area, max_area) * area / count
            aspect_ratio = math.exp(rnd.uniform(*log_aspect))
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if attempts is not None:
                attempts.append(attempt)
            if w < W and h < H:
                top = rnd.randint(0, H - h)
                left = rnd.randint(0, W - w)
                found.append((k, top, top + h, left, left + w))
                break
    return found


@pytest.mark.parametrize("counts", [(1, 1), (1, 3)], ids=["count1", "count1to3"])
@pytest.mark.parametrize("probability", [0., 0.25, 1.])
def test_draws_in_timms_order(probability, counts):
    B, H, W = 16, 24, 40
    erased, filled = 0, set()
    for seed in range(6):
        mine, theirs = random.Random(seed), random.Random(seed)
        er = RandomErasing(probability=probability, min_count=counts[0], max_count=counts[1], rng=mine)
        table = er.draw(B, H, W)
        assert table.dtype == np.int32 and table.shape == (B, counts[1], 4)
        want = np.zeros_like(table)
        for b in range(B):
            for k, y0, y1, x0, x1 in replay_sample(theirs, H, W, probability, *counts):
                want[b, k] = (y0, y1, x0, x1)
                filled.add(k)
        assert np.array_equal(table, want), seed
        assert mine.getstate() == theirs.getstate(), seed         # drew exactly what timm draws
        K.check_erase_rects(table, B, H, W)
        erased += int((table[:, 0, 0] < table[:, 0, 1]).sum())
    assert (erased == 0) == (probability == 0.) and (erased == 6 * B) == (probability == 1.)
    assert probability == 0. or filled == set(range(counts[1]))   # the seeds fill every slot of the table


def test_global_generator_is_the_default_and_a_private_one_leaves_it_alone():
    random.seed(5)
    table = RandomErasing(probability=1.).draw(4, 24, 40)
    after = random.getstate()
    random.seed(5)
    want = [replay_sample(random, 24, 40, 1., 1, 1) for _ in range(4)]
    assert random.getstate() == after
    assert [tuple(r[0]) for r in table] == [w[0][1:] for w in want]
    RandomErasing(probability=1., rng=random.Random(1)).draw(4, 24, 40)
    assert random.getstate() == after


def test_small_images_fail_attempts_and_leave_empty_rectangles():
    """6 x 8 pixels: with the whole area as the upper bound most attempts give h >= H or w >= W; ten failures leave the slot empty."""
    H, W = 6, 8
    empty = full = retried = 0
    for seed in range(40):
        mine, theirs = random.Random(seed), random.Random(seed)
        table = RandomErasing(probability=1., min_area=0.5, max_area=1.0, rng=mine).draw(1, H, W)
        attempts = []
        got = replay_sample(theirs, H, W, 1., 1, 1, min_area=0.5, max_area=1.0, attempts=attempts)
        assert mine.getstate() == theirs.getstate()
        if got:
            assert tuple(table[0, 0]) == got[0][1:]
            full += 1
            retried += len(attempts) > 1                          # an attempt failed before one fitted
        else:
            assert tuple(table[0, 0]) == (0, 0, 0, 0) and len(attempts) == 10
            empty += 1
    assert empty > 0 and full > 0 and retried > 0, (empty, full, retried)


def test_table_limits_and_resuming():
    with pytest.raises(ValueError, match="at most 4"):
        RandomErasing(max_count=5)
    with pytest.raises(ValueError, match="mode"):
        RandomErasing(mode="noise")
    assert RandomErasing(min_count=2).max_count == 2 and RandomErasing(max_count=4).draw(2, 8, 8).shape == (2, 4, 4)
    er = RandomErasing(probability=0.5, max_count=2, seed=2 ** 63 + 5, rng=random.Random(3))
    first = er.next_args(4, 24, 40)
    assert (first["seed"], first["call"], first["mode"], er.call) == (2 ** 63 + 5, 0, "pixel", 1) and first["table"] is None
    state = er.state_dict()
    nxt = [er.next_args(4, 24, 40) for _ in range(3)]
    again = RandomErasing(probability=0.5, max_count=2, seed=0, rng=random.Random(99))
    again.load_state_dict(state)
    for a in nxt:
        b = again.next_args(4, 24, 40)
        assert np.array_equal(a["rects"], b["rects"]) and (a["seed"], a["call"]) == (b["seed"], b["call"])
    assert [a["call"] for a in nxt] == [1, 2, 3] and again.call == er.call == 4
    import json
    through_json = json.loads(json.dumps(er.state_dict()))         # a checkpoint may flatten the tuples
    again.load_state_dict(through_json)
    assert np.array_equal(again.next_args(4, 24, 40)["rects"], er.next_args(4, 24, 40)["rects"])
    shared = RandomErasing(seed=9)
    assert shared.state_dict() == dict(seed=9, call=0, rng=None)
    with pytest.raises(ValueError, match="private"):
        shared.load_state_dict(state)


def test_rectangle_check_is_the_host_wrappers():
    rects = np.zeros((4, 2, 4), dtype=np.int32)
    rects[:, 1] = (0, 8, 0, 16)
    assert K.check_erase_rects(rects, 4, 8, 16).dtype == np.int32
    for field, value in ((1, 9), (3, 17), (0, -1), (2, -1), (0, 9), (2, 17)):
        bad = rects.copy()
        bad[2, 1, field] = value
        with pytest.raises(RuntimeError, match="VR_EINVAL.*number 1 of sample 2"):
            K.check_erase_rects(bad, 4, 8, 16)
    for shape in ((3, 2, 4), (4, 5, 4), (4, 0, 4), (4, 2, 3)):
        with pytest.raises(ValueError, match="table"):
            K.check_erase_rects(np.zeros(shape, dtype=np.int32), 4, 8, 16)
    with pytest.raises(ValueError, match="mode"):
        K.erase_args(rects, "noise", 0, 0)
    x = torch.zeros(4, 3, 8, 16)
    bad = rects.copy()
    bad[0, 0] = (0, 9, 0, 1)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):          # refused before the CPU tensor is
        K.random_erase(x, K.erase_args(bad, "pixel", 0, 0))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):           # CPU tensors: there is no CPU path
        K.random_erase(x, K.erase_args(rects, "pixel", 0, 0))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        K.normalize_u8_erase(x.to(torch.uint8), MEAN, STD, K.erase_args(rects, "pixel", 0, 0))
    with pytest.raises(TypeError):
        K.random_erase(x.to(torch.uint8), K.erase_args(rects, "pixel", 0, 0))


# ---- the entry points' checks -----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vitres_hip.h")).read()
    declared = set(re.findall(r"^int\s+(vr_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.lib()
    for name in ("vr_random_erase", "vr_normalize_u8_erase", "vr_token_mix_u8_erase", "vr_mixup_u8_erase"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.vr_version() >= 1004
    assert ctypes.sizeof(_lib.EraseArgs) == 32 and [n for n, _ in _lib.EraseArgs._fields_] == ["rects", "R", "mode", "seed", "call"]
    assert re.search(r"int32_t y0, y1, x0, x1;\s*}\s*vr_erase_rect;", hdr)
    assert re.search(r"const vr_erase_rect\* rects;\s*int32_t R, mode;\s*uint64_t seed, call;\s*}\s*vr_erase_args;", hdr)
    assert K.ERASE_MODES == dict(const=0, rand=1, pixel=2) == erase_ref.MODES
    assert re.search(r"VR_ERASE_CONST = 0, VR_ERASE_RAND = 1, VR_ERASE_PIXEL = 2", hdr)


def _ea(rects=P * 7, R=2, mode=2, erase=True):
    return ctypes.byref(_lib.EraseArgs(rects, R, mode, 5, 6)) if erase else None


def _erase(x=P, B=4, C=3, H=8, W=16, rects=P * 7, R=2, mode=2):
    return _lib.lib().vr_random_erase(x, B, C, H, W, rects, R, mode, 2 ** 63 + 5, 2 ** 40, None)


def _norm(inp=P, out=P * 2, B=4, C=3, H=8, W=16, mean=True, **kw):
    m, s = K.norm_constants(MEAN + (0.5,), STD + (0.25,))
    return _lib.lib().vr_normalize_u8_erase(inp, out, B, C, H, W, m if mean else None, s, _ea(**kw), None)


def _tmix(samples=P, out=P * 2, labels=P * 3, partner=P * 4, targets=P * 5, patch_targets=P * 6, B=4, C=3, H=8, W=16, half=2,
          mean=True, **kw):
    m, s = K.norm_constants(MEAN + (0.5,), STD + (0.25,))
    return _lib.lib().vr_token_mix_u8_erase(samples, out, labels, partner, targets, patch_targets, B, C, H, W, 10, 4, half, 0, 1, 0, 1,
                                            0.5, 0.5, 0.5, 0.5, 0.9, 0.01, m if mean else None, s, _ea(**kw), None)


def _mixup(samples=P, out=P * 2, labels=P * 3, targets=P * 4, params=P * 5, B=4, C=3, H=8, W=16, mean=True, **kw):
    m, s = K.norm_constants(MEAN + (0.5,), STD + (0.25,))
    return _lib.lib().vr_mixup_u8_erase(samples, out, labels, targets, params, B, C, H, W, 10, 0.9, 0.01, m if mean else None, s,
                                        _ea(**kw), None)


BIG = 2 ** 24 + 2                                                 # one sample too many for counter word 1 (even: vr_mixup's own rule)


@pytest.mark.parametrize("call", [_erase, _norm, _tmix, _mixup], ids=["random_erase", "normalize", "token_mix", "mixup"])
def test_entry_points_validate_the_erase_arguments_before_any_launch(call):
    assert call(rects=None) == EINVAL
    assert call(R=0) == EINVAL and call(R=5) == EINVAL and call(R=-1) == EINVAL
    assert call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    assert call(B=0) == EINVAL and call(H=-1) == EINVAL
    assert call(B=BIG) == EUNSUPPORTED
    assert call(C=5) == EUNSUPPORTED and call(W=18) == EUNSUPPORTED
    assert call(rects=P * 7 + 2) == EALIGN and call(rects=P * 7 + 1) == EALIGN
    assert call(R=5, B=BIG, rects=P * 7 + 2) == EINVAL and call(B=BIG, rects=P * 7 + 2) == EUNSUPPORTED   # EINVAL, EUNSUPPORTED, EALIGN
    if call is _erase:
        assert call(x=None) == EINVAL and call(x=P + 4) == EALIGN and call(x=P + 8) == EALIGN
    else:
        assert call(erase=False) == EINVAL and call(mean=False) == EINVAL
        assert call(out=None) == EINVAL and call(out=P * 2 + 4) == EALIGN


def test_existing_checks_are_kept_by_the_erase_entries():
    assert _norm(inp=None) == EINVAL and _norm(inp=P + 1) == EALIGN and _norm(C=5, out=P * 2 + 4) == EUNSUPPORTED
    for name in ("samples", "out", "labels", "partner", "targets", "patch_targets"):
        assert _tmix(**{name: None}) == EINVAL, name
    assert _tmix(half=5) == EINVAL and _tmix(H=6) == EUNSUPPORTED and _tmix(samples=P + 2) == EALIGN
    for name in ("samples", "out", "labels", "targets", "params"):
        assert _mixup(**{name: None}) == EINVAL, name
    assert _mixup(B=3) == EUNSUPPORTED and _mixup(out=P) == EUNSUPPORTED and _mixup(params=P * 5 + 2) == EALIGN


# ---- the engine, on the emulation ----------------------------------------------------------------------------------------------------------
class Crit(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, t):
        loss = O.soft_target_ce(x, t)
        self.seen.append(float(loss.detach()))
        return loss


class Quiet:
    info = staticmethod(lambda s: None)


def micro():
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    m = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                            num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0,
                            drop_block_rate=None, **kw)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 100)
    m.load_state_dict(sd)
    m.set_compute_dtype(torch.float32)
    m.train()
    m.set_epoch(31)
    m.load_state_dict(sd)
    return m


def u8_batches(n):
    out = []
    for it in range(n):
        g = torch.Generator().manual_seed(600 + it)
        out.append((torch.randint(0, 256, (8, 3, recipe.MICRO_IMG, recipe.MICRO_IMG), dtype=torch.uint8, generator=g),
                    (torch.arange(8) * (it + 1) + it) % recipe.MICRO_CLASSES))
    return out


class RefTokenMix:
    """The oracle's SwitchTokenMix on the class's own draws: the plain emulated mix for CPU tensors."""

    def __init__(self, mixer):
        self.mixer = mixer

    def __call__(self, x, t):
        d = self.mixer.draw(len(x))
        return O.switch_token_mix(x, t, self.mixer.patch_len, self.mixer.num_classes, self.mixer.smoothing, draw=emu_erase.oracle_draw(d))


def new_erase(mode):
    return RandomErasing(probability=0.75, mode=mode, max_count=2, seed=0x1234, rng=random.Random(0))


@pytest.mark.parametrize("mode", ["pixel", "rand", "const"])
@pytest.mark.parametrize("kind", ["mixup", "token_mix"])
def test_eager_epoch_on_uint8_with_erase_equals_normalise_erase_mix(monkeypatch, kind, mode):
    emu_kernels.install(monkeypatch)
    mixup_ref.install(monkeypatch)
    calls = emu_erase.install(monkeypatch)
    norm = K.norm_constants(MEAN, STD)
    runs = []
    # fused: the uint8 batches through the erase wrapper; staged: the three stages written out, mixed by the reference; and for the
    # token mix a third run, the staged batches through SwitchTokenMix's own un-erased path (kernels.token_mix, emulated by name)
    for variant in ("fused", "staged") + (("by_name",) if kind == "token_mix" else ()):
        fused = variant == "fused"
        er = new_erase(mode)
        if fused:
            kw = dict(input_norm=(MEAN, STD), erase=er)
            loader = u8_batches(3)
        else:                                                     # the three stages, written out: the same tables, seed and calls
            kw = {}
            loader = []
            for u8, y in u8_batches(3):
                args = er.next_args(*((len(u8),) + tuple(u8.shape[-2:])))
                loader.append((emu_erase.erased(emu_erase.normalized(u8, norm), args)[0], y))
            assert er.call == 3
        if kind == "mixup":
            mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", num_classes=recipe.MICRO_CLASSES, **kw)
            how = dict(mixup_fn=mix)
        else:
            mix = SwitchTokenMix(1, num_classes=recipe.MICRO_CLASSES, **kw)
            how = dict(patch_mixup_fn=RefTokenMix(mix) if variant == "staged" else mix)
        m = micro()
        opt = torch.optim.AdamW(engine.param_groups_weight_decay(m, 0.05), lr=1e-3)
        crit = Crit()
        torch.manual_seed(77)
        np.random.seed(2)
        before = len(calls)
        stats = engine.train_one_epoch(m, crit, loader, opt, "cpu", 31, None, max_norm=None, print_freq=0, arch_sample="multi",
                                       logger=Quiet, **how)
        runs.append((stats, crit.seen, m.state_dict(), np.random.get_state(), calls[before:], loader))
    (sa, la, pa, ga, ca, _), (sb, lb, pb, gb, cb, staged) = runs[:2]
    for sc, lc, pc, gc, cc, _ in runs[2:]:                        # the un-erased mix by name IS the reference mix
        assert [(c["what"], c["erase"]) for c in cc] == [("token_mix", None)] * 3
        assert lc == lb and sc == sb and all(torch.equal(pc[k], pb[k]) for k in pb)
        assert gc[0] == gb[0] and np.array_equal(gc[1], gb[1]) and gc[2:] == gb[2:]
    assert len(ca) == 3 and not cb                                # the fused run went through the erase wrapper, once per batch
    want = "mixup_u8_erase" if kind == "mixup" else "token_mix_u8_erase"
    any_erased = False
    for i, c in enumerate(ca):
        assert c["what"] == want and (c["erase"]["seed"], c["erase"]["call"], c["erase"]["mode"]) == (0x1234, i, mode)
        # what the mix was handed inside the wrapper IS the staged batch, bit for bit -- noise pixels included, both being the
        # emulation's own values -- and outside the rectangles it is the normalised batch
        assert mixup_ref.bits_equal(c["erased"], staged[i][0])
        plain = emu_erase.normalized(u8_batches(3)[i][0], norm)
        assert torch.equal(c["erased"][~c["mask"]].view(torch.int32), plain[~c["mask"]].view(torch.int32))
        any_erased = any_erased or bool(c["mask"].any())
        assert not bool(c["mask"].all())
    assert any_erased
    assert len(la) >= 3 and la == lb and sa == sb
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    assert ga[0] == gb[0] and np.array_equal(ga[1], gb[1]) and ga[2:] == gb[2:]


def test_mix_replays_a_recorded_erase_and_leaves_fp32_input_alone(monkeypatch):
    mixup_ref.install(monkeypatch)
    calls = emu_erase.install(monkeypatch)
    u8, y = u8_batches(1)[0]
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=recipe.MICRO_CLASSES, input_norm=(MEAN, STD), erase=new_erase("pixel"))
    np.random.seed(4)
    d = mix.draw(8, (56, 56))
    x1, t1 = mix(u8, y, draw=d)
    assert mix.last_erase["call"] == 0 and mix.erase.call == 1
    replay = Mixup(num_classes=recipe.MICRO_CLASSES, input_norm=(MEAN, STD))          # no RandomErasing of its own: the table rides in the draw
    x2, t2 = replay(u8, y, draw=dict(d, erase=mix.last_erase))
    assert mixup_ref.bits_equal(x1, x2) and mixup_ref.bits_equal(t1, t2) and replay.last_erase is mix.last_erase
    x3, _ = mix(u8, y, draw=d)                                    # the next call: another table, another call number
    assert mix.last_erase["call"] == 1 and not mixup_ref.bits_equal(x1, x3)
    # fp32 batches: a copy is erased (vr_random_erase), the caller's batch keeps its bits
    xf = emu_erase.normalized(u8, K.norm_constants(MEAN, STD))
    keep = xf.clone()
    mixf = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=recipe.MICRO_CLASSES, erase=new_erase("pixel"))
    x4, t4 = mixf(xf, y, draw=d)
    assert calls[-1]["what"] == "random_erase" and torch.equal(xf, keep)
    assert mixup_ref.bits_equal(x4, x1) and mixup_ref.bits_equal(t4, t1)             # the same table, seed and call as the first


def test_prefetch_loader_erases_only_where_it_normalises(monkeypatch):
    calls = emu_erase.install(monkeypatch)
    batches = [(u8[:, :, :8, :8].contiguous(), y) for u8, y in u8_batches(2)]
    with pytest.raises(ValueError, match="normalize=False.*SwitchTokenMix"):
        data.DevicePrefetchLoader(batches, "cpu", normalize=False, erase=new_erase("pixel"))
    er = new_erase("pixel")
    got = list(data.DevicePrefetchLoader(batches, "cpu", erase=er))
    assert er.call == 2 and [c["what"] for c in calls] == ["normalize_u8_erase"] * 2
    twin = new_erase("pixel")
    for (x, t), (u8, y) in zip(got, batches):
        want = emu_erase.erased(emu_erase.normalized(u8, K.norm_constants(MEAN, STD)), twin.next_args(8, 8, 8))[0]
        assert mixup_ref.bits_equal(x, want) and torch.equal(t, y)
