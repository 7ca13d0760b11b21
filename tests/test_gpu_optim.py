"""The step tail of csrc/optim.hip against the contracts of tests/optim_ref64.py: the AdamW pass through its four entry points
(vr_adamw_flat, _dev, _dev_capped, _clip with the structs in host and in device memory) and vr_grad_sumsq / vr_clip_finish with their
gated forms, on every launch path of adamw_launch and sumsq_launch (the literal tables below), at the smallest sizes that reach them.

Calls go through the C ABI with buffers the test owns.  Every array is a view at an 8-element offset inside a larger allocation whose
guard zones hold one NaN bit pattern that must still be there afterwards; regions a kernel must not read into a result (the gradient of a
255 stretch, the partial sums before a launch, the words behind the struct array) hold NaN.  Bounded outputs (p, m, v, ema, the partial
sums) compare per element against first-principles bounds, exact ones (the bf16 shadow, untouched elements, zero slots, coef / skip /
skipped, refusals) as integers.

`pytest -s` prints one line per case (OPTIM ...) and, last, the worst error / bound per kernel and output."""
import math

import numpy as np
import pytest
import torch

import optim_ref64 as R
import recipe
import vitres
import vitres.kernels as K
import vitres_oracle as O
from vitres import _lib, engine
from vitres.losses import SoftTargetCrossEntropy
from vitres.optim import NORM_PARTIALS, FlatAdamW

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32

# ---- the launch paths, read from optim.hip ------------------------------------------------------------------------------------------------------
# adamw_launch: (n, max_blocks) -> (workgroups, grid-stride passes, threads live in the last pass)
ADAMW_PATHS = {(8, 0): (1, 1, 1), (2040, 0): (1, 1, 255), (2048, 0): (1, 1, 256), (2056, 0): (2, 1, 257), (4096, 2): (2, 1, 512),
               (4104, 2): (2, 2, 1), (8200, 2): (2, 3, 1), (16779272, 0): (8192, 2, 257)}
# sumsq_launch: (n, n_partials, max_blocks) -> (workgroups with work, workgroups that write 0, terms of the longest chain)
SUMSQ_PATHS = {(8, 1, 0): (1, 0, 1), (8, 5, 0): (1, 4, 1), (2048, 1, 0): (1, 0, 1), (2056, 2, 0): (2, 0, 1), (2056, 1, 0): (1, 0, 2),
               (6152, 4, 2): (2, 2, 2), (614400, 1, 0): (1, 0, 300)}


def test_path_tables_match_the_code_and_cover_every_path():
    check_path_tables()


def check_path_tables():
    """shared with the host suite, which runs it without a device"""
    assert set(ADAMW_PATHS) == set(R.ADAMW_CASES) | {(R.ADAMW_BIG, 0)}
    assert all(R.adamw_path(*k) == v for k, v in ADAMW_PATHS.items())
    # one workgroup partly / exactly filled, a second workgroup, the cap met exactly, a second and a third pass of one thread, and the
    # default cap with a second pass of one whole workgroup and one thread of the next
    assert {(w, p) for w, p, _ in ADAMW_PATHS.values()} == {(1, 1), (2, 1), (2, 2), (2, 3), (8192, 2)}
    assert {l for w, p, l in ADAMW_PATHS.values() if (w, p) == (1, 1)} == {1, 255, 256}
    assert ADAMW_PATHS[(R.ADAMW_BIG, 0)][2] == 257 and ADAMW_PATHS[(R.ADAMW_BIG, 0)][0] == R.DEFAULT_CAP
    assert set(SUMSQ_PATHS) == set(R.SUMSQ_CASES) and all(R.sumsq_path(*k) == v for k, v in SUMSQ_PATHS.items())
    # slots without work (n_partials above the need, and the cap below n_partials), chains of one, two and 300 terms
    assert {z > 0 for _, z, _ in SUMSQ_PATHS.values()} == {True, False} and {c for _, _, c in SUMSQ_PATHS.values()} == {1, 2, 300}
    assert any(k[2] > 0 and v[0] == k[2] < k[1] for k, v in SUMSQ_PATHS.items())             # the cap decides
    assert any(v[0] == k[1] and v[2] > 1 for k, v in SUMSQ_PATHS.items())                    # n_partials decides


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------------
def L():
    return _lib.lib()


def stream():
    return K._stream()


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                      # a device error: nothing more is launched in this session
        pytest.exit("the device reported an error, the run ends here: %s" % e, returncode=3)


INT = {4: np.int32, 2: np.int16, 1: np.uint8}
TAIL = 64


class Buf:
    """a numpy array on the device, R.GUARD elements into a larger allocation of canary words (bytes of 0 for the group bytes: a byte
    read from a guard would select group 0 and write where nothing may be written)"""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.dtype, self.n, self.item = arr.dtype, arr.size, arr.dtype.itemsize
        self.fill = {4: R.CANARY32, 2: R.CANARY16, 1: 0}[self.item]
        whole = np.full(R.GUARD + self.n + TAIL, self.fill, dtype={4: np.uint32, 2: np.uint16, 1: np.uint8}[self.item])
        whole[R.GUARD:R.GUARD + self.n] = R.bits(arr).reshape(-1)
        self.t = torch.from_numpy(whole.view(INT[self.item])).to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr() + R.GUARD * self.item

    def at(self, lo):
        return self.ptr + lo * self.item

    def get(self):
        torch.cuda.synchronize()
        w = R.bits(self.t.cpu().numpy())
        assert (w[:R.GUARD] == self.fill).all() and (w[R.GUARD + self.n:] == self.fill).all(), "a guard zone was written"
        return w[R.GUARD:R.GUARD + self.n].view(self.dtype).copy()


ENTRIES = ["flat", "dev", "capped", "clip_host", "clip_dev"]
OUT_KEYS = ["p", "m", "v", "shadow", "ema"]


def clip_words(max_norm=1.0, grad_scale=1.0, norm=0.0, coef=1.0, skip=0, skipped=0):
    w = np.zeros(8, np.uint32)
    w[:4] = R.bits(np.array([max_norm, grad_scale, norm, coef], f32))
    w[4:6] = [skip, skipped]
    return w


def device_adamw(entry, a, gid, groups, d=None, coef=None, skip=0, launches=None, n_groups=None):
    """One or more launches of `entry` on the same guarded buffers.  a: dict of numpy arrays p, g, m, v fp32, shadow uint16 or None,
    ema fp32 (passed to the kernel when d is given).  launches: [(lo, hi, max_blocks)], default the whole arena once.
    -> (return codes, dict of the arrays afterwards); the guard zones of every buffer, the gradient, the group bytes, the structs and
    the clip state are checked to be as they were."""
    n = a["p"].size
    B = {k: Buf(a[k]) for k in ("p", "g", "m", "v", "ema")}
    if a.get("shadow") is not None:
        B["shadow"] = Buf(a["shadow"])
    B["gid"] = Buf(gid)
    groups = np.ascontiguousarray(groups, dtype=f32)
    G = len(groups) if n_groups is None else n_groups
    on_dev = entry in ("dev", "capped", "clip_dev")
    B["groups"] = Buf(groups.reshape(-1))            # (behind the structs on the device: NaN)
    gptr = B["groups"].ptr if on_dev else groups.ctypes.data
    if entry.startswith("clip"):
        B["clip"] = Buf(clip_words(coef=1.0 if coef is None else coef, skip=skip))
    else:
        assert coef is None and skip == 0
    rcs = []
    for lo, hi, cap in launches or [(0, n, 0)]:
        ptrs = [B[k].at(lo) for k in "pgmv"] + [B["shadow"].at(lo) if "shadow" in B else None, B["ema"].at(lo) if d is not None else None]
        head = ptrs + [float(d or 0.0), B["gid"].at(lo // 8), gptr]
        cnt = hi - lo
        if entry == "flat":
            assert cap == 0
            rcs.append(L().vr_adamw_flat(*head, G, cnt, stream()))
        elif entry == "dev" and cap == 0:
            rcs.append(L().vr_adamw_flat_dev(*head, G, cnt, stream()))
        elif entry in ("dev", "capped"):
            rcs.append(L().vr_adamw_flat_dev_capped(*head, G, cnt, cap, stream()))
        else:
            rcs.append(L().vr_adamw_flat_clip(*head, int(on_dev), G, cnt, B["clip"].ptr, cap, stream()))
    got = {k: B[k].get() for k in B}
    for k, before in (("g", a["g"]), ("gid", gid), ("groups", groups.reshape(-1))):
        assert (R.bits(got[k]) == R.bits(before).reshape(-1)).all(), "%s was written" % k
    if "clip" in B:
        assert (got["clip"] == clip_words(coef=1.0 if coef is None else coef, skip=skip)).all(), "the clip state was written"
    if d is None:
        assert (R.bits(got["ema"]) == R.bits(a["ema"])).all(), "ema was written without a decay"
    return rcs, {k: got[k] for k in ["g"] + OUT_KEYS if k in got}


def arena(n, seed=3, shadow=True):
    a = R.adamw_inputs(n, seed)
    a["shadow"] = np.full(n, R.CANARY16, np.uint16) if shadow else None
    return a


def judge(tag, kernel, a, got, gid, groups, coef=None, d=None, dev=False, where=None):
    v = R.adamw_verdict(a, got, gid, groups, coef, d, dev, where)
    for k, r in v.items():
        R.record((kernel, k), r)
    print("OPTIM %-66s %s" % (tag, " ".join("%s %.3f" % kv for kv in sorted(v.items()))))
    assert max(v.values()) <= 1.0, (tag, v)
    return v


def same_bits(x, y, keys=OUT_KEYS):
    return all((R.bits(x[k]) == R.bits(y[k])).all() for k in keys if k in x)


def entry_cases():
    out = []
    for e in ENTRIES:
        for n, cap in R.ADAMW_CASES:
            if cap == 0 or e not in ("flat", "dev"):      # vr_adamw_flat and vr_adamw_flat_dev take no workgroup cap
                out.append((e, n, cap))
    return out


# ---- AdamW: every path x family x hyper-parameter set, on every entry point -------------------------------------------------------------------------
@pytest.mark.parametrize("entry,n,cap", entry_cases())
def test_adamw_within_bounds_on_every_path_and_hyper_set(entry, n, cap):
    """the six input families share the arena; p, m, v, ema per element against the float64 contract, the shadow exactly"""
    clip = entry.startswith("clip")
    a = arena(n)
    worst = {}
    for h in R.hyper_sets(R.COEFS if clip else [None]):
        t, kind, gs, coef, d = h
        groups = R.groups_f32(kind, t, gs)
        gid = R.group_bytes(n, len(groups))
        rcs, got = device_adamw("capped" if entry == "dev" and cap else entry, a, gid, groups, d, coef, launches=[(0, n, cap)])
        assert rcs == [0]
        v = R.adamw_verdict(a, got, gid, groups, coef, d, dev=entry in ("dev", "capped", "clip_dev"))
        assert max(v.values()) <= 1.0, (entry, n, cap, R.hyper_name(h), v)
        for k, r in v.items():
            worst[k] = max(worst.get(k, 0.0), R.record(("adamw " + entry, k), r))
    print("OPTIM adamw %-9s n=%-5d cap=%d, %d hyper sets: %s" % (entry, n, cap, len(R.hyper_sets(R.COEFS if clip else [None])),
                                                               " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("h", [(1, "two", 1.0, None, 0.99996), (2, "sixteen", 0.125, None, None), (100000, "two", 0.125, None, 0.99)],
                         ids=R.hyper_name)
def test_every_entry_point_gives_the_host_forms_bits(h):
    """structs by value, structs in device memory, capped at the default grid, and the clip forms at coefficient 1"""
    t, kind, gs, _, d = h
    n = 2056
    a, groups = arena(n), R.groups_f32(kind, t, gs)
    gid = R.group_bytes(n, len(groups))
    ref = device_adamw("flat", a, gid, groups, d)[1]
    judge("bits: flat %s" % R.hyper_name(h), "adamw flat", a, ref, gid, groups, None, d)
    for entry in ENTRIES[1:]:
        rcs, got = device_adamw(entry, a, gid, groups, d)
        assert rcs == [0] and same_bits(got, ref), entry


@pytest.mark.parametrize("entry", ["capped", "clip_host", "clip_dev"])
def test_pieces_and_a_capped_grid_give_the_single_launch_bits(entry):
    """the per-element result does not depend on the launch geometry: [0, n) at once, [0, a) + [a, n) into the middle of the arena,
    and two workgroups striding three passes"""
    n, cut = 8200, 3000
    h = (2, "sixteen", 0.125, 0.37 if entry != "capped" else None, 0.99996)
    t, kind, gs, coef, d = h
    a, groups = arena(n), R.groups_f32(kind, t, gs)
    gid = R.group_bytes(n, len(groups))
    whole = device_adamw(entry, a, gid, groups, d, coef)[1]
    judge("pieces: whole %s" % entry, "adamw " + entry, a, whole, gid, groups, coef, d, dev=entry != "clip_host")
    for launches in ([(0, cut, 0), (cut, n, 0)], [(cut, n, 0), (0, cut, 2)], [(0, n, 2)]):
        assert R.adamw_path(n, 2)[1] == 3
        rcs, got = device_adamw(entry, a, gid, groups, d, coef, launches=launches)
        assert set(rcs) == {0} and same_bits(got, whole), launches
    # one range alone: everything outside [cut, n) keeps its bits
    _, got = device_adamw(entry, a, gid, groups, d, coef, launches=[(cut, n, 0)])
    for k in OUT_KEYS:
        assert (R.bits(got[k][:cut]) == R.bits(a[k][:cut])).all() and (R.bits(got[k][cut:]) == R.bits(whole[k][cut:])).all(), k


def test_big_arena_second_pass_under_the_default_cap_equals_single_pass_pieces():
    """n = 8 (8192 * 256 + 257): the shipped arenas take up to nine passes under the 8192-workgroup cap; two passes here, the second of 257
    threads, bit for bit against the same arena updated by two single-pass range launches, and within the float64 bounds on a sample"""
    n = R.ADAMW_BIG
    first = R.DEFAULT_CAP * 256 * 8
    assert R.adamw_path(n)[1] == 2 and R.adamw_path(first)[1] == 1 and R.adamw_path(n - first)[1] == 1
    base = arena(2 ** 20 + 40, seed=9)
    a = {k: np.resize(x, n) for k, x in base.items()}
    t, kind, gs, d = 10, "two", 0.125, 0.99996
    groups = R.groups_f32(kind, t, gs)
    gid = R.group_bytes(n, len(groups), holes=[(first // 8 - 3, first // 8 + 2)])
    whole = device_adamw("flat", a, gid, groups, d)[1]
    rcs, pieces = device_adamw("dev", a, gid, groups, d, launches=[(0, first, 0), (first, n, 0)])
    assert rcs == [0, 0] and same_bits(whole, pieces)
    n8 = n // 8
    i8 = np.unique(np.concatenate([np.arange(0, n8, 65), np.arange(first // 8 - 8, n8)]))
    idx = (i8[:, None] * 8 + np.arange(8)).reshape(-1)
    assert idx.size <= R.BIG_SAMPLE and (i8 >= first // 8).sum() >= 257
    sub = lambda x: {k: v[idx] for k, v in x.items()}                                       # noqa: E731
    judge("big n=%d, %d sampled" % (n, idx.size), "adamw flat", sub(a), sub(whole), gid[i8], groups, None, d)
    live = np.repeat(gid != 255, 8)
    for k in OUT_KEYS:                                                                       # every 255 element of the whole arena
        assert (R.bits(whole[k])[~live] == R.bits(a[k])[~live]).all(), k


# ---- what must not be touched -------------------------------------------------------------------------------------------------------------------
def holes_of(n8):
    return [(0, 2), (n8 // 2, n8 // 2 + 3), (n8 - 1, n8)]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n,cap", [(2056, 0), (4104, 2)])
def test_group_255_stretches_keep_every_bit_and_the_norm_ignores_them(entry, n, cap):
    """255 at the head, in the middle and at the tail with NaN in the gradient there"""
    if cap and entry in ("flat", "dev"):
        entry = "capped"
    h = (2, "two", 1.0, 0.37 if entry.startswith("clip") else None, 0.99)
    t, kind, gs, coef, d = h
    a, groups = arena(n), R.groups_f32(kind, t, gs)
    holes = holes_of(n // 8)
    gid = R.group_bytes(n, 2, holes)
    for lo, hi in holes:
        a["g"][lo * 8:hi * 8] = np.nan
    rcs, got = device_adamw(entry, a, gid, groups, d, coef, launches=[(0, n, cap)])
    assert rcs == [0]
    v = judge("255 stretches %s n=%d cap=%d" % (entry, n, cap), "adamw " + entry, a, got, gid, groups, coef, d,
              dev=entry in ("dev", "capped", "clip_dev"))
    assert v["untouched"] == 0.0
    hole = np.repeat(gid == 255, 8)
    assert hole.sum() == 8 * 6 and all((R.bits(got[k])[hole] == R.bits(a[k])[hole]).all() for k in OUT_KEYS)
    part, state = device_norm(a["g"], gid, 2, cap, max_norm=1.0)
    assert np.isfinite(part).all() and np.isfinite(state["norm"]) and state["skip"] == 0 and state["skipped"] == 0


@pytest.mark.parametrize("entry", ["dev", "capped", "clip_dev"])
@pytest.mark.parametrize("zero", [0, 1])
def test_dev_forms_skip_an_all_zero_group(entry, zero):
    n = 4104
    t, kind, gs, coef, d = 1, "two", 0.125, (0.37 if entry == "clip_dev" else None), 0.99996
    a, groups = arena(n), R.groups_f32(kind, t, gs)
    groups[zero] = 0.0
    gid = R.group_bytes(n, 2)
    rcs, got = device_adamw(entry, a, gid, groups, d, coef, launches=[(0, n, 2 if entry != "dev" else 0)])
    assert rcs == [0]
    judge("zero group %d %s" % (zero, entry), "adamw " + entry, a, got, gid, groups, coef, d, dev=True)
    dead = np.repeat(gid == zero, 8)
    assert dead.sum() >= n // 2 - 8 and all((R.bits(got[k])[dead] == R.bits(a[k])[dead]).all() for k in OUT_KEYS)
    assert (R.bits(got["p"])[~dead] != R.bits(a["p"])[~dead]).any()


@pytest.mark.parametrize("entry", ["clip_host", "clip_dev"])
def test_clip_skip_writes_nothing_and_a_coefficient_scales_the_gradient(entry):
    n = 4104
    t, kind, gs, d = 2, "two", 1.0, 0.99
    a, groups = arena(n), R.groups_f32(kind, t, gs)
    gid = R.group_bytes(n, 2)
    for cap in (0, 2):
        rcs, got = device_adamw(entry, a, gid, groups, d, coef=0.0, skip=1, launches=[(0, n, cap)])
        assert rcs == [0] and same_bits(got, a), "a skipped step wrote"
    rcs, got = device_adamw(entry, a, gid, groups, d, coef=0.37, skip=0)
    judge("coef 0.37 %s" % entry, "adamw " + entry, a, got, gid, groups, 0.37, d, dev=entry == "clip_dev")
    plain = R.adamw_contract(a, gid, groups, None, d)                                        # the coefficient matters: far outside without it
    assert R.ratio(got["m"], plain[0]["m"], plain[1]["m"]) > 100.0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("entry", ["flat", "dev"])
def test_a_non_finite_gradient_element_stays_in_its_element(entry, bad):
    """without clipping: exactly that element's p', m', v', shadow and ema are non-finite, as the formula gives them; the other seven of its
    group of eight and the neighbouring groups stay within bounds"""
    n, d = 2056, 0.99
    groups = R.groups_f32("two", 2, 1.0)
    gid = R.group_bytes(n, 2)
    for k in (0, 1003, n - 1):                                  # a first, an inner and the last lane of a group of eight
        a = arena(n)
        a["g"][k] = bad
        rcs, got = device_adamw(entry, a, gid, groups, d)
        assert rcs == [0]
        judge("g[%d] = %s %s" % (k, bad, entry), "adamw " + entry, a, got, gid, groups, None, d, dev=entry == "dev")
        ref = R.adamw_contract(a, gid, groups, None, d)[0]
        assert np.isnan(ref["p"][k]) and np.isnan(ref["ema"][k]) and not np.isfinite(ref["m"][k]) and not np.isfinite(ref["v"][k])
        for key in ("p", "m", "v", "ema"):
            fin = np.isfinite(got[key])
            assert not fin[k] and fin.sum() == n - 1, key
        sh_nan = (got["shadow"] & 0x7fff) > 0x7f80
        assert sh_nan[k] and sh_nan.sum() == 1


# ---- the gradient norm --------------------------------------------------------------------------------------------------------------------------
def read_state(words):
    f = words[:4].view(f32)
    return {"max_norm": f[0], "grad_scale": f[1], "norm": f[2], "coef": f[3], "skip": int(words[4]), "skipped": int(words[5]),
            "words": words.copy()}


def device_sumsq(g, gid, n_partials, cap, gate=None, before=None):
    """-> (rc, partials fp32 after the launch); the buffer holds the canary before it"""
    G, I, P = Buf(g), Buf(gid), Buf(R.canary32(n_partials) if before is None else before)
    if gate is None:
        rc = L().vr_grad_sumsq(G.ptr, I.ptr, g.size, P.ptr, n_partials, cap, stream())
    else:
        W = Buf(np.array([gate], np.int32))
        rc = L().vr_grad_sumsq_gated(G.ptr, I.ptr, g.size, P.ptr, n_partials, cap, W.ptr, stream())
        assert W.get()[0] == gate
    assert (R.bits(G.get()) == R.bits(g)).all()
    return rc, P.get()


def device_finish(partials, words, gate=None):
    P, S = Buf(partials), Buf(words)
    if gate is None:
        rc = L().vr_clip_finish(P.ptr, partials.size, S.ptr, stream())
    else:
        W = Buf(np.array([gate], np.int32))
        rc = L().vr_clip_finish_gated(P.ptr, partials.size, S.ptr, W.ptr, stream())
    assert (R.bits(P.get()) == R.bits(partials)).all()
    return rc, S.get()


def device_norm(g, gid, n_partials, cap, max_norm=math.inf, grad_scale=1.0):
    rc, part = device_sumsq(g, gid, n_partials, cap)
    assert rc == 0
    rc, words = device_finish(part, clip_words(max_norm, grad_scale, norm=-1.0, coef=-1.0))
    assert rc == 0
    return part, read_state(words)


def check_finish(tag, partials, before, after):
    """the state behind vr_clip_finish against the contract: norm to one ulp, the rest exactly from the device's own norm"""
    b, s = read_state(before), read_state(after)
    assert (after[:2] == before[:2]).all() and (after[6:] == before[6:]).all(), "an input or reserved word was written"
    assert R.norm_matches(s["norm"], partials, b["grad_scale"]), (tag, s["norm"], R.norm_ref(partials, b["grad_scale"]))
    coef, skip, skipped = R.clip_outputs(s["norm"], b["max_norm"], b["skipped"])
    print("OPTIM %-66s norm %.9g coef %.9g skip %d skipped %d" % (tag, s["norm"], s["coef"], s["skip"], s["skipped"]))
    assert (int(R.bits(s["coef"])[0]), s["skip"], s["skipped"]) == (int(R.bits(coef)[0]), skip, skipped), (tag, s, coef, skip, skipped)
    return s


@pytest.mark.parametrize("n,n_partials,cap", R.SUMSQ_CASES)
def test_sumsq_partials_within_bounds_and_idle_workgroups_write_zero(n, n_partials, cap):
    gid = R.group_bytes(n, 2)
    for kind in R.SUMSQ_FAMILIES:
        g = R.sumsq_inputs(kind, n)
        ref, bound, active = R.sumsq_contract(g, gid, n_partials, cap)
        rc, got = device_sumsq(g, gid, n_partials, cap)
        assert rc == 0
        r = R.record(("sumsq", kind), R.ratio(got[:active], ref[:active], bound[:active]))
        print("OPTIM sumsq %-5s n=%-6d partials=%d cap=%d: active %d chain %d err/bound %.3f" % ((kind, n, n_partials, cap, active)
                                                                                                   + (R.sumsq_path(n, n_partials, cap)[2], r)))
        assert r <= 1.0 and (R.bits(got[active:]) == 0).all()                                  # +0.0 over the canary, not -0.0, not stale
        rc, gated = device_sumsq(g, gid, n_partials, cap, gate=7)
        assert rc == 0 and (R.bits(gated) == R.bits(got)).all()
        stale = np.arange(n_partials, dtype=f32) - 3.5
        rc, kept = device_sumsq(g, gid, n_partials, cap, gate=0, before=stale)
        assert rc == 0 and (R.bits(kept) == R.bits(stale)).all()
        # the norm of the whole launch: within the derived relative bound of the float64 norm, and the finish contract on these partials
        want = 0.125 * math.sqrt(ref.sum())
        before = clip_words(max_norm=0.25 * want, grad_scale=0.125, norm=-1.0, coef=-1.0, skipped=2)
        rc, after = device_finish(got, before)
        assert rc == 0
        s = check_finish("finish %s n=%d" % (kind, n), got, before, after)
        assert abs(float(s["norm"]) - want) <= R.norm_bound_rel(n, n_partials, cap) * want and 0.0 < float(s["coef"]) < 1.0


def test_sumsq_ignores_255_stretches():
    n = 6152
    g = R.sumsq_inputs("randn", n)
    gid = R.group_bytes(n, 2, holes_of(n // 8))
    g[np.repeat(gid == 255, 8)] = 1e30                            # (1e30^2 overflows fp32: counted once, the partial is inf)
    ref, bound, active = R.sumsq_contract(g, gid, 4, 2)
    rc, got = device_sumsq(g, gid, 4, 2)
    assert rc == 0 and R.ratio(got[:active], ref[:active], bound[:active]) <= 1.0 and (R.bits(got[active:]) == 0).all()


FINISH_EDGES = {
    "zero gradient": (np.zeros(5, f32), 1.0, 1.0),
    "max_norm inf": (np.full(300, 1e-6, f32), math.inf, 1.0),
    "norm below max_norm": (np.full(300, 1e-6, f32), 1.0, 1.0),
    "norm above max_norm": (np.full(300, 4.0, f32), 1.0, 0.5),
    "overflow with finite partials": (np.full(7, 3e38, f32), 1.0, 1e20),
    "inf partial": (np.array([1, np.inf, 1], f32), 1.0, 1.0),
    "nan partial": (np.array([1, 1, np.nan, 1], f32), math.inf, 1.0),
}


def test_clip_finish_edges_and_the_running_count():
    skipped = 5
    for tag, (part, max_norm, gs) in FINISH_EDGES.items():
        before = clip_words(max_norm, gs, norm=-1.0, coef=-1.0, skip=3, skipped=skipped)
        rc, after = device_finish(part, before)
        assert rc == 0
        s = check_finish(tag, part, before, after)
        bad = tag in ("overflow with finite partials", "inf partial", "nan partial")
        assert s["skip"] == int(bad) and s["skipped"] == skipped + int(bad) and (float(s["coef"]) == 0.0) == bad
        skipped = s["skipped"]
        rc, gated = device_finish(part, before, gate=-1)
        assert rc == 0 and (gated == after).all()
        rc, kept = device_finish(part, before, gate=0)
        assert rc == 0 and (kept == before).all()
    assert skipped == 8
    for tag in ("zero gradient", "max_norm inf", "norm below max_norm"):          # nothing to clip: the coefficient is exactly 1
        part, max_norm, gs = FINISH_EDGES[tag]
        assert float(read_state(device_finish(part, clip_words(max_norm, gs))[1])["coef"]) == 1.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_write_nothing():
    """(group bytes >= n_groups other than 255 are the caller's contract and are not passed here)"""
    n = 2056
    a, groups = arena(n), R.groups_f32("two", 1, 1.0)
    gid = R.group_bytes(n, 2)
    B = {k: Buf(a[k]) for k in ("p", "g", "m", "v", "ema", "shadow")}
    I, GD, C = Buf(gid), Buf(groups.reshape(-1)), Buf(clip_words())
    big = np.zeros((17, 8), f32)
    big[:2] = groups
    G17 = Buf(big.reshape(-1))
    st = stream()

    def call(entry, n_=n, G=2, cap=0, clip=True, **over):
        p = {k: B[k].ptr for k in B}
        p.update(gid=I.ptr, groups=groups.ctypes.data if entry in ("flat", "clip_host") else GD.ptr)
        p.update(over)
        head = [p[k] for k in ("p", "g", "m", "v", "shadow", "ema")] + [0.99, p["gid"], p["groups"]]
        if entry == "flat":
            return L().vr_adamw_flat(*head, G, n_, st)
        if entry == "dev":
            return L().vr_adamw_flat_dev(*head, G, n_, st)
        if entry == "capped":
            return L().vr_adamw_flat_dev_capped(*head, G, n_, cap, st)
        return L().vr_adamw_flat_clip(*head, int(entry == "clip_dev"), G, n_, C.ptr if clip else None, cap, st)

    for entry in ENTRIES:
        for k in ("p", "g", "m", "v", "gid", "groups"):
            assert call(entry, **{k: None}) == R.VR_EINVAL, (entry, k)
        assert call(entry, n_=0) == R.VR_EINVAL and call(entry, n_=-8) == R.VR_EINVAL and call(entry, G=0) == R.VR_EINVAL
        assert call(entry, n_=n - 4) == R.VR_EALIGN and call(entry, n_=12) == R.VR_EALIGN
        for k in ("p", "g", "m", "v", "ema"):
            assert call(entry, **{k: B[k].ptr + 4}) == R.VR_EALIGN, (entry, k)
        assert call(entry, shadow=B["shadow"].ptr + 4) == R.VR_EALIGN
        assert call(entry, G=17, groups=big.ctypes.data if entry in ("flat", "clip_host") else G17.ptr) == R.VR_EUNSUPPORTED
    assert call("capped", cap=-1) == R.VR_EINVAL
    for entry in ("clip_host", "clip_dev"):
        assert call(entry, cap=-1) == R.VR_EINVAL and call(entry, clip=False) == R.VR_EINVAL
    # the norm launches
    P, W = Buf(R.canary32(4)), Buf(np.array([1], np.int32))
    g_, i_ = B["g"].ptr, I.ptr
    sumsq, gated = L().vr_grad_sumsq, L().vr_grad_sumsq_gated
    assert sumsq(None, i_, n, P.ptr, 4, 0, st) == R.VR_EINVAL and sumsq(g_, None, n, P.ptr, 4, 0, st) == R.VR_EINVAL
    assert sumsq(g_, i_, n, None, 4, 0, st) == R.VR_EINVAL and sumsq(g_, i_, 0, P.ptr, 4, 0, st) == R.VR_EINVAL
    assert sumsq(g_, i_, n, P.ptr, 0, 0, st) == R.VR_EINVAL and sumsq(g_, i_, n, P.ptr, 4, -1, st) == R.VR_EINVAL
    assert sumsq(g_, i_, n - 4, P.ptr, 4, 0, st) == R.VR_EALIGN and sumsq(g_ + 4, i_, n - 8, P.ptr, 4, 0, st) == R.VR_EALIGN
    assert gated(g_, i_, n, P.ptr, 4, 0, None, st) == R.VR_EINVAL and gated(g_, i_, n, P.ptr, 4, 0, W.ptr + 2, st) == R.VR_EALIGN
    assert gated(g_, i_, n, P.ptr, 4, -1, W.ptr, st) == R.VR_EINVAL
    fin, fing = L().vr_clip_finish, L().vr_clip_finish_gated
    assert fin(None, 4, C.ptr, st) == R.VR_EINVAL and fin(P.ptr, 4, None, st) == R.VR_EINVAL and fin(P.ptr, 0, C.ptr, st) == R.VR_EINVAL
    assert fin(P.ptr, 4, C.ptr + 2, st) == R.VR_EALIGN
    assert fing(P.ptr, 4, C.ptr, None, st) == R.VR_EINVAL and fing(None, 4, C.ptr, W.ptr, st) == R.VR_EINVAL
    assert fing(P.ptr, 4, C.ptr + 2, W.ptr, st) == R.VR_EALIGN and fing(P.ptr, 4, C.ptr, W.ptr + 2, st) == R.VR_EALIGN
    # nothing was launched: every buffer, guard zones included, holds what it held
    for k in B:
        assert (R.bits(B[k].get()) == R.bits(a[k])).all(), k
    assert (I.get() == gid).all() and (R.bits(GD.get()) == R.bits(groups.reshape(-1))).all() and (C.get() == clip_words()).all()
    assert (R.bits(P.get()) == R.CANARY32).all() and W.get()[0] == 1 and (R.bits(G17.get()) == R.bits(big.reshape(-1))).all()


# ---- through FlatAdamW ----------------------------------------------------------------------------------------------------------------------------
def micro_model():
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30, single_arch=False,
              hybrid_arch=False)
    nd = recipe.MICRO_DEFS[0]
    prod = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                               num_classes=recipe.MICRO_CLASSES, network_def=nd, drop_path_rate=0.0, drop_block_rate=None, **kw)
    orc = O.OracleViTSR(nd, img_size=recipe.MICRO_IMG, num_classes=recipe.MICRO_CLASSES, supernet=True, patch_output=True, **kw)
    sd = recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in orc.state_dict().items()], 100)
    prod.load_state_dict(sd)
    prod = prod.to(DEV)
    prod.set_compute_dtype(torch.bfloat16)
    prod.train()
    prod.set_epoch(31)
    prod.load_state_dict(sd)
    return prod


def test_flat_adamw_keeps_padding_zero_frozen_parameters_untouched_and_reports_the_float64_norm():
    """three steps on the micro model with one parameter of each group left out of the optimizer (its groups of eight are 255): the padding
    words behind parameters whose size is no multiple of 8 stay exactly 0 in the parameters, the gradient and both moments, the 255 regions
    keep every bit, and grad_norm() is the float64 norm over the optimizer's own parameters within the derived bound"""
    model = micro_model()
    crit = SoftTargetCrossEntropy()
    x, t, pt, _ = (v.to(DEV) for v in recipe.inputs(7, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1))
    spec = engine.param_groups_weight_decay(model, 0.05)
    frozen = [grp["params"].pop(len(grp["params"]) // 2) for grp in spec]
    opt = FlatAdamW(model, spec, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, ema_decay=0.99, max_norm=float("inf"))
    a = opt._bind()
    n = a["flat"].numel()
    own = torch.zeros(n, dtype=torch.bool)
    dead = torch.zeros(n, dtype=torch.bool)
    for p, (off, cnt) in zip(a["params"], a["offsets"]):
        (dead if any(p is q for q in frozen) else own)[off:off + cnt] = True
        if any(p is q for q in frozen):
            dead[off:(off + cnt + 7) // 8 * 8] = True
    pad = ~own & ~dead
    gid = opt._flat_state["gid"].cpu()
    assert int(pad.sum()) > 0 and int(dead.sum()) > 0 and bool((gid.repeat_interleave(8) == 255)[dead].all())
    assert bool((gid.repeat_interleave(8) != 255)[own | pad].all())               # the padding behind a live parameter IS updated
    words = lambda t_: t_.detach().cpu().view(torch.int32)                              # noqa: E731
    flat0, ema0 = words(a["flat"]).clone(), words(opt._flat_state["ema"]).clone()
    count = min((n // 8 + 255) // 256, NORM_PARTIALS)
    for it in range(3):
        torch.manual_seed(300 + it)
        model.zero_grad(set_to_none=True)                           # (the parameters left out of the optimizer too)
        out = model(x, patch_output_type="seq")
        (crit(out[0], t) + crit(out[1], pt)).backward()
        opt.step()
        torch.cuda.synchronize()
        g = a["gcur"].detach().cpu()
        want = float(torch.sqrt((g.double()[own] ** 2).sum()))
        got = float(opt.grad_norm())
        rel = abs(got - want) / want
        print("OPTIM FlatAdamW step %d: norm %.9g float64 %.9g rel.err %.3g bound %.3g" % (it, got, want, rel, R.norm_bound_rel(n, count)))
        assert rel <= R.norm_bound_rel(n, count)
        st = opt._flat_state
        for name, buf in (("flat", a["flat"]), ("grad", a["gcur"]), ("m", st["m"]), ("v", st["v"])):
            assert bool((words(buf)[pad] == 0).all()), "padding of %s at step %d" % (name, it)
        assert torch.equal(words(a["flat"])[dead], flat0[dead]) and torch.equal(words(st["ema"])[dead], ema0[dead])
        assert bool((words(st["m"])[dead] == 0).all()) and bool((words(st["v"])[dead] == 0).all())
        assert not torch.equal(words(a["flat"])[own], flat0[own])
    assert opt.skipped_steps() == 0


def test_zz_worst_ratios():
    for key in sorted(R.WORST, key=str):
        print("OPTIM WORST %-18s %-10s err/bound %.3f" % (key[0], key[1], R.WORST[key]))
    assert not R.WORST or max(R.WORST.values()) <= 1.0
