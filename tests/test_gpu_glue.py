"""The glue kernels of csrc/misc.hip against the contracts of tests/glue_ref64.py: casts, cast_transpose, zero_ranges, the re-layouts,
column / batch / token sums, scale_mask_cast, the two im2col forms, embed_cls, mask_rows and the spatial-reduction pieces, on every
form and pass count their launchers can take (the literal tables below), at the smallest shapes that reach them.

Exact contracts compare as integers; bounded ones per element against first-principles bounds.  Every output is a view into a larger
allocation whose guard zones, pad columns and untouched rows hold one NaN bit pattern that must still be there afterwards, and every
input region a kernel must not read into a result holds NaN.  Calls go through the C ABI with buffers the test owns.

`pytest -s` prints one line per case (GLUE ...) and, last, the worst error / bound per bounded kernel."""
import ctypes

import pytest
import torch

import glue_ref64 as R
import vitres.kernels as K
from glue_ref64 import BF16, F16, F32
from vitres import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---- the launch paths, read from misc.hip ------------------------------------------------------------------------------------------------------
# n -> (workgroups, groups of eight on the vector form, trailing elements on the scalar form, passes).  The workgroup count comes from
# n / 8 rounded DOWN, so a tail behind a whole number of workgroups (2049, 4099) is a second grid-stride pass of thread 0, long before the
# 4096-workgroup cap makes one at 8 388 608 elements.
CAST_PATHS = {1: (1, 0, 1, 1), 7: (1, 0, 7, 1), 8: (1, 1, 0, 1), 9: (1, 1, 1, 1), 2047: (1, 255, 7, 1), 2048: (1, 256, 0, 1),
              2049: (1, 256, 1, 2), 4099: (2, 512, 3, 2), 8388637: (4096, 1048579, 5, 2)}
# index into R.CT_SHAPES -> (wide tiles, ragged tiles)
CT_PATHS = {0: (2, 0), 1: (0, 1), 2: (0, 2), 3: (0, 1), 4: (0, 1), 5: (0, 1), 6: (1, 3), 7: (0, 1), 8: (0, 1), 9: (1, 0)}
# (word address, count, workgroups) -> (head, float4 count, x4 iterations of thread 0, of the last thread, remainder iterations of thread 0, tail)
ZERO_PATHS = {(4, 4096, 1): (0, 1024, 1, 1, 0, 0), (5, 4096, 1): (3, 1023, 1, 0, 0, 1), (4, 4092, 1): (0, 1023, 1, 0, 0, 0),
              (4, 4100, 1): (0, 1025, 1, 1, 1, 0), (4, 4101, 1): (0, 1025, 1, 1, 1, 1), (4, 8192, 2): (0, 2048, 1, 1, 0, 0),
              (7, 8188, 2): (1, 2046, 1, 0, 0, 3), (5, 3, 25): (3, 0, 0, 0, 0, 0), (16, 100000, 25): (0, 25000, 1, 0, 0, 0),
              (107, 2, 1): (1, 0, 0, 0, 0, 1), (49, 1, 1): (1, 0, 0, 0, 0, 0), (85, 2, 1): (2, 0, 0, 0, 0, 0), (208, 5, 1): (0, 1, 0, 0, 1, 1),
              (26, 0, 1): (0, 0, 0, 0, 0, 0)}
# (A, B, C) -> (workgroups, passes)
RELAYOUT_PATHS = {(3, 5, 7): (1, 1), (4, 1, 37): (1, 1), (1, 1, 1000): (4, 1), (2, 9, 4): (1, 1), (5, 3, 1): (1, 1), (1, 300, 3): (4, 1),
                  (3, 7, 49933): (4096, 2)}
# (Cin, W, P) -> load form; the store form is "st8" for a 16-bit type with ldk % 8 == 0 and a 16-byte aligned col, else "st1"
PATCH_LOADS = {(3, 6, 2): "ld1", (3, 4, 2): "ld4", (3, 21, 7): "ld1", (3, 42, 14): "ld1", (3, 28, 14): "ld4", (2, 48, 16): "ld4"}
PATCH_STORES = {(12, F32, 0): "st1", (16, F32, 0): "st1", (12, BF16, 0): "st1", (16, BF16, 0): "st8", (16, F16, 0): "st8", (15, F16, 0): "st1",
                (16, BF16, 1): "st1", (592, BF16, 0): "st8", (588, BF16, 0): "st1", (512, F16, 0): "st8", (512, F16, 1): "st1"}
# (B, g, C, dtype, y offset, col offset) -> (form, workgroups, passes)
SR_IM2COL_PATHS = {(2, 2, 8, BF16, 0, 0): ("v8", 1, 1), (2, 14, 72, F16, 0, 0): ("v8", 32, 1), (2, 4, 76, BF16, 0, 0): ("scalar", 72, 1),
                   (2, 4, 72, F32, 0, 0): ("scalar", 72, 1), (2, 4, 72, BF16, 1, 0): ("scalar", 72, 1), (2, 4, 72, F16, 0, 4): ("scalar", 72, 1),
                   (9512, 14, 8, BF16, 0, 0): ("v8", 16384, 2)}
SR_COL2IM_PATHS = {(2, 2, 8, BF16, 0, 0): ("v8", 1, 1), (2, 14, 72, BF16, 0, 0): ("v8", 14, 1), (2, 4, 100, BF16, 0, 0): ("scalar", 32, 1),
                   (2, 4, 72, F32, 0, 0): ("scalar", 32, 1), (2, 4, 72, BF16, 0, 1): ("scalar", 32, 1), (2, 4, 72, BF16, 4, 0): ("scalar", 32, 1),
                   (2, 4, 72, F16, 0, 0): R.VR_EUNSUPPORTED, (21400, 14, 8, BF16, 0, 0): ("v8", 16384, 2)}
# M -> (row chunks of 128, rows of the last chunk); N -> column groups of 256
COLSUM_ROWS = {1: (1, 1), 127: (1, 127), 128: (1, 128), 129: (2, 1), 300: (3, 44)}
COLSUM_COLS = {1: 1, 255: 1, 256: 1, 257: 2}
# B -> (bper, chunks, {(unrolled steps of eight, remainder) of the first and the last chunk})
BATCHSUM_PATHS = {1: (1, 1, {(0, 1)}), 7: (7, 1, {(0, 7)}), 8: (8, 1, {(1, 0)}), 9: (9, 1, {(1, 1)}), 15: (15, 1, {(1, 7)}),
                  16: (8, 2, {(1, 0)}), 17: (8, 3, {(1, 0), (0, 1)}), 23: (8, 3, {(1, 0), (0, 7)}), 63: (8, 8, {(1, 0), (0, 7)}),
                  64: (16, 4, {(2, 0)}), 65: (16, 5, {(2, 0), (0, 1)})}
# scale_mask_cast: M -> workgroups of four rows; C -> (float4 steps per lane, lanes live in a partial last step)
SMC_ROWS = {1: 1, 3: 1, 4: 1, 5: 2, 9: 3}
SMC_COLS = {4: (1, 1), 252: (1, 63), 256: (1, 0), 260: (2, 1), 1028: (5, 1)}
# token_mean: C -> (columns per thread, threads live in a partial last step)
TM_COLS = {1: (1, 1), 255: (1, 255), 256: (1, 0), 257: (2, 1), 520: (3, 8)}


def test_path_tables_match_the_code_and_cover_every_path():
    check_path_tables()


def check_path_tables():
    """shared with the host suite, which runs it without a device"""
    assert set(CAST_PATHS) == set(R.CAST_N) | {R.CAST_BIG} and all(R.cast_path(n) == v for n, v in CAST_PATHS.items())
    assert {(v[1] > 0, v[2] > 0, v[3]) for v in CAST_PATHS.values()} == {(False, True, 1), (True, False, 1), (True, True, 1), (True, True, 2)}
    descs = R.ct_layout()[0]
    assert set(CT_PATHS) == set(range(len(R.CT_SHAPES))) and all(R.ct_path(descs[i]) == v for i, v in CT_PATHS.items())
    assert {(w > 0, r > 0) for w, r in CT_PATHS.values()} == {(True, False), (False, True), (True, True)}
    tiles = [w + r for w, r in CT_PATHS.values()]
    assert min(tiles) == 1 and max(tiles) > 1                                     # workgroups that return early exist
    assert all(R.zero_path(*k) == v for k, v in ZERO_PATHS.items())
    seen = set()
    for _, base, ranges in R.zero_launches():
        bx = R.zero_bx([c for _, c in ranges])
        for lo, cnt in ranges:
            seen.add((base + lo, cnt, bx))
    assert set(ZERO_PATHS) <= seen
    paths = {k: R.zero_path(*k) for k in seen}
    assert {v[0] for v in paths.values()} == {0, 1, 2, 3} and {v[5] for v in paths.values()} == {0, 1, 2, 3}
    assert {(v[2], v[3]) for v in paths.values()} >= {(0, 0), (1, 1), (1, 0)}      # the x4 loop: not at all, once for all, once for some
    assert {v[4] for v in paths.values()} >= {0, 1}
    assert any(k[1] in (1, 2) and v[0] == k[1] and (4 - (k[0] & 3)) & 3 > k[1] for k, v in paths.items())   # the head capped at count
    assert any(k[2] > 1 and k[1] < 4 for k in seen)                                # a short range in a long one's launch
    assert set(RELAYOUT_PATHS) == {c[:3] for c in R.RELAYOUT_CASES} | {R.RELAYOUT_BIG}
    assert all(R.relayout_path(*k) == v for k, v in RELAYOUT_PATHS.items()) and {v[1] for v in RELAYOUT_PATHS.values()} == {1, 2}
    assert set(PATCH_LOADS) == {(c, w, p) for c, _, w, p in R.PATCH_GEOM}
    assert all(R.im2col_patch_path(c, w, p, c * p * p, F32)[0] == v for (c, w, p), v in PATCH_LOADS.items())
    assert all(R.im2col_patch_path(3, 4, 2, ldk, dt, off)[1] == v for (ldk, dt, off), v in PATCH_STORES.items())
    assert set(PATCH_LOADS.values()) == {"ld1", "ld4"} and set(PATCH_STORES.values()) == {"st1", "st8"}
    assert {(dt, v) for (_, dt, _), v in PATCH_STORES.items()} >= {(BF16, "st1"), (BF16, "st8"), (F16, "st1"), (F16, "st8"), (F32, "st1")}
    assert {p for _, _, _, p in R.PATCH_GEOM} == {2, 7, 14, 16}
    assert R.im2col_patch_path(3, 352, 16, 768, F32) == R.VR_EUNSUPPORTED
    assert all(R.sr_im2col_path(*k) == v for k, v in SR_IM2COL_PATHS.items())
    assert all(R.sr_col2im_path(*k) == v for k, v in SR_COL2IM_PATHS.items())
    assert {(k[3], v[0], v[2]) for k, v in SR_IM2COL_PATHS.items()} >= {(BF16, "v8", 1), (F16, "v8", 1), (BF16, "scalar", 1), (F32, "scalar", 1),
                                                                         (F16, "scalar", 1), (BF16, "v8", 2)}
    assert {(k[3], v[0], v[2]) for k, v in SR_COL2IM_PATHS.items() if v != R.VR_EUNSUPPORTED} == {(BF16, "v8", 1), (BF16, "scalar", 1),
                                                                                                  (F32, "scalar", 1), (BF16, "v8", 2)}
    assert R.SR_IM2COL_BIG + (BF16, 0, 0) in SR_IM2COL_PATHS and R.SR_COL2IM_BIG + (BF16, 0, 0) in SR_COL2IM_PATHS
    assert {c % 8 == 0 for c in R.SR_C} == {True, False}
    assert set(COLSUM_ROWS) == set(R.COLSUM_M) and set(COLSUM_COLS) == set(R.COLSUM_N)
    assert all(R.colsum_path(m, n) == (COLSUM_COLS[n],) + COLSUM_ROWS[m] for m in COLSUM_ROWS for n in COLSUM_COLS)
    assert set(BATCHSUM_PATHS) == set(R.BATCHSUM_B) and all(R.batchsum_path(b, 1) == v for b, v in BATCHSUM_PATHS.items())
    assert {v[0] for v in BATCHSUM_PATHS.values()} == {1, 7, 8, 9, 15, 16}
    assert set().union(*(v[2] for v in BATCHSUM_PATHS.values())) >= {(0, 1), (0, 7), (1, 0), (1, 1), (1, 7), (2, 0)}
    assert set(SMC_ROWS) == set(R.SMC_M) and set(SMC_COLS) == set(R.SMC_C)
    assert all(R.scale_mask_cast_path(m, c) == (SMC_ROWS[m],) + SMC_COLS[c] for m in SMC_ROWS for c in SMC_COLS)
    assert set(TM_COLS) == set(R.TM_C) and all(R.token_mean_path(2, c) == (2,) + v for c, v in TM_COLS.items())


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------
def L():
    return _lib.lib()


_LIVE = []


def cu(t):
    """upload; the device tensor stays alive until the test ends (launches only get its address)"""
    if t is None:
        return None
    _LIVE.append(t.to(DEV))
    return _LIVE[-1]


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                      # a device error: nothing more is launched in this session
        pytest.exit("the device reported an error, the run ends here: %s" % e, returncode=3)
    _LIVE.clear()


def ptr(t):
    return None if t is None else t.data_ptr()


class Buf:
    """a tensor inside canary guard zones on the device; get() checks the zones and returns the contents on the CPU"""

    def __init__(self, before, off=0):
        self.n, self.off = before.numel(), off
        self.whole, self.view = R.guarded(before, off, DEV)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        torch.cuda.synchronize()
        assert R.guards_intact(self.whole, self.n, self.off), "a guard zone was written"
        return self.view.cpu()


def exact(tag, got, exp):
    bad = R.mismatches(got, exp)
    n = int(bad.sum())
    print("GLUE %-58s exact %d elements, %d wrong" % (tag, got.numel(), n))
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d elements differ, first at flat index %d: got 0x%x, expected 0x%x"
                             % (tag, n, i, int(R.ibits(got).reshape(-1)[i]) & 0xffffffff, int(R.ibits(exp).reshape(-1)[i]) & 0xffffffff))


def bounded(kernel, tag, got, ref, b32, dtype=F32):
    r = R.record(kernel, R.ratio(got, ref, R.out_bound(ref, b32, dtype)))
    print("GLUE %-58s err/bound %.3f" % (tag, r))
    assert r <= 1.0, (tag, r)


def stream():
    return K._stream()


def code(dt):
    return K._dtcode(dt)


# ---- casts --------------------------------------------------------------------------------------------------------------------------------------
CASTS = {BF16: "vr_cast_f32_bf16", F16: "vr_cast_f32_f16"}


def run_cast(dt, src, n):
    o = Buf(R.canary(n, dt))
    s = Buf(src[:n])
    rc = getattr(L(), CASTS[dt])(s.ptr, o.ptr, n, stream())
    return rc, o.get()


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_body_and_tail(n, dt):
    """the packed converter of the vector body and the C++ converter of the tail against torch's CPU cast; edge values in both where they fit"""
    tail0 = n - n % 8
    src = R.with_edges(R.pattern32(n, n), [0, tail0] + ([64] if n > 200 else []))
    rc, got = run_cast(dt, src, n)
    assert rc == 0
    exact("cast %s n=%d" % (R.name(dt), n), got, R.cast_contract(R.canary(n, dt), src, n))


@pytest.mark.parametrize("dt", [BF16, F16])
def test_cast_every_edge_value_in_the_vector_body_and_in_the_scalar_tail(dt):
    """all edge values in the body (groups of eight) and seven of them at a time in the n % 8 tail of the same launch"""
    e = R.edge_values()
    body = torch.cat([e, R.pattern32(-e.numel() % 8)])
    for k in range(0, e.numel(), 7):
        src = torch.cat([body, e[k:k + 7]])
        n = src.numel()
        assert n % 8 == e[k:k + 7].numel() and R.cast_path(n)[1] == body.numel() // 8
        rc, got = run_cast(dt, src, n)
        assert rc == 0
        exp = R.cast_contract(R.canary(n, dt), src, n)
        exact("cast %s edges, tail = edges %d.." % (R.name(dt), k), got, exp)
        assert not R.mismatches(got[body.numel():], got[k:k + len(got) - body.numel()]).any()     # the two converters agree


@pytest.mark.parametrize("dt", [BF16, F16])
def test_cast_second_pass_equals_single_pass_pieces(dt):
    n = R.CAST_BIG
    src = R.with_edges(R.pattern32(n), [8388608 - 16, n - 5 - 48])
    s = cu(src)
    big = Buf(R.canary(n, dt))
    assert getattr(L(), CASTS[dt])(ptr(s), big.ptr, n, stream()) == 0
    pieces = Buf(R.canary(n, dt))
    for lo, hi in ((0, 4194304), (4194304, n)):
        assert R.cast_path(hi - lo)[3] == 1
        assert getattr(L(), CASTS[dt])(s[lo:].data_ptr(), pieces.view[lo:].data_ptr(), hi - lo, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(R.ibits(big.view), R.ibits(pieces.view))
    exact("cast %s n=%d (two passes), pieces" % (R.name(dt), n), pieces.get(), R.cast_contract(R.canary(n, dt), src, n))
    big.get()


def test_cast_transpose_wide_and_ragged_tiles_in_one_launch():
    descs, ns, nd = R.ct_layout()
    src = R.canary(ns, F32)                                    # gaps between the matrices are NaN
    for i, (so, do, r, c, ld) in enumerate(descs):
        src[so:so + r * c] = R.with_edges(R.pattern32(r * c, i), [0, r * c // 2])
    d = Buf(R.canary(nd, BF16))
    s = Buf(src)
    dev = K.tr_descs(descs, DEV)
    assert dev[1] == max(w + r for w, r in CT_PATHS.values())
    rc = L().vr_cast_transpose_batch(s.ptr, d.ptr, ptr(dev[0]), len(descs), dev[1], stream())
    assert rc == 0
    exact("cast_transpose %d matrices" % len(descs), d.get(), R.cast_transpose_contract(R.canary(nd, BF16), src, descs))


# ---- zero_ranges --------------------------------------------------------------------------------------------------------------------------------
def zero_struct(ranges, n=None):
    zr = _lib.ZeroRanges()
    zr.n = len(ranges) if n is None else n
    for j, (lo, cnt) in enumerate(ranges[:_lib.MAX_ZERO_RANGES]):
        zr.lo[j], zr.count[j] = lo, cnt
    return zr


def run_zero(base, ranges, gate=None):
    """-> rc, words before, words after (int32, CPU); the buffer's float view is what the kernel gets"""
    n = base + max([lo + c for lo, c in ranges if lo >= 0] + [8]) + 8
    before = R.zero_words(n)
    b = Buf(before)
    zr = zero_struct(ranges)
    p = b.view[base:].data_ptr()
    if gate is None:
        rc = L().vr_zero_ranges(p, ctypes.byref(zr), stream())
    else:
        rc = L().vr_zero_ranges_gated(p, ctypes.byref(zr), ptr(gate), stream())
    return rc, before, b.get()


@pytest.mark.parametrize("gated", [False, True])
def test_zero_ranges_head_body_tail_at_their_boundaries(gated):
    gate = torch.ones(1, dtype=torch.int32, device=DEV) if gated else None
    for tag, base, ranges in R.zero_launches():
        rc, before, after = run_zero(base, ranges, gate)
        assert rc == 0
        exact("zero_ranges%s %s, %d ranges from word %d" % ("_gated" if gated else "", tag, len(ranges), base + ranges[0][0]), after,
              R.zero_ranges_contract(before, base, ranges))


def test_zero_ranges_gate_zero_leaves_every_bit():
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    for tag, base, ranges in R.zero_launches()[:3]:
        rc, before, after = run_zero(base, ranges, gate)
        assert rc == 0
        exact("zero_ranges_gated gate=0 %s" % tag, after, R.zero_ranges_contract(before, base, ranges, gate=0))
        assert torch.equal(after, before)


def test_zero_ranges_wrapper_splits_25_ranges_into_two_launches():
    spans = [(9 * i + (i & 3), 9 * i + (i & 3) + 5) for i in range(25)]
    before = R.zero_words(9 * 25 + 16)
    b = Buf(before.view(F32))
    K.zero_ranges(b.view, spans)
    exact("zero_ranges wrapper, 25 ranges", b.get().view(torch.int32), R.zero_ranges_contract(before, 0, [(lo, hi - lo) for lo, hi in spans]))


# ---- relayout, relayout_add, conv_w_flip ----------------------------------------------------------------------------------------------------------
def relayout_src(A, B, C, src_ld, dt, salt):
    """[A, src_ld] flat: payload from the flat index (edge values for fp32 sources), NaN in the pad columns"""
    src = R.canary(A * src_ld, dt).view(A, src_ld)
    vals = R.pattern(A * B * C, dt, salt)
    if dt == F32:
        vals = R.with_edges(vals, [0, A * B * C // 2])
    src[:, :B * C] = vals.view(A, B * C)
    return src.view(-1)


@pytest.mark.parametrize("sd,dd", R.RELAYOUT_PAIRS)
def test_relayout_every_type_pair(sd, dd):
    for A, B, C, sp, dp in R.RELAYOUT_CASES:
        src_ld, dst_ld = B * C + sp, B * C + dp
        src = relayout_src(A, B, C, src_ld, sd, A + C)
        s, d = Buf(src), Buf(R.canary(A * dst_ld, dd))
        rc = L().vr_relayout(s.ptr, d.ptr, A, B, C, src_ld, dst_ld, code(sd), code(dd), stream())
        assert rc == 0
        exact("relayout %s->%s A%d B%d C%d ld %d->%d" % (R.name(sd), R.name(dd), A, B, C, src_ld, dst_ld), d.get(),
              R.relayout_contract(R.canary(A * dst_ld, dd), src, A, B, C, src_ld, dst_ld))


def int_payload(n):
    """int32 words that are signalling NaNs, denormals, infinities, -0 and plain integers when read as fp32"""
    w = R.zero_words(n).clone()
    special = torch.tensor([0x7f800001 - 2 ** 32 * 0, 0x7fa00000, -0x7fffff, 0x00000001, 0x007fffff, -0x80000000, 0x7f800000, -0x800000, 0x7fffffff,
                            -1, 0, 1, 196, 0x00400000], dtype=torch.int64)
    special = torch.where(special >= 2 ** 31, special - 2 ** 32, special).to(torch.int32)
    w[:special.numel()] = special
    w[n // 2:n // 2 + special.numel()] = special[:max(0, min(special.numel(), n - n // 2))]
    return w


def test_relayout_f32_preserves_every_int32_bit_pattern():
    """what copy_i32_from_pinned relies on: the fp32 -> fp32 form moves words, signalling NaNs and denormals included"""
    for A, B, C, sp, dp in R.RELAYOUT_CASES:
        src_ld, dst_ld = B * C + sp, B * C + dp
        src = int_payload(A * src_ld)
        s, d = Buf(src), Buf(R.canary(A * dst_ld, torch.int32))
        assert L().vr_relayout(s.ptr, d.ptr, A, B, C, src_ld, dst_ld, code(F32), code(F32), stream()) == 0
        got, exp = d.get(), R.relayout_contract(R.canary(A * dst_ld, torch.int32), src, A, B, C, src_ld, dst_ld)
        print("GLUE relayout int32 payload A%d B%d C%d" % (A, B, C))
        assert torch.equal(got, exp)
    host = int_payload(1000).pin_memory()
    d = Buf(R.canary(1000, torch.int32))
    K.copy_i32_from_pinned(host, d.view)
    assert torch.equal(d.get(), host)


def test_relayout_add_is_one_fp32_add():
    for A, B, C, sp, dp in R.RELAYOUT_CASES + [(1, 1, 4099, 0, 0)]:
        src_ld, dst_ld = B * C + sp, B * C + dp
        src = relayout_src(A, B, C, src_ld, F32, 3)
        before = R.canary(A * dst_ld, F32).view(A, dst_ld)
        before[:, :B * C] = R.pattern32(A * B * C, 11).view(A, B * C)
        before = before.view(-1)
        s, d = Buf(src), Buf(before)
        assert L().vr_relayout_add(s.ptr, d.ptr, A, B, C, src_ld, dst_ld, stream()) == 0
        got, exp = d.get(), R.relayout_add_contract(before, src, A, B, C, src_ld, dst_ld)
        exact("relayout_add A%d B%d C%d ld %d->%d" % (A, B, C, src_ld, dst_ld), got, exp)
        fin = ~torch.isnan(exp)
        assert torch.equal(got[fin], exp[fin])


@pytest.mark.parametrize("dd", [F32, BF16])
def test_relayout_second_pass_equals_single_pass_pieces(dd):
    A, B, C = R.RELAYOUT_BIG
    ld = B * C
    src = R.with_edges(R.pattern32(A * ld), [1048576 - 20, A * ld - 44])
    s = cu(src)
    big, pieces = Buf(R.canary(A * ld, dd)), Buf(R.canary(A * ld, dd))
    assert L().vr_relayout(ptr(s), big.ptr, A, B, C, ld, ld, code(F32), code(dd), stream()) == 0
    for a in range(A):
        assert R.relayout_path(1, B, C)[1] == 1
        assert L().vr_relayout(s[a * ld:].data_ptr(), pieces.view[a * ld:].data_ptr(), 1, B, C, ld, ld, code(F32), code(dd), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(R.ibits(big.view), R.ibits(pieces.view))
    exact("relayout f32->%s A%d B%d C%d (two passes), pieces" % (R.name(dd), A, B, C), pieces.get(),
          R.relayout_contract(R.canary(A * ld, dd), src, A, B, C, ld, ld))
    big.get()


@pytest.mark.parametrize("dd", [F32, BF16])
def test_conv_w_flip(dd):
    for Co, Ci in R.CONV_W_FLIP:
        src = R.with_edges(R.pattern32(Co * Ci * 9, Co), [0, 256]).view(Co, Ci, 3, 3)
        s, d = Buf(src), Buf(R.canary(Ci * 9 * Co, dd).view(Ci, 9 * Co))
        assert L().vr_conv_w_flip(s.ptr, d.ptr, Co, Ci, code(dd), stream()) == 0
        exact("conv_w_flip %s Co%d Ci%d" % (R.name(dd), Co, Ci), d.get(), R.conv_w_flip_contract(R.canary(Ci * 9 * Co, dd).view(Ci, 9 * Co), src))


# ---- colsum, batchsum -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum(M, dt):
    for N in R.COLSUM_N:
        for rm in (None, R.COLSUM_MAP):
            x, out0, ld = R.colsum_inputs(M, N, rm, dt)
            ref, b32 = R.colsum_ref(x, out0, M, N, rm)
            o = Buf(out0)
            rc = L().vr_colsum(ptr(cu(x)), o.ptr, M, N, ld, code(dt), _lib.RowMap(*(rm or (0, 0, 0))), stream())
            assert rc == 0
            bounded("colsum", "colsum %s M%d N%d ld%d %s" % (R.name(dt), M, N, ld, "mapped" if rm else "plain"), o.get(), ref, b32)


@pytest.mark.parametrize("B", R.BATCHSUM_B)
def test_batchsum(B):
    for inner in R.BATCHSUM_INNER:
        x, out0 = R.batchsum_inputs(B, inner)
        ref, b32 = R.batchsum_ref(x[:B], out0)
        o = Buf(out0)
        assert L().vr_batchsum(ptr(cu(x)), o.ptr, B, inner, stream()) == 0
        bounded("batchsum", "batchsum B%d inner%d" % (B, inner), o.get(), ref, b32)


# ---- scale_mask_cast --------------------------------------------------------------------------------------------------------------------------------
def smc_inputs(M, C, rps=2):
    """rows from the flat index with edge values; NaN in every column >= keep; sample 1's scale is 0 and its rows hold NaN and inf"""
    S = (M + rps - 1) // rps
    keep = R.smc_keep(C, S)
    scale = torch.tensor([1.0, 0.0, -0.5, 1.7, 3.0e-5])[torch.arange(S) % 5]
    x = R.with_edges(R.pattern32(M * C, M + C), [0, (M // 2) * C]).view(M, C).clone()
    if M > rps:
        x[rps, :2] = torch.tensor([float("nan"), float("inf")])
    return x, scale, keep


@pytest.mark.parametrize("dt", R.DT3)
@pytest.mark.parametrize("M", R.SMC_M)
def test_scale_mask_cast(M, dt):
    for C in R.SMC_C:
        x, scale, keep = smc_inputs(M, C)
        for sc, kp in ((scale, keep), (None, keep), (scale, None)):
            xin = x.clone()
            if kp is not None:
                s = torch.arange(M) // 2
                xin = torch.where(torch.arange(C).view(1, C) < kp[s].view(M, 1), xin, torch.full_like(xin, float("nan")))
            o = Buf(R.canary(M * C, dt).view(M, C))
            rc = L().vr_scale_mask_cast(ptr(cu(xin)), o.ptr, ptr(cu(sc)), ptr(cu(kp)), M, C, 2, code(dt), stream())
            assert rc == 0
            exact("scale_mask_cast %s M%d C%d %s%s" % (R.name(dt), M, C, "scale " if sc is not None else "", "keep" if kp is not None else ""),
                  o.get(), R.scale_mask_cast_contract(R.canary(M * C, dt).view(M, C), xin, sc, kp, 2))


# ---- token_mean ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DT3)
@pytest.mark.parametrize("n", R.TM_N)
def test_token_mean(n, dt):
    for first in R.TM_FIRST:
        for C in R.TM_C:
            y = R.token_inputs(first, n, C, dt)
            ref, b32 = R.token_mean_ref(y, first)
            o = Buf(R.canary(2 * C, dt).view(2, C))
            assert L().vr_token_mean(ptr(cu(y)), o.ptr, 2, first + n, C, first, code(dt), stream()) == 0
            bounded("token_mean", "token_mean %s first%d n%d C%d" % (R.name(dt), first, n, C), o.get(), ref, b32, dt)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("n", R.TM_N)
def test_token_mean_bwd(n, dt):
    for first in R.TM_FIRST:
        for C in R.TM_C:
            dmean = R.split_unit(2, C, n + C + first, dt)
            before = R.canary(2 * (first + n) * C, dt).view(2, first + n, C)
            o = Buf(before)
            assert L().vr_token_mean_bwd(ptr(cu(dmean)), o.ptr, 2, first + n, C, first, code(dt), stream()) == 0
            got = o.get()
            ref, b32 = R.token_mean_bwd_ref(dmean, n)
            exact("token_mean_bwd %s first%d n%d C%d: rows below first" % (R.name(dt), first, n, C), got[:, :first], before[:, :first])
            bounded("token_mean_bwd", "token_mean_bwd %s first%d n%d C%d" % (R.name(dt), first, n, C), got[:, first:],
                    ref[:, None, :].expand(2, n, C), b32[:, None, :].expand(2, n, C), dt)


# ---- im2col_patch -------------------------------------------------------------------------------------------------------------------------------------
def patch_image(Cin, H, W, B=3):
    img = R.pattern32(B * Cin * H * W, H + W).view(B, Cin, H, W).clone()
    img.view(B, -1)[0, :R.edge_values().numel()] = R.edge_values()[:Cin * H * W]
    return img


@pytest.mark.parametrize("dt", R.DT3)
@pytest.mark.parametrize("Cin,H,W,P", R.PATCH_GEOM)
def test_im2col_patch(Cin, H, W, P, dt):
    img = patch_image(Cin, H, W)
    rows = 3 * (H // P) * (W // P)
    for ldk in sorted(set(R.patch_ldks(Cin * P * P))):
        for off in ((0, 1) if dt != F32 and ldk % 8 == 0 else (0,)):
            for smap in (None, torch.tensor(R.PATCH_MAP)):
                src = img.clone()
                if smap is not None:
                    src[1] = float("nan")                                       # the image the map never names
                o = Buf(R.canary(rows * ldk, dt).view(rows, ldk), off)
                if smap is None:
                    rc = L().vr_im2col_patch(ptr(cu(src)), o.ptr, 3, Cin, H, W, P, ldk, code(dt), stream())
                else:
                    rc = L().vr_im2col_patch_map(ptr(cu(src)), o.ptr, ptr(cu(smap)), 3, Cin, H, W, P, ldk, code(dt), stream())
                assert rc == 0
                exact("im2col_patch %s Cin%d %dx%d P%d ldk%d off%d %s %s" % ((R.name(dt), Cin, H, W, P, ldk, off, "map" if smap is not None else "id")
                                                                           + (R.im2col_patch_path(Cin, W, P, ldk, dt, off),)),
                      o.get(), R.im2col_patch_contract(R.canary(rows * ldk, dt).view(rows, ldk), src, smap, P, ldk))


# ---- embed_cls, mask_rows ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [255, 257])
@pytest.mark.parametrize("T", [1, 2])
def test_embed_cls(T, C):
    B, N = 3, T + 2
    tokens, pos = R.pattern32(T * C, 1).view(T, C), R.pattern32(N * C, 2).view(N, C)
    for keep in (None, torch.tensor([0, 8, C], dtype=torch.int32), torch.tensor([C, 0, 8], dtype=torch.int32)):
        before = R.canary(B * N * C, F32).view(B, N, C)
        o = Buf(before)
        assert L().vr_embed_cls(ptr(cu(tokens)), ptr(cu(pos)), o.ptr, ptr(cu(keep)), B, N, C, T, stream()) == 0
        exact("embed_cls T%d C%d keep %s" % (T, C, None if keep is None else keep.tolist()), o.get(), R.embed_cls_contract(before, tokens, pos, keep, T))


def test_mask_rows():
    M, C, rps = 5, 520, 2
    before = R.pattern32(M * C).view(M, C).clone()
    before[:, 7] = float("nan")
    for keep in ([0, C, 259], [C, 0, 1], [C, C, C]):
        kp = torch.tensor(keep, dtype=torch.int32)
        o = Buf(before)
        assert L().vr_mask_rows(o.ptr, ptr(cu(kp)), M, C, rps, stream()) == 0
        exact("mask_rows C%d keep %s" % (C, keep), o.get(), R.mask_rows_contract(before, kp, rps))


# ---- spatial reduction ----------------------------------------------------------------------------------------------------------------------------------
def sr_y(B, g, C, T, dt):
    """[B, T + g g, C]: patch rows from the flat index, token rows NaN"""
    y = R.canary(B * (T + g * g) * C, dt).view(B, T + g * g, C)
    y[:, T:] = R.pattern(B * g * g * C, dt, g + C).view(B, g * g, C)
    return y


def sr_offsets(dt, C):
    return [(0, 0), (1, 0), (0, 4)] if dt != F32 and C % 8 == 0 else [(0, 0)]


@pytest.mark.parametrize("dt", R.DT3)
@pytest.mark.parametrize("g", R.SR_G)
def test_sr_im2col(g, dt):
    B = 2
    for T in R.SR_T:
        for C in R.SR_C:
            y = sr_y(B, g, C, T, dt)
            ncol = B * (g // 2) ** 2 * 9 * C
            for yo, co in sr_offsets(dt, C) if g == 4 else [(0, 0)]:
                s, o = Buf(y, yo), Buf(R.canary(ncol, dt), co)
                assert L().vr_sr_im2col(s.ptr, o.ptr, B, g, C, T, code(dt), stream()) == 0
                exact("sr_im2col %s g%d T%d C%d off %d,%d %s" % (R.name(dt), g, T, C, yo, co, R.sr_im2col_path(B, g, C, dt, yo, co)[0]), o.get(),
                      R.sr_im2col_contract(R.canary(ncol, dt), y, B, g, C, T))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("g", R.SR_G)
def test_sr_col2im(g, dt):
    B = 2
    for T in R.SR_T:
        for C in R.SR_C:
            dcol = R.signed_unit((B * (g // 2) ** 2, 9 * C), g * 100 + C + T, dt)
            ref, b32 = R.sr_col2im_ref(dcol, B, g, C)
            before = R.canary(B * (T + g * g) * C, dt).view(B, T + g * g, C)
            for do_, yo in sr_offsets(dt, C) if g == 4 else [(0, 0)]:
                s, o = Buf(dcol, do_), Buf(before, yo)
                assert L().vr_sr_col2im(s.ptr, o.ptr, B, g, C, T, code(dt), stream()) == 0
                got = o.get()
                tag = "sr_col2im %s g%d T%d C%d off %d,%d %s" % (R.name(dt), g, T, C, do_, yo, R.sr_col2im_path(B, g, C, dt, do_, yo)[0])
                exact(tag + ": token rows", got[:, :T], before[:, :T])
                bounded("sr_col2im", tag, got[:, T:], ref, b32, dt)


@pytest.mark.parametrize("Cin,Cout", R.SR_RESID)
@pytest.mark.parametrize("T", R.SR_T)
def test_sr_resid_and_bwd(T, Cin, Cout):
    B = 2
    for g in (2, 6):
        go = g // 2
        x = R.signed_unit((B, T + g * g, Cin), g + T + Cin)
        x[:, :T] = R.pattern32(B * T * Cin, 5).view(B, T, Cin)
        before = R.canary(B * (T + go * go) * Cout, F32).view(B, T + go * go, Cout)
        o = Buf(before)
        assert L().vr_sr_resid(ptr(cu(x)), o.ptr, B, g, Cin, Cout, T, stream()) == 0
        got = o.get()
        exp = R.sr_resid_exact(before, x, B, g, Cin, Cout, T)
        tag = "sr_resid g%d T%d Cin%d Cout%d" % (g, T, Cin, Cout)
        exact(tag + ": token rows, pad columns", torch.cat([got[:, :T].reshape(-1), got[:, T:, Cin:].reshape(-1)]),
              torch.cat([exp[:, :T].reshape(-1), exp[:, T:, Cin:].reshape(-1)]))
        ref, b32 = R.sr_resid_ref(x, B, g, Cin, T)
        bounded("sr_resid", tag, got[:, T:, :Cin], ref, b32)
        dout = R.canary(B * (T + go * go) * Cout, F32).view(B, T + go * go, Cout)           # pad columns of dout are NaN
        dout[:, :, :Cin] = R.pattern32(B * (T + go * go) * Cin, 9).view(B, T + go * go, Cin)
        for acc in (0, 1):
            dx0 = R.pattern32(B * (T + g * g) * Cin, 13).view(B, T + g * g, Cin) if acc else R.canary(B * (T + g * g) * Cin, F32).view(B, T + g * g, Cin)
            d = Buf(dx0)
            assert L().vr_sr_resid_bwd(ptr(cu(dout)), d.ptr, B, g, Cin, Cout, acc, T, stream()) == 0
            exact("sr_resid_bwd g%d T%d Cin%d Cout%d acc%d" % (g, T, Cin, Cout, acc), d.get(), R.sr_resid_bwd_contract(dx0, dout, B, g, Cin, Cout, acc, T))


def dev_pattern16(n, lo, span, mul):
    """bf16 bit patterns on the device: lo + (index * mul) % span with a sign bit that changes every few elements"""
    i = torch.arange(n, dtype=torch.int32, device=DEV)
    v = lo + ((i % span) * mul) % span + ((((i % 1024) * 11) >> 3) & 1) * 0x8000
    return torch.where(v >= 32768, v - 65536, v).to(torch.int16).view(BF16)


def test_sr_im2col_v8_second_pass_equals_single_pass_pieces():
    B, g, C = R.SR_IM2COL_BIG
    T, go = 1, g // 2
    y = dev_pattern16(B * (T + g * g) * C, 1, 0x7800 - 1, 7).view(B, T + g * g, C)
    big = torch.empty(B * go * go, 9 * C, dtype=BF16, device=DEV)
    pieces = torch.empty_like(big)
    assert L().vr_sr_im2col(ptr(y), ptr(big), B, g, C, T, code(BF16), stream()) == 0
    half = B // 2
    for b0, b1 in ((0, half), (half, B)):
        assert R.sr_im2col_path(b1 - b0, g, C, BF16)[2] == 1
        assert L().vr_sr_im2col(y[b0:].data_ptr(), pieces[b0 * go * go:].data_ptr(), b1 - b0, g, C, T, code(BF16), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(R.ibits(big), R.ibits(pieces))
    for b0 in (0, half - 1, B - 2):
        exact("sr_im2col v8 B%d (two passes), pieces, samples %d.." % (B, b0), pieces[b0 * go * go:(b0 + 2) * go * go].cpu().reshape(-1),
              R.sr_im2col_contract(R.canary(2 * go * go * 9 * C, BF16), y[b0:b0 + 2].cpu(), 2, g, C, T))


def test_sr_col2im_v8_second_pass_equals_single_pass_pieces():
    B, g, C = R.SR_COL2IM_BIG
    T, go = 1, g // 2
    dcol = dev_pattern16(B * go * go * 9 * C, 0x3f00, 256, 37).view(B * go * go, 9 * C)             # |x| in [0.5, 2)
    big = R.canary(1, BF16).to(DEV).repeat(B * (T + g * g) * C).view(B, T + g * g, C)
    pieces = big.clone()
    assert L().vr_sr_col2im(ptr(dcol), ptr(big), B, g, C, T, code(BF16), stream()) == 0
    half = B // 2
    for b0, b1 in ((0, half), (half, B)):
        assert R.sr_col2im_path(b1 - b0, g, C, BF16)[2] == 1
        assert L().vr_sr_col2im(dcol[b0 * go * go:].data_ptr(), pieces[b0:].data_ptr(), b1 - b0, g, C, T, code(BF16), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(R.ibits(big), R.ibits(pieces))
    for b0 in (0, half - 1, B - 2):
        got = pieces[b0:b0 + 2].cpu()
        ref, b32 = R.sr_col2im_ref(dcol[b0 * go * go:(b0 + 2) * go * go].cpu(), 2, g, C)
        exact("sr_col2im v8 B%d (two passes): token rows %d.." % (B, b0), got[:, :T], R.canary(2 * T * C, BF16).view(2, T, C))
        bounded("sr_col2im", "sr_col2im v8 B%d (two passes), pieces, samples %d.." % (B, b0), got[:, T:], ref, b32, BF16)


# ---- refusals: the documented code, nothing written -----------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_write_nothing():
    lib, st = L(), stream()
    f = lambda n, dt=F32: Buf(R.canary(n, dt))                                     # noqa: E731
    src = cu(R.pattern32(4096))
    outs = []

    def refused(tag, rc, want, *bufs):
        print("GLUE refusal %-44s rc %d" % (tag, rc))
        assert rc == want, (tag, rc, want)
        outs.extend((tag, b) for b in bufs)

    o = f(64, BF16)
    refused("cast: src 4 bytes off", lib.vr_cast_f32_bf16(src[1:].data_ptr(), o.ptr, 16, st), R.VR_EALIGN, o)
    o = f(64, F16)
    refused("cast: dst 2 bytes off", lib.vr_cast_f32_f16(ptr(src), o.view[1:].data_ptr(), 16, st), R.VR_EALIGN, o)
    o = f(64, BF16)
    refused("scale_mask_cast: C % 4", lib.vr_scale_mask_cast(ptr(src), o.ptr, None, None, 2, 6, 2, code(BF16), st), R.VR_EINVAL, o)
    o = f(4096)
    refused("im2col_patch: H % P", lib.vr_im2col_patch(ptr(src), o.ptr, 1, 3, 15, 14, 7, 147, code(F32), st), R.VR_EINVAL, o)
    refused("im2col_patch: W % P", lib.vr_im2col_patch(ptr(src), o.ptr, 1, 3, 14, 15, 7, 147, code(F32), st), R.VR_EINVAL, o)
    refused("im2col_patch: ldk < K", lib.vr_im2col_patch(ptr(src), o.ptr, 1, 3, 14, 14, 7, 146, code(F32), st), R.VR_EINVAL, o)
    img = cu(R.pattern32(3 * 16 * 352))
    o = f(22 * 768)
    refused("im2col_patch: 66 KiB of LDS", lib.vr_im2col_patch(ptr(img), o.ptr, 1, 3, 16, 352, 16, 768, code(F32), st), R.VR_EUNSUPPORTED, o)
    o = f(4096)
    refused("sr_im2col: odd g", lib.vr_sr_im2col(ptr(src), o.ptr, 1, 3, 8, 1, code(F32), st), R.VR_EINVAL, o)
    refused("sr_col2im: odd g", lib.vr_sr_col2im(ptr(src), o.ptr, 1, 3, 8, 1, code(F32), st), R.VR_EINVAL, o)
    refused("sr_resid: odd g", lib.vr_sr_resid(ptr(src), o.ptr, 1, 3, 8, 8, 1, st), R.VR_EINVAL, o)
    refused("sr_resid_bwd: odd g", lib.vr_sr_resid_bwd(ptr(src), o.ptr, 1, 3, 8, 8, 0, 1, st), R.VR_EINVAL, o)
    refused("sr_resid: Cout < Cin", lib.vr_sr_resid(ptr(src), o.ptr, 1, 2, 8, 4, 1, st), R.VR_EINVAL, o)
    refused("token_mean: first >= N", lib.vr_token_mean(ptr(src), o.ptr, 2, 3, 8, 3, code(F32), st), R.VR_EINVAL, o)
    refused("token_mean_bwd: first >= N", lib.vr_token_mean_bwd(ptr(src), o.ptr, 2, 3, 8, 3, code(F32), st), R.VR_EINVAL, o)
    o = f(4096, F16)
    h = cu(R.pattern16(4096, F16))
    refused("token_mean_bwd: fp16", lib.vr_token_mean_bwd(ptr(h), o.ptr, 2, 3, 8, 1, code(F16), st), R.VR_EUNSUPPORTED, o)
    refused("sr_col2im: fp16", lib.vr_sr_col2im(ptr(h), o.ptr, 1, 2, 8, 1, code(F16), st), R.VR_EUNSUPPORTED, o)
    refused("relayout: fp16 -> bf16", lib.vr_relayout(ptr(h), o.ptr, 2, 3, 4, 12, 12, code(F16), code(BF16), st), R.VR_EUNSUPPORTED, o)
    refused("relayout: bf16 -> fp16", lib.vr_relayout(ptr(h), o.ptr, 2, 3, 4, 12, 12, code(BF16), code(F16), st), R.VR_EUNSUPPORTED, o)
    o = f(4096)
    refused("relayout: dst_ld < B C", lib.vr_relayout(ptr(src), o.ptr, 2, 3, 4, 12, 11, code(F32), code(F32), st), R.VR_EINVAL, o)
    refused("relayout: src_ld < B C", lib.vr_relayout(ptr(src), o.ptr, 2, 3, 4, 11, 12, code(F32), code(F32), st), R.VR_EINVAL, o)
    refused("relayout_add: dst_ld < B C", lib.vr_relayout_add(ptr(src), o.ptr, 2, 3, 4, 12, 11, st), R.VR_EINVAL, o)
    refused("colsum: fp16", lib.vr_colsum(ptr(h), o.ptr, 4, 8, 8, code(F16), _lib.RowMap(0, 0, 0), st), R.VR_EUNSUPPORTED, o)
    refused("conv_w_flip: fp16", lib.vr_conv_w_flip(ptr(src), o.ptr, 2, 2, code(F16), st), R.VR_EUNSUPPORTED, o)
    zr = zero_struct([(4 * i, 2) for i in range(24)], n=25)
    refused("zero_ranges: 25 ranges", lib.vr_zero_ranges(o.ptr, ctypes.byref(zr), st), R.VR_EINVAL, o)
    zr = zero_struct([(8, 4), (-4, 8)])
    refused("zero_ranges: negative lo", lib.vr_zero_ranges(o.ptr, ctypes.byref(zr), st), R.VR_EINVAL, o)
    gate = torch.ones(1, dtype=torch.int32, device=DEV)
    refused("zero_ranges_gated: negative count", lib.vr_zero_ranges_gated(o.ptr, ctypes.byref(zero_struct([(8, -1)])), ptr(gate), st),
            R.VR_EINVAL, o)
    for tag, b in outs:
        got = b.get()
        assert not R.mismatches(got, R.canary_like(got)).any(), tag


def test_zz_worst_ratios():
    """printed last: the worst error / bound per bounded kernel of this run"""
    for k, r in sorted(R.WORST.items()):
        print("GLUE WORST %-16s %.3f" % (k, r))
    assert set(R.WORST) == {"colsum", "batchsum", "token_mean", "token_mean_bwd", "sr_col2im", "sr_resid"}
    assert all(r <= 1.0 for r in R.WORST.values())
