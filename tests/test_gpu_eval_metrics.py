"""vr_eval_metrics (loss and top-k hit counts on the device) against torch in float64 on the same fp32 logits, and engine.evaluate /
evo_eval.score_candidate running on it."""
import os

import numpy as np
import pytest
import torch

import recipe
import vitres
from test_eval_metrics_host import HAND_ROWS, f8_batches, hand_case
from vitres import _lib, engine, evo_eval
from vitres import kernels as K

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
TAU = 1e-5        # twice the fp32 error of a probability (<= 2e-6: two __expf of ~2 ulp, the lse's sum and log), with margin

SHAPES = [(1, 10, 10),          # a single row, K below a wave
          (8, 10, 10),          # the micro classes
          (7, 1000, 1000),      # R below a workgroup's waves
          (256, 1000, 1000),    # the evaluation shape
          (64, 1003, 1008),     # K off the vector width, padded rows
          (130, 72, 72)]        # K just over one wave, ragged R
_CASES = {}


def case(R, K_, ld):
    """Inputs and float64 reference of a shape, made once: (x, x2, y) on the device as [R, K] views of NaN-padded [R, ld] buffers."""
    if (R, K_, ld) in _CASES:
        return _CASES[(R, K_, ld)]
    g = torch.Generator().manual_seed(0)
    x = 3 * torch.randn(R, K_, generator=g)
    x2 = 3 * torch.randn(R, K_, generator=g)
    y = torch.randint(0, K_, (R,), generator=g)
    x[torch.arange(0, R, 2), y[::2]] += 7.5                       # every second row's label logit is lifted: hits and misses
    x2[torch.arange(0, R, 3), y[::3]] += 6.0
    top = min(5, K_)
    col = torch.arange(K_)[None, :]

    def ranks(v, vy):
        return ((v > vy) | ((v == vy) & (col < y[:, None]))).masked_fill(col == y[:, None], False).sum(1)

    ref = {"loss": float(torch.nn.functional.cross_entropy(x.double(), y))}
    for name, v in (("", x), ("dst_", x2)):
        r = ranks(v, v.gather(1, y[:, None]))
        ref[name + "top1"], ref[name + "top5"] = int((r < 1).sum()), int((r < top).sum())
    p = torch.softmax(x.double(), 1) + torch.softmax(x2.double(), 1)
    py = p.gather(1, y[:, None])
    for k, bound in (("1", 1), ("5", top)):
        lo, hi = ranks(p, py * (1 - TAU)) < bound, ranks(p, py * (1 + TAU)) < bound
        ref["jnt_certain" + k], ref["jnt_ambiguous" + k] = int((lo & hi).sum()), int((lo != hi).sum())

    def padded(v):
        buf = torch.full((R, ld), float("nan"))
        buf[:, :K_] = v
        return buf.to(DEV)[:, :K_]
    _CASES[(R, K_, ld)] = (padded(x), padded(x2), y.to(DEV), ref)
    return _CASES[(R, K_, ld)]


@pytest.mark.parametrize("R,K_,ld", SHAPES)
def test_eval_metrics_against_float64(R, K_, ld):
    x, x2, y, ref = case(R, K_, ld)
    assert x.stride(0) == ld
    st = K.read_eval_state(K.eval_metrics(x, y, K.eval_state(DEV), logits2=x2))
    print("shape", (R, K_, ld), "state", st, "reference", ref)
    assert (st["calls"], st["rows"], st["reserved"]) == (1, R, 0)
    for k in ("top1", "top5", "dst_top1", "dst_top5"):
        assert st[k] == ref[k], k
    # a lane's fp32 chain of <= 16 terms, the shuffle tree and expf's 2 ulp
    assert abs(st["loss_sum"] - ref["loss"]) < 1e-5 * abs(ref["loss"])
    for k in ("1", "5"):
        assert ref["jnt_ambiguous" + k] <= 0.01 * R               # (a condition of the check, not a tolerance)
        assert ref["jnt_certain" + k] <= st["jnt_top" + k] <= ref["jnt_certain" + k] + ref["jnt_ambiguous" + k], k
    if (R, K_) == (256, 1000):
        assert (ref["top1"], ref["top5"]) == (26, 54)             # the recipe gives hits and misses


@pytest.mark.parametrize("R,K_,ld", [(8, 10, 10), (64, 1003, 1008)])
def test_one_head_leaves_the_other_fields_alone_and_calls_accumulate(R, K_, ld):
    x, x2, y, ref = case(R, K_, ld)
    state = K.eval_state(DEV)
    state[5:9] = 12345
    state[9] = -7
    K.eval_metrics(x, y, state)
    K.eval_metrics(x, y, state)
    st = K.read_eval_state(state)
    assert [st[k] for k in ("dst_top1", "dst_top5", "jnt_top1", "jnt_top5", "reserved")] == [12345] * 4 + [-7]
    assert (st["calls"], st["rows"], st["top1"], st["top5"]) == (2, 2 * R, 2 * ref["top1"], 2 * ref["top5"])
    assert abs(st["loss_sum"] - 2 * ref["loss"]) < 1e-5 * abs(2 * ref["loss"])


def test_equal_inputs_give_equal_bytes():
    x, x2, y, _ = case(256, 1000, 1000)
    runs = []
    for _ in range(3):
        state = K.eval_state(DEV)
        K.eval_metrics(x, y, state, logits2=x2)
        K.eval_metrics(x2, y, state, logits2=x)
        runs.append(state.cpu())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("K_", sorted(HAND_ROWS))
def test_rank_and_tie_rule_on_hand_made_rows(K_):
    x, y, top1, top5 = hand_case(K_)
    xd, yd = x.to(DEV), y.to(DEV)
    for r in range(x.shape[0]):
        st = K.read_eval_state(K.eval_metrics(xd[r:r + 1], yd[r:r + 1], K.eval_state(DEV), logits2=xd[r:r + 1]))
        assert (st["top1"], st["top5"], st["dst_top1"], st["dst_top5"]) == (top1[r], top5[r], top1[r], top5[r]), (K_, r)
    st = K.read_eval_state(K.eval_metrics(xd, yd, K.eval_state(DEV)))
    assert (st["top1"], st["top5"]) == (sum(top1), sum(top5))


def test_bad_rows_are_misses_and_make_the_loss_nan():
    x, x2, y, ref = case(130, 72, 72)
    for what in ("label_high", "label_negative", "nan", "nan_second_head"):
        xb, x2b, yb = x.clone(), x2.clone(), y.clone()
        clean = K.read_eval_state(K.eval_metrics(xb[1:], yb[1:], K.eval_state(DEV), logits2=x2b[1:]))
        if what == "label_high":
            yb[0] = 72
        elif what == "label_negative":
            yb[0] = -1
        elif what == "nan":
            xb[0, 5] = float("nan")
        else:
            x2b[0, 71] = float("nan")
        st = K.read_eval_state(K.eval_metrics(xb, yb, K.eval_state(DEV), logits2=x2b))
        assert np.isnan(st["loss_sum"]), what
        assert st["rows"] == 130
        for k in ("top1", "top5", "dst_top1", "dst_top5", "jnt_top1", "jnt_top5"):
            assert st[k] == clean[k], (what, k)                    # row 0 adds no hit anywhere; the other rows count as before


def test_argument_checks_return_their_codes():
    x, _, y, _ = case(8, 10, 10)
    lib, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    state = torch.zeros(12, dtype=torch.int64, device=DEV)
    call = lambda R, K_, ld, st: lib.vr_eval_metrics(x.data_ptr(), None, y.data_ptr(), R, K_, ld, st, s)   # noqa: E731
    assert call(0, 10, 10, state.data_ptr()) == -1
    assert call(8, 0, 10, state.data_ptr()) == -1
    assert call(8, 10, 9, state.data_ptr()) == -1
    assert call(8, 10, 10, state.data_ptr() + 4) == -2
    assert call(8, 10, 10, state.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(state[1]) == 1 and int(state[2]) == 8


# ---- engine.evaluate ------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model(two_token, et):
    if (two_token, et) not in _MODELS:
        name = "flexible_vit_sr_distill_patch14_224" if two_token else "flexible_vit_sr_patch14_224_patch_output"
        m = vitres.create_model(name, img_size=recipe.MICRO_IMG, num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[et],
                                drop_path_rate=0.0)
        m.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], (140 if two_token else 100) + et))
        _MODELS[(two_token, et)] = m.to(DEV)
    return _MODELS[(two_token, et)]


_BATCHES = []


def batches():
    if not _BATCHES:
        for it in range(4):
            x, _, _, labels = recipe.inputs(500 + it, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
            _BATCHES.append((x.to(DEV), labels.to(DEV)))
    return _BATCHES


QUIET = type("L", (), {"info": staticmethod(lambda s: None)})


class ReadCounter:
    """Counts device-to-host reads: Tensor.item / tolist / cpu on CUDA tensors and torch.cuda.synchronize."""

    def __init__(self, monkeypatch):
        self.events = []
        for name in ("item", "tolist", "cpu"):
            orig = getattr(torch.Tensor, name)

            def wrapped(t, *a, _orig=orig, _name=name, **kw):
                if t.is_cuda:
                    self.events.append(_name)
                return _orig(t, *a, **kw)
            monkeypatch.setattr(torch.Tensor, name, wrapped)
        sync = torch.cuda.synchronize
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (self.events.append("synchronize"), sync(*a, **kw))[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("two_token,et", [(False, 0), (False, 4), (True, 0), (True, 4)])
def test_evaluate_on_device_meters_equals_the_torch_statement(monkeypatch, two_token, et, dtype):
    m = model(two_token, et).set_compute_dtype(dtype)
    off = engine.evaluate(batches(), m, DEV, logger=QUIET, device_meters=False)
    seen = []

    class Loader:                                                 # records how many reads had happened when each batch was drawn
        def __iter__(self):
            for b in batches():
                seen.append(len(counter.events))
                yield b
            seen.append(len(counter.events))
    counter = ReadCounter(monkeypatch)
    on = engine.evaluate(Loader(), m, DEV, logger=QUIET, device_meters=True)
    monkeypatch.undo()
    assert seen == [0] * 5 and len(counter.events) == 1, (seen, counter.events)   # one read, after the last batch
    auto = engine.evaluate(batches(), m, DEV, logger=QUIET)
    assert auto == on                                             # None: on for CUDA logits
    assert list(on) == list(off) and len(on) == (7 if two_token else 3)
    print("on", on, "off", off)
    for k in on:
        if k == "loss":
            assert abs(on[k] - off[k]) < 1e-5 * abs(off[k])
        else:
            assert on[k] == off[k], k


def test_evaluate_fp32_against_the_reference_fixture():
    """Fixture F8 (the reference's own engine.evaluate on the micro net).  This is the first check of F8 on the GPU: the suite held
    it on the CPU only (tests/test_oracle_golden.py, 1e-5).  The band is the one the GPU fp32 path holds the reference's loss to,
    1e-4 relative (tests/test_gpu_model.py, test_micro_fp32_vs_reference_golden_and_oracle); the accuracies are counts."""
    g = np.load(os.path.join(G, "f8_engine_eval.npz"))
    m = model(False, 0).set_compute_dtype(torch.float32)
    stats = engine.evaluate([(x.to(DEV), y.to(DEV)) for x, y in f8_batches()], m, DEV, logger=QUIET, device_meters=True)
    assert abs(stats["loss"] - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    assert abs(stats["acc1"] - float(g["acc1"])) < 1e-4 and abs(stats["acc5"] - float(g["acc5"])) < 1e-4


def test_score_candidate_equals_argmax_on_the_same_logits():
    sup = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                              num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0],
                              num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    sup.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in sup.state_dict().items()], 100))
    sup = sup.to(DEV).set_compute_dtype(torch.float32).eval()
    data = []
    for s in (9, 10):
        x, _, _, labels = recipe.inputs(s, 6, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
        data.append((x.to(DEV), labels.to(DEV)))
    for nd in recipe.MICRO_CANDIDATES:
        hits = 0
        with torch.no_grad():
            for x, labels in data:
                out = sup(x, plan=evo_eval.plan_for_subnet(sup, nd, 6))
                hits += int((out.argmax(dim=1) == labels).sum())
        assert evo_eval.score_candidate(sup, nd, data) == 100.0 * float(hits) / 12
