"""engine.evaluate(device_meters=True) and vr_eval_metrics' rank / tie rule on the CPU, under tests/emu_eval.py (the kernel itself
is checked on the GPU by tests/test_gpu_eval_metrics.py, which shares HAND_ROWS with this file)."""
import os

import numpy as np
import pytest
import torch

import emu_eval
import recipe
import vitres
from vitres import engine
from vitres import kernels as K

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (logits row, label, top1 hit, top5 hit): ties below and above the label's index, K < 5, top5 with K = 3
HAND_ROWS = {
    8: [([1., 2., 3., 4., 5., 6., 7., 8.], 7, 1, 1),               # the maximum
        ([1., 2., 3., 4., 5., 6., 7., 8.], 3, 0, 1),               # four larger values: rank 4, the last top-5 place
        ([1., 2., 3., 4., 5., 6., 7., 8.], 2, 0, 0),               # five larger values: rank 5
        ([5., 5., 1., 1., 1., 1., 1., 1.], 0, 1, 1),               # tie ABOVE the label's index only: the lower index wins
        ([5., 5., 1., 1., 1., 1., 1., 1.], 1, 0, 1),               # tie BELOW the label's index: the label loses top-1
        ([2., 2., 2., 2., 2., 2., 2., 2.], 4, 0, 1),               # all equal: rank = index 4
        ([2., 2., 2., 2., 2., 2., 2., 2.], 5, 0, 0),               # all equal: rank = index 5
        ([9., 3., 3., 3., 3., 3., 3., 1.], 4, 0, 1),               # one larger + three equal below the index: rank 4
        ([9., 3., 3., 3., 3., 3., 3., 1.], 5, 0, 0)],              # one larger + four equal below the index: rank 5
    3: [([0., 1., 2.], 0, 0, 1),                                   # K = 3: top5 = rank < 3, always a hit for a valid row
        ([0., 1., 2.], 2, 1, 1),
        ([4., 4., 4.], 2, 0, 1)],
    1: [([0.5], 0, 1, 1)],
}


def hand_case(K_):
    rows = HAND_ROWS[K_]
    x = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    y = torch.tensor([r[1] for r in rows], dtype=torch.int64)
    return x, y, [r[2] for r in rows], [r[3] for r in rows]


@pytest.mark.parametrize("K_", sorted(HAND_ROWS))
def test_rank_and_tie_rule_on_hand_made_rows(K_):
    x, y, top1, top5 = hand_case(K_)
    for r in range(x.shape[0]):                                   # row by row: each expected bit is checked on its own
        st = K.read_eval_state(emu_eval.eval_metrics(x[r:r + 1], y[r:r + 1], K.eval_state("cpu")))
        assert (st["top1"], st["top5"]) == (top1[r], top5[r]), (K_, r)
        assert st["top1"] == int(torch.argmax(x[r]) == y[r])      # torch's argmax takes the first of equal maxima
    st = K.read_eval_state(emu_eval.eval_metrics(x, y, K.eval_state("cpu")))
    assert (st["top1"], st["top5"], st["rows"], st["calls"]) == (sum(top1), sum(top5), x.shape[0], 1)
    want = torch.nn.functional.cross_entropy(x.double(), y).item()
    assert abs(st["loss_sum"] - want) < 1e-6 * max(abs(want), 1.0)
    assert (st["dst_top1"], st["jnt_top5"]) == (0, 0)


def test_bad_rows_are_misses_and_poison_the_loss():
    x, y, _, _ = hand_case(8)
    y2 = y.clone()
    y2[0] = 8
    st = K.read_eval_state(emu_eval.eval_metrics(x, y2, K.eval_state("cpu")))
    assert np.isnan(st["loss_sum"]) and st["top1"] == 1 and st["rows"] == 9
    x2 = x.clone()
    x2[3, 6] = float("nan")
    st = K.read_eval_state(emu_eval.eval_metrics(x2, y, K.eval_state("cpu")))
    assert np.isnan(st["loss_sum"]) and st["top1"] == 1


def _model(name, nd, sup, seed):
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30) if sup else {}
    m = vitres.create_model(name + ("_supernet" if sup else ""), img_size=recipe.MICRO_IMG, num_classes=recipe.MICRO_CLASSES,
                            network_def=nd, drop_path_rate=0.0, **kw)
    m.load_state_dict(recipe.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed))
    return m.set_compute_dtype(torch.float32)


def f8_batches():
    out = []
    for it in range(2):
        x, _, _, labels = recipe.inputs(400 + it, 8 if it == 0 else 4, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
        out.append((x, labels))
    return out


def test_evaluate_on_device_meters_equals_the_torch_statement_and_f8(monkeypatch):
    emu_eval.install(monkeypatch)
    g = np.load(os.path.join(G, "f8_engine_eval.npz"))
    m = _model("flexible_vit_sr_patch14_224_patch_output", recipe.MICRO_DEFS[0], False, 100)
    lines = []
    log = type("L", (), {"info": staticmethod(lines.append)})
    on = engine.evaluate(f8_batches(), m, "cpu", logger=log, device_meters=True)
    off = engine.evaluate(f8_batches(), m, "cpu", logger=log, device_meters=False)
    auto = engine.evaluate(f8_batches(), m, "cpu", logger=log)      # None: CPU logits -> the torch statement
    assert list(on) == list(off) == ["loss", "acc1", "acc5"] and auto == off
    assert lines[0] == lines[1]                                   # the same log line
    for k in on:
        assert abs(on[k] - off[k]) < 1e-6 * max(abs(off[k]), 1.0), k
        assert abs(on[k] - float(g[k])) < 1e-6 * max(abs(float(g[k])), 1.0), k


@pytest.mark.parametrize("et,sup", [(0, False), (4, True)])
def test_evaluate_on_device_meters_two_token_models(monkeypatch, et, sup):
    emu_eval.install(monkeypatch)
    m = _model("flexible_vit_sr_distill_patch14_224", recipe.MICRO_DEFS[et], sup, 140 + et)
    quiet = type("L", (), {"info": staticmethod(lambda s: None)})
    on = engine.evaluate(f8_batches(), m, "cpu", logger=quiet, device_meters=True)
    off = engine.evaluate(f8_batches(), m, "cpu", logger=quiet, device_meters=False)
    assert list(on) == list(off) == ["loss", "acc1", "acc5", "dst_acc1", "dst_acc5", "jnt_acc1", "jnt_acc5"]
    for k in on:
        assert abs(on[k] - off[k]) < 1e-6 * max(abs(off[k]), 1.0), k


def test_score_candidate_through_the_state_equals_the_torch_expression(monkeypatch):
    from vitres import evo_eval
    emu_eval.install(monkeypatch)
    sup = _model("flexible_vit_sr_patch14_224_patch_output", recipe.MICRO_DEFS[0], True, 100).eval()
    batches = []
    for s in (9, 10):
        x, _, _, labels = recipe.inputs(s, 6, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
        batches.append((x, labels))
    for nd in recipe.MICRO_CANDIDATES:
        assert evo_eval.score_candidate(sup, nd, batches, device_meters=True) == evo_eval.score_candidate(sup, nd, batches, device_meters=False)


def test_abi_declares_the_entry_point():
    from vitres import _lib
    hdr = open(os.path.join(os.path.dirname(G), "..", "include", "vitres_hip.h")).read()
    assert "int vr_eval_metrics(" in hdr and "typedef struct vr_eval_state" in hdr
    assert len(_lib.SYMBOLS["vr_eval_metrics"]) == 8
    assert len(K.EVAL_STATE_FIELDS) * 8 == 80                      # sizeof(vr_eval_state): one double and nine int64
    assert _lib.lib().vr_version() >= 1001
