"""CPU emulation of vitres.kernels.eval_metrics (vr_eval_metrics of include/vitres_hip.h), on top of tests/emu_kernels.py.
Never imported by the product.  `install(monkeypatch)` swaps the function of vitres.kernels for the emulation; the state is the
product's own (kernels.eval_state / read_eval_state work on CPU tensors as they are)."""
import torch

import emu_kernels


def _ranks(v, y):
    """#{k : v[k] > v[y]} + #{k < y : v[k] == v[y]} per row."""
    vy = v.gather(1, y[:, None])
    k = torch.arange(v.shape[1])[None, :]
    return ((v > vy) | ((v == vy) & (k < y[:, None]))).sum(1)


def eval_metrics(logits, labels, state, logits2=None):
    assert logits.dtype == torch.float32 and labels.dtype == torch.int64 and state.dtype == torch.int64 and state.numel() == 10
    R, K = logits.shape
    bad = (labels < 0) | (labels >= K) | torch.isnan(logits).any(1)
    if logits2 is not None:
        bad = bad | torch.isnan(logits2).any(1)
    y = torch.where(bad, torch.zeros_like(labels), labels)
    top = min(5, K)
    lse = torch.logsumexp(logits, 1)
    ce = (lse - logits.gather(1, y[:, None])[:, 0]).double()
    ce[bad] = float("nan")
    loss = state[:1].view(torch.float64)
    loss += ce.sum() / R
    state[1] += 1
    state[2] += R
    heads = [(3, logits)]
    if logits2 is not None:
        lse2 = torch.logsumexp(logits2, 1)
        heads += [(5, logits2), (7, torch.exp(logits - lse[:, None]) + torch.exp(logits2 - lse2[:, None]))]
    for at, v in heads:
        rank = _ranks(v, y)
        state[at] += int(((rank < 1) & ~bad).sum())
        state[at + 1] += int(((rank < top) & ~bad).sum())
    return state


def install(monkeypatch):
    import vitres.kernels as K
    emu_kernels.install(monkeypatch)
    monkeypatch.setattr(K, "eval_metrics", eval_metrics)
