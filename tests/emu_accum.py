"""CPU emulation of the entry points gradient accumulation added (vitres.kernels.relayout_add), on top of tests/emu_kernels.py.
Never imported by the product.  `install(monkeypatch)` swaps the functions of vitres.kernels for the emulations."""
import torch

import emu_kernels


def relayout_add(src, dst, A, B, C, dst_ld=None, src_ld=None):
    """dst[a * dst_ld + c * B + b] += src[a * src_ld + b * C + c] (vr_relayout_add)."""
    assert src.dtype == torch.float32 and dst.dtype == torch.float32
    dst_ld = B * C if dst_ld is None else dst_ld
    src_ld = B * C if src_ld is None else src_ld
    sidx = (torch.arange(A)[:, None] * src_ld + torch.arange(B * C)[None, :]).reshape(-1)
    v = src.reshape(-1)[sidx].view(A, B, C).permute(0, 2, 1).reshape(-1)
    didx = (torch.arange(A)[:, None] * dst_ld + torch.arange(B * C)[None, :]).reshape(-1)
    flat = dst.reshape(-1)
    assert flat.data_ptr() == dst.data_ptr()                      # (a view: the sum lands in the caller's tensor)
    flat[didx] += v
    return dst


def install(monkeypatch):
    import vitres.kernels as K
    emu_kernels.install(monkeypatch)
    monkeypatch.setattr(K, "relayout_add", relayout_add)
