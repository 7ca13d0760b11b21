"""CPU emulation of vitres.kernels.normalize_u8 (vr_normalize_u8 of include/vitres_hip.h): timm's PrefetchLoader statement in
torch fp32.  Never imported by the product.  `install(monkeypatch)` swaps the function of vitres.kernels for the emulation and
returns the list every call is logged to as (input, out-or-None, result)."""
import torch


def normalize_u8_reference(u8, mean, std):
    """(u8.float() - mean * 255) / (std * 255) with the constants rounded to fp32 from the Python double product."""
    m = torch.tensor([x * 255 for x in mean], dtype=torch.float32).view(1, -1, 1, 1)
    s = torch.tensor([x * 255 for x in std], dtype=torch.float32).view(1, -1, 1, 1)
    return u8.float().sub_(m).div_(s)


def install(monkeypatch):
    import vitres.kernels as K
    calls = []

    def normalize_u8(u8, mean, std, out=None):
        assert u8.dtype == torch.uint8 and u8.dim() == 4
        m = torch.tensor(list(mean), dtype=torch.float32).view(1, -1, 1, 1)      # (already in uint8 units: norm_constants)
        s = torch.tensor(list(std), dtype=torch.float32).view(1, -1, 1, 1)
        res = u8.float().sub_(m).div_(s)
        if out is not None:
            assert out.dtype == torch.float32 and out.shape == u8.shape and out.is_contiguous()
            out.copy_(res)
            res = out
        calls.append((u8, out, res))
        return res
    monkeypatch.setattr(K, "normalize_u8", normalize_u8)
    return calls
