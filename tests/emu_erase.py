"""CPU emulation of the erase wrappers of vitres.kernels (random_erase, normalize_u8_erase, mixup_u8_erase, token_mix_u8_erase), each
as the three-stage statement its entry point is specified by: timm's PrefetchLoader normalisation in torch fp32, tests/erase_ref.py's
float64 fill rounded to fp32, then the existing emulated mix (tests/mixup_ref.py's table emulation; the oracle's SwitchTokenMix).
Never imported by the product.  `install(monkeypatch)` swaps the four functions and returns the list every call is logged to."""
import numpy as np
import torch

import erase_ref
import mixup_ref
import vitres_oracle as O


def erased(xf, erase):
    """(a new fp32 tensor: xf with the reference fill inside the rectangles of `erase`, the boolean mask of the erased elements)"""
    out, inside, _ = erase_ref.erase(xf.numpy(), erase["rects"], erase["mode"], erase["seed"], erase["call"])
    res = xf.clone()
    mask = torch.from_numpy(inside)
    res[mask] = torch.from_numpy(out.astype(np.float32))[mask]    # (outside: xf's own bits, -0.0 included)
    return res, mask


def normalized(u8, norm):
    m = torch.tensor(list(norm[0]), dtype=torch.float32).view(1, -1, 1, 1)          # (already in uint8 units: norm_constants)
    s = torch.tensor(list(norm[1]), dtype=torch.float32).view(1, -1, 1, 1)
    return u8.float().sub_(m).div_(s)


def oracle_draw(d):
    """SwitchTokenMix.draw's dict as the oracle's switch_token_mix takes it."""
    h = d["half"]
    return dict(half=h, perm_a=d["partner"][:h], perm_b=d["partner"][h:] - h, box=d["box"], lam_patch=d["lam_patch"],
                lam_img=d["lam_img"])


def _into(given, val):
    if given is None:
        return val
    assert given.dtype == torch.float32 and given.shape == val.shape and given.is_contiguous()
    return given.copy_(val)


def install(monkeypatch):
    import vitres.kernels as K
    calls = []

    def check(x, erase):
        B, _, H, W = x.shape
        K.check_erase_rects(erase["rects"], B, H, W)
        assert erase["mode"] in K.ERASE_MODES and 0 <= erase["seed"] < 2 ** 64 and 0 <= erase["call"] < 2 ** 64

    def random_erase(x, erase):
        assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
        check(x, erase)
        res, mask = erased(x, erase)
        x.copy_(res)
        calls.append(dict(what="random_erase", erase=erase, mask=mask, result=x))
        return x

    def normalize_u8_erase(u8, mean, std, erase, out=None):
        assert u8.dtype == torch.uint8 and u8.dim() == 4
        check(u8, erase)
        res, mask = erased(normalized(u8, (mean, std)), erase)
        res = _into(out, res)
        calls.append(dict(what="normalize_u8_erase", erase=erase, mask=mask, result=res))
        return res

    def mixup_u8_erase(x, labels, params, num_classes, on, off, norm, erase, out=None, targets_out=None):
        assert x.dtype == torch.uint8 and x.dim() == 4
        check(x, erase)
        xe, mask = erased(normalized(x, norm), erase)
        res = mixup_ref.emulate(xe, labels, params, num_classes, on, off, norm=None, out=out, targets_out=targets_out)
        calls.append(dict(what="mixup_u8_erase", erase=erase, mask=mask, erased=xe, result=res))
        return res

    def token_mix(x, labels, draw, patch_len, num_classes, on, off, norm=None, erase=None, out=None, targets_out=None,
                  patch_targets_out=None):
        """All three forms by the one name SwitchTokenMix calls: the erased one is logged as before, the others as 'token_mix'."""
        assert x.dim() == 4 and x.dtype == (torch.float32 if norm is None else torch.uint8) and (erase is None or norm is not None)
        xe, mask = x if norm is None else normalized(x, norm), None
        if erase is not None:
            check(x, erase)
            xe, mask = erased(xe, erase)
        s0 = off * num_classes                                    # the smoothing whose one-hot values these are (the oracle takes it)
        smoothing = [s for s in (s0, np.nextafter(s0, 0.), np.nextafter(s0, 1.))
                     if s / num_classes == off and 1. - s + s / num_classes == on][0]
        xs, t, pt, _ = O.switch_token_mix(xe, labels, patch_len, num_classes, smoothing, draw=oracle_draw(draw))
        res = (_into(out, xs), _into(targets_out, t), _into(patch_targets_out, pt))
        calls.append(dict(what="token_mix" if erase is None else "token_mix_u8_erase", erase=erase, mask=mask, erased=xe, result=res))
        return res

    def token_mix_u8_erase(x, labels, draw, patch_len, num_classes, on, off, norm, erase, out=None, targets_out=None,
                           patch_targets_out=None):
        assert norm is not None and erase is not None
        return token_mix(x, labels, draw, patch_len, num_classes, on, off, norm, erase, out, targets_out, patch_targets_out)

    for fn in (random_erase, normalize_u8_erase, mixup_u8_erase, token_mix, token_mix_u8_erase):
        monkeypatch.setattr(K, fn.__name__, fn)
    return calls
