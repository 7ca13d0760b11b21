"""timm 0.3.2's Mixup tensor statements (timm/data/mixup.py: _mix_batch, _mix_elem, _mix_pair, mixup_target) restated in CPU torch,
taking the draw that vitres.mixup.Mixup.draw returns instead of drawing -- the reference the device kernels are compared with bit for
bit -- and a CPU emulation of vitres.kernels.mixup (vr_mixup / vr_mixup_u8) working from the parameter TABLE, as the kernels do.
Never imported by the product.  `install(monkeypatch)` swaps the function of vitres.kernels for the emulation and returns the list every
call is logged to."""
import numpy as np
import torch


def bits_equal(a, b):
    """Equal as bit patterns: torch.equal calls -0.0 and +0.0 equal, this does not."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def normalized(u8, mean, std):
    """timm's PrefetchLoader statement: input.float().sub_(mean).div_(std), the constants = the 0..1 ones * 255 rounded to fp32."""
    C = u8.shape[1]
    m = torch.tensor([x * 255 for x in mean[:C]], dtype=torch.float32).view(1, C, 1, 1)
    s = torch.tensor([x * 255 for x in std[:C]], dtype=torch.float32).view(1, C, 1, 1)
    return u8.float().sub_(m).div_(s)


def one_hot(x, num_classes, on_value=1., off_value=0.):
    x = x.long().view(-1, 1)
    return torch.full((x.size()[0], num_classes), off_value).scatter_(1, x, on_value)


def mixup_target(target, num_classes, lam=1., smoothing=0.0):
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    y1 = one_hot(target, num_classes, on_value=on_value, off_value=off_value)
    y2 = one_hot(target.flip(0), num_classes, on_value=on_value, off_value=off_value)
    return y1 * lam + y2 * (1. - lam)


def mix(x, target, draw, num_classes, smoothing=0.1):
    """timm's Mixup.__call__ on a CPU fp32 batch with the random part given: returns (mixed copy of x, mixed targets)."""
    assert x.dtype == torch.float32 and not x.is_cuda and len(x) % 2 == 0
    x = x.clone()
    B = len(x)
    if draw["mode"] == 'batch':
        lam = draw["lam"]                                         # a Python double
        if draw["box"] is not None:
            yl, yh, xl, xh = draw["box"]
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        elif lam != 1. and not draw["cutmix"]:
            x_flipped = x.flip(0).mul_(1. - lam)
            x.mul_(lam).add_(x_flipped)
        return x, mixup_target(target, num_classes, lam, smoothing)
    pair = draw["mode"] == 'pair'
    n = B // 2 if pair else B
    lam_batch = np.array(draw["lam"], dtype=np.float32)           # timm's float32 array, the corrected lam already stored in it
    assert lam_batch.shape == (n,)
    x_orig = x.clone()
    for i in range(n):
        j = B - i - 1
        lam = lam_batch[i]                                        # a np.float32: 1 - lam below is an fp32 subtraction
        if draw["box"][i] is not None:
            yl, yh, xl, xh = draw["box"][i]
            x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
            if pair:
                x[j][:, yl:yh, xl:xh] = x_orig[i][:, yl:yh, xl:xh]
        elif lam != 1. and not draw["cutmix"][i]:
            x[i] = x[i] * float(lam) + x_orig[j] * float(1 - lam)
            if pair:
                x[j] = x[j] * float(lam) + x_orig[i] * float(1 - lam)
    if pair:
        lam_batch = np.concatenate((lam_batch, lam_batch[::-1]))
    lam_t = torch.tensor(lam_batch, dtype=x.dtype).unsqueeze(1)
    return x, mixup_target(target, num_classes, lam_t, smoothing)


class RefMixup:
    """A mixup_fn for the eager loop on CPU tensors: Mixup's draws (so the generator is used exactly as by the class under test), timm's
    statements above."""

    def __init__(self, mixer):
        self.mixer = mixer

    def __call__(self, x, target):
        d = self.mixer.draw(len(x), tuple(x.shape[-2:]))
        return mix(x, target, d, self.mixer.num_classes, self.mixer.label_smoothing)


def emulate(x, labels, params, num_classes, on, off, norm=None, out=None, targets_out=None):
    """vitres.kernels.mixup from its arguments alone: the table's fp32 lam / oml, its boxes and flags, partner B-1-i."""
    import vitres.kernels as K
    want = torch.float32 if norm is None else torch.uint8
    if x.dim() != 4 or x.dtype != want:
        raise TypeError("a %s [B,C,H,W] tensor expected" % want)
    B, C, H, W = x.shape
    params = K.check_mixup_params(params, B, H, W)
    if norm is None:
        xf = x
    else:
        m = torch.tensor(list(norm[0]), dtype=torch.float32).view(1, -1, 1, 1)          # (already in uint8 units: norm_constants)
        s = torch.tensor(list(norm[1]), dtype=torch.float32).view(1, -1, 1, 1)
        xf = x.float().sub_(m).div_(s)
    res = xf.clone()
    for i in range(B):
        j, p = B - 1 - i, params[i]
        if p["cutmix"]:
            res[i][:, p["y0"]:p["y1"], p["x0"]:p["x1"]] = xf[j][:, p["y0"]:p["y1"], p["x0"]:p["x1"]]
        elif p["lam"] != 1 or p["oml"] != 0:                      # (a double just below 1 rounds to lam = 1.f, but its oml is not 0)
            res[i] = xf[i] * float(p["lam"]) + xf[j] * float(p["oml"])
    y = one_hot(labels, num_classes, float(np.float32(on)), float(np.float32(off)))
    lam = torch.tensor(params["lam"].copy()).unsqueeze(1)
    oml = torch.tensor(params["oml"].copy()).unsqueeze(1)
    t = y * lam + y.flip(0) * oml
    for given, val, shape in ((out, res, (B, C, H, W)), (targets_out, t, (B, num_classes))):
        if given is not None and (given.dtype != torch.float32 or tuple(given.shape) != shape or not given.is_contiguous()):
            raise ValueError("out / targets_out must be a contiguous fp32 tensor of shape %s" % (shape,))
    if out is not None:
        res = out.copy_(res)
    if targets_out is not None:
        t = targets_out.copy_(t)
    return res, t


def install(monkeypatch):
    import vitres.kernels as K
    calls = []

    def mixup(x, labels, params, num_classes, on, off, norm=None, out=None, targets_out=None):
        res = emulate(x, labels, params, num_classes, on, off, norm=norm, out=out, targets_out=targets_out)
        calls.append(dict(x=x, params=np.array(params, dtype=K.MIXUP_PARAM), on=on, off=off, norm=norm, out=out,
                          targets_out=targets_out, result=res))
        return res
    monkeypatch.setattr(K, "mixup", mixup)
    return calls
