"""SwitchTokenMix for the HIP path (reference token_mixup.py:39-162; constructed in main.py:316-322 as `patch_mixup_fn`).

Every call mixes the first half of the batch at patch level (a random box of the patch_len x patch_len grid is taken from a
permuted partner; the per-patch soft targets follow the box) and the second half at image level (mixup with lam ~ Beta(.8,.8)).
The random draws use the SAME generators in the SAME order as the reference -- torch's CPU generator for the two
permutations, numpy's global generator for the Beta samples and the box -- so a run seeded like the reference sees the same
mixes; the tensor work is one `vr_token_mix` call (two streaming kernels).  Returns the reference's 4-tuple
`(samples, targets, patch_targets, 'seq')`; unlike the reference the input batch is not modified in place (`out=`,
`targets_out=` and `patch_targets_out=` let the caller mix straight into e.g. the static input buffers of a captured hipGraph).

`input_norm=(mean, std)` (0..1 units, e.g. the ImageNet defaults) makes the mix the normaliser of a uint8 input pipeline: the
batch arrives as uint8 NCHW (timm's fast_collate; `vitres.data.DevicePrefetchLoader(..., normalize=False)`) and one
`vr_token_mix_u8` pass reads the bytes, normalises as timm's PrefetchLoader does and mixes -- the same bits as normalising first.

`erase=RandomErasing(...)` (vitres/random_erasing.py) erases every sample before it is mixed, as the reference's loader transform does:
uint8 batches take `vr_token_mix_u8_erase` (still one pass); fp32 batches are copied, erased by `vr_random_erase` and mixed as before.
The table of a call is left in `last_erase`; `draw=` replays it when the draw carries it as draw["erase"].
"""
import numpy as np
import torch

from . import kernels
from .kernels import norm_constants
from .mixup import erase_of


class SwitchTokenMix:
    def __init__(self, patch_len, switch_prob=0.5, num_classes=1000, smoothing=0.1, input_norm=None, erase=None):
        self.patch_len, self.switch_prob, self.num_classes, self.smoothing = patch_len, switch_prob, num_classes, smoothing
        # (mean, std) in uint8 units as two host float arrays, or None: the samples arrive normalised
        self.input_norm = None if input_norm is None else norm_constants(*input_norm)
        self.erase, self.last_erase = erase, None                 # a vitres.random_erasing.RandomErasing, or None

    @property
    def normalizes(self):
        """True: takes uint8 samples and normalises them (input_norm=); False: takes normalised fp32 samples."""
        return self.input_norm is not None

    def check_dtype(self, samples):
        """The dtype rules, before anything is drawn or launched."""
        if samples.dtype == torch.uint8 and self.input_norm is None:
            raise ValueError('SwitchTokenMix got uint8 samples but no input_norm=(mean, std): they would be mixed un-normalised')
        if samples.dtype != torch.uint8 and self.input_norm is not None:
            raise ValueError('SwitchTokenMix(input_norm=...) normalises uint8 samples; %s samples would be normalised twice'
                             % samples.dtype)

    def __repr__(self):
        return '(patch_len={}, switch_prob={})'.format(self.patch_len, self.switch_prob)

    def draw(self, batch):
        """Host-side randomness of one call (reference order: token_mixup.py:149-150 -> 104-106 -> 74-95, then 126-127)."""
        pl, h = self.patch_len, batch // 2
        perm_a = torch.randperm(h)

        def randint(lo, hi, size=None):
            return np.random.randint(lo, lo + 1 if lo == hi else hi, size=size)
        lam = np.random.beta(1., 1.)
        area = int(pl * pl * lam)
        ch = randint(1, max(1, min(pl, area) - 1))
        cw = area // ch
        if cw > pl:
            cw, ch = pl, area // pl
        y0 = int(randint(0, max(0, pl - ch), size=2)[1])
        x0 = int(randint(0, max(0, pl - cw), size=2)[1])
        lam_patch = 1 - (ch * cw + 0.0) / (pl * pl)
        perm_b = torch.randperm(batch - h)
        lam_img = np.random.beta(0.8, 0.8)
        partner = torch.cat([perm_a, perm_b + h])
        return dict(half=h, partner=partner, box=(y0, y0 + int(ch), x0, x0 + int(cw)), lam_patch=float(lam_patch),
                    lam_img=float(lam_img))

    def __call__(self, samples, targets, out=None, draw=None, targets_out=None, patch_targets_out=None):
        self.check_dtype(samples)
        if self.erase is not None or (draw is not None and draw.get("erase") is not None):
            return self._erase_and_mix(samples, targets, out, draw, targets_out, patch_targets_out)
        return self._mix(samples, targets, out, draw, targets_out, patch_targets_out)

    def _erase_and_mix(self, samples, targets, out, draw, targets_out, patch_targets_out):
        B, C, H, W = samples.shape
        d = draw or self.draw(B)
        ea = self.last_erase = erase_of(self.erase, d, samples)
        if self.input_norm is None:                               # fp32: erase a copy, then the mix as it is
            x = kernels.random_erase(samples.float().clone(memory_format=torch.contiguous_format), ea)
            return self._mix(x, targets, out, d, targets_out, patch_targets_out)
        return self._mix(samples, targets, out, d, targets_out, patch_targets_out, ea)

    def _mix(self, samples, targets, out, draw, targets_out, patch_targets_out, erase=None):
        d = draw or self.draw(samples.shape[0])
        off = self.smoothing / self.num_classes
        x = samples if self.input_norm is not None else samples.float()
        res = kernels.token_mix(x, targets, d, self.patch_len, self.num_classes, 1. - self.smoothing + off, off, self.input_norm, erase,
                                out=out, targets_out=targets_out, patch_targets_out=patch_targets_out)
        return res + ('seq',)
