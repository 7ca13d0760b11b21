"""timm's Mixup / CutMix for the HIP path (timm 0.3.2 timm/data/mixup.py, pinned by the reference's requirements.txt; constructed in
main.py:308-314 as `mixup_fn`, the reference's default input mix: --mixup 0.8 --cutmix 1.0 --mixup-switch-prob 0.5 --mixup-mode batch).

Every sample i is mixed with sample B-1-i (timm's x.flip(0)): a random pixel box is copied from the partner (cutmix) or the two
images are blended x * lam + partner * (1 - lam) (mixup); the targets are the smoothed one-hots blended by the same lam.  `mode`
says who shares a draw: the whole batch ('batch'), nobody ('elem'), or sample i and B-1-i ('pair').  The random draws use numpy's
global generator in timm's call order, so a run seeded like the reference sees the same mixes; the tensor work is one `vr_mixup`
call (two streaming kernels) driven by a per-sample parameter table, to which all three modes come down.  Returns timm's 2-tuple
`(x, target)`; unlike timm the input batch is not modified in place (`out=` and `targets_out=` let the caller mix straight into e.g.
the static input buffers of a captured hipGraph).

`input_norm=(mean, std)` (0..1 units) makes the mix the normaliser of a uint8 input pipeline, as for vitres.token_mixup.SwitchTokenMix:
the batch arrives as uint8 NCHW and one `vr_mixup_u8` pass reads the bytes, normalises as timm's PrefetchLoader does and mixes --
the same bits as normalising first.

`erase=RandomErasing(...)` (vitres/random_erasing.py) erases every sample before it is mixed, as the reference's loader transform does:
uint8 batches take `vr_mixup_u8_erase` (still one pass); fp32 batches are copied, erased by `vr_random_erase` and mixed as before.
The table of a call is left in `last_erase`; `draw=` replays it when the draw carries it as draw["erase"].
"""
import numpy as np
import torch

from . import kernels as K

MODES = ('batch', 'elem', 'pair')


def param_table(draw, batch):
    """One draw -> the MIXUP_PARAM rows of the `batch` samples, with the rounding each mode has in timm.
    batch mode: lam is a Python double that torch rounds when it multiplies, so lam32 = fp32(lam), oml32 = fp32(1. - lam), the
    subtraction in double.  elem / pair: timm keeps lam in a float32 array, so oml32 = fp32(1) - lam32, the subtraction in fp32 (an ulp
    off the other rule for some lam).  pair: sample batch-1-i gets sample i's row.  A cutmix sample that drew no box (lam == 1:
    timm leaves it alone) is an identity row."""
    rows = np.zeros(batch, dtype=K.MIXUP_PARAM)
    if draw["mode"] == 'batch':
        lam = float(draw["lam"])
        rows["lam"], rows["oml"] = np.float32(lam), np.float32(1. - lam)
        if draw["cutmix"] and draw["box"] is not None:
            rows["cutmix"] = 1
            rows["y0"], rows["y1"], rows["x0"], rows["x1"] = draw["box"]
        return rows
    n = batch if draw["mode"] == 'elem' else batch // 2
    lam32 = np.asarray(draw["lam"], dtype=np.float32)
    if lam32.shape != (n,) or len(draw["cutmix"]) != n or len(draw["box"]) != n:
        raise ValueError('a %s-mode draw for %d samples holds %d entries, got %d' % (draw["mode"], batch, n, lam32.size))
    part = np.zeros(n, dtype=K.MIXUP_PARAM)
    part["lam"], part["oml"] = lam32, np.float32(1) - lam32
    for i, (cut, box) in enumerate(zip(draw["cutmix"], draw["box"])):
        if cut and box is not None:
            part["cutmix"][i] = 1
            part["y0"][i], part["y1"][i], part["x0"][i], part["x1"][i] = box
    if draw["mode"] == 'elem':
        return part
    rows[:n], rows[n:] = part, part[::-1]
    return rows


def erase_of(erase, draw, x):
    """The erase arguments of one call of a mix on the batch x: the replayed ones (draw["erase"], what an earlier call left in
    `last_erase`), else the next table of the mix's RandomErasing, else None."""
    if draw.get("erase") is not None:
        return draw["erase"]
    if erase is None:
        return None
    B, _, H, W = x.shape
    return erase.next_args(B, H, W, x.device if x.is_cuda else None)


class Mixup:
    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, input_norm=None, erase=None):
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0                               # (timm: the box comes from minmax, the alpha only switches cutmix on)
        if mode not in MODES:
            raise ValueError('mode must be one of %s, got %r' % (MODES, mode))
        self.mix_prob, self.switch_prob, self.label_smoothing, self.num_classes = prob, switch_prob, label_smoothing, num_classes
        self.mode, self.correct_lam = mode, correct_lam
        self.mixup_enabled = True                                 # (timm: set to False to turn mixing off)
        # (mean, std) in uint8 units as two host float arrays, or None: the samples arrive normalised
        self.input_norm = None if input_norm is None else K.norm_constants(*input_norm)
        self.erase, self.last_erase = erase, None                 # a vitres.random_erasing.RandomErasing, or None

    @property
    def normalizes(self):
        """True: takes uint8 samples and normalises them (input_norm=); False: takes normalised fp32 samples."""
        return self.input_norm is not None

    def check_dtype(self, x):
        """The dtype rules, before anything is drawn or launched."""
        if x.dtype == torch.uint8 and self.input_norm is None:
            raise ValueError('Mixup got uint8 samples but no input_norm=(mean, std): they would be mixed un-normalised')
        if x.dtype != torch.uint8 and self.input_norm is not None:
            raise ValueError('Mixup(input_norm=...) normalises uint8 samples; %s samples would be normalised twice' % x.dtype)

    def __repr__(self):
        return '(mixup_alpha={}, cutmix_alpha={}, mode={})'.format(self.mixup_alpha, self.cutmix_alpha, self.mode)

    # ---- the draws: numpy's global generator, timm's call order -----------------------------------------------------------------------
    def _box_and_lam(self, H, W, lam):
        """timm's cutmix_bbox_and_lam: rand_bbox (margin 0) or rand_bbox_minmax, then lam corrected to the box's area."""
        if self.cutmix_minmax is not None:
            lo, hi = self.cutmix_minmax
            cut_h = np.random.randint(int(H * lo), int(H * hi))
            cut_w = np.random.randint(int(W * lo), int(W * hi))
            yl = np.random.randint(0, H - cut_h)
            xl = np.random.randint(0, W - cut_w)
            yu, xu = yl + cut_h, xl + cut_w
        else:
            ratio = np.sqrt(1 - lam)                              # (elem / pair: lam is a np.float32 and so is the ratio, as in timm)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy = np.random.randint(0, H)
            cx = np.random.randint(0, W)
            yl, yu = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
            xl, xu = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1. - (yu - yl) * (xu - xl) / float(H * W)
        return (int(yl), int(yu), int(xl), int(xu)), lam

    def _params_per_batch(self):
        lam, use_cutmix = 1., False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = bool(np.random.rand() < self.switch_prob)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.:
                use_cutmix = True
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha)
            else:
                assert False, "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
            lam = float(lam_mix)
        return lam, use_cutmix

    def _params_per_elem(self, n):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand(n) < self.switch_prob
                lam_mix = np.where(use_cutmix, np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n),
                                   np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            elif self.cutmix_alpha > 0.:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            else:
                assert False, "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
            lam = np.where(np.random.rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def draw(self, batch, hw=(224, 224)):
        """Everything random about one call on `batch` samples of hw = (H, W) pixels (timm: _mix_batch / _mix_elem / _mix_pair).
        batch mode: dict(mode, lam: Python double, cutmix: bool, box: (y0, y1, x0, x1) or None); elem and pair modes: lam a float32
        array, cutmix a bool array and box a list, one entry per sample (elem) or per pair (pair: batch / 2 entries).  A box is drawn
        only where timm draws one: for a cutmix whose lam is not 1; lam is then the corrected one (correct_lam or minmax)."""
        H, W = hw
        if self.mode == 'batch':
            lam, use_cutmix = self._params_per_batch()
            box = None
            if lam != 1. and use_cutmix:
                box, lam = self._box_and_lam(H, W, lam)
            return dict(mode='batch', lam=lam, cutmix=use_cutmix, box=box)
        n = batch if self.mode == 'elem' else batch // 2
        lam_batch, use_cutmix = self._params_per_elem(n)
        boxes = [None] * n
        for i in range(n):
            lam = lam_batch[i]
            if lam != 1. and use_cutmix[i]:
                boxes[i], lam = self._box_and_lam(H, W, lam)
                lam_batch[i] = lam
        return dict(mode=self.mode, lam=lam_batch, cutmix=use_cutmix, box=boxes)

    def __call__(self, x, target, out=None, draw=None, targets_out=None):
        self.check_dtype(x)
        if x.dim() != 4:
            raise ValueError('Mixup mixes [B,C,H,W] image batches, got a tensor of shape %s' % (tuple(x.shape),))
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        B, _, H, W = x.shape
        d = draw or self.draw(B, (H, W))
        off = self.label_smoothing / self.num_classes
        on = 1. - self.label_smoothing + off
        x = x if self.input_norm is not None else x.float()
        ea = self.last_erase = erase_of(self.erase, d, x)
        if ea is None:
            return K.mixup(x, target, param_table(d, B), self.num_classes, on, off, norm=self.input_norm, out=out,
                           targets_out=targets_out)
        if self.input_norm is not None:
            return K.mixup_u8_erase(x, target, param_table(d, B), self.num_classes, on, off, self.input_norm, ea, out=out,
                                    targets_out=targets_out)
        return K.mixup(K.random_erase(x.clone().contiguous(), ea), target, param_table(d, B), self.num_classes, on, off, out=out,
                       targets_out=targets_out)
