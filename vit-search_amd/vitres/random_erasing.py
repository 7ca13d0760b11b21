"""timm's RandomErasing for the HIP path (timm 0.3.2 timm/data/random_erasing.py; the reference hands --reprob 0.25 --remode pixel
--recount 1, the main.py:152 defaults, to timm's create_transform in datasets.py:117-119).

In the reference the erase runs per sample on the NORMALISED tensor inside the loader's transform, before collation and so before
Mixup / SwitchTokenMix.  A uint8 input pipeline normalises on the device, so the erase has to happen there too: the host draws the
rectangles -- Python's `random` module in timm's call order, so a run seeded like the reference sees the same rectangles per sample --
and the device fills them with a counter-based noise that is a pure function of (seed, call, sample, channel, y, x)
(include/vitres_hip.h has the contract).  That makes "erase, then mix" free of a pass of its own: `SwitchTokenMix(..., erase=)`,
`Mixup(..., erase=)` and `DevicePrefetchLoader(..., erase=)` fold it into the uint8 kernels they already run; `__call__` is the
stand-alone form for fp32 batches.

timm is not vendored by the reference and is not importable here: the statements below are restated from timm 0.3.2's source as
remembered, the way vitres/mixup.py restates its Mixup, and parity is NOT pinned at the timm boundary by a golden file.  What differs
by construction: timm draws the fill values from torch's generator per sample inside the loader workers; here they come from
Philox(seed, call, ...), so the rectangles can match a reference run but the noise values cannot.  timm's `num_splits`
(augmentation splits) is not implemented.
"""
import math
import random

import numpy as np

from . import kernels as K


class RandomErasing:
    def __init__(self, probability=0.25, mode='pixel', min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1,
                 max_count=None, seed=0, rng=None):
        if mode not in K.ERASE_MODES:
            raise ValueError('mode must be one of %s, got %r' % (sorted(K.ERASE_MODES), mode))
        self.probability, self.mode = probability, mode
        self.min_area, self.max_area = min_area, max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.min_count, self.max_count = min_count, max_count or min_count
        if not 1 <= self.min_count <= self.max_count:
            raise ValueError('1 <= min_count <= max_count expected, got %r and %r' % (min_count, max_count))
        if self.max_count > K.ERASE_MAX_RECTS:
            raise ValueError('the device table holds at most %d rectangles per sample, max_count = %d' % (K.ERASE_MAX_RECTS,
                                                                                                          self.max_count))
        self.seed, self.call = int(seed) & (2 ** 64 - 1), 0
        self.rng = rng                                            # None: the `random` module's own generator, as timm

    def __repr__(self):
        return '(probability={}, mode={}, count=({}, {}))'.format(self.probability, self.mode, self.min_count, self.max_count)

    # ---- the draws: timm's _erase, per sample, minus the tensor statement ----------------------------------------------------------------
    def _draw_sample(self, H, W, row):
        rnd = self.rng if self.rng is not None else random
        if rnd.random() > self.probability:
            return
        area = H * W
        count = self.min_count if self.min_count == self.max_count else rnd.randint(self.min_count, self.max_count)
        for k in range(count):
            for _attempt in range(10):
                target_area = rnd.uniform(self.min_area, self.max_area) * area / count
                aspect_ratio = math.exp(rnd.uniform(*self.log_aspect_ratio))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < W and h < H:
                    top = rnd.randint(0, H - h)
                    left = rnd.randint(0, W - w)
                    row[k] = (top, top + h, left, left + w)
                    break

    def draw(self, B, H, W):
        """The rectangles of one batch: an int32 [B, R, 4] host array of (y0, y1, x0, x1), R = max_count, drawn sample by sample in
        timm's order.  Slot k of a sample is the k-th rectangle of its count loop; a sample that is not erased, a slot past the
        drawn count and a rectangle whose ten attempts all failed stay empty (all zeros)."""
        rects = np.zeros((B, self.max_count, 4), dtype=np.int32)
        for b in range(B):
            self._draw_sample(H, W, rects[b])
        return rects

    def next_args(self, B, H, W, device=None):
        """What the erase kernels take for the NEXT batch (vitres.kernels.erase_args): a fresh table -- uploaded to `device` from
        pinned memory without a host wait -- with this object's seed and mode, and the call counter, which it advances."""
        args = K.erase_args(self.draw(B, H, W), self.mode, self.seed, self.call, device)
        self.call = (self.call + 1) & (2 ** 64 - 1)
        return args

    def __call__(self, x):
        """Erase a normalised fp32 device batch [B,C,H,W] in place (vr_random_erase); returns it."""
        B, _, H, W = x.shape
        return K.random_erase(x, self.next_args(B, H, W, x.device if x.is_cuda else None))

    # ---- resuming --------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """seed, call and -- with a private generator -- its state.  (With rng=None the draws are the `random` module's, whose
        state belongs to whoever seeds it.)"""
        return dict(seed=self.seed, call=self.call, rng=None if self.rng is None else self.rng.getstate())

    def load_state_dict(self, state):
        self.seed, self.call = int(state["seed"]), int(state["call"])
        if state.get("rng") is not None:
            if self.rng is None:
                raise ValueError('the state holds a private generator, this RandomErasing draws from the random module')
            s = state["rng"]
            self.rng.setstate((s[0], tuple(s[1]), s[2]))
