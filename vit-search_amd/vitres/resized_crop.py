"""The geometric head of the input chain for the HIP path: the draws of timm's RandomResizedCropAndInterpolation +
torchvision's RandomHorizontalFlip (training) and the arithmetic of Resize + CenterCrop (evaluation), as box tables for
vr_resample_u8 (include/vitres_hip.h).  The reference gets both chains from timm's create_transform (datasets.py:117-119); there
PIL does the resampling per image on the host, here the loader only decodes and pads (vitres.data.pad_collate_u8) and the device
crops, resizes and mirrors in one pass whose bytes are PIL's.

timm and torchvision are not vendored by the reference and are not importable here: the statements below are restated from timm
0.3.2's transforms.py and torchvision's functional.py as documented, the way vitres/mixup.py and vitres/random_erasing.py restate
theirs, and parity is NOT pinned at that boundary by a golden file.  What IS pinned is the pixel side: vr_resample_u8 against PIL
itself (tests/golden/f20_resample_pil.npz).

What is not here: RandAugment, which sits between the flip and ToTensor, is vitres/rand_augment.py and runs on this stage's output
(DeviceCropLoader(augment=)).  ColorJitter is not implemented: timm skips it whenever auto_augment is set, so no shipped recipe runs
it.  Decoding is not here either: a loader decodes with PIL and pads (pad_collate_u8), or ships JPEG coefficients that the device turns
into the same canvases (vitres.data.jpeg_collate / DeviceJpegLoader, vr_jpeg_reconstruct_u8).  interpolation='random' (timm picks bilinear or bicubic per sample) is not implemented: one launch
has one filter.
"""
import math
import random

import numpy as np
import torch

from . import kernels as K

_FILTERS = ("bilinear", "bicubic")


def _sizes(sizes):
    sizes = np.asarray(sizes.cpu() if isinstance(sizes, torch.Tensor) else sizes, dtype=np.int64)
    if sizes.ndim != 2 or sizes.shape[1] != 2 or (sizes < 1).any():
        raise ValueError("sizes must be a [B, 2] array of positive (height, width) pairs, got shape %s" % (sizes.shape,))
    return sizes


def _pair(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


class RandomResizedCrop:
    """timm 0.3.2's RandomResizedCropAndInterpolation followed by torchvision's RandomHorizontalFlip(hflip), per sample: .draw(sizes)
    makes the [B, 12] int32 box table (vitres.kernels.RESAMPLE_BOX_FIELDS) from each sample's real (h, w); the resampling itself is
    vr_resample_u8 with .size and .filter.  The box draws come from Python's `random` (or rng=, a random.Random), the flips from
    torch's generator (or generator=), one sample after the other: crop, then flip, as a per-sample transform pipeline consumes both."""

    def __init__(self, size=224, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), interpolation='bicubic', hflip=0.5, rng=None,
                 generator=None):
        if interpolation == 'random':
            raise NotImplementedError("interpolation='random' draws a filter per sample; one vr_resample_u8 launch has one filter")
        if interpolation not in _FILTERS:
            raise ValueError("interpolation must be one of %s, got %r" % (_FILTERS, interpolation))
        self.size, self.scale, self.ratio = _pair(size), tuple(scale), tuple(ratio)
        self.interpolation, self.filter, self.hflip = interpolation, K.RESAMPLE_FILTERS[interpolation], float(hflip)
        self.rng, self.generator = rng, generator

    def __repr__(self):
        return 'RandomResizedCrop(size={}, scale={}, ratio={}, interpolation={}, hflip={})'.format(
            self.size, tuple(round(s, 4) for s in self.scale), tuple(round(r, 4) for r in self.ratio), self.interpolation, self.hflip)

    def get_params(self, height, width):
        """timm's get_params on an image of that size: (i, j, h, w) = top, left, height, width of the crop."""
        rnd = self.rng if self.rng is not None else random
        area = width * height
        for _attempt in range(10):
            target_area = rnd.uniform(*self.scale) * area
            log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
            aspect_ratio = math.exp(rnd.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 1 <= w <= width and 1 <= h <= height:          # (timm has no lower bound: an empty crop fails in PIL there)
                i = rnd.randint(0, height - h)
                j = rnd.randint(0, width - w)
                return i, j, h, w
        in_ratio = width / height                             # fallback: the central crop, clamped to the ratio range
        if in_ratio < min(self.ratio):
            w = width
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = height
            w = int(round(h * max(self.ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def draw(self, sizes):
        sizes = _sizes(sizes)
        boxes = K.resample_boxes(len(sizes))
        for b, (height, width) in enumerate(sizes):
            i, j, h, w = self.get_params(int(height), int(width))
            flip = self.hflip > 0 and bool(torch.rand(1, generator=self.generator) < self.hflip)
            boxes[b, :9] = (j, i, w, h, self.size[1], self.size[0], 0, 0, int(flip))
        return boxes


class ResizeCenterCrop:
    """The evaluation transform of timm's create_transform: Resize(int(size / crop_pct), interpolation) then CenterCrop(size), with
    torchvision's integer rules: the short side becomes s = int(size / crop_pct), the long side int(s * long / short), the crop
    origin int(round((dim - size) / 2.0)).  .draw(sizes) gives the box table: box = the whole image, (ow, oh) = the resized size,
    window = the centre crop -- only the window's pixels are computed."""

    def __init__(self, size=224, crop_pct=224 / 256, interpolation='bicubic'):
        if interpolation not in _FILTERS:
            raise ValueError("interpolation must be one of %s, got %r" % (_FILTERS, interpolation))
        self.size, self.crop_pct = _pair(size), float(crop_pct)
        if self.size[0] != self.size[1]:
            raise ValueError("ResizeCenterCrop resizes the short side to one number: a square size is expected, got %s" % (self.size,))
        self.interpolation, self.filter = interpolation, K.RESAMPLE_FILTERS[interpolation]
        self.scale_size = int(self.size[0] / self.crop_pct)
        if self.scale_size < self.size[0]:
            raise ValueError("crop_pct > 1 would crop outside the resized image (torchvision pads there; not implemented)")

    def __repr__(self):
        return 'ResizeCenterCrop(size={}, crop_pct={:.4f}, interpolation={})'.format(self.size, self.crop_pct, self.interpolation)

    def resized(self, height, width):
        """torchvision's Resize(int) on an image of that size: (oh, ow)."""
        s = self.scale_size
        if width <= height:
            return (height, width) if width == s else (int(s * height / width), s)
        return (height, width) if height == s else (s, int(s * width / height))

    def draw(self, sizes):
        sizes = _sizes(sizes)
        boxes = K.resample_boxes(len(sizes))
        for b, (height, width) in enumerate(sizes):
            oh, ow = self.resized(int(height), int(width))
            wy, wx = int(round((oh - self.size[0]) / 2.0)), int(round((ow - self.size[1]) / 2.0))
            boxes[b, :9] = (0, 0, width, height, ow, oh, wx, wy, 0)
        return boxes
