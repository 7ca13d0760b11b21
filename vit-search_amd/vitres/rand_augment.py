"""RandAugment for the HIP input chain: the draws of timm 0.3.2's rand_augment_transform / RandAugment / AugmentOp as op tables for
vr_rand_augment_u8 (include/vitres_hip.h).  The reference trains every recipe with --aa rand-m9-mstd0.5-inc1 (main.py's default) and
gets the transform from timm's create_transform, where it sits between the flip and ToTensor and PIL does two passes per image on
the host; here the device applies it to the uint8 [B,3,S,S] batch vr_resample_u8 wrote, with PIL's bytes.

timm is not vendored by the reference and is not importable here: the statements below are restated from timm 0.3.2's
auto_augment.py and transforms_factory.py as documented, the way vitres/resized_crop.py and vitres/random_erasing.py restate theirs,
and parity is NOT pinned at that boundary by a golden file.  What IS pinned is the pixel side: vr_rand_augment_u8 against PIL itself
(tests/golden/f21_randaugment_pil.npz), and the rotation matrix against Image.rotate where PIL is importable.

Restated, per sample: np.random.choice(ops, n) picks the layers' ops (uniformly; the `w` section's choice weights are not
implemented); then, per op in order, from Python's `random`: random() > 0.5 skips the op; the magnitude is gauss(m, mstd) if
mstd > 0, clipped to [0, 10]; the op's level function turns it into the argument (`_randomly_negate` is one more random());
interpolation='random' draws choice((BILINEAR, BICUBIC)) per affine op, last.  With L = magnitude / 10:
    Rotate +-30 L degrees, ShearX / ShearY +-0.3 L, TranslateXRel / TranslateYRel +-0.45 L of the width / height,
    Color / Contrast / Brightness / Sharpness 0.1 + 1.8 L (increasing: 1 +- 0.9 L), Posterize int(4 L) bits (increasing: 4 - int(4 L);
    8 or more bits return the image), Solarize int(256 L) (increasing: 256 - int(256 L)), SolarizeAdd int(110 L) below 128.
The `inc` section switches to the increasing list whatever its digit (timm tests bool() of the digit's STRING).  The fill colour of
the affine ops is create_transform's img_mean: min(255, round(255 m)) per channel.  ColorJitter is not implemented: timm skips it
whenever auto_augment is set, so no recipe that reaches this file runs it.
"""
import math
import random
import re

import numpy as np

from . import kernels as K

_MAX_LEVEL = 10.
_BILINEAR, _BICUBIC = K.RESAMPLE_FILTERS["bilinear"], K.RESAMPLE_FILTERS["bicubic"]

# timm's _RAND_TRANSFORMS and _RAND_INCREASING_TRANSFORMS, in their order
RAND_TRANSFORMS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast',
                   'Brightness', 'Sharpness', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')
RAND_INCREASING_TRANSFORMS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'PosterizeIncreasing', 'SolarizeIncreasing',
                              'SolarizeAdd', 'ColorIncreasing', 'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing',
                              'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')
_PLAIN = {'AutoContrast': 'autocontrast', 'Equalize': 'equalize', 'Invert': 'invert'}
_ENHANCE = {'Color': 'color', 'Contrast': 'contrast', 'Brightness': 'brightness', 'Sharpness': 'sharpness'}
_AFFINE = ('Rotate', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')


def rotate_matrix(angle, width, height):
    """The matrix Image.rotate(angle) hands to Image.transform for an image of that size (no expand, centre, translate), or None
    where PIL returns a copy (angle % 360 == 0).  The multiples of 90 degrees PIL serves by transposing are not affine resamplings."""
    angle = angle % 360.0
    if angle == 0:
        return None
    if angle == 180 or (angle in (90, 270) and width == height):
        raise NotImplementedError("Image.rotate(%r) transposes the image; vr_rand_augment_u8 has no such op" % angle)
    cx, cy = width / 2, height / 2
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def parse_config(config_str):
    """timm's rand_augment_transform: (magnitude, layers, magnitude_std, increasing) of e.g. 'rand-m9-mstd0.5-inc1'"""
    magnitude, layers, mstd, increasing = _MAX_LEVEL, 2, 0., False
    config = config_str.split('-')
    if config[0] != 'rand':
        raise ValueError("a RandAugment config string starts with 'rand', got %r" % config_str)
    for c in config[1:]:
        cs = re.split(r'(\d.*)', c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == 'mstd':
            mstd = float(val)
        elif key == 'inc':
            increasing = bool(val)                        # (timm: the string, so 'inc0' switches it on as well)
        elif key == 'm':
            magnitude = int(val)
        elif key == 'n':
            layers = int(val)
        elif key == 'w':
            raise NotImplementedError("RandAugment choice weights (the 'w' section) are not implemented")
        else:
            raise ValueError("Unknown RandAugment config section %r in %r" % (key, config_str))
    return magnitude, layers, mstd, increasing


class RandAugment:
    """timm 0.3.2's rand_augment_transform(config_str, hparams) as create_transform calls it (img_mean = the fill colour,
    interpolation = the affine ops' filter, 'random' = bilinear or bicubic per op): .draw(B) makes the host op table
    (vitres.kernels.ra_table, [B, layers]) for a batch of `size` x `size` (or (H, W)) images; vr_rand_augment_u8 applies it with
    .fill.  The op choice comes from numpy's global state (or np_rng=, a RandomState), everything else from Python's `random` (or
    rng=, a random.Random), one sample after the other, as a per-sample transform pipeline consumes both.  .layers is the table's
    second dimension.  DeviceCropLoader(augment=) is where it runs."""

    def __init__(self, config_str='rand-m9-mstd0.5-inc1', size=224, mean=K.IMAGENET_DEFAULT_MEAN, interpolation='bicubic', rng=None,
                 np_rng=None):
        if interpolation not in ('bilinear', 'bicubic', 'random'):
            raise ValueError("interpolation must be 'bilinear', 'bicubic' or 'random', got %r" % (interpolation,))
        self.config_str, self.interpolation = config_str, interpolation
        self.magnitude, self.layers, self.magnitude_std, self.increasing = parse_config(config_str)
        if not 1 <= self.layers <= K.RA_MAX_LAYERS:
            raise ValueError("vr_rand_augment_u8 takes 1..%d layers, the config asks for %d" % (K.RA_MAX_LAYERS, self.layers))
        self.ops = RAND_INCREASING_TRANSFORMS if self.increasing else RAND_TRANSFORMS
        self.prob = 0.5
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))      # (H, W)
        self.fill = tuple(min(255, round(255 * m)) for m in mean)
        self.rng, self.np_rng = rng, np_rng

    def __repr__(self):
        return 'RandAugment({!r}, size={}, fill={}, interpolation={})'.format(self.config_str, self.size, self.fill, self.interpolation)

    def _negate(self, rnd, v):
        return -v if rnd.random() > 0.5 else v

    def _filter(self, rnd):
        if self.interpolation == 'random':
            return rnd.choice((_BILINEAR, _BICUBIC))
        return K.RESAMPLE_FILTERS[self.interpolation]

    def level_to_record(self, name, level, rnd, rec):
        """AugmentOp's level function and op for a magnitude already drawn and clipped: fills the record `rec` (one element of an
        ra_table) and consumes what timm consumes from `rnd`"""
        H, W = self.size
        L = level / _MAX_LEVEL
        if name in _PLAIN:
            rec['op'] = K.RA_OPS[_PLAIN[name]]
        elif name in _AFFINE:
            if name == 'Rotate':
                m = rotate_matrix(self._negate(rnd, L * 30.), W, H)
            elif name == 'ShearX':
                m = (1, self._negate(rnd, L * 0.3), 0, 0, 1, 0)
            elif name == 'ShearY':
                m = (1, 0, 0, self._negate(rnd, L * 0.3), 1, 0)
            elif name == 'TranslateXRel':
                m = (1, 0, self._negate(rnd, L * 0.45) * W, 0, 1, 0)
            else:
                m = (1, 0, 0, 0, 1, self._negate(rnd, L * 0.45) * H)
            filt = self._filter(rnd)
            if m is not None:                             # (a rotation by 0 degrees is PIL's copy)
                rec['op'], rec['filter'], rec['m'] = K.RA_OPS['affine'], filt, m
        elif name.endswith('Increasing') and name[:-10] in _ENHANCE:
            rec['op'], rec['factor'] = K.RA_OPS[_ENHANCE[name[:-10]]], 1.0 + self._negate(rnd, L * .9)
        elif name in _ENHANCE:
            rec['op'], rec['factor'] = K.RA_OPS[_ENHANCE[name]], L * 1.8 + 0.1
        elif name in ('Posterize', 'PosterizeIncreasing'):
            bits = int(L * 4) if name == 'Posterize' else 4 - int(L * 4)
            if bits < 8:
                rec['op'], rec['iarg'] = K.RA_OPS['posterize'], bits
        elif name in ('Solarize', 'SolarizeIncreasing'):
            rec['op'], rec['iarg'] = K.RA_OPS['solarize'], int(L * 256) if name == 'Solarize' else 256 - int(L * 256)
        elif name == 'SolarizeAdd':
            rec['op'], rec['iarg'] = K.RA_OPS['solarize_add'], int(L * 110)
        else:
            raise ValueError("unknown RandAugment op %r" % name)

    def draw(self, B):
        rnd = self.rng if self.rng is not None else random
        nrnd = self.np_rng if self.np_rng is not None else np.random
        table = K.ra_table(B, self.layers)
        for b in range(B):
            chosen = nrnd.choice(len(self.ops), self.layers)
            for k, i in enumerate(chosen):
                if self.prob < 1.0 and rnd.random() > self.prob:
                    continue
                magnitude = self.magnitude
                if self.magnitude_std and self.magnitude_std > 0:
                    magnitude = rnd.gauss(magnitude, self.magnitude_std)
                magnitude = min(_MAX_LEVEL, max(0, magnitude))
                self.level_to_record(self.ops[int(i)], magnitude, rnd, table[b, k:k + 1])
        return table
