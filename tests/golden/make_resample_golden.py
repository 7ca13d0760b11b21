"""Writes tests/golden/f20_resample_pil.npz: seeded random uint8 canvases, box tables and what PIL itself makes of them --
    crop((x0, y0, x0+w, y0+h)).resize((ow, oh), filter).crop((wx, wy, wx+So_w, wy+So_h)) [.transpose(FLIP_LEFT_RIGHT)]
per sample and channel -- for the cases tests/test_gpu_resample.py and tests/test_resample_host.py pin.  Needs PIL (written with
12.2.0); the tests read only the .npz.  Run from the repository root:  python tests/golden/make_resample_golden.py

Every case <name> stores <name>.src uint8 [B,C,Hs,Ws], <name>.boxes int32 [B,9] (x0, y0, w, h, ow, oh, wx, wy, flip),
<name>.meta int32 (So_h, So_w, filter) and <name>.out uint8 [B,C,So_h,So_w].  Where a case's image is smaller than its canvas, the
canvas bytes outside the image are 255, so that a kernel reading past its box shows.
"""
import os

import numpy as np
from PIL import Image

BILINEAR, BICUBIC = 2, 3


def pil_case(src, boxes, So_h, So_w, filt):
    B, C = src.shape[:2]
    out = np.empty((B, C, So_h, So_w), dtype=np.uint8)
    for b in range(B):
        x0, y0, w, h, ow, oh, wx, wy, flip = (int(v) for v in boxes[b])
        for c in range(C):
            im = Image.fromarray(np.ascontiguousarray(src[b, c]))
            im = im.crop((x0, y0, x0 + w, y0 + h)).resize((ow, oh), filt).crop((wx, wy, wx + So_w, wy + So_h))
            if flip:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            out[b, c] = np.asarray(im)
    return out


def canvas(seed, B, C, Hs, Ws, image=None):
    """random bytes; with image=(h, w) everything outside the top-left h x w image is 255"""
    src = np.random.RandomState(seed).randint(0, 256, (B, C, Hs, Ws)).astype(np.uint8)
    if image is not None:
        src[:, :, image[0]:, :] = 255
        src[:, :, :, image[1]:] = 255
    return src


def cases():
    S = 16
    full = lambda h, w, flip=0: (0, 0, w, h, S, S, 0, 0, flip)                                     # noqa: E731
    yield "down_bicubic", canvas(1, 1, 3, 40, 56, (37, 53)), [full(37, 53)], (S, S, BICUBIC)
    yield "down_bilinear", canvas(1, 1, 3, 40, 56, (37, 53)), [full(37, 53)], (S, S, BILINEAR)
    yield "up_bicubic", canvas(2, 1, 3, 12, 12, (9, 12)), [full(9, 12)], (S, S, BICUBIC)
    yield "up_bilinear", canvas(2, 1, 3, 12, 12, (9, 12)), [full(9, 12)], (S, S, BILINEAR)
    yield "wide_bicubic", canvas(3, 1, 3, 100, 80, (97, 80)), [full(97, 80)], (S, S, BICUBIC)        # scale about 6: 25 taps
    yield "wide_bilinear", canvas(3, 1, 3, 100, 80, (97, 80)), [full(97, 80)], (S, S, BILINEAR)
    # one-pixel boxes: w = 1, h = 1, both
    yield "thin", canvas(4, 3, 1, 24, 28), [(13, 2, 1, 19, S, S, 0, 0, 0), (3, 11, 22, 1, S, S, 0, 0, 1), (27, 23, 1, 1, S, S, 0, 0, 0)], \
        (S, S, BICUBIC)
    # image 41 x 57 inside a 48 x 64 canvas padded with 255: boxes flush with the image's four edges, then with the canvas's
    yield "edges", canvas(5, 6, 1, 48, 64, (41, 57)), [
        (0, 0, 30, 20, S, S, 0, 0, 0), (27, 5, 30, 20, S, S, 0, 0, 0), (10, 21, 25, 20, S, S, 0, 0, 1), (0, 0, 57, 41, S, S, 0, 0, 0),
        (40, 30, 24, 18, S, S, 0, 0, 0), (0, 0, 64, 48, S, S, 0, 0, 1)], (S, S, BICUBIC)
    yield "edges_bilinear", canvas(5, 6, 1, 48, 64, (41, 57)), [
        (0, 0, 30, 20, S, S, 0, 0, 0), (27, 5, 30, 20, S, S, 0, 0, 0), (10, 21, 25, 20, S, S, 0, 0, 1), (0, 0, 57, 41, S, S, 0, 0, 0),
        (40, 30, 24, 18, S, S, 0, 0, 0), (0, 0, 64, 48, S, S, 0, 0, 1)], (S, S, BILINEAR)
    # the same box mirrored and not, in one batch (the two sources are equal)
    flip_src = np.repeat(canvas(6, 1, 3, 32, 36, (30, 33)), 2, axis=0)
    yield "flip", flip_src, [(2, 3, 29, 25, S, S, 0, 0, 0), (2, 3, 29, 25, S, S, 0, 0, 1)], (S, S, BICUBIC)
    # the centre-crop form: the whole image resized to 32 x 24, a 16 x 16 window at (wx, wy) = (8, 4); and the full resize it is cut from
    yield "window", canvas(7, 1, 3, 44, 60, (43, 57)), [(0, 0, 57, 43, 32, 24, 8, 4, 0)], (S, S, BICUBIC)
    yield "window_full", canvas(7, 1, 3, 44, 60, (43, 57)), [(0, 0, 57, 43, 32, 24, 0, 0, 0)], (24, 32, BICUBIC)
    # three different boxes, one and three channels
    b3 = [(5, 4, 40, 31, S, S, 0, 0, 1), (0, 0, 13, 9, S, S, 0, 0, 0), (20, 10, 31, 37, 24, 20, 5, 2, 0)]
    yield "b3_c1", canvas(8, 3, 1, 48, 52), b3, (S, S, BICUBIC)
    yield "b3_c3", canvas(9, 3, 3, 48, 52), b3, (S, S, BICUBIC)
    # several row bands: a 64 x 64 canvas to 48 x 16 runs in bands of 32 rows, the boundary in mid-image
    yield "bands", canvas(10, 2, 3, 64, 64), [(3, 1, 60, 63, 16, 48, 0, 0, 0), (0, 0, 64, 40, 20, 50, 2, 1, 1)], (48, 16, BICUBIC)
    # graph replay: one source, two box tables
    yield "graph_a", canvas(11, 2, 3, 40, 44), [(1, 2, 30, 33, S, S, 0, 0, 0), (9, 0, 35, 40, S, S, 0, 0, 1)], (S, S, BICUBIC)
    yield "graph_b", canvas(11, 2, 3, 40, 44), [(0, 7, 44, 21, S, S, 0, 0, 1), (12, 12, 9, 11, 20, 18, 3, 1, 0)], (S, S, BICUBIC)
    # one realistic sample: a 256 x 320 canvas, a random-resized-crop box, 224 x 224 (one channel keeps the file small)
    yield "real", canvas(12, 1, 1, 256, 320), [(23, 11, 281, 236, 224, 224, 0, 0, 1)], (224, 224, BICUBIC)


def main():
    out = {}
    for name, src, boxes, (So_h, So_w, filt) in cases():
        boxes = np.asarray(boxes, dtype=np.int32)
        out[name + ".src"], out[name + ".boxes"] = src, boxes
        out[name + ".meta"] = np.asarray([So_h, So_w, filt], dtype=np.int32)
        out[name + ".out"] = pil_case(src, boxes, So_h, So_w, filt)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f20_resample_pil.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(out) // 4, os.path.getsize(path)))


if __name__ == "__main__":
    main()
