"""Writes tests/golden/f23_ragged_pil.npz: the cases tests/test_gpu_ragged.py and tests/test_ragged_host.py pin for the ragged route
(vr_resample_ragged_u8, vr_jpeg_reconstruct_ragged_u8) -- images of very different sizes, box tables, and what PIL itself makes of
them:
    crop((x0, y0, x0+w, y0+h)).resize((ow, oh), filter).crop((wx, wy, wx+So_w, wy+So_h)) [.transpose(FLIP_LEFT_RIGHT)]
per sample and channel, and Image.open(stream).convert('RGB') for the encoded files.  Needs PIL (written with 12.2.0 and
libjpeg-turbo); the tests read only the .npz.  Run from the repository root:  python tests/golden/make_ragged_golden.py

Resample cases <name>:  <name>.img<k> uint8 [C,h,w] (the images; how they are laid out as ragged planes -- pitches, gaps, fill
bytes -- is the tests' business), <name>.map int32 [B] (sample -> image), <name>.boxes int32 [B,9] (x0, y0, w, h, ow, oh, wx, wy,
flip), <name>.meta int32 (So_h, So_w, filter), <name>.out uint8 [B,C,So_h,So_w].
jpeg_big:  jpeg_big.stream<k> uint8 (the encoded files), jpeg_big.pixels<k> uint8 [h,w,3] (PIL's RGB), and boxes / meta / out as
above, the crop-resize taken from PIL's pixels.
The images are gradients with sparse impulses and small noise patches: they compress, and every tap of a wide support still matters.
"""
import io
import os

import numpy as np
from PIL import Image

BILINEAR, BICUBIC = 2, 3


def image(seed, C, h, w):
    """[C,h,w]: a diagonal gradient per channel, one pixel in about 389 set to a random byte, and a noise patch of up to 24 x 24"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((C, h, w), dtype=np.uint8)
    for c in range(C):
        fx, fy = rs.randint(1, 4), rs.randint(1, 4)
        out[c] = ((xx * fx * 255 // max(w - 1, 1) + yy * fy * 255 // max(h - 1, 1)) // (fx + fy) + 40 * c) % 256
        n = max(1, h * w // 389)
        out[c, rs.randint(0, h, n), rs.randint(0, w, n)] = rs.randint(0, 256, n)
        ph, pw = min(h, 24), min(w, 24)
        y0, x0 = rs.randint(0, h - ph + 1), rs.randint(0, w - pw + 1)
        out[c, y0:y0 + ph, x0:x0 + pw] = rs.randint(0, 256, (ph, pw))
    return out


def pil_resample(img, box, So_h, So_w, filt):
    x0, y0, w, h, ow, oh, wx, wy, flip = (int(v) for v in box)
    out = np.empty((img.shape[0], So_h, So_w), dtype=np.uint8)
    for c in range(img.shape[0]):
        im = Image.fromarray(np.ascontiguousarray(img[c]))
        im = im.crop((x0, y0, x0 + w, y0 + h)).resize((ow, oh), filt).crop((wx, wy, wx + So_w, wy + So_h))
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        out[c] = np.asarray(im)
    return out


def cases():
    S = 16
    wide = image(1, 1, 16, 8192)
    # the launch the padded entry refuses: 2049 (bicubic) and 1025 (bilinear) taps per output column
    yield "wide_bicubic", [wide], [0], [(0, 0, 8192, 16, S, S, 0, 0, 0)], (S, S, BICUBIC)
    yield "wide_bilinear", [wide], [0], [(0, 0, 8192, 16, S, S, 0, 0, 0)], (S, S, BILINEAR)
    # 2049 vertical taps per output row
    yield "tall", [image(2, 1, 8192, 16)], [0], [(0, 0, 16, 8192, S, S, 0, 0, 1)], (S, S, BICUBIC)
    # 301 x 1999, three channels: the whole image, a box flush with the bottom-right corner, a one-pixel box, one flush with the top
    # and the right edge mirrored
    yield "both", [image(3, 3, 301, 1999)], [0, 0, 0, 0], [
        (0, 0, 1999, 301, 8, 8, 0, 0, 0), (700, 90, 1299, 211, 8, 8, 0, 0, 0), (1998, 300, 1, 1, 8, 8, 0, 0, 0),
        (1000, 0, 999, 150, 8, 8, 0, 0, 1)], (8, 8, BICUBIC)
    # four samples of four shapes: up-scaling, a wide and a tall down-scaling, a plain one; mirrored and not; one window
    yield "mixed", [image(4, 3, 5, 7), image(5, 3, 40, 1800), image(6, 3, 1500, 12), image(7, 3, 64, 64)], [0, 1, 2, 3], [
        (0, 0, 7, 5, S, S, 0, 0, 1), (3, 1, 1797, 38, S, S, 0, 0, 0), (1, 0, 11, 1500, S, S, 0, 0, 1), (5, 9, 50, 41, 20, 18, 3, 1, 0)], \
        (S, S, BICUBIC)
    yield "mixed_bilinear", [image(4, 3, 5, 7), image(5, 3, 40, 1800), image(6, 3, 1500, 12), image(7, 3, 64, 64)], [0, 1, 2, 3], [
        (0, 0, 7, 5, S, S, 0, 0, 1), (3, 1, 1797, 38, S, S, 0, 0, 0), (1, 0, 11, 1500, S, S, 0, 0, 1), (5, 9, 50, 41, 20, 18, 3, 1, 0)], \
        (S, S, BILINEAR)
    # ResizeCenterCrop(32) of a 96 x 2048 image: the short side to int(32 / 0.875) = 36, so a 768 x 36 virtual image, the window in
    # its middle
    yield "eval_window", [image(8, 3, 96, 2048)], [0], [(0, 0, 2048, 96, 768, 36, 368, 2, 0)], (32, 32, BICUBIC)
    # graph replay: the same planes, two box tables
    pair = [image(9, 3, 30, 900), image(10, 3, 700, 20)]
    yield "graph_a", pair, [0, 1], [(0, 0, 900, 30, S, S, 0, 0, 0), (2, 100, 17, 500, S, S, 0, 0, 1)], (S, S, BICUBIC)
    yield "graph_b", pair, [0, 1], [(450, 3, 449, 25, S, S, 0, 0, 1), (0, 0, 20, 700, S, S, 0, 0, 0)], (S, S, BICUBIC)


def encode(img_hwc, **kw):
    buf = io.BytesIO()
    Image.fromarray(img_hwc).save(buf, **kw)
    return buf.getvalue()


def jpeg_big():
    """three baseline streams -- 4:2:0 at 48 x 4100, 4:4:4, grayscale -- and a PNG (a raw record)"""
    rgb = lambda seed, h, w: np.ascontiguousarray(image(seed, 3, h, w).transpose(1, 2, 0))          # noqa: E731
    files = [encode(rgb(11, 48, 4100), format="JPEG", quality=85, subsampling=2),
             encode(rgb(12, 33, 70), format="JPEG", quality=90, subsampling=0),
             encode(image(13, 1, 20, 37)[0], format="JPEG", quality=80),
             encode(rgb(14, 25, 31), format="PNG")]
    pixels = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    boxes = [(0, 0, 4100, 48, 16, 16, 0, 0, 0), (3, 2, 60, 30, 16, 16, 0, 0, 1), (0, 0, 37, 20, 16, 16, 0, 0, 0),
             (0, 0, 31, 25, 24, 20, 4, 2, 1)]
    return files, pixels, boxes, (16, 16, BICUBIC)


def main():
    out = {}
    n = 0
    for name, images, index, boxes, (So_h, So_w, filt) in cases():
        boxes = np.asarray(boxes, dtype=np.int32)
        for k, img in enumerate(images):
            out["%s.img%d" % (name, k)] = img
        out[name + ".map"], out[name + ".boxes"] = np.asarray(index, dtype=np.int32), boxes
        out[name + ".meta"] = np.asarray([So_h, So_w, filt], dtype=np.int32)
        out[name + ".out"] = np.stack([pil_resample(images[i], boxes[b], So_h, So_w, filt) for b, i in enumerate(index)])
        n += 1
    files, pixels, boxes, (So_h, So_w, filt) = jpeg_big()
    for k, (f, p) in enumerate(zip(files, pixels)):
        out["jpeg_big.stream%d" % k] = np.frombuffer(f, dtype=np.uint8)
        out["jpeg_big.pixels%d" % k] = p
    out["jpeg_big.boxes"] = np.asarray(boxes, dtype=np.int32)
    out["jpeg_big.meta"] = np.asarray([So_h, So_w, filt], dtype=np.int32)
    out["jpeg_big.out"] = np.stack([pil_resample(np.ascontiguousarray(p.transpose(2, 0, 1)), boxes[b], So_h, So_w, filt)
                                    for b, p in enumerate(pixels)])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f23_ragged_pil.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases + jpeg_big, %d bytes" % (path, n, os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
