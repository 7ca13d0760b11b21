"""Writes f22_jpeg_pil.npz: JPEG streams encoded by PIL (libjpeg-turbo) and the pixels PIL decodes from them -- the fixture of
tests/test_jpeg_host.py and tests/test_gpu_jpeg.py.  Needs PIL; the tests do not.

    python tests/golden/make_jpeg_golden.py

Every record has a name, a kind (0: a baseline stream the fast path takes, 1: a file that takes the PIL fallback, 2: a damaged stream
PIL refuses, 3: a damaged stream PIL still reads) and its bytes; kinds 0, 1 and 3 also have np.asarray(Image.open(...).convert('RGB')).  All records are concatenated:
`streams` / `stream_off`, `pixels` / `pixel_off` / `shapes`.
  sizes      1x1 3x5 5x3 8x8 16x16 9x17 17x23 37x53 16x6 33x2 2x33 48x40 31x64 (H x W): non-multiples of the MCU, one block, several
             MCU rows, chroma plane widths on both sides of libjpeg's `downsampled_width > 2` rule
  sampling   4:4:4, 4:2:2, 4:2:0, grayscale
  settings   quality 30 with a restart marker every 2 MCUs; quality 85; quality 95 with a restart marker every MCU row; quality 100
             with optimised Huffman tables
"""
import io
import os

import numpy as np
from PIL import Image

SIZES = [(1, 1), (3, 5), (5, 3), (8, 8), (16, 16), (9, 17), (17, 23), (37, 53), (16, 6), (33, 2), (2, 33), (48, 40), (31, 64)]
SAMPLINGS = [("444", 0), ("422", 1), ("420", 2), ("gray", None)]
SETTINGS = [("q30r2", dict(quality=30, restart_marker_blocks=2)), ("q85", dict(quality=85)),
            ("q95rr", dict(quality=95, restart_marker_rows=1)), ("q100opt", dict(quality=100, optimize=True))]


def picture(rng, H, W):
    """smooth colour gradients plus fine noise, so that every frequency and both chroma planes carry something"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((H, W, 3))
    for c in range(3):
        a, b, p = rng.uniform(-1, 1, 3)
        img[:, :, c] = 128 + 90 * np.sin(0.35 * a * yy + 0.29 * b * xx + 3 * p) + rng.normal(0, 18, (H, W))
    img[rng.random((H, W)) < 0.04] = rng.choice([0.0, 255.0])
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(img, fmt="JPEG", **kw):
    buf = io.BytesIO()
    img.save(buf, fmt, **kw)
    return buf.getvalue()


def decoded(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def segment(data, marker):
    """(start, end) of the first segment with that marker byte, the FF included"""
    pos = 2
    while True:
        assert data[pos] == 0xFF
        m, L = data[pos + 1], data[pos + 2] << 8 | data[pos + 3]
        if m == marker:
            return pos, pos + 2 + L
        assert m != 0xDA
        pos += 2 + L


def main():
    rng = np.random.default_rng(22)
    names, kinds, streams, pixels = [], [], [], []
    for H, W in SIZES:
        src = picture(rng, H, W)
        for sname, sub in SAMPLINGS:
            img = Image.fromarray(src).convert("L") if sub is None else Image.fromarray(src)
            for qname, kw in SETTINGS:
                data = encode(img, **kw) if sub is None else encode(img, subsampling=sub, **kw)
                names.append("%dx%d.%s.%s" % (H, W, sname, qname))
                kinds.append(0)
                streams.append(data)
                pixels.append(decoded(data))
    src = picture(rng, 24, 20)
    fallback = [("progressive", encode(Image.fromarray(src), quality=85, progressive=True)),
                ("cmyk", encode(Image.fromarray(src).convert("CMYK"), quality=85)),
                ("png", encode(Image.fromarray(src), "PNG"))]
    for name, data in fallback:
        names.append("fallback." + name)
        kinds.append(1)
        streams.append(data)
        pixels.append(decoded(data))
    good = streams[names.index("17x23.420.q85")]
    sos = segment(good, 0xDA)
    dht = segment(good, 0xC4)
    damaged = [("cut_header", good[:sos[0] - 9]), ("cut_scan", good[:(sos[1] + len(good)) // 2]),
               ("no_huffman_table", good[:dht[0]] + good[dht[1]:])]
    for name, data in damaged:
        try:                                                    # (libjpeg-turbo decodes with the standard tables when one is missing)
            pix, kind = decoded(data), 3
        except Exception:                                       # noqa: BLE001
            pix, kind = np.zeros((0, 0, 3), dtype=np.uint8), 2
        assert kind == 2 or name == "no_huffman_table", name
        names.append("damaged." + name)
        kinds.append(kind)
        streams.append(data)
        pixels.append(pix)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f22_jpeg_pil.npz")
    np.savez_compressed(
        out, names=np.array(names), kinds=np.array(kinds, dtype=np.int32),
        streams=np.frombuffer(b"".join(streams), dtype=np.uint8), stream_off=np.cumsum([0] + [len(s) for s in streams]).astype(np.int64),
        pixels=np.concatenate([p.ravel() for p in pixels]), pixel_off=np.cumsum([0] + [p.size for p in pixels]).astype(np.int64),
        shapes=np.array([p.shape[:2] for p in pixels], dtype=np.int32))
    print("%s: %d records, %d stream bytes, %d pixel bytes, %d bytes on disk" % (
        out, len(names), sum(len(s) for s in streams), sum(p.size for p in pixels), os.path.getsize(out)))


if __name__ == "__main__":
    main()
