#!/usr/bin/env python
"""What the device crop-and-resize stage costs per batch (vr_resample_u8; vitres.resized_crop.RandomResizedCrop draws the boxes).

B = 128 canvases of 256 x 320 (every image fills its canvas), 3 channels, to 224 x 224 bicubic, boxes from RandomResizedCrop at the
recipe's scale range (0.08, 1) with the flip at 0.5; a handful of seeded box tables are rotated through so that one lucky draw does
not set the number.  Reported:

  device time per batch      HIP events around `--calls` launches queued back to back (the box tables already on the device),
                             median over `--runs` runs, and one launch at a time (median of single launches, each behind a sync)
  canvas copy per batch      the pinned host canvas (B x 3 x 256 x 320 bytes) to the device, HIP events, the same way
  bytes-moved floor          canvas bytes inside the boxes' row ranges (whole canvas rows of the rows each box touches, every
                             channel) plus the output bytes, at the 6.3 TB/s a streaming kernel achieves on the MI355X
  PIL on one host core       --pil: crop + resize + flip of the same crops with PIL on the host this script runs on (no GPU
                             needed: measured where PIL is installed, quoted beside the device numbers for orientation only)

  python tools/resample_bench.py > profiles/resample_bench.txt          (on the GPU)
  python tools/resample_bench.py --pil                                  (where PIL is; prints the PIL line only)
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-search_amd"))

from vitres import kernels as K                                                    # noqa: E402
from vitres.resized_crop import RandomResizedCrop                                  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s: what streaming kernels reach on the MI355X (8 TB/s peak)


def tables(args):
    sizes = np.tile(np.asarray([[args.hs, args.ws]]), (args.batch, 1))
    tf = RandomResizedCrop(args.size, rng=random.Random(args.seed), generator=torch.Generator().manual_seed(args.seed))
    return tf, [K.check_resample_boxes(tf.draw(sizes), args.batch, args.hs, args.ws, args.size) for _ in range(args.tables)]


def floor_bytes(table, C, Ws, size):
    return int(table[:, 3].astype(np.int64).sum()) * C * Ws + table.shape[0] * C * size * size


def pil_line(args):
    from PIL import Image
    tf, tabs = tables(args)
    img = Image.fromarray(np.random.RandomState(0).randint(0, 256, (args.hs, args.ws, 3)).astype(np.uint8))
    rows = tabs[0]
    best = []
    for _ in range(5):
        t0 = time.perf_counter()
        for x0, y0, w, h, ow, oh, _wx, _wy, flip in rows[:, :9].tolist():
            im = img.crop((x0, y0, x0 + w, y0 + h)).resize((ow, oh), tf.filter)
            if flip:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            np.asarray(im)
        best.append((time.perf_counter() - t0) / len(rows))
    import PIL
    print("PIL %s on one host core, the same %d crops (RGB %d x %d -> %d x %d bicubic, + flip): %.3f ms per image, median of 5 passes "
          "(min %.3f) = %.1f ms per batch of %d on one core" % (PIL.__version__, len(rows), args.hs, args.ws, args.size, args.size,
                                                                statistics.median(best) * 1e3, min(best) * 1e3,
                                                                statistics.median(best) * 1e3 * args.batch, args.batch))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hs", type=int, default=256)
    ap.add_argument("--ws", type=int, default=320)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pil", action="store_true")
    args = ap.parse_args()
    if args.pil:
        return pil_line(args)
    if not torch.cuda.is_available():
        sys.exit("resample_bench.py measures on the GPU: no device visible (--pil measures the host side)")
    dev = torch.device("cuda")
    B, C = args.batch, 3
    tf, tabs = tables(args)
    host = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (B, C, args.hs, args.ws)).astype(np.uint8)).pin_memory()
    canvas = host.to(dev)
    dtabs = [torch.from_numpy(t).to(dev) for t in tabs]
    out = torch.empty((B, C, args.size, args.size), dtype=torch.uint8, device=dev)
    launch = lambda i: K.resample_u8(canvas, dtabs[i % len(dtabs)], args.size, tf.filter, out=out)       # noqa: E731
    copy = lambda i: canvas.copy_(host, non_blocking=True)                                               # noqa: E731
    for i in range(10):
        launch(i)
        copy(i)
    torch.cuda.synchronize()
    queued = [timed(launch, args.calls) for _ in range(args.runs)]
    single = []
    for i in range(60):
        single.append(timed(lambda _i: launch(i), 1))
        torch.cuda.synchronize()
    copies = [timed(copy, args.calls) for _ in range(args.runs)]
    floors = [floor_bytes(t, C, args.ws, args.size) for t in tabs]
    floor_ms = statistics.mean(floors) / HBM_ACHIEVABLE * 1e3
    band = K.resample_band_rows(C, args.hs, args.ws, args.size, tf.filter)
    q = statistics.median(queued)
    print("vr_resample_u8 per batch: B = %d canvases of %d x %d x %d -> %d x %d %s, boxes of RandomResizedCrop(scale=(0.08, 1), "
          "hflip=0.5), %d seeded tables in rotation, already on the device; bands of %d output rows; HIP events"
          % (B, C, args.hs, args.ws, args.size, args.size, tf.interpolation, len(tabs), band))
    print("  device time, %d launches queued back to back, median of %d runs: %.4f ms per batch (min %.4f, max %.4f) = %.0f images/s"
          % (args.calls, args.runs, q, min(queued), max(queued), B / q * 1e3))
    single.sort()
    print("  device time, one launch at a time (60 launches, each behind a sync): median %.4f ms (min %.4f, quartiles %.4f .. %.4f)"
          % (statistics.median(single), single[0], single[len(single) // 4], single[3 * len(single) // 4]))
    c = statistics.median(copies)
    print("  canvas copy, pinned host -> device, %.1f MB, %d copies queued back to back, median of %d runs: %.4f ms per batch "
          "(min %.4f, max %.4f) = %.1f GB/s" % (host.numel() / 1e6, args.calls, args.runs, c, min(copies), max(copies),
                                                host.numel() / c / 1e6))
    print("  bytes-moved floor: %.1f MB per batch (canvas rows inside the boxes' row ranges, all channels: %.1f MB; output: %.1f MB) at "
          "%.1f TB/s = %.4f ms;  device time / floor = %.1f;  canvas copy / device time = %.1f"
          % (statistics.mean(floors) / 1e6, (statistics.mean(floors) - B * C * args.size ** 2) / 1e6, B * C * args.size ** 2 / 1e6,
             HBM_ACHIEVABLE / 1e12, floor_ms, q / floor_ms, c / q))


if __name__ == "__main__":
    main()
