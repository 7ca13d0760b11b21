#!/usr/bin/env python
"""What the device RandAugment stage costs per batch (vr_rand_augment_u8; vitres.rand_augment.RandAugment draws the op tables).

B = 128 images of 3 x 224 x 224, tables of the recipes' config rand-m9-mstd0.5-inc1 (two layers, each applied with probability
0.5, bicubic affine ops); a handful of seeded tables are rotated through so that one lucky draw does not set the number.  Reported:

  device time per batch      HIP events around `--calls` launches queued back to back (the op tables already on the device, the
                             workspace allocated once), median over `--runs` runs, and one launch at a time (median of single
                             launches, each behind a sync)
  by op kind                 the same batch with ONE layer that applies the same kind to every sample (queued, median): which ops
                             the time goes to.  A workgroup owns a sample, so a launch lasts as long as its slowest sample.
  bytes-moved floor          source + output bytes, plus a write and a read of the workspace plane for every sample with two applied
                             layers, at the 6.3 TB/s a streaming kernel achieves on the MI355X
  PIL on one host core       --pil: the same records applied with PIL on the host this script runs on (no GPU needed: measured where
                             PIL is installed, quoted beside the device numbers for orientation only)

  python tools/randaugment_bench.py > profiles/randaugment_bench.txt      (on the GPU)
  python tools/randaugment_bench.py --pil                                 (where PIL is; prints the PIL line only)
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
from vitres.rand_augment import RandAugment, rotate_matrix                         # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s: what streaming kernels reach on the MI355X (8 TB/s peak)


def tables(args):
    ra = RandAugment(args.config, size=args.size, rng=random.Random(args.seed), np_rng=np.random.RandomState(args.seed))
    return ra, [ra.draw(args.batch) for _ in range(args.tables)]


def images(args):
    """low-frequency content plus noise, so that histograms, means and interpolation see something like a photograph"""
    rs = np.random.RandomState(0)
    S = args.size
    y, x = np.mgrid[0:S, 0:S]
    out = np.empty((args.batch, 3, S, S), dtype=np.uint8)
    for b in range(args.batch):
        for c in range(3):
            f = rs.uniform(0.01, 0.08, 2)
            v = 128 + 120 * np.sin(f[0] * x + rs.uniform(0, 6)) * np.cos(f[1] * y + rs.uniform(0, 6)) + rs.normal(0, 10, (S, S))
            out[b, c] = np.clip(v, 0, 255).astype(np.uint8)
    return out


def one_kind(args, kind):
    t = K.ra_table(args.batch, 1)
    name, filt = kind if isinstance(kind, tuple) else (kind, 0)
    t["op"], t["filter"], t["iarg"], t["factor"] = K.RA_OPS[name], filt, 4 if name == "posterize" else 100, 1.7
    t["m"] = rotate_matrix(27.0, args.size, args.size)
    return t


def pil_line(args):
    import PIL
    from PIL import Image, ImageEnhance, ImageOps
    ra, tabs = tables(args)
    enh = {K.RA_OPS["brightness"]: ImageEnhance.Brightness, K.RA_OPS["color"]: ImageEnhance.Color,
           K.RA_OPS["contrast"]: ImageEnhance.Contrast, K.RA_OPS["sharpness"]: ImageEnhance.Sharpness}

    def apply(img, r):
        op, a = int(r["op"]), int(r["iarg"])
        if op == K.RA_OPS["identity"]:
            return img
        if op == K.RA_OPS["invert"]:
            return ImageOps.invert(img)
        if op == K.RA_OPS["posterize"]:
            return ImageOps.posterize(img, a)
        if op == K.RA_OPS["solarize"]:
            return ImageOps.solarize(img, a)
        if op == K.RA_OPS["solarize_add"]:
            return img.point([min(255, i + a) if i < 128 else i for i in range(256)] * 3)
        if op == K.RA_OPS["autocontrast"]:
            return ImageOps.autocontrast(img)
        if op == K.RA_OPS["equalize"]:
            return ImageOps.equalize(img)
        if op in enh:
            return enh[op](img).enhance(float(r["factor"]))
        return img.transform(img.size, Image.AFFINE, tuple(r["m"].tolist()), resample=int(r["filter"]), fillcolor=ra.fill)

    src = images(args)
    pics = [Image.fromarray(np.ascontiguousarray(src[b].transpose(1, 2, 0)), "RGB") for b in range(args.batch)]
    passes = []
    for t in tabs[:5]:
        t0 = time.perf_counter()
        for b in range(args.batch):
            img = pics[b]
            for k in range(t.shape[1]):
                img = apply(img, t[b, k])
            np.asarray(img)
        passes.append((time.perf_counter() - t0) / args.batch)
    print("  PIL %s on one host core, the same records (RGB %d x %d, %s): %.3f ms per image, median of %d tables (min %.3f, max %.3f) = "
          "%.1f ms per batch of %d on one core" % (PIL.__version__, args.size, args.size, args.config, statistics.median(passes) * 1e3,
                                                   len(passes), min(passes) * 1e3, max(passes) * 1e3,
                                                   statistics.median(passes) * 1e3 * args.batch, args.batch))


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
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--config", default="rand-m9-mstd0.5-inc1")
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pil", action="store_true")
    args = ap.parse_args()
    if args.pil:
        return pil_line(args)
    if not torch.cuda.is_available():
        sys.exit("randaugment_bench.py measures on the GPU: no device visible (--pil measures the host side)")
    dev = torch.device("cuda")
    B, S = args.batch, args.size
    ra, tabs = tables(args)
    src = torch.from_numpy(images(args)).to(dev)
    out = torch.empty_like(src)
    L = K._lib.lib()

    def launcher(host_tables):
        dt = [torch.from_numpy(K.check_ra_table(t, B)).to(dev) for t in host_tables]
        layers = dt[0].shape[1]
        need = int(L.vr_rand_augment_ws_bytes(B, S, S, layers))
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        word = K.ra_fill(ra.fill)

        def launch(i):
            K._lib.check(L.vr_rand_augment_u8(src.data_ptr(), dt[i % len(dt)].data_ptr(), out.data_ptr(), B, S, S, layers, word,
                                              ws.data_ptr() if need else None, need, torch.cuda.current_stream().cuda_stream),
                         "vr_rand_augment_u8")
        return launch

    launch = launcher(tabs)
    for i in range(10):
        launch(i)
    torch.cuda.synchronize()
    queued = [timed(launch, args.calls) for _ in range(args.runs)]
    single = []
    for i in range(60):
        single.append(timed(lambda _i: launch(i), 1))
        torch.cuda.synchronize()
    applied = np.stack([(t["op"] != 0).sum(axis=1) for t in tabs])
    kinds = np.bincount(np.concatenate([t["op"].ravel() for t in tabs]), minlength=12)
    q = statistics.median(queued)
    print("vr_rand_augment_u8 per batch: B = %d images of 3 x %d x %d, tables of RandAugment(%r, interpolation='bicubic'), %d seeded "
          "tables in rotation, already on the device; one workgroup per sample; HIP events" % (B, S, S, args.config, len(tabs)))
    print("  records: %.1f%% identity; samples with 0 / 1 / 2 applied layers: %s; affine records: %.1f%%"
          % (100. * kinds[0] / kinds.sum(), " / ".join("%.1f%%" % (100. * (applied == n).mean()) for n in range(3)),
             100. * kinds[11] / kinds.sum()))
    print("  device time, %d launches queued back to back, median of %d runs: %.4f ms per batch (min %.4f, max %.4f) = %.0f images/s"
          % (args.calls, args.runs, q, min(queued), max(queued), B / q * 1e3))
    single.sort()
    print("  device time, one launch at a time (60 launches, each behind a sync): median %.4f ms (min %.4f, quartiles %.4f .. %.4f)"
          % (statistics.median(single), single[0], single[len(single) // 4], single[3 * len(single) // 4]))
    floor = B * 3 * S * S * (2 + 2 * float((applied >= 2).mean()))
    floor_ms = floor / HBM_ACHIEVABLE * 1e3
    print("  bytes-moved floor: %.1f MB per batch at %.1f TB/s = %.4f ms;  device time / floor = %.1f"
          % (floor / 1e6, HBM_ACHIEVABLE / 1e12, floor_ms, q / floor_ms))
    print("  by op kind, one layer, every sample the same kind (queued, median of %d runs of %d launches), ms per batch:" % (args.runs, args.calls))
    row = []
    for kind in ("identity", "invert", "autocontrast", "equalize", "brightness", "color", "contrast", "sharpness",
                 ("affine", 2), ("affine", 3)):
        fn = launcher([one_kind(args, kind)])
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        t = statistics.median([timed(fn, args.calls) for _ in range(args.runs)])
        row.append("%s %.4f" % (kind if isinstance(kind, str) else "%s(%s)" % (kind[0], {2: "bilinear", 3: "bicubic"}[kind[1]]), t))
    print("    " + ";  ".join(row))
    print("  the stage's neighbours (profiles/resample_bench.txt): vr_resample_u8 0.10 ms, canvas copy 0.56 ms per batch")


if __name__ == "__main__":
    main()
