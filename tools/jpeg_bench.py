#!/usr/bin/env python
"""What the two halves of JPEG decoding cost (vitres.data.jpeg_collate on the host, vr_jpeg_reconstruct_u8 on the device).

The files are a synthetic set made here by PIL: 500 x 375, 4:2:0, quality 90, smooth noise plus fine noise (the mean file size is
printed).  Reported:

  --host   on ONE core (the process pins itself to the core it runs on, torch and numpy at one thread), per image:
             jpeg_collate                  probe + entropy decode + blob assembly, batches of 16 files
             its parts                     vitres.jpeg.probe and vitres.jpeg.entropy_decode (into a zeroed buffer) alone
             the path it replaces          Image.open().convert('RGB') alone, + np.asarray, and + pad_collate_u8 (batches of 16)
           and what 16 such cores deliver against the 18.3 k images/s the captured train step consumes.
  default  on the GPU, B = 128 of the same files:
             device time per batch         HIP events around `--calls` entries queued back to back, median over `--runs` runs, and
                                           one entry at a time (each behind a sync)
             blob upload                   the pinned coefficient blob to the device, the same way; beside it the canvas copy that
                                           the pad_collate_u8 path makes instead (the canvas of the same batch, pinned)
             bytes-moved floor             128 B read per block + 64 B written and read again per block (the sample planes) + 3 B
                                           written per canvas pixel, at the 6.3 TB/s a streaming kernel achieves on the MI355X

  python tools/jpeg_bench.py --host                                     (any machine with PIL)
  python tools/jpeg_bench.py                                            (on the GPU)
"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-search_amd"))

HBM_ACHIEVABLE = 6.3e12      # bytes / s: what streaming kernels reach on the MI355X (8 TB/s peak)
STEP_IMAGES_PER_S = 18.3e3   # what the captured train step consumes
CORES = 16


def make_files(n, H, W, quality, seed):
    from PIL import Image
    rs = np.random.RandomState(seed)
    files = []
    for _ in range(n):
        coarse = rs.uniform(0, 255, (H // 25 + 2, W // 25 + 2, 3)).astype(np.float32)
        img = np.stack([np.asarray(Image.fromarray(coarse[:, :, c]).resize((W, H), Image.BICUBIC)) for c in range(3)], axis=2)
        img = img + rs.normal(0, 12, (H, W, 3))
        buf = io.BytesIO()
        Image.fromarray(np.clip(np.rint(img), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=quality, subsampling=2)
        files.append(buf.getvalue())
    return files


def per_image(fn, n_images, passes):
    times = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) / n_images)
    return statistics.median(times) * 1e3, min(times) * 1e3


def host(args):
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    import torch
    torch.set_num_threads(1)
    import PIL
    from PIL import Image
    from vitres import data
    from vitres import jpeg as J
    files = make_files(args.files, args.h, args.w, args.quality, args.seed)
    n = len(files)
    mean_kb = sum(len(f) for f in files) / n / 1e3
    batches = [[(f, 0) for f in files[lo:lo + 16]] for lo in range(0, n, 16)]
    infos = [J.probe(f) for f in files]
    assert all(i["supported"] for i in infos)
    for a, b in zip(data.jpeg_collate(batches[0])[3].tolist(), [(args.h, args.w)] * 16):
        assert tuple(a) == b

    def pil_only():
        for f in files:
            Image.open(io.BytesIO(f)).convert("RGB").load()

    def pil_array():
        for f in files:
            np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))

    def pil_collate():
        for b in batches:
            data.pad_collate_u8([(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), y) for f, y in b])

    def ours():
        for b in batches:
            data.jpeg_collate(b)

    def probes():
        for f in files:
            J.probe(f)

    bufs = [np.zeros(64 * sum(i["blocks"]), dtype=np.int16) for i in infos]
    qt = np.zeros((3, 64), dtype=np.uint16)

    def entropy():
        for f, buf in zip(files, bufs):
            J.entropy_decode(f, coef=buf, qtab=qt)

    def zero():
        for buf in bufs:
            buf[...] = 0

    for fn in (pil_only, ours):
        fn()
    print("host side on one core (pinned), %d files made by PIL %s: %d x %d, 4:2:0, quality %d, smooth noise + fine noise, mean %.1f KB;"
          " median (min) of %d passes, ms per image" % (n, PIL.__version__, args.w, args.h, args.quality, mean_kb, args.passes))
    rows = [("Image.open().convert('RGB')", pil_only), ("  + np.asarray", pil_array), ("  + pad_collate_u8, batches of 16", pil_collate),
            ("vitres.jpeg.probe", probes), ("vitres.jpeg.entropy_decode into a zeroed buffer", entropy),
            ("(zeroing those buffers again)", zero), ("jpeg_collate, batches of 16", ours)]
    res = {}
    for name, fn in rows:
        res[name] = per_image(fn, n, args.passes)
        print("  %-52s %.3f (%.3f)" % (name, *res[name]))
    old, new = res["  + pad_collate_u8, batches of 16"][0], res["jpeg_collate, batches of 16"][0]
    for name, ms in (("the PIL path", old), ("jpeg_collate", new)):
        rate = CORES / ms * 1e3
        print("  %d cores of %s: %.1f k images/s, %s the %.1f k images/s the captured step consumes"
              % (CORES, name, rate / 1e3, "above" if rate >= STEP_IMAGES_PER_S else "BELOW", STEP_IMAGES_PER_S / 1e3))
    print("  jpeg_collate / the PIL path = %.2f (host time per image)" % (new / old))


def timed(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def device(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("jpeg_bench.py measures the device half on the GPU: no device visible (--host measures the host side)")
    from vitres import data
    from vitres import kernels as K
    dev = torch.device("cuda")
    files = make_files(min(args.files, args.batch), args.h, args.w, args.quality, args.seed)
    B = args.batch
    samples = [(files[i % len(files)], 0) for i in range(B)]
    blob, descs, qtabs, sizes, _ = data.jpeg_collate(samples)
    Hs, Ws = ((int(v) + 3) // 4 * 4 for v in sizes.numpy().max(axis=0))
    K.check_jpeg_table(descs.numpy(), blob.numel(), Hs, Ws)
    rec = descs.numpy().view(K.JPEG_DESC_DTYPE).reshape(-1)
    blocks = int((rec["bw"].astype(np.int64) * rec["bh"]).sum())
    hblob = blob.pin_memory()
    hcanvas = torch.zeros((B, 3, Hs, Ws), dtype=torch.uint8).pin_memory()
    dblob, ddescs, dq = hblob.to(dev), descs.to(dev), qtabs.to(dev)
    canvas = torch.empty((B, 3, Hs, Ws), dtype=torch.uint8, device=dev)
    ws = torch.empty(K.jpeg_ws_bytes(blob.numel()), dtype=torch.uint8, device=dev)
    launch = lambda i: K.jpeg_reconstruct_u8(dblob, ddescs, dq, Hs, Ws, out=canvas, workspace=ws)       # noqa: E731
    up_blob = lambda i: dblob.copy_(hblob, non_blocking=True)                                           # noqa: E731
    up_canvas = lambda i: canvas.copy_(hcanvas, non_blocking=True)                                      # noqa: E731
    for i in range(5):
        launch(i)
        up_blob(i)
        up_canvas(i)
    torch.cuda.synchronize()
    queued = [timed(torch, launch, args.calls) for _ in range(args.runs)]
    single = []
    for i in range(40):
        single.append(timed(torch, launch, 1))
        torch.cuda.synchronize()
    blobs = [timed(torch, up_blob, args.calls) for _ in range(args.runs)]
    canv = [timed(torch, up_canvas, args.calls) for _ in range(args.runs)]
    launch(0)
    torch.cuda.synchronize()
    from PIL import Image
    want = np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB")).transpose(2, 0, 1)
    assert np.array_equal(canvas[0, :, :args.h, :args.w].cpu().numpy(), want), "the entry's pixels are not PIL's"
    floor = blocks * (128 + 64 + 64) + B * 3 * Hs * Ws
    floor_ms = floor / HBM_ACHIEVABLE * 1e3
    q, single = statistics.median(queued), sorted(single)
    print("vr_jpeg_reconstruct_u8 per batch: B = %d streams of %d x %d, 4:2:0, quality %d (mean %.1f KB) -> canvas %d x 3 x %d x %d; "
          "%d blocks, blob %.1f MB, workspace %.1f MB; two launches per entry; HIP events; pixels checked against PIL's"
          % (B, args.w, args.h, args.quality, sum(len(f) for f in files) / len(files) / 1e3, B, Hs, Ws, blocks, blob.numel() / 1e6,
             ws.numel() / 1e6))
    print("  device time, %d entries queued back to back, median of %d runs: %.4f ms per batch (min %.4f, max %.4f) = %.0f images/s"
          % (args.calls, args.runs, q, min(queued), max(queued), B / q * 1e3))
    print("  device time, one entry at a time (40 entries, each behind a sync): median %.4f ms (min %.4f, quartiles %.4f .. %.4f)"
          % (statistics.median(single), single[0], single[len(single) // 4], single[3 * len(single) // 4]))
    print("  bytes-moved floor: %.1f MB per batch (coefficients read %.1f, sample planes written and read %.1f, canvas written %.1f) at "
          "%.1f TB/s = %.4f ms;  device time / floor = %.1f"
          % (floor / 1e6, blocks * 128 / 1e6, blocks * 128 / 1e6, B * 3 * Hs * Ws / 1e6, HBM_ACHIEVABLE / 1e12, floor_ms, q / floor_ms))
    for name, times, nbytes in (("coefficient blob upload", blobs, hblob.numel()), ("canvas copy it replaces", canv, hcanvas.numel())):
        c = statistics.median(times)
        print("  %s, pinned host -> device, %.1f MB, %d copies queued back to back, median of %d runs: %.4f ms per batch (min %.4f, "
              "max %.4f) = %.1f GB/s" % (name, nbytes / 1e6, args.calls, args.runs, c, min(times), max(times), nbytes / c / 1e6))
    print("  blob upload / canvas copy = %.2f;  device time / canvas copy = %.2f;  the 31.5 MB canvas copy of profiles/resample_bench.txt "
          "took 0.5610 ms" % (statistics.median(blobs) / statistics.median(canv), q / statistics.median(canv)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--h", type=int, default=375)
    ap.add_argument("--w", type=int, default=500)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    return host(args) if args.host else device(args)


if __name__ == "__main__":
    main()
