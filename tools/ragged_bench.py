#!/usr/bin/env python
"""The padded and the ragged input chain side by side: coefficients -> pixels -> 224 x 224 bicubic crops, per batch of 128.

  padded   vr_jpeg_reconstruct_u8 into one canvas [B,3,Hs,Ws] of the batch maxima, then vr_resample_u8
  ragged   vr_jpeg_reconstruct_ragged_u8 into planes of every image's own size, then vr_resample_ragged_u8

Three batches, all in one job:
  (a) standard      128 streams of 256 x 320 (the batch of profiles/resample_bench.txt): both chains
  (b) one large     127 streams of 375 x 500 and one of 1536 x 2048: both chains (the padded resample runs in bands of one row)
  (c) one camera    127 streams of 375 x 500 and one of 2848 x 4288: the ragged chain only -- vr_resample_u8 refuses the launch --
                    with the bytes either route allocates
Per case the two chains are timed ALTERNATELY (run k of one, run k of the other), HIP events around `--calls` chains queued back
to back, and one chain at a time behind a sync; a handful of seeded box tables of RandomResizedCrop(scale=(0.08, 1), hflip=0.5)
are rotated through.  The spread of the padded chain between its alternating runs is printed beside every comparison: a difference
inside it is no difference.  The streams are made by PIL (4:2:0, quality 90) and Huffman-decoded by jpeg_collate; before timing, both
chains' crops are compared byte for byte wherever both run.

  python tools/ragged_bench.py > profiles/ragged_bench.txt          (on the GPU)
"""
import argparse
import io
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-search_amd"))

from vitres import data                                                            # noqa: E402
from vitres import kernels as K                                                    # noqa: E402
from vitres.resized_crop import RandomResizedCrop                                  # noqa: E402


def stream(seed, h, w):
    from PIL import Image
    rs = np.random.RandomState(seed)
    low = rs.randint(0, 256, (h // 16 + 2, w // 16 + 2, 3)).astype(np.uint8)
    img = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC)).astype(np.int16) + rs.randint(-12, 13, (h, w, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90, subsampling=2)
    return buf.getvalue()


def batch(B, small, large, distinct=8):
    files = [stream(k, *small) for k in range(distinct)]
    out = [files[k % distinct] for k in range(B)]
    if large is not None:
        out[B // 2] = stream(100, *large)
    return data.jpeg_collate([(f, 0) for f in out])


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def line(name, xs):
    return "%s median %.4f ms (min %.4f, max %.4f)" % (name, statistics.median(xs), min(xs), max(xs))


def case(title, collated, args, padded_too):
    dev = torch.device("cuda")
    blob, descs, qtabs, sizes, _ = collated
    B, S = descs.shape[0], args.size
    sizes = sizes.numpy()
    Hs, Ws = ((int(v) + 3) // 4 * 4 for v in sizes.max(axis=0))
    tf = RandomResizedCrop(S, rng=random.Random(args.seed), generator=torch.Generator().manual_seed(args.seed))
    draws = [tf.draw(sizes) for _ in range(args.tables)]
    K.check_jpeg_table(descs.numpy(), blob.numel(), Hs, Ws)
    blob, descs, qtabs = (t.to(dev) for t in (blob, descs, qtabs))
    jws = torch.empty(K.jpeg_ws_bytes(blob.numel()), dtype=torch.uint8, device=dev)
    out_p = torch.empty((B, 3, S, S), dtype=torch.uint8, device=dev)
    out_r = torch.empty_like(out_p)

    layout, nbytes = K.ragged_layout(sizes, 3)
    bounds = K.ragged_bounds(layout)
    flat = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rtabs, need = [], 0
    for d in draws:
        planes = layout.copy()
        boxes = K.check_ragged_boxes(d, planes, S)
        need = max(need, K.ragged_ws_offsets(planes, 3, S, boxes[:, 3]))
        rtabs.append((torch.from_numpy(K.check_ragged_planes(planes, 3, nbytes, sizes)).to(dev), torch.from_numpy(boxes).to(dev)))
    rws = torch.empty(need, dtype=torch.uint8, device=dev)

    def ragged(i):
        planes, boxes = rtabs[i % len(rtabs)]
        K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, planes, dst=flat, workspace=jws, bounds=bounds)
        K.resample_ragged_u8(flat, planes, boxes, 3, S, tf.filter, out=out_r, workspace=rws, bounds=bounds)

    padded_bytes = B * 3 * Hs * Ws
    print("%s: B = %d, canvas %d x %d, blob %.1f MB" % (title, B, Hs, Ws, blob.numel() / 1e6))
    print("  bytes allocated for the pixels and the resample's workspace: padded %.1f MB canvas + 0 (%s); ragged %.1f MB planes + %.1f MB "
          "intermediate" % (padded_bytes / 1e6, "allocated" if padded_too else "NOT allocated: computed", nbytes / 1e6, need / 1e6))
    if padded_too:
        canvas = torch.empty((B, 3, Hs, Ws), dtype=torch.uint8, device=dev)
        ptabs = [torch.from_numpy(K.check_resample_boxes(d, B, Hs, Ws, S)).to(dev) for d in draws]
        band = K.resample_band_rows(3, Hs, Ws, S, tf.filter)

        def padded(i):
            K.jpeg_reconstruct_u8(blob, descs, qtabs, Hs, Ws, out=canvas, workspace=jws)
            K.resample_u8(canvas, ptabs[i % len(ptabs)], S, tf.filter, out=out_p)
        for i in range(len(draws)):
            padded(i)
            ragged(i)
            assert torch.equal(out_p, out_r), "the two chains differ"
        print("  the two chains give the same bytes on all %d box tables; padded resample: bands of %d output rows" % (len(draws), band))
    else:
        try:
            K.resample_band_rows(3, Hs, Ws, S, tf.filter)
            refused = "NOT refused"
        except RuntimeError as e:
            refused = "refused: %s" % e
        print("  padded chain not run: vr_resample_u8 at this canvas is %s" % refused)
        for i in range(3):
            ragged(i)
    torch.cuda.synchronize()
    qp, qr = [], []
    for _ in range(args.runs):
        if padded_too:
            qp.append(timed(padded, args.calls))
        qr.append(timed(ragged, args.calls))
    sp, sr = [], []
    for i in range(args.single):
        if padded_too:
            sp.append(timed(lambda _i: padded(i), 1))
            torch.cuda.synchronize()
        sr.append(timed(lambda _i: ragged(i), 1))
        torch.cuda.synchronize()
    print("  %d chains queued back to back, %d alternating runs:" % (args.calls, args.runs))
    if padded_too:
        print("    " + line("padded", qp) + "; its own spread between runs: %.4f ms" % (max(qp) - min(qp)))
    print("    " + line("ragged", qr))
    if padded_too:
        print("    ragged - padded = %+.4f ms (%.2fx)" % (statistics.median(qr) - statistics.median(qp),
                                                         statistics.median(qr) / statistics.median(qp)))
    print("  one chain at a time (%d each, every one behind a sync):" % args.single)
    if padded_too:
        print("    " + line("padded", sp))
    print("    " + line("ragged", sr))
    # the ragged chain's two stages on their own
    planes, boxes = rtabs[0]
    rec = [timed(lambda i: K.jpeg_reconstruct_ragged_u8(blob, descs, qtabs, planes, dst=flat, workspace=jws, bounds=bounds),
                 args.calls) for _ in range(args.runs)]
    res = [timed(lambda i: K.resample_ragged_u8(flat, rtabs[i % len(rtabs)][0], rtabs[i % len(rtabs)][1], 3, S, tf.filter, out=out_r,
                                                workspace=rws, bounds=bounds), args.calls) for _ in range(args.runs)]
    print("  ragged stages alone, queued: " + line("reconstruct", rec) + "; " + line("resample (two launches)", res))
    return statistics.median(qr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--single", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_bench.py measures on the GPU: no device visible")
    print("padded chain (vr_jpeg_reconstruct_u8 + vr_resample_u8) against ragged chain (vr_jpeg_reconstruct_ragged_u8 + "
          "vr_resample_ragged_u8): streams 4:2:0 quality 90 -> %d x %d bicubic, boxes of RandomResizedCrop(scale=(0.08, 1), hflip=0.5), "
          "%d seeded tables in rotation, tables on the device; HIP events" % (args.size, args.size, args.tables))
    a = case("(a) standard, 256 x 320", batch(args.batch, (256, 320), None), args, True)
    case("(b) 127 of 375 x 500 and one of 1536 x 2048", batch(args.batch, (375, 500), (1536, 2048)), args, True)
    case("(c) 127 of 375 x 500 and one of 2848 x 4288", batch(args.batch, (375, 500), (2848, 4288)), args, False)
    print("the copy the input stages run beside is the 1.33 ms blob upload of profiles/jpeg_bench.txt; the RandAugment stage "
          "(profiles/randaugment_bench.txt, not changed here) takes 0.37 ms: ragged chain (a) + RandAugment = %.3f ms" % (a + 0.37))


if __name__ == "__main__":
    main()
