"""What the input side of one training batch costs, in front of the captured step of bench.py's default workload (sr_tiny supernet,
B = 128, 3 x 224 x 224, patch_len 4, K = 1000, bf16): the fp32 path as it stands against the uint8 path of
SwitchTokenMix(input_norm=...) mixing straight into the step's static inputs.

  a   pinned fp32 host batch -> device; vr_token_mix into fresh tensors; the three copy_ into the step's static x / t / pt
      (train_one_epoch with a patch_mixup_fn that does not write into the step: GraphedTrainStep._replay's copies)
  b   pinned uint8 host batch -> device; vr_token_mix_u8 into the step's static x / t / pt (no copy at replay)
  c   vr_normalize_u8 alone, device-resident uint8 -> fp32 (the evaluation side: ResidentU8Batches)

One process, the three lines alternating; every timed stage is followed by an untimed replay of the captured step, so each stage
starts from the caches a training step leaves behind.  HIP events bracket the host-to-device copy and the device work of every
stage; per line the MEDIAN over --iters batches after --warmup.  GB/s = the bytes the line must move (from the shapes and the fixed
draw: a 2 x 2 box of the 4 x 4 grid, so the partner is read for 1/4 of the first half and all of the second) over its time.  Before
timing, a and b are checked to leave the same bits in x / t / pt.

    python tools/input_bench.py [--iters 60] [--warmup 10] [--out FILE]

--case mixup: the same question for timm's Mixup / CutMix (vitres.mixup.Mixup, the reference's default mix), B = 128, 3 x 224 x 224,
K = 1000, batch mode, once for a blend (lam = 0.37) and once for a cutmix (a 112 x 112 box), into a pair of static x / t buffers:

  f   pinned fp32 host batch -> device; vr_mixup into fresh tensors; two copy_ into the static x / t
  u   pinned uint8 host batch -> device; vr_mixup_u8 straight into the static x / t
  t   pinned fp32 host batch -> device; timm's torch statements on the device batch (x.flip(0), mul_, add_ / the box assignment,
      mixup_target on the smoothed one-hots); two copy_ into the static x / t

No model here: the lines alternate back to back.  f and u are checked to leave the same bits; whether t does is reported.

--case erase: what random erasing costs inside the uint8 token mix (vitres.random_erasing.RandomErasing, the recipe's mode 'pixel',
count 1; probability 0.25 -- the recipe's -- and 1.0), with the first protocol: B = 128, the uint8 batch resident on the device, into
the static x / t / pt of the captured sr_tiny step, a replay between stages:

  u   vr_token_mix_u8 as it is (no erase)
  e   vr_token_mix_u8_erase
  3   vr_normalize_u8 -> vr_random_erase -> vr_token_mix, the three stages e is specified by

The 2 KB rectangle table of a batch is uploaded (pinned, non-blocking) in front of the timed stage: in training that copy is queued
behind the previous step, here -- every stage starts on an idle device -- it would be timed as device time.  e and 3 are checked to
leave the same bits.  Medians, quartiles and extremes per line."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-search_amd"))

import torch  # noqa: E402

import bench  # noqa: E402

PL, NC = 4, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--case", default="token_mix", choices=["token_mix", "mixup", "erase"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("input_bench.py times the GPU path and needs the MI355X")
    if args.case == "mixup":
        return mixup_case(args)
    if args.case == "erase":
        return erase_case(args)
    from vitres import engine, kernels as K
    from vitres.losses import SoftTargetCrossEntropy
    from vitres.optim import FlatAdamW
    from vitres.token_mixup import SwitchTokenMix
    dev = torch.device("cuda:0")
    B = bench.WORKLOADS["sr_tiny_supernet"]["batch"]
    mean, std = K.IMAGENET_DEFAULT_MEAN, K.IMAGENET_DEFAULT_STD

    # host batches: the fp32 one is the uint8 one normalised on the CPU (timm's statement), both pinned
    g = torch.Generator().manual_seed(0)
    u8_host = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=g)
    m255 = torch.tensor([x * 255 for x in mean]).view(1, 3, 1, 1)
    s255 = torch.tensor([x * 255 for x in std]).view(1, 3, 1, 1)
    f32_host = u8_host.float().sub_(m255).div_(s255).pin_memory()
    u8_host = u8_host.pin_memory()
    labels = torch.randint(0, NC, (B,), generator=g).to(dev)
    h = B // 2
    draw = dict(half=h, partner=torch.cat([torch.randperm(h, generator=g), torch.randperm(B - h, generator=g) + h]),
                box=(1, 3, 1, 3), lam_patch=1 - 4 / 16, lam_img=0.37)
    mix_f, mix_u = SwitchTokenMix(PL, num_classes=NC), SwitchTokenMix(PL, num_classes=NC, input_norm=(mean, std))

    # the captured step whose static inputs are the destination
    torch.manual_seed(0)
    model, _ = bench.build_model("sr_tiny_supernet", torch.bfloat16, dev)
    model.train()
    model.set_epoch(31)
    opt = FlatAdamW(model, engine.param_groups_weight_decay(model, 0.05), lr=5e-4 * B / 512.0)
    opt.own_shadow()
    x0, t0, pt0, _ = mix_f(f32_host.to(dev), labels, draw=draw)
    step = engine.GraphedTrainStep(model, SoftTargetCrossEntropy(), x0, t0, pt0, "seq", optimizer=opt)
    u8_dev, norm_out = u8_host.to(dev), torch.empty((B, 3, 224, 224), device=dev)
    it = [0]

    def replay():
        opt.prepare_step()
        step(step.x, step.t, step.pt, epoch=31, train_iter=it[0], arch_sample="multi")
        it[0] += 1

    def stage_a(ev):
        ev[0].record()
        s = f32_host.to(dev, non_blocking=True)
        ev[1].record()
        xs, t, pt, _ = mix_f(s, labels, draw=draw)
        step.x.copy_(xs, non_blocking=True)
        step.t.copy_(t, non_blocking=True)
        step.pt.copy_(pt, non_blocking=True)
        ev[2].record()

    def stage_b(ev):
        ev[0].record()
        s = u8_host.to(dev, non_blocking=True)
        ev[1].record()
        mix_u(s, labels, out=step.x, targets_out=step.t, patch_targets_out=step.pt, draw=draw)
        ev[2].record()

    def stage_c(ev):
        ev[0].record()
        ev[1].record()
        K.normalize_u8(u8_dev, mean, std, out=norm_out)
        ev[2].record()

    # same bits (a against b against c) before any timing
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    stage_a(evs)
    want = [step.x.clone(), step.t.clone(), step.pt.clone()]
    for buf in (step.x, step.t, step.pt):
        buf.zero_()
    stage_b(evs)
    same = all(torch.equal(a, b) for a, b in zip(want, (step.x, step.t, step.pt)))
    stage_c(evs)
    same = same and torch.equal(norm_out.cpu(), f32_host)
    if not same:
        sys.exit("input_bench.py: the uint8 path does not reproduce the fp32 path's bits")

    N = B * 3 * 224 * 224
    T = 4 * (B * NC + B * PL * PL * NC)                           # targets + patch targets, fp32
    partner = (0.25 * h + (B - h)) / B                            # share of the batch whose partner pixel is read
    lines = [("a fp32 H2D + vr_token_mix + 3 copy_", stage_a, 4 * N, (1 + partner) * 4 * N + 4 * N + T + 2 * (4 * N + T)),
             ("b uint8 H2D + vr_token_mix_u8 in place", stage_b, N, (1 + partner) * N + 4 * N + T),
             ("c vr_normalize_u8 alone", stage_c, 0, N + 4 * N)]
    times = {name: ([], []) for name, _, _, _ in lines}
    for i in range(args.warmup + args.iters):
        for name, fn, _, _ in lines:
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            fn(evs)
            replay()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name][0].append(evs[0].elapsed_time(evs[1]))
                times[name][1].append(evs[1].elapsed_time(evs[2]))
    out = ["input stage per batch: B = %d, 3 x 224 x 224, patch_len %d, K = %d, sr_tiny supernet (bf16 step replayed between stages); "
           "median of %d after %d warm-up, HIP events; x / t / pt of a and b bit-identical" % (B, PL, NC, args.iters, args.warmup)]
    med = {}
    for name, _, host_bytes, dev_bytes in lines:
        h2d, work = statistics.median(times[name][0]), statistics.median(times[name][1])
        total = statistics.median([p + q for p, q in zip(*times[name])])
        med[name[0]] = total
        lo, hi = min(p + q for p, q in zip(*times[name])), max(p + q for p, q in zip(*times[name]))
        row = "%-40s total %7.3f ms (min %.3f max %.3f)" % (name, total, lo, hi)
        if host_bytes:
            row += " | H2D %6.1f MB %7.3f ms %6.1f GB/s" % (host_bytes / 1e6, h2d, host_bytes / h2d / 1e6)
        row += " | device %6.1f MB %7.3f ms %7.1f GB/s" % (dev_bytes / 1e6, work, dev_bytes / work / 1e6)
        out.append(row)
    out.append("b / a = %.3f (%s)" % (med["b"] / med["a"], "b is faster" if med["b"] < med["a"] else "b is NOT faster"))
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def mixup_case(args):
    from vitres import kernels as K
    from vitres.mixup import Mixup
    dev = torch.device("cuda:0")
    B, S, smoothing = bench.WORKLOADS["sr_tiny_supernet"]["batch"], 224, 0.1
    mean, std = K.IMAGENET_DEFAULT_MEAN, K.IMAGENET_DEFAULT_STD
    g = torch.Generator().manual_seed(0)
    u8_host = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, generator=g)
    m255 = torch.tensor([x * 255 for x in mean]).view(1, 3, 1, 1)
    s255 = torch.tensor([x * 255 for x in std]).view(1, 3, 1, 1)
    f32_host = u8_host.float().sub_(m255).div_(s255).pin_memory()
    u8_host = u8_host.pin_memory()
    labels = torch.randint(0, NC, (B,), generator=g).to(dev)
    box = (40, 152, 70, 182)                                      # 112 x 112 pixels, aligned to no lane
    draws = {"blend": dict(mode="batch", lam=0.37, cutmix=False, box=None),
             "cutmix": dict(mode="batch", lam=1. - 112 * 112 / float(S * S), cutmix=True, box=box)}
    mix_f, mix_u = Mixup(num_classes=NC, label_smoothing=smoothing), Mixup(num_classes=NC, label_smoothing=smoothing,
                                                                          input_norm=(mean, std))
    sx, st = torch.empty((B, 3, S, S), device=dev), torch.empty((B, NC), device=dev)

    def one_hot(y, on, off):
        return torch.full((y.size(0), NC), off, device=dev).scatter_(1, y.long().view(-1, 1), on)

    def timm_statements(x, y, d):                                 # timm 0.3.2 Mixup._mix_batch + mixup_target, on the device
        lam = d["lam"]
        if d["box"] is not None:
            yl, yh, xl, xh = d["box"]
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        elif lam != 1.:
            x_flipped = x.flip(0).mul_(1. - lam)
            x.mul_(lam).add_(x_flipped)
        off = smoothing / NC
        on = 1. - smoothing + off
        return x, one_hot(y, on, off) * lam + one_hot(y.flip(0), on, off) * (1. - lam)

    def stage_f(ev, d):
        ev[0].record()
        s = f32_host.to(dev, non_blocking=True)
        ev[1].record()
        x, t = mix_f(s, labels, draw=d)
        sx.copy_(x, non_blocking=True)
        st.copy_(t, non_blocking=True)
        ev[2].record()

    def stage_u(ev, d):
        ev[0].record()
        s = u8_host.to(dev, non_blocking=True)
        ev[1].record()
        mix_u(s, labels, draw=d, out=sx, targets_out=st)
        ev[2].record()

    def stage_t(ev, d):
        ev[0].record()
        s = f32_host.to(dev, non_blocking=True)
        ev[1].record()
        x, t = timm_statements(s, labels, d)
        sx.copy_(x, non_blocking=True)
        st.copy_(t, non_blocking=True)
        ev[2].record()

    N = B * 3 * S * S
    T = 4 * B * NC
    stages = (("f fp32 H2D + vr_mixup + 2 copy_", stage_f, 4 * N), ("u uint8 H2D + vr_mixup_u8 in place", stage_u, N),
              ("t fp32 H2D + timm's torch statements + 2 copy_", stage_t, 4 * N))
    same_t = {}
    for dn, d in draws.items():                                   # the bits, before any timing
        got = []
        for _, fn, _ in stages:
            sx.zero_(), st.zero_()
            fn([torch.cuda.Event(enable_timing=True) for _ in range(3)], d)
            got.append((sx.clone(), st.clone()))
        if not (torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])):
            sys.exit("input_bench.py: vr_mixup_u8 does not reproduce vr_mixup's bits (%s)" % dn)
        same_t[dn] = torch.equal(got[0][0], got[2][0]) and torch.equal(got[0][1], got[2][1])
    # the bytes each of OUR lines must move on the device (the partner is read for the whole batch in a blend, for the box in a cutmix)
    partner = {"blend": 1., "cutmix": 112 * 112 / float(S * S)}
    times = {(name, dn): ([], []) for name, _, _ in stages for dn in draws}
    for i in range(args.warmup + args.iters):
        for dn, d in draws.items():
            for name, fn, _ in stages:
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                fn(evs, d)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[(name, dn)][0].append(evs[0].elapsed_time(evs[1]))
                    times[(name, dn)][1].append(evs[1].elapsed_time(evs[2]))
    out = ["Mixup / CutMix input stage per batch: B = %d, 3 x %d x %d, K = %d, batch mode, into static x / t; median of %d after %d "
           "warm-up, HIP events, lines alternating back to back (no model step between them); x / t of f and u bit-identical"
           % (B, S, S, NC, args.iters, args.warmup)]
    for dn in draws:
        out.append("%s (%s): timm's torch statements on the device leave %s bits as vr_mixup" % (
            dn, "lam = 0.37" if dn == "blend" else "box %s" % (box,), "the same" if same_t[dn] else "NOT the same"))
        for name, _, host_bytes in stages:
            h2d, work = statistics.median(times[(name, dn)][0]), statistics.median(times[(name, dn)][1])
            tot = [p + q for p, q in zip(*times[(name, dn)])]
            row = "  %-48s total %7.3f ms (min %.3f max %.3f) | H2D %6.1f MB %7.3f ms %6.1f GB/s | device %7.3f ms" % (
                name, statistics.median(tot), min(tot), max(tot), host_bytes / 1e6, h2d, host_bytes / h2d / 1e6, work)
            if name[0] == "f":
                dev_bytes = (1 + partner[dn]) * 4 * N + 4 * N + T + 2 * (4 * N + T)
                row += " %6.1f MB %7.1f GB/s" % (dev_bytes / 1e6, dev_bytes / work / 1e6)
            elif name[0] == "u":
                dev_bytes = (1 + partner[dn]) * N + 4 * N + T
                row += " %6.1f MB %7.1f GB/s" % (dev_bytes / 1e6, dev_bytes / work / 1e6)
            out.append(row)
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def erase_case(args):
    import random

    from vitres import engine, kernels as K
    from vitres.losses import SoftTargetCrossEntropy
    from vitres.optim import FlatAdamW
    from vitres.random_erasing import RandomErasing
    from vitres.token_mixup import SwitchTokenMix
    dev = torch.device("cuda:0")
    B, S = bench.WORKLOADS["sr_tiny_supernet"]["batch"], 224
    mean, std = K.IMAGENET_DEFAULT_MEAN, K.IMAGENET_DEFAULT_STD
    g = torch.Generator().manual_seed(0)
    u8_dev = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, NC, (B,), generator=g).to(dev)
    h = B // 2
    draw = dict(half=h, partner=torch.cat([torch.randperm(h, generator=g), torch.randperm(B - h, generator=g) + h]),
                box=(1, 3, 1, 3), lam_patch=1 - 4 / 16, lam_img=0.37)
    mix_f, mix_u = SwitchTokenMix(PL, num_classes=NC), SwitchTokenMix(PL, num_classes=NC, input_norm=(mean, std))
    probs = (0.25, 1.0)
    tables = {p: RandomErasing(probability=p, rng=random.Random(0)).draw(B, S, S) for p in probs}     # the recipe's: pixel, count 1
    share = {p: float(((t[:, 0, 1] - t[:, 0, 0]) * (t[:, 0, 3] - t[:, 0, 2])).sum()) / (B * S * S) for p, t in tables.items()}
    seed = 0x5EED

    torch.manual_seed(0)
    model, _ = bench.build_model("sr_tiny_supernet", torch.bfloat16, dev)
    model.train()
    model.set_epoch(31)
    opt = FlatAdamW(model, engine.param_groups_weight_decay(model, 0.05), lr=5e-4 * B / 512.0)
    opt.own_shadow()
    norm_out = torch.empty((B, 3, S, S), device=dev)
    x0, t0, pt0, _ = mix_f(K.normalize_u8(u8_dev, mean, std, out=norm_out), labels, draw=draw)
    step = engine.GraphedTrainStep(model, SoftTargetCrossEntropy(), x0, t0, pt0, "seq", optimizer=opt)
    into = dict(out=step.x, targets_out=step.t, patch_targets_out=step.pt)
    it = [0]

    def replay():
        opt.prepare_step()
        step(step.x, step.t, step.pt, epoch=31, train_iter=it[0], arch_sample="multi")
        it[0] += 1

    def stage_u(p, ea):                                           # vr_token_mix_u8 as it is
        mix_u(u8_dev, labels, draw=draw, **into)

    def stage_e(p, ea):                                           # vr_token_mix_u8_erase
        mix_u(u8_dev, labels, draw=dict(draw, erase=ea), **into)

    def stage_3(p, ea):                                           # the three stages the fused entry is specified by
        K.normalize_u8(u8_dev, mean, std, out=norm_out)
        K.random_erase(norm_out, ea)
        mix_f(norm_out, labels, draw=draw, **into)

    stages = (("u vr_token_mix_u8 (no erase)", stage_u), ("e vr_token_mix_u8_erase", stage_e),
              ("3 vr_normalize_u8 + vr_random_erase + vr_token_mix", stage_3))
    for p in probs:                                               # the bits, before any timing
        stage_e(p, K.erase_args(tables[p], "pixel", seed, 3, dev))
        want = [b.clone() for b in (step.x, step.t, step.pt)]
        for b in (step.x, step.t, step.pt):
            b.zero_()
        stage_3(p, K.erase_args(tables[p], "pixel", seed, 3, dev))
        if not all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, (step.x, step.t, step.pt))):
            sys.exit("input_bench.py: vr_token_mix_u8_erase does not reproduce the three stages' bits (probability %s)" % p)
    times = {(name, p): [] for name, _ in stages for p in probs}
    for i in range(args.warmup + args.iters):
        for p in probs:
            for name, fn in stages:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ea = K.erase_args(tables[p], "pixel", seed, i, dev)        # (the 2 KB table goes up in front of the timed stage)
                ev[0].record()
                fn(p, ea)
                ev[1].record()
                replay()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[(name, p)].append(ev[0].elapsed_time(ev[1]))
    out = ["random erasing in the uint8 token mix, per batch: B = %d, 3 x %d x %d, patch_len %d, K = %d, mode 'pixel', count 1, uint8 batch "
           "resident on the device, into the static x / t / pt of the captured sr_tiny step (bf16, replayed between stages); median of "
           "%d after %d warm-up, HIP events, the lines alternating in one process; x / t / pt of e and 3 bit-identical"
           % (B, S, S, PL, NC, args.iters, args.warmup)]
    for p in probs:
        out.append("probability %.2f (%.1f%% of the batch's pixels inside a rectangle):" % (p, 100 * share[p]))
        med = {}
        for name, _ in stages:
            ts = times[(name, p)]
            med[name[0]] = statistics.median(ts)
            q = statistics.quantiles(ts, n=4)
            out.append("  %-52s %7.3f ms (min %.3f, quartiles %.3f .. %.3f, max %.3f)" % (name, med[name[0]], min(ts), q[0], q[2], max(ts)))
        out.append("  e - u = %+.3f ms (e / u = %.2f);  3 - e = %+.3f ms (3 / e = %.2f)" % (
            med["e"] - med["u"], med["e"] / med["u"], med["3"] - med["e"], med["3"] / med["e"]))
    # The lines above start every stage on an idle device, so whatever the host does before a stage's first launch is inside its time
    # (e checks and marshals the table before its only launch; 3 does the same behind its first kernel).  A training loop keeps the
    # device busy, so the second figure is the device's: 40 calls of a line queued back to back between two events, no replay.
    out.append("the same lines queued back to back (40 calls between two events, no replay: the caches stay warm, the host's work is "
               "hidden behind the device's); median of 7 such runs, ms per call:")
    for p in probs:
        ea = K.erase_args(tables[p], "pixel", seed, 0, dev)
        per = {}
        for name, fn in stages:
            runs = []
            for _ in range(7):
                fn(p, ea)
                torch.cuda.synchronize()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                for _ in range(40):
                    fn(p, ea)
                ev[1].record()
                torch.cuda.synchronize()
                runs.append(ev[0].elapsed_time(ev[1]) / 40)
            per[name[0]] = (statistics.median(runs), min(runs), max(runs))
        out.append("  probability %.2f: " % p + ";  ".join("%s %.4f (min %.4f max %.4f)" % ((k,) + per[k]) for k in "ue3")
                   + ";  e - u = %+.4f, 3 - e = %+.4f" % (per["e"][0] - per["u"][0], per["3"][0] - per["e"][0]))
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
