"""What the public epoch loops cost around the captured step, on bench.py's default workload (sr_tiny supernet, B = 128, bf16, two
architecture groups of 64, epoch 31) with a list loader of device-resident batches, and by bench.py's protocol (warm-up, then timed
steps closed by ONE synchronise).

Timed in one process, alternating, --rounds times each, --steps steps per round:
  eager    engine.train_one_epoch(fast=None)         the autograd loop: train_step, ~600 launches issued from Python per step
  fast     engine.train_one_epoch(fast=FastPath())   the same loop on the captured step
  hand     engine.GraphedTrainStep driven by hand, as INTEGRATION section 2 shows it (what bench.py times)
  hand_copy  the same, given the loader's tensors: the target copies into the static buffers happen, as in `fast` (hand_copy - hand
             is what those copies cost as launches in the stream, not as bytes; fast - hand_copy what the epoch loop itself adds)
Every variant has its own model and FlatAdamW, sees the same batches and draws SwitchTokenMix's two permutations per step.  The epoch
loops read their losses back once per epoch (sync_every = steps), as `hand` does; --sync-every 1 is the reference's per-step read.

`allowance` is what the loop adds per step outside the graph, from bytes: the soft targets and patch targets (and, where the patch
gather does not read the caller's batch directly, the images) are copied into the step's static buffers -- `hand` is given the
captured tensors themselves and skips those copies -- at the device-to-device copy rate this run measures on the same tensors; plus
the spread `hand` shows between its own rounds.

The same tool times engine.evaluate with device_meters on and off (ref_tiny, bf16, 16 batches of 256).

    python tools/epoch_loop_bench.py [--steps 40] [--warmup 10] [--rounds 3] [--sync-every 0] [--out FILE]

Prints one JSON line per round and a summary line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-search_amd"))

import torch  # noqa: E402

import bench  # noqa: E402

QUIET = type("Quiet", (), {"info": staticmethod(lambda s: None)})


class Train:
    def __init__(self, device, kind, data):
        from vitres import engine
        from vitres.losses import SoftTargetCrossEntropy
        from vitres.optim import FlatAdamW
        self.engine, self.kind, self.data, self.device = engine, kind, data, device
        self.B = data[0][0].shape[0]
        torch.manual_seed(0)
        self.model, _ = bench.build_model("sr_tiny_supernet", torch.bfloat16, device)
        self.model.train()
        self.model.set_epoch(31)
        self.crit = SoftTargetCrossEntropy()
        self.opt = FlatAdamW(self.model, engine.param_groups_weight_decay(self.model, 0.05), lr=5e-4 * self.B / 512.0)
        self.fast = engine.FastPath() if kind == "fast" else None
        self.patch = {t.data_ptr(): pt for _, t, pt in data}
        self.graphed, self.i = None, 0
        if kind.startswith("hand"):
            self.model._ensure_arena(device)
            self.opt.own_shadow()
            self.graphed = engine.GraphedTrainStep(self.model, self.crit, *data[0], "seq", optimizer=self.opt)

    def mix(self, x, t):
        torch.randperm(self.B // 2)                                # (bench.py: SwitchTokenMix's draws from the CPU generator)
        torch.randperm(self.B - self.B // 2)
        return x, t, self.patch[t.data_ptr()], "seq"

    def run(self, steps, sync_every):
        """`steps` steps; returns the losses' device tensors or the epoch's stats (both synchronise at most at their end)."""
        if self.kind.startswith("hand"):
            g = self.graphed
            for _ in range(steps):
                torch.randperm(self.B // 2)
                torch.randperm(self.B - self.B // 2)
                self.opt.prepare_step()
                x, t, pt = (g.x, g.t, g.pt) if self.kind == "hand" else self.data[self.i % len(self.data)]
                g(x, t, pt, epoch=31, train_iter=self.i, arch_sample="multi")
                self.i += 1
            return
        loader = [self.data[i % len(self.data)][:2] for i in range(steps)]
        self.engine.train_one_epoch(self.model, self.crit, loader, self.opt, self.device, 31, patch_mixup_fn=self.mix, print_freq=0,
                                    logger=QUIET, arch_sample="multi", sync_every=sync_every or steps, fast=self.fast)

    def timed(self, warmup, steps, sync_every):
        self.run(warmup, sync_every)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(steps, sync_every)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / steps * 1e3, 4)


def copy_rate(tensors, reps=20):
    """Device-to-device copy rate (GB/s of bytes written) on the tensors the step copies."""
    dst = [torch.empty_like(v) for v in tensors]
    for d, s in zip(dst, tensors):
        d.copy_(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for d, s in zip(dst, tensors):
            d.copy_(s, non_blocking=True)
    torch.cuda.synchronize()
    return sum(v.numel() * v.element_size() for v in tensors) * reps / (time.perf_counter() - t0) / 1e9


def time_evaluate(device, rounds, batches=16, val_bs=256):
    from vitres import engine
    torch.manual_seed(0)
    model, _ = bench.build_model("ref_tiny", torch.bfloat16, device)
    g = torch.Generator().manual_seed(1)
    data = [(torch.randn(val_bs, 3, 224, 224, generator=g).to(device), torch.randint(0, 1000, (val_bs,), generator=g).to(device))
            for _ in range(2)]
    loader = [data[i % 2] for i in range(batches)]
    out = []
    for r in range(rounds + 1):                                    # (round 0 warms up and is dropped)
        ms = {}
        for name, flag in (("device_meters_on", True), ("device_meters_off", False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = engine.evaluate(loader, model, device, logger=QUIET, device_meters=flag)
            torch.cuda.synchronize()
            ms[name] = round((time.perf_counter() - t0) / batches * 1e3, 4)
            ms[name + "_acc1"] = stats["acc1"]
        if r:
            out.append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sync-every", type=int, default=0, help="0: once per epoch")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B = bench.WORKLOADS["sr_tiny_supernet"]["batch"]
    data = [bench.synthetic_batch(B, device, 1000 + i) for i in range(4)]
    kinds = ("eager", "fast", "hand", "hand_copy")
    vs = {kind: Train(device, kind, data) for kind in kinds}
    lines = [json.dumps({"workload": "sr_tiny_supernet", "batch": B, "dtype": "bf16", "example_per_arch": 64, "epoch": 31,
                         "steps": args.steps, "warmup": args.warmup, "sync_every": args.sync_every or args.steps})]
    print(lines[-1], flush=True)
    rounds = []
    for r in range(args.rounds):
        ms = {"round": r}
        for kind in kinds:
            ms[kind] = vs[kind].timed(args.warmup, args.steps, args.sync_every)
        rounds.append(ms)
        lines.append(json.dumps(ms))
        print(lines[-1], flush=True)
    step = vs["fast"].fast.steps[0]
    copied = [data[0][1], data[0][2]] + ([] if step.col_static is not None else [data[0][0]])
    rate = copy_rate(copied)
    nbytes = sum(v.numel() * v.element_size() for v in copied)
    med = lambda key: sorted(r[key] for r in rounds)[len(rounds) // 2]      # noqa: E731
    spread = round(max(r["hand"] for r in rounds) - min(r["hand"] for r in rounds), 4)
    allowance = round(nbytes / rate / 1e6 + spread, 4)
    lines.append(json.dumps({"median_ms": {k: med(k) for k in kinds}, "fast_minus_hand_ms": round(med("fast") - med("hand"), 4),
                             "hand_copy_minus_hand_ms": round(med("hand_copy") - med("hand"), 4),
                             "fast_minus_hand_copy_ms": round(med("fast") - med("hand_copy"), 4),
                             "copied_bytes_per_step": nbytes, "copy_rate_GBps": round(rate, 1), "hand_spread_ms": spread,
                             "allowance_ms": allowance, "within_allowance": med("fast") - med("hand") <= allowance,
                             "captured_steps": len(vs["fast"].fast.steps)}))
    print(lines[-1], flush=True)
    ev = time_evaluate(device, args.rounds)
    emed = lambda key: sorted(r[key] for r in ev)[len(ev) // 2]             # noqa: E731
    lines.append(json.dumps({"evaluate": {"workload": "ref_tiny", "batch": 256, "batches": 16, "dtype": "bf16", "rounds": ev,
                                          "median_ms_per_batch": {k: emed(k) for k in ("device_meters_on", "device_meters_off")}}}))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
