"""What gradient-norm clipping costs inside the captured train step, on bench.py's default workload (sr_tiny supernet, B = 128, two
architecture groups of 64, bf16, hipGraph replay) and by bench.py's protocol (warm-up, then timed replays closed by ONE synchronise).

Timed in one process, alternating, --rounds times each:
  a       AdamW inside the graph, no clipping                                  (what bench.py times)
  b       AdamW inside the graph with optimizer.max_norm set and active        (early sums of squares beside the backward)
  b_late  the same with opt_overlap=0: one full-width sum of squares after the backward
  c       the only way to clip without it: graph without optimizer, torch.nn.utils.clip_grad_norm_, optimizer.step()

    python tools/clip_bench.py [--steps 40] [--warmup 10] [--rounds 3] [--out FILE]

Prints one JSON line per round and a summary line; exits non-zero if b is not faster than c in every round."""
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


class Variant:
    def __init__(self, name, device, in_graph, clip, overlap=1, torch_clip=False):
        from vitres import engine
        from vitres.losses import SoftTargetCrossEntropy
        from vitres.optim import FlatAdamW
        self.name, self.torch_clip = name, torch_clip
        w = bench.WORKLOADS["sr_tiny_supernet"]
        self.B = w["batch"]
        torch.manual_seed(0)
        self.model, _ = bench.build_model("sr_tiny_supernet", torch.bfloat16, device)
        self.x, self.t, self.pt = bench.synthetic_batch(self.B, device, 1000)
        self.model.train()
        self.model.set_epoch(31)
        self.model._ensure_arena(device)
        self.opt = FlatAdamW(self.model, engine.param_groups_weight_decay(self.model, 0.05), lr=5e-4 * self.B / 512.0,
                             max_norm=float("inf") if clip and not torch_clip else None)
        self.opt.own_shadow()
        self.max_norm = None
        self.graphed = engine.GraphedTrainStep(self.model, SoftTargetCrossEntropy(), self.x, self.t, self.pt, "seq",
                                               optimizer=self.opt if in_graph else None, opt_overlap=overlap)
        self.i = 0

    def step(self):
        torch.randperm(self.B // 2)                                # (bench.py: SwitchTokenMix's draws from the CPU generator)
        torch.randperm(self.B - self.B // 2)
        i, self.i = self.i, self.i + 1
        if self.graphed.optimizer is not None:
            self.opt.prepare_step()
            return self.graphed(self.x, self.t, self.pt, epoch=31, train_iter=i, arch_sample="multi")
        loss = self.graphed(self.x, self.t, self.pt, epoch=31, train_iter=i, arch_sample="multi")
        if self.torch_clip:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_norm)
        self.opt.step()
        return loss

    def timed(self, warmup, steps):
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    vs = [Variant("a", device, True, False), Variant("b", device, True, True), Variant("b_late", device, True, True, overlap=0),
          Variant("c", device, False, True, torch_clip=True)]
    # an ACTIVE clip: measure the norm over a few steps (max_norm = inf), then clip at half of the last one
    b = vs[1]
    for _ in range(5):
        b.step()
    norm = float(b.opt.grad_norm())
    max_norm = 0.5 * norm
    for v in vs[1:]:
        v.max_norm = max_norm
        if not v.torch_clip:
            v.opt.max_norm = max_norm
    lines = [json.dumps({"workload": "sr_tiny_supernet", "batch": b.B, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup,
                         "grad_norm_before": round(norm, 4), "max_norm": round(max_norm, 4),
                         "arena_MB": round(b.model._arena["flat"].numel() * 4 / 1e6, 1)})]
    print(lines[-1], flush=True)
    ok = True
    rounds = []
    for r in range(args.rounds):
        ms = {v.name: round(v.timed(args.warmup, args.steps), 4) for v in vs}
        coef = float(b.opt._clip["state"][3])
        ms.update(round=r, b_minus_a=round(ms["b"] - ms["a"], 4), b_late_minus_a=round(ms["b_late"] - ms["a"], 4),
                  c_minus_b=round(ms["c"] - ms["b"], 4), last_coef_b=round(coef, 4), last_norm_b=round(float(b.opt.grad_norm()), 4))
        ok = ok and ms["b"] < ms["c"]
        rounds.append(ms)
        lines.append(json.dumps(ms))
        print(lines[-1], flush=True)
    med = lambda k: sorted(r[k] for r in rounds)[len(rounds) // 2]      # noqa: E731
    lines.append(json.dumps({"median_ms": {k: med(k) for k in ("a", "b", "b_late", "c")}, "b_faster_than_c_in_every_round": ok,
                             "skipped_steps_b": b.opt.skipped_steps()}))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
