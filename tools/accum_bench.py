"""What a micro-step of gradient accumulation costs inside the captured train step, on bench.py's default workload (sr_tiny supernet,
B = 128, two architecture groups of 64, bf16, hipGraph replay, AdamW inside the graph) and by bench.py's protocol (warm-up, then timed
replays closed by ONE synchronise).

Timed in one process, alternating, --rounds times each, with max_norm off and on (measure only: float("inf")):
  step     accum_steps = 1: the step as it was before accumulation existed (what bench.py times)
  cycle    accum_steps = k: replays in their natural order, ms per micro-step averaged over whole windows
  first    the same graph with every replay played as micro-step 0      (clears the arena, no update)
  middle   ... as a micro-step that is neither first nor last            (adds, no update)
  final    ... as micro-step k - 1                                        (adds, norm / clip / AdamW / EMA / shadow)
The forced positions replay ONE captured graph of their own: only the two control words and the hyper-parameter block differ, which
is all that differs between the micro-steps of a real window.  A run of forced `final` replays never clears the arena, so that model
is stepped with lr = 0 (the same launches and traffic; the parameters stay put instead of following an ever-growing sum), and the
summary reports every optimizer's skipped_steps(): a skipped update would be a cheaper one, all must be 0.

    python tools/accum_bench.py [--k 4] [--steps 40] [--warmup 10] [--rounds 3] [--out FILE]

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


class Variant:
    def __init__(self, device, k, clip, lr_scale=1.0):
        from vitres import engine
        from vitres.losses import SoftTargetCrossEntropy
        from vitres.optim import FlatAdamW
        w = bench.WORKLOADS["sr_tiny_supernet"]
        self.B, self.k = w["batch"], k
        torch.manual_seed(0)
        self.model, _ = bench.build_model("sr_tiny_supernet", torch.bfloat16, device)
        self.x, self.t, self.pt = bench.synthetic_batch(self.B, device, 1000)
        self.model.train()
        self.model.set_epoch(31)
        self.model._ensure_arena(device)
        self.opt = FlatAdamW(self.model, engine.param_groups_weight_decay(self.model, 0.05), lr=lr_scale * 5e-4 * self.B * k / 512.0,
                             max_norm=float("inf") if clip else None)
        self.opt.own_shadow()
        kw = {"accum_steps": k} if k > 1 else {}
        self.graphed = engine.GraphedTrainStep(self.model, SoftTargetCrossEntropy(), self.x, self.t, self.pt, "seq",
                                               optimizer=self.opt, **kw)
        self.i = 0

    def step(self, position=None):
        """position: None = the window's natural order; otherwise the micro-step every replay is played as."""
        torch.randperm(self.B // 2)                                # (bench.py: SwitchTokenMix's draws from the CPU generator)
        torch.randperm(self.B - self.B // 2)
        g = self.graphed
        if position is not None:
            g.micro_step = position
        i, self.i = self.i, self.i + 1
        self.opt.prepare_step(apply=(g.micro_step == self.k - 1))
        return g(self.x, self.t, self.pt, epoch=31, train_iter=i // self.k, arch_sample="multi")

    def timed(self, warmup, steps, position=None):
        self.graphed.micro_step = 0
        for _ in range(warmup):
            self.step(position)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(position)
        torch.cuda.synchronize()
        self.graphed.micro_step = 0
        return round((time.perf_counter() - t0) / steps * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.k < 3 or args.steps % args.k:
        ap.error("--k must be >= 3 (a window with a first, a middle and a final micro-step) and divide --steps")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    k = args.k
    vs = {("step", clip): Variant(device, 1, clip) for clip in (False, True)}
    vs.update({("accum", clip): Variant(device, k, clip) for clip in (False, True)})
    vs.update({("forced", clip): Variant(device, k, clip, lr_scale=0.0) for clip in (False, True)})
    warm = (args.warmup + k - 1) // k * k                          # whole windows: the timed part starts at micro-step 0
    lines = [json.dumps({"workload": "sr_tiny_supernet", "batch": vs[("step", False)].B, "dtype": "bf16", "accum_steps": k,
                         "steps": args.steps, "warmup": warm,
                         "arena_MB": round(vs[("step", False)].model._arena["flat"].numel() * 4 / 1e6, 1)})]
    print(lines[-1], flush=True)
    rounds = []
    for r in range(args.rounds):
        ms = {"round": r}
        for clip in (False, True):
            tag = "clip" if clip else "plain"
            a, b, f = vs[("step", clip)], vs[("accum", clip)], vs[("forced", clip)]
            ms[tag] = {"step": a.timed(warm, args.steps), "cycle": b.timed(warm, args.steps),
                       "first": f.timed(warm, args.steps, 0), "middle": f.timed(warm, args.steps, 1),
                       "final": f.timed(warm, args.steps, k - 1)}
            ms[tag]["middle_minus_step"] = round(ms[tag]["middle"] - ms[tag]["step"], 4)
            ms[tag]["final_minus_step"] = round(ms[tag]["final"] - ms[tag]["step"], 4)
        rounds.append(ms)
        lines.append(json.dumps(ms))
        print(lines[-1], flush=True)
    med = lambda tag, key: sorted(r[tag][key] for r in rounds)[len(rounds) // 2]      # noqa: E731
    keys = ("step", "cycle", "first", "middle", "final")
    lines.append(json.dumps({"median_ms": {tag: {key: med(tag, key) for key in keys} for tag in ("plain", "clip")},
                             "skipped_steps": {n: v.opt.skipped_steps() for (n, c), v in vs.items() if c},
                             "last_grad_norm": {n: round(float(v.opt.grad_norm()), 4) for (n, c), v in vs.items() if c}}))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
