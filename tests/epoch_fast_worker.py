"""Worker of tests/test_gpu_epoch_fast.py::test_two_ranks_*: one rank of a 2-rank job (torch.distributed.run) on the GPU.  The same
two updates (four micro-batches, accum_steps 2, max_norm 1.0, bf16) run through engine.train_one_epoch with a GradSync twice from
the same state -- the eager loop and fast=FastPath() -- on per-rank data.  Rank 0 prints what the test asserts."""
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "vit-search_amd"), HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import recipe  # noqa: E402
import vitres  # noqa: E402
from vitres import engine  # noqa: E402
from vitres.losses import SoftTargetCrossEntropy  # noqa: E402
from vitres.optim import FlatAdamW  # noqa: E402

QUIET = type("L", (), {"info": staticmethod(lambda s: None)})


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-6))


def main():
    backend = os.environ.get("VITRES_DIST_BACKEND", "nccl")
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    dev = torch.device("cuda", local if torch.cuda.device_count() > local else 0)     # gloo run: both ranks share GPU 0
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    data = []
    for i in range(4):
        x, t, pt, _ = recipe.inputs(600 + 10 * i + rank, 8, recipe.MICRO_IMG, recipe.MICRO_CLASSES, 1)
        data.append((x.to(dev), t.to(dev), pt.to(dev)))
    patch = {t.data_ptr(): pt for _, t, pt in data}

    def mix(x, t):
        torch.rand(3)
        return x, t, patch[t.data_ptr()], "seq"
    crit = SoftTargetCrossEntropy()
    runs = []
    for use_fast in (False, True):
        torch.manual_seed(100)                                    # same weights and draws in both runs (and on both ranks)
        model = vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                                    num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0,
                                    num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
        model = model.to(dev).set_compute_dtype(torch.bfloat16)
        model.train()
        model.set_epoch(31)
        sync = engine.GradSync(model)
        sync.broadcast_parameters()
        opt = FlatAdamW(model, engine.param_groups_weight_decay(model, 0.05), lr=2e-3, ema_decay=0.9)
        fp = engine.FastPath() if use_fast else None
        torch.manual_seed(900 + 17 * rank)                        # different sub-networks per rank
        stats = engine.train_one_epoch(model, crit, [(x, t) for x, t, _ in data], opt, dev, 31, max_norm=1.0, patch_mixup_fn=mix,
                                       print_freq=0, logger=QUIET, arch_sample="multi", grad_sync=sync, accum_steps=2, fast=fp)
        torch.cuda.synchronize()
        a = model._arena
        runs.append({"stats": stats, "flat": a["flat"].clone(), "ema": opt._flat_state["ema"].clone(), "steps": opt._step,
                     "norm": float(opt.grad_norm()), "skipped": opt.skipped_steps(), "grad_scale": opt.grad_scale,
                     "shadow_in_step": bool(torch.equal(a["shadow"].float(), a["flat"].bfloat16().float())) if use_fast else None,
                     "split": None if fp is None else (len(fp.steps), fp.steps[0].optimizer is None, len(fp.steps[0].more_graphs),
                                                       fp.steps[0].micro_step)})
    e, f = runs
    mine = torch.stack([f["flat"].double().sum(), f["flat"].double().abs().sum()])
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    out = {"backend": dist.get_backend(), "world": dist.get_world_size(), "steps": [e["steps"], f["steps"]],
           "loss": [e["stats"]["loss"], f["stats"]["loss"]], "lr": [e["stats"]["lr"], f["stats"]["lr"]],
           "norm": [e["norm"], f["norm"]], "skipped": [e["skipped"], f["skipped"]], "grad_scale_after": f["grad_scale"],
           "param_rel": rel(f["flat"], e["flat"]), "ema_rel": rel(f["ema"], e["ema"]), "shadow_in_step": f["shadow_in_step"],
           "split": f["split"], "ranks_agree": all(torch.equal(both[0], o) for o in both[1:]),
           "moved": not torch.equal(f["flat"], f["ema"])}
    if rank == 0:
        print("FAST " + json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
