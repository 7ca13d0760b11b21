"""Train / eval loops: the build's counterpart of reference engine.py (train_one_epoch :57-190,
evaluate :194-261), same call signature and per-iteration protocol:

  (patch-)mixup -> save CPU RNG -> [manual_seed(epoch*10000+iter) if single/hybrid] -> forward ->
  loss = CE(cls) + CE(patch) -> restore CPU RNG -> finite check -> zero_grad -> backward (+ gradient
  exchange over RCCL) -> optimizer step -> meters.

Differences, all deliberate: bf16 compute needs no GradScaler (loss_scaler may be None); gradients of all
ranks are averaged by one flat all-reduce (GradSync) instead of DDP buckets; the non-finite-loss check is
done on the device and read back every `sync_every` iterations (reference: every iteration).
"""
import contextlib
import functools
import math
import sys
import time
from collections import defaultdict

import torch
import torch.distributed as dist

from . import functional as Fn, kernels as K, stem
from .losses import SoftTargetCrossEntropy
from .mixup import Mixup
from .optim import FlatAdamW, _check_accum_steps
from .token_mixup import SwitchTokenMix


def is_dist():
    return dist.is_available() and dist.is_initialized()


def world_size():
    return dist.get_world_size() if is_dist() else 1


class Meter:
    """Running sum / count with cross-process reduction (reference utils.SmoothedValue :24-88)."""

    def __init__(self):
        self.total, self.count = 0.0, 0

    def update(self, value, n=1):
        self.total += float(value) * n
        self.count += n

    def synchronize_between_processes(self):
        if not is_dist():
            return
        dev = 'cuda' if dist.get_backend() == 'nccl' else 'cpu'
        t = torch.tensor([self.count, self.total], dtype=torch.float64, device=dev)
        dist.barrier()
        dist.all_reduce(t)
        t = t.tolist()
        self.count, self.total = int(t[0]), t[1]

    @property
    def global_avg(self):
        return self.total / max(self.count, 1)


class _WireWork:
    """Handle of an all-reduce that ran on the wire buffer: the work + the arena range GradSync.finish() copies back."""
    __slots__ = ("work", "lo", "hi")

    def __init__(self, work, lo, hi):
        self.work, self.lo, self.hi = work, lo, hi

    def wait(self):
        return self.work.wait()


class GradSync:
    """Data-parallel gradient exchange for a vitres model: parameters are broadcast once from rank 0
    (reference DDP constructor, main.py:367) and, every step, the flat gradient arena is all-reduced
    (sum) and scaled by 1/world -- one RCCL call over xGMI instead of DDP's 25 MB buckets."""

    def __init__(self, model, wire_dtype=torch.float32):
        """wire_dtype=torch.bfloat16: the gradients cross xGMI as bf16 -- half the bytes of the exchange the ring pays per link
        (279 MB of fp32 per step for sr_tiny).  Every range is rounded to bf16 into a persistent wire buffer,
        all-reduced there (RCCL sums bf16 in bf16: each of the world - 1 additions rounds once more) and written back to the fp32
        arena by finish(); AdamW's moments and the master weights stay fp32.  Error of an averaged gradient element against the
        fp32 exchange: at most world bf16 roundings (unit roundoff 2^-8) of the operands' mean magnitude; tests/test_dist_gloo.py
        pins it at world 2: every element within 2 * 2^-8 * mean(|g_rank|), the whole arena within 2^-8 in the L2 norm.
        The default stays fp32 -- the reference's DDP reduces fp32 gradients (main.py:366-367)."""
        self.model = model
        self.world = world_size()
        self.wire_dtype = wire_dtype
        self._wire = None
        self._warned = False

    def broadcast_parameters(self):
        if self.world == 1:
            return
        arena = self.model._arena
        if arena is not None:
            dist.broadcast(arena["flat"], src=0)
        else:
            for p in self.model.parameters():
                dist.broadcast(p.data, src=0)
        for b in self.model.buffers():
            dist.broadcast(b, src=0)
        if hasattr(self.model, "invalidate_shadow"):
            self.model.invalidate_shadow()          # ranks > 0 just received new fp32 weights: re-cast a bf16 shadow kept by FlatAdamW

    def broadcast_buffers(self):
        """DDP's `broadcast_buffers=True` default (reference main.py:367): before every forward rank 0's buffers --
        here the BatchNorm running statistics of the convolutional patch embedding, the only buffers of the model -- overwrite
        the other ranks'.  A no-op for buffer-free models (type-0 patch embedding) and on one rank."""
        if self.world == 1:
            return
        bufs = [b for b in self.model.buffers() if b.numel()]
        if not bufs:
            return
        fl = [b for b in bufs if b.is_floating_point()]
        if fl:
            flat = torch.cat([b.reshape(-1).float() for b in fl])
            dist.broadcast(flat, src=0)
            off = 0
            for b in fl:
                b.copy_(flat[off:off + b.numel()].view(b.shape))
                off += b.numel()
        for b in bufs:
            if not b.is_floating_point():
                dist.broadcast(b, src=0)

    def all_reduce_range(self, lo, hi):
        """Asynchronous all-reduce (sum) of elements [lo, hi) of the flat gradient arena; returns the work handle (None
        on one rank).  RCCL runs it on the process group's stream after everything queued so far on the current one."""
        if self.world == 1 or hi <= lo:
            return None
        g = self.model._arena["gcur"]
        if self.wire_dtype == torch.float32:
            return dist.all_reduce(g[lo:hi], async_op=True)
        wire = self._wire_buffer(g)
        self._to_wire(g[lo:hi], wire[lo:hi])
        # the range travels WITH its handle: finish() copies back exactly the ranges whose handles it was given (a handle dropped
        # by an exception, or waited on by the caller, leaves nothing behind that a later finish() could copy over valid gradients)
        return _WireWork(dist.all_reduce(wire[lo:hi], async_op=True), lo, hi)

    def _wire_buffer(self, g):
        if self._wire is None or self._wire.numel() != g.numel() or self._wire.device != g.device:
            self._wire = torch.empty(g.numel(), dtype=self.wire_dtype, device=g.device)
        return self._wire

    @staticmethod
    def _to_wire(src, dst):
        if src.is_cuda and dst.dtype == torch.bfloat16:
            K.cast_bf16(src, dst)              # vr_cast_f32_bf16: round-to-nearest-even, 16-byte accesses
        else:
            dst.copy_(src)

    def finish(self, works, average=True):
        """Wait for all_reduce_range handles and apply the 1/world averaging (average=False leaves the SUM: an optimizer
        that scales gradients itself -- vitres.optim.FlatAdamW.grad_scale -- saves the extra pass over the arena).  The ranges of
        `works` must cover every gradient the optimizer consumes (bf16 wire: only the exchanged ranges are copied back / averaged)."""
        if self.world == 1:
            return
        works = list(works)                    # (a generator would be exhausted by the waits below)
        for w in works:
            if w is not None:
                w.wait()
        g = self.model._arena["gcur"]
        wired = [w for w in works if isinstance(w, _WireWork)]
        if wired:                              # bf16 wire: summed ranges back into the fp32 arena (averaging folded in)
            if len(wired) != sum(1 for w in works if w is not None):
                raise RuntimeError("GradSync.finish: fp32 and wire-dtype handles mixed in one exchange")
            for w in wired:
                g[w.lo:w.hi].copy_(self._wire[w.lo:w.hi])
                if average:
                    g[w.lo:w.hi].mul_(1.0 / self.world)
            return
        if average:
            g.mul_(1.0 / self.world)

    def all_reduce_grads(self, average=True):
        if self.world == 1:
            return
        a = self.model._arena
        g = a.get("gcur") if a is not None else None
        p0 = a["params"][0] if a is not None else None
        if g is not None and p0.grad is not None and p0.grad.data_ptr() == g.data_ptr() + 4 * a["offsets"][0][0]:
            if self.wire_dtype != torch.float32:
                return self.finish([self.all_reduce_range(0, g.numel())], average=average)
            dist.all_reduce(g)                                    # .grad tensors are views of the flat arena
            if average:
                g.mul_(1.0 / self.world)
            return
        if self.wire_dtype != torch.float32 and not self._warned:
            import warnings
            warnings.warn("GradSync: gradients are not views of the flat arena (autograd cloned them): the per-tensor fallback "
                          "exchanges fp32, wire_dtype=%s is ignored" % self.wire_dtype)
            self._warned = True
        for p in self.model.parameters():                         # autograd cloned the views: per-tensor fallback
            if p.grad is not None:
                dist.all_reduce(p.grad)
                if average:
                    p.grad.mul_(1.0 / self.world)


class KnowledgeDistillationLoss(torch.nn.Module):
    """Distillation term on the distillation token's logits (reference engine.py:25-46): hard = cross entropy against the
    teacher's arg-max class; soft = T^2 * mean_b sum_k -softmax(teacher / T) * log_softmax(x / T) with T = soft_temperature."""

    def __init__(self, hard_distill=True, soft_temperature=3.0):
        super().__init__()
        self.hard_distill = hard_distill
        self.soft_temperature = None if hard_distill else float(soft_temperature)

    def forward(self, x, teacher_output):
        if self.hard_distill:
            return torch.nn.functional.cross_entropy(x, torch.argmax(teacher_output, dim=1))
        t = self.soft_temperature
        soft = torch.softmax(teacher_output / t, dim=1)
        return torch.mean(torch.sum(-soft * torch.log_softmax(x / t, dim=1), 1)) * (t * t)

    def extra_repr(self):
        return 'hard_distill={}'.format(self.hard_distill) + ('' if self.hard_distill else
                                                              ', soft_temperature={}'.format(self.soft_temperature))


@contextlib.contextmanager
def _arch_seed(arch_sample, epoch, train_iter):
    """The reference's `arch_sample` seed rule around a forward (engine.py:119-131, 164-165); the CPU RNG state is back on exit."""
    if arch_sample is None:
        yield
        return
    rng = torch.random.get_rng_state()
    if arch_sample in ('single', 'hybrid'):
        torch.manual_seed(epoch * 10000 + train_iter)
    elif arch_sample != 'multi':
        raise ValueError('arch_sample has invalid value {}.'.format(arch_sample))
    try:
        yield
    finally:
        torch.random.set_rng_state(rng)


def _patch_loss(criterion, cls_pred, patch_pred, targets, patch_targets, patch_output_type):
    """criterion(cls) + criterion(patch): per token against the patch targets ('seq') or of the mean token against the targets ('avg')."""
    if patch_output_type not in ('seq', 'avg'):
        raise ValueError()
    return criterion(cls_pred, targets) + criterion(patch_pred, patch_targets if patch_output_type == 'seq' else targets)


def train_step(model, criterion, optimizer, samples, targets, patch_targets=None, patch_output_type=None, epoch=0,
               train_iter=0, arch_sample=None, grad_sync=None, loss_scaler=None, max_norm=None, average_grads=True,
               teacher_output=None, kd_criterion=None, alpha=0.5, accum_steps=1, micro_step=0):
    """One optimisation step -- or, with accum_steps = k > 1, micro-step `micro_step` (0..k-1) of an update window: micro-step 0 clears
    the gradients, every micro-step adds its own, only micro-step k-1 exchanges, clips and steps the optimizer, on the MEAN over the
    window (a vitres.optim.FlatAdamW divides by its accum_steps attribute, which is set here; for any other optimizer the loss is
    divided by k before backward).  train_iter is the index of the optimizer UPDATE: all micro-steps of a window share the
    'single' / 'hybrid' seed, as all ranks of one reference iteration do.
    Returns this micro-batch's own (undivided) loss tensor (on device, not synchronised).  average_grads=False leaves the
    all-reduced SUM in the arena (optimizer applies 1/world: vitres.optim.FlatAdamW.grad_scale).  teacher_output +
    kd_criterion: knowledge distillation, loss = (1 - alpha) * criterion(cls) + alpha * kd(dst, teacher) (engine.py:135-148;
    a one-token model distils through its class logits, as the reference's `output_dst = outputs`).
    max_norm (reference: loss_scaler(..., clip_grad=max_norm), engine.py:178-180) without a loss_scaler: a vitres.optim.FlatAdamW
    clips on the device inside its own step (optimizer.max_norm is set to it: vr_grad_sumsq -> vr_clip_finish ->
    vr_adamw_flat_clip; optimizer.grad_norm() holds the norm afterwards); any other optimizer gets
    torch.nn.utils.clip_grad_norm_.  Either way after the all-reduce, so every rank clips the same averaged gradients."""
    accum_steps = _check_accum(accum_steps, micro_step)
    last = micro_step == accum_steps - 1
    with _arch_seed(arch_sample, epoch, train_iter):
        if patch_targets is None:
            outputs = model(samples)
            output_cls, output_dst = (outputs[0], outputs[1]) if isinstance(outputs, tuple) else (outputs, outputs)
            loss = criterion(output_cls, targets)
            if teacher_output is not None:
                loss = loss * (1 - alpha) + kd_criterion(output_dst, teacher_output) * alpha
        else:
            cls_pred, patch_pred = model(samples, patch_output_type=patch_output_type)
            loss = _patch_loss(criterion, cls_pred, patch_pred, targets, patch_targets, patch_output_type)
    if micro_step == 0:
        optimizer.zero_grad(set_to_none=True)
    if accum_steps > 1:
        flat_opt = hasattr(optimizer, "accum_steps")              # FlatAdamW averages inside its own pass
        if flat_opt:
            optimizer.accum_steps = accum_steps
        own_loss, loss = loss, (loss if flat_opt else loss / accum_steps)
        if not last:                                              # gradients only: autograd adds them to the window's sum
            scaler = getattr(loss_scaler, '_scaler', None)
            if loss_scaler is not None and scaler is None:
                raise RuntimeError('gradient accumulation with a loss_scaler needs a NativeScaler-like object exposing `_scaler`')
            (scaler.scale(loss) if scaler is not None else loss).backward()
            if micro_step > 0 and hasattr(model, "rebind_grad_arena"):
                model.rebind_grad_arena()
            return own_loss.detach()
    else:
        own_loss = loss
    if loss_scaler is not None and (grad_sync is None or grad_sync.world == 1):
        loss_scaler(loss, optimizer, clip_grad=max_norm, parameters=model.parameters(), create_graph=False)
    elif loss_scaler is not None:
        # timm NativeScaler does scale -> backward -> unscale -> clip -> step in one call; with a gradient exchange the
        # all-reduce has to sit between backward and unscale (DDP does it inside backward, main.py:367), so the call is unrolled
        scaler = getattr(loss_scaler, '_scaler', None)
        if scaler is None:
            raise RuntimeError('loss_scaler with grad_sync on several ranks needs a NativeScaler-like object exposing `_scaler` '
                               '(torch.cuda.amp.GradScaler); bf16 / fp32 training needs no scaler: pass loss_scaler=None')
        scaler.scale(loss).backward()
        grad_sync.all_reduce_grads(average=average_grads)
        scaler.unscale_(optimizer)
        if max_norm:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        scaler.step(optimizer)
        scaler.update()
    else:
        loss.backward()
        if micro_step > 0 and hasattr(model, "rebind_grad_arena"):
            model.rebind_grad_arena()                             # (autograd added this backward to the window's arena views)
        if grad_sync is not None:
            grad_sync.all_reduce_grads(average=average_grads)
        if max_norm and hasattr(optimizer, "clip_enabled"):       # FlatAdamW: one clipping path per optimizer type
            optimizer.max_norm = max_norm
        elif max_norm:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        optimizer.step()
    return own_loss.detach()


def _check_accum(accum_steps, micro_step=0):
    _check_accum_steps(accum_steps)
    if not 0 <= micro_step < accum_steps:
        raise ValueError("micro_step must lie in 0..accum_steps-1, got %r" % (micro_step,))
    return accum_steps


def _window(micro_step, accum_steps):
    """Bookkeeping of an update window: (clear the arena?, apply the update?, position of the next micro-step)."""
    return micro_step == 0, micro_step == accum_steps - 1, (micro_step + 1) % accum_steps


# bounded run-ahead: the host needs ~3 ms for a 7.5 ms step, so left alone it queues replay after replay until the runtime's
# queue limit stops it (~25 steps in); on the way the runtime grows its per-launch resources a few times, and each growth
# stalls the device for ~1 ms (six 8.3 - 8.9 ms steps among the first 26 of a run, none after).  RUN_AHEAD replays in
# flight keep the device fed with the host two steps ahead from the third step on.
RUN_AHEAD = 2


def _cuts(model, n):
    """The first n backward cuts of model.split_plan(parts >= 3) as a list (shorter when the layout has fewer); [] for none."""
    cuts = model.split_plan(parts=max(n + 1, 3)) if n >= 1 else None
    return cuts[:n] if cuts else []


@contextlib.contextmanager
def _rng_preserved(model):
    """The CPU generator and the model's private DropPath generator are, on exit, where they were on entry."""
    # the warm-up steps and the capture's plan must not advance the streams a checkpoint restored (the first replay then continues
    # exactly where the saved run stopped)
    rng, dp_rng = torch.random.get_rng_state(), model.drop_path_rng_state()
    try:
        yield
    finally:
        torch.random.set_rng_state(rng)
        model.set_drop_path_rng_state(dp_rng)


class _ReplayInputs:
    """The ONE static int32 device buffer through which what the host makes per replay reaches the graph, and its staging ring."""
    # buf = the keep rows of every ChannelDrop and the DropPath scale vectors (bit-cast floats) of the replay's plan
    # (model.plan_host_buffer) and, behind them when accum_steps > 1, the control words {clear, apply} of the update window: one
    # staging copy per replay serves both.  No plan words and no window: no buffer, no ring, upload() does nothing.
    # upload() goes through a ring of pinned staging blocks: the host runs several replays ahead of the device, a single block would
    # be overwritten before its copy has executed.  The copy is a small KERNEL reading the pinned block, not a memcpy: a
    # hipMemcpyAsync crosses to the copy engine and back, 28 against 15 us of GPU time per step.
    RING = 64

    def __init__(self, model, plan, accum_steps, device):
        flat, self.nk = model.plan_host_buffer(plan)
        self.n_plan = flat.size
        n = flat.size + (2 if accum_steps > 1 else 0)
        self.buf = self.plan = self.ctl = None
        self._ring, self._next = [], 0
        if not n:
            return
        self.buf = torch.ones(n, dtype=torch.int32, device=device)       # (the control words start as {1, 1})
        if flat.size:
            self.buf[:flat.size].copy_(torch.from_numpy(flat))
            self.plan = self.buf[:flat.size]
        if accum_steps > 1:
            self.ctl = self.buf[flat.size:]
        self._ring = [[torch.empty(n, dtype=torch.int32).pin_memory(), None] for _ in range(self.RING)]

    def upload(self, model, plan, first, last):
        """The words of `plan` and {clear, apply} = {first, last} -> the next staging block -> the device buffer (stream-ordered)."""
        if self.buf is None:
            return
        block = self._ring[self._next % self.RING]
        self._next += 1
        if block[1] is not None:
            block[1].synchronize()                                # the host runs ahead of the device: the block's last copy is done?
        host = block[0].numpy()
        if self.plan is not None:
            host[:self.n_plan] = model.plan_host_buffer(plan)[0]
        if self.ctl is not None:
            host[self.n_plan], host[self.n_plan + 1] = int(first), int(last)
        K.copy_i32_from_pinned(block[0], self.buf)
        block[1] = torch.cuda.current_stream().record_event()


class GraphedTrainStep:
    """forward + loss + backward of one iteration captured ONCE into a hipGraph and replayed every step
    (the step issues ~600 kernel launches; replay removes their host cost).  What changes between iterations goes
    through static device buffers: the batch, the soft targets, and the int32 keep rows of every ChannelDrop, which
    are still sampled on the host with the reference's RNG protocol before each replay, and the DropPath scale vectors, drawn
    from the model's private CPU generator (model.drop_path_generator(): seeded from torch.initial_seed() + rank, saved and
    restored with the checkpoint's RNG bundle).  The gradient exchange and the optimizer stay outside the graph.

    accum_steps = k > 1: gradient accumulation over k micro-batches per optimizer update with the SAME single graph.  Replay number
    `micro_step` (0..k-1, the position of the NEXT replay; checkpoints belong where it is 0) of a window clears the arena only when it
    is the first and runs the norm / clip / AdamW / EMA / shadow refresh only when it is the last: two int32 control words
    {clear, apply} in device memory, rewritten before each replay over the plan buffer's pinned-staging route, gate those launches
    (vr_zero_ranges_gated, vr_grad_sumsq_gated, vr_clip_finish_gated; AdamW reads the all-zero hyper-parameter block that
    optimizer.prepare_step(apply=False) uploads).  Every gradient writer adds in place; the optimizer divides by k."""

    def __init__(self, model, criterion, samples, targets, patch_targets=None, patch_output_type=None, warmup=2,
                 split_for_sync=False, optimizer=None, opt_overlap=1, opt_overlap_blocks=256, accum_steps=1):
        """split_for_sync: capture the backward as TWO graphs cut after the last stage (model.split_plan()), so that
        step_with_sync() can all-reduce the finished tail of the gradient arena (most of the parameters) while the rest
        of the backward -- most of the time -- is still running.
        opt_overlap / opt_overlap_blocks (with optimizer): number of arena ranges updated early, beside the rest of the backward,
        and the workgroup cap of those updates (see _capture_update).  With optimizer.max_norm set at capture no parameter may change
        before the whole gradient norm is known: the early launches then are the SUMS OF SQUARES of those ranges (same stream, ranges
        and cap), and the remaining range's sum, the finish and ONE full-width AdamW follow the backward.  The replays follow
        optimizer.max_norm from value to value (float("inf"): measure only); switching it on or off after the capture makes
        optimizer.prepare_step() raise.
        accum_steps: micro-batches per optimizer update (class docstring).  With optimizer= the caller calls
        optimizer.prepare_step(apply=(step.micro_step == accum_steps - 1)) before every replay."""
        self.accum_steps = _check_accum(accum_steps)
        self.micro_step = 0
        model._check_fp16_eval(True)              # (fp16 is an evaluation mode: nothing is captured or launched)
        self.model, self.criterion, self.pot = model, criterion, patch_output_type
        self.graph_b, self.split, self.more_graphs, self.ranges = None, None, [], []
        self._inflight = []
        self.exposed = None                  # bench.py: a list here collects (backward done, exchange done) event pairs
        # optimizer (a vitres.optim.FlatAdamW, single rank): the update becomes part of the graph (_capture_update).  Call
        # optimizer.prepare_step() before every replay instead of optimizer.step().
        self.optimizer = optimizer if (optimizer is not None and hasattr(optimizer, "step_device")) else None
        if self.optimizer is not None and split_for_sync:
            raise ValueError("optimizer-in-graph is for one rank; with a gradient exchange step the optimizer after step_with_sync")
        self.defer = None                    # (the deferred in-graph update is gone; bench.py still reads the attribute)
        if self.accum_steps > 1 and self.optimizer is not None:
            self.optimizer.accum_steps = self.accum_steps             # the update uses the window's mean
        # soft-target CE is the training loss of every shipped recipe (main.py:390-398): the whole step then runs without
        # autograd and without torch glue between the heads and the backward (model.loss_and_grad / vr_softce_train)
        self.fused_loss = isinstance(criterion, SoftTargetCrossEntropy) and hasattr(model, "loss_and_grad")
        self.x, self.t = samples.clone(), targets.clone()
        self.pt = patch_targets.clone() if patch_targets is not None else None
        with _rng_preserved(model):
            self._warm_up(warmup)
            plan = model.sample_plan(samples.shape[0])
            self._static_inputs(samples, plan)
            model.zero_grad(set_to_none=True)
            self.graph = torch.cuda.CUDAGraph()
            K.ensure_workspaces(samples.device, roles=(0, 1))         # stream-K workspaces exist before anything is captured
            self._loss_buf = torch.zeros(1, dtype=torch.float32, device=samples.device)
            clip = self.optimizer.prepare_capture() if self.optimizer is not None else False
            # the backward is cut for ONE of two reasons.  split_for_sync = number of backward parts (True = 2): part k's graph is
            # followed by the all-reduce of the arena range it completed, overlapping part k+1.  optimizer: opt_overlap ranges are
            # updated early, the parts follow one another in the same capture
            parts = 2 if split_for_sync is True else int(split_for_sync or 0)
            cuts = _cuts(model, opt_overlap if self.optimizer is not None else parts - 1)
            if cuts and self.optimizer is None:
                self.split = cuts[0]
            with model.backward_capture(split=[c for c, _ in cuts] or None, join_parts=not cuts or self.optimizer is None,
                                        clear_gate=None if self._ctl is None else self._ctl[0:1]):
                self._capture_step(plan, cuts, clip, opt_overlap_blocks)
                self._capture_rest(cuts)
        self.loss = self.loss.detach()

    def _warm_up(self, steps):
        """Eager steps on a side stream before the capture (arena, LDS attributes, allocator)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(steps):
                self.model.zero_grad(set_to_none=True)
                self._step_body(None)
        torch.cuda.current_stream().wait_stream(side)

    def _static_inputs(self, samples, plan):
        """The static device buffers the replays write besides x / t / pt: the plan + control words, the patchify operand."""
        self._inputs = _ReplayInputs(self.model, plan, self.accum_steps, samples.device)
        self.keep_static, self._ctl = self._inputs.plan, self._inputs.ctl             # (names kept: tests / tools look at them)
        self._ctl_all = self._inputs.buf if self._ctl is not None else None
        # for the type-0 patch embedding the patch gather runs in front of the graph, straight from the caller's batch (no copy of
        # the images into a static buffer, no re-ordering pass)
        model, self.col_static = self.model, None
        if model.embed_type == 0 and model.compute_dtype == torch.bfloat16:
            ldk = (model.in_chans * model.patch_size ** 2 + 7) // 8 * 8
            self.col_static = torch.empty((samples.shape[0] * model.patch_embed.num_patches, ldk), dtype=torch.bfloat16,
                                          device=samples.device)
            self._gather(samples, plan)

    def _capture_step(self, plan, cuts, clip, cap):
        """self.graph: forward + loss + the first backward part and, with an optimizer, the other parts and the update."""
        with torch.cuda.graph(self.graph):
            if self.keep_static is not None:
                self.model.attach_plan_buffer(plan, self.keep_static, self._inputs.nk)
            plan.embed_col = self.col_static
            self.loss = self._step_body(plan)
            if self.optimizer is not None:
                self._capture_update(cuts, clip, cap)

    def _capture_update(self, cuts, clip, cap):
        """The in-graph optimizer sequence, issued into the running capture behind the first backward part (clip: see __init__)."""
        # The arena tail (last stage + heads, most parameters) is updated on the side stream as soon as its gradients are final, beside
        # the rest of the backward; the remainder after it.  opt_overlap = len(cuts) = number of arena ranges updated EARLY (0 off, 1
        # (default): head + last stage, 2: + the stage before; measured round 4: 7.47 -> 7.36 - 7.39 ms with 1 or 2,
        # profiles/r04_optimizer_overlap.txt): the backward is cut in front of the spatial reductions (model.split_plan) and the range
        # a part completes is updated on the weight gradients' side stream -- IN ORDER with the groups there: a third branch would land
        # on their hardware queue in front of them (round 4) -- by at most `cap` = opt_overlap_blocks resident workgroups (256: one per
        # CU; the uncapped update took the chip and cost more than it hid in rounds 1 - 3), beside the rest of the backward; what is
        # left (the first stage + embedding) follows the backward at full width.
        opt, model = self.optimizer, self.model
        gate = None if self._ctl is None else self._ctl[1:2]       # `apply`, read at run time by the gated norm launches
        cap = cap if Fn.OVERLAP else 0
        hi = n_arena = model._arena["flat"].numel()
        if model._bwd_state is not None:
            for _, lo in cuts:                                     # ranges complete from the arena's end backwards
                if clip:                                           # (each range fills its own slice of the partial sums)
                    early = functools.partial(opt.norm_range_device, lo, hi, opt.reserve_norm_slice(lo, hi), max_blocks=cap,
                                              gate=gate)
                else:
                    early = functools.partial(opt.step_device, lo, hi, max_blocks=cap)
                if Fn.OVERLAP:
                    Fn.on_side(early)
                else:
                    early()
                hi = lo
                if model._bwd_state is not None:
                    model.resume_backward()
        if clip:
            # the last backward part joined the side stream: every early sum is complete in stream order
            opt.norm_range_device(0, hi, opt.reserve_norm_slice(0, hi), gate=gate)
            opt.clip_finish_device(gate=gate)
            opt.step_device(0, n_arena, clip=True)
        else:
            opt.step_device(0, hi)

    def _capture_rest(self, cuts):
        """The backward parts still pending, one graph each (more_graphs), and the arena range every part completes (ranges)."""
        while self.model._bwd_state is not None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self.graph.pool()):
                self.model.resume_backward()
            self.more_graphs.append(g)
        if self.more_graphs:
            self.graph_b = self.more_graphs[0]
            bounds = [self.model._arena["gcur"].numel()] + [start for _, start in cuts] + [0]
            self.ranges = list(zip(bounds[1:], bounds[:-1]))       # arena range completed by part 1, 2, ... (the rest: last part)

    def _gather(self, samples, plan):
        """Patch gather of the caller's batch into the graph's static patchify operand (internal, arch-grouped sample order)."""
        smap = None
        if plan.order is not None:
            smap, _ = self.model._order_tensors(plan.order, samples.device)
        K.im2col_patch(samples.contiguous().float(), self.model.patch_size, self.col_static.shape[1], torch.bfloat16,
                       sample_map=smap, out=self.col_static)

    def _step_body(self, plan):
        """forward + loss + (first part of the) backward of one step; returns the loss tensor."""
        if self.fused_loss:
            return self.model.loss_and_grad(self.x, self.t, self.pt, self.pot, plan=plan,
                                            loss_out=self._loss_buf if plan is not None else None)
        loss = self._loss(self.model(self.x, patch_output_type=self.pot, plan=plan))
        loss.backward()
        return loss

    def _loss(self, out):
        if self.pt is None:
            return self.criterion(out[0] if isinstance(out, tuple) else out, self.t)
        return _patch_loss(self.criterion, out[0], out[1], self.t, self.pt, self.pot)

    def __call__(self, samples, targets, patch_targets=None, epoch=0, train_iter=0, arch_sample=None):
        self._replay(None, samples, targets, patch_targets, epoch, train_iter, arch_sample)
        return self.loss

    def _replay(self, grad_sync, samples, targets, patch_targets=None, epoch=0, train_iter=0, arch_sample=None):
        """One replay of the step on the caller's batch.  grad_sync (step_with_sync): on the final micro-step of a window the arena
        range a backward part completed is all-reduced right behind that part's replay, beside the next part's; returns those works."""
        self.model._check_fp16_eval(True)         # (the model was switched to fp16 after the capture: no replay)
        if self.optimizer is not None:
            self.optimizer.check_graph_clip()
        with _arch_seed(arch_sample, epoch, train_iter):
            plan = self.model.sample_plan(samples.shape[0])
        first, last, following = _window(self.micro_step, self.accum_steps)
        self._inputs.upload(self.model, plan, first, last)
        if self.col_static is not None:
            self._gather(samples, plan)                           # reads the caller's tensor directly
        elif samples.data_ptr() != self.x.data_ptr():
            self.x.copy_(samples, non_blocking=True)
        if targets.data_ptr() != self.t.data_ptr():
            self.t.copy_(targets, non_blocking=True)
            if self.pt is not None:
                self.pt.copy_(patch_targets, non_blocking=True)
        if len(self._inflight) >= RUN_AHEAD:                       # (bounded run-ahead: RUN_AHEAD)
            self._inflight.pop(0).synchronize()
        self.graph.replay()
        stem.drop_fold(self.model)                                 # (the replay moved BatchNorm's running statistics)
        works = []
        for k, g in enumerate(self.more_graphs):
            if grad_sync is not None and last:                    # the arena range of the part just replayed is final: exchange it now
                works.append(grad_sync.all_reduce_range(*self.ranges[k]))
            g.replay()
        self._inflight.append(torch.cuda.current_stream().record_event())
        self.micro_step = following
        return works

    def finish_update(self):
        """No-op: every replay's optimizer update is complete with the replay itself (kept for callers that call it before
        evaluating, checkpointing or changing the learning rate, as the removed deferred update required)."""

    def step_with_sync(self, grad_sync, samples, targets, patch_targets=None, average=True, **kw):
        """Replay + data-parallel gradient exchange: with split_for_sync the all-reduce of the last stage's gradients
        overlaps the second backward graph; the remainder follows it.  Gradients are averaged on return (average=False:
        summed -- for an optimizer that applies 1/world itself).  accum_steps > 1: only the final micro-step of a window exchanges
        (the window's summed gradients; the optimizer's accum_steps divides); the others issue no collective at all."""
        _, last, _ = _window(self.micro_step, self.accum_steps)
        works = self._replay(grad_sync, samples, targets, patch_targets, **kw)
        if not last:
            return self.loss
        ev = None
        if self.exposed is not None and grad_sync.world > 1:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()                                           # the backward is complete here (on the compute stream)
        if self.more_graphs:
            works.append(grad_sync.all_reduce_range(*self.ranges[-1]))
            grad_sync.finish(works, average=average)
        else:
            grad_sync.all_reduce_grads(average=average)
        if ev is not None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()                                          # work.wait() made the compute stream wait for the exchange
            self.exposed.append((ev, ev1))
        return self.loss


class FastPath:
    """What train_one_epoch(..., fast=FastPath()) keeps between batches and epochs: the captured steps of one (model, optimizer) pair.

    A step is captured on the first batch and whenever its key changes -- batch, target and patch-target shapes, patch_output_type,
    accum_steps, clipping on / off, compute dtype, several ranks or one, the model's arena -- after optimizer.max_norm and
    optimizer.accum_steps were set from the epoch loop's arguments and, in the 16-bit modes, optimizer.own_shadow() was called.  One
    rank: GraphedTrainStep(..., optimizer=optimizer, accum_steps=k), the update inside the graph, optimizer.prepare_step(apply=last)
    before every replay.  Several ranks (grad_sync.world > 1): optimizer=None, split_for_sync=True; the final micro-step of a window
    runs step_with_sync(..., average=False) and optimizer.step() with grad_scale / world.  At most MAX_STEPS captured steps are kept,
    least recently used first out; a step whose arena is no longer the model's is dropped.  set_epoch (keep tables, rewiring) and
    load_state_dict change values in place: the steps survive them and are reused across epochs.
    The capture's eager warm-up steps leave no trace: the CPU RNG and the DropPath generator are restored by GraphedTrainStep,
    the model's buffers (BatchNorm running statistics of the conv stems) here."""

    MAX_STEPS = 2

    def __init__(self):
        self._entries = []                    # [key, arena, GraphedTrainStep], most recently used last
        self._pair = None                     # the (optimizer, criterion) the steps were captured for

    @property
    def steps(self):
        """The captured steps, least recently used first."""
        return [e[2] for e in self._entries]

    def validate(self, model, criterion, optimizer, device, loss_scaler, teacher_model):
        """The fast path serves what it serves and nothing else: no silent fallback to the eager loop.  Touches no device."""
        if not isinstance(optimizer, FlatAdamW) or optimizer.model is not model:
            raise ValueError("optimizer: fast= needs a vitres.optim.FlatAdamW constructed for this model")
        if self._pair is None:
            self._pair = (optimizer, criterion)
        if self._pair[0] is not optimizer:
            raise ValueError("optimizer: this FastPath holds steps captured for another optimizer; use one FastPath per pair")
        if self._pair[1] is not criterion:
            raise ValueError("criterion: this FastPath holds steps captured for another criterion; use one FastPath per pair")
        if loss_scaler is not None:
            raise ValueError("loss_scaler: fast= trains in bf16 or fp32 without a scaler, pass loss_scaler=None")
        if teacher_model is not None:
            raise ValueError("teacher_model: fast= has no teacher inside the captured step, use the eager loop for distillation")
        if torch.device(device).type != "cuda":
            raise ValueError("device: fast= replays a captured hipGraph and needs the GPU, got %s" % (device,))
        p = next(model.parameters(), None)
        if p is None or not p.is_cuda:
            raise ValueError("model: fast= needs the model's parameters on the GPU")

    @staticmethod
    def _key(model, samples_shape, targets_shape, patch_targets_shape, patch_output_type, max_norm, accum_steps, several):
        return (tuple(samples_shape), tuple(targets_shape), None if patch_targets_shape is None else tuple(patch_targets_shape),
                patch_output_type, accum_steps, bool(max_norm), model.compute_dtype, several)

    def static_inputs(self, model, samples_shape, targets_shape, patch_targets_shape, patch_output_type, max_norm, accum_steps,
                      several):
        """The static (x, t, pt) buffers of the captured step that a batch of these shapes would replay, or None before that step's
        first capture.  What is written into them on the current stream is what the next replay reads, and the replay then issues no
        input copy (train_one_epoch mixes straight into them).  Changes nothing: no capture, no reordering of the kept steps."""
        arena = getattr(model, "_arena", None)
        key = self._key(model, samples_shape, targets_shape, patch_targets_shape, patch_output_type, max_norm, accum_steps, several)
        for e in self._entries:
            if e[0] == key and e[1] is arena and arena is not None:
                return e[2].x, e[2].t, e[2].pt
        return None

    def _step_for(self, model, criterion, optimizer, samples, targets, patch_targets, patch_output_type, max_norm, accum_steps,
                  several):
        arena = model._ensure_arena(next(model.parameters()).device)
        key = self._key(model, samples.shape, targets.shape, None if patch_targets is None else patch_targets.shape,
                        patch_output_type, max_norm, accum_steps, several)
        self._entries = [e for e in self._entries if e[1] is arena]
        optimizer.max_norm = max_norm or None
        optimizer.accum_steps = accum_steps
        for i, e in enumerate(self._entries):
            if e[0] == key:
                self._entries.append(self._entries.pop(i))
                # (the optimizer serves whichever of its graphs is replayed next; several ranks: none holds the update)
                optimizer.serve_graph(bool(max_norm) if e[2].optimizer is not None else None)
                return e[2]
        del self._entries[:max(len(self._entries) - (self.MAX_STEPS - 1), 0)]
        if K.is_fast16(model.compute_dtype):
            optimizer.own_shadow()
        buffers = [(b, b.clone()) for b in model.buffers()]
        step = GraphedTrainStep(model, criterion, samples, targets, patch_targets, patch_output_type,
                                optimizer=None if several else optimizer, split_for_sync=several, accum_steps=accum_steps)
        if several:
            optimizer.serve_graph(None)                           # (clipping runs in optimizer.step(), after the exchange)
        with torch.no_grad():
            for b, saved in buffers:
                b.copy_(saved)                                    # (the first replay drops the evaluation stem folded from them)
        self._entries.append([key, arena, step])
        return step

    def micro_step(self, model, criterion, optimizer, samples, targets, patch_targets, patch_output_type, epoch, train_iter,
                   arch_sample, grad_sync, max_norm, accum_steps, micro_step):
        """Micro-step `micro_step` of update `train_iter`: returns a device copy of the step's loss buffer (not synchronised)."""
        several = grad_sync is not None and grad_sync.world > 1
        step = self._step_for(model, criterion, optimizer, samples, targets, patch_targets, patch_output_type, max_norm, accum_steps,
                              several)
        assert step.micro_step == micro_step, "captured step is at micro-step %d of its window, the epoch loop at %d" % (
            step.micro_step, micro_step)
        last = micro_step == accum_steps - 1
        kw = dict(epoch=epoch, train_iter=train_iter, arch_sample=arch_sample)
        if not several:
            optimizer.prepare_step(apply=last)
            return step(samples, targets, patch_targets, **kw).clone()
        loss = step.step_with_sync(grad_sync, samples, targets, patch_targets, average=False, **kw).clone()
        if last:
            scale = optimizer.grad_scale
            optimizer.grad_scale = scale / grad_sync.world        # the exchange left the SUM over the ranks in the arena
            try:
                optimizer.step()
            finally:
                optimizer.grad_scale = scale
        return loss


def train_one_epoch(model, criterion, data_loader, optimizer, device, epoch, loss_scaler=None, max_norm=0,
                    model_ema=None, mixup_fn=None, print_freq=100, teacher_model=None, hard_distill=True, alpha=0.5,
                    logger=None, arch_sample=False, patch_mixup_fn=None, grad_sync=None, sync_every=1, accum_steps=1, fast=None):
    """accum_steps = k > 1: every k consecutive batches of the loader form one optimizer update (train_step's accum_steps /
    micro_step); the iteration index of the seed rule, the EMA update and the learning-rate meter follow the UPDATES, the loss
    meter every micro-batch.  A trailing incomplete window is dropped (the reference's loader is drop_last).
    fast = a FastPath (one per (model, optimizer) pair, passed to every epoch of a run): the same loop on the captured step --
    GraphedTrainStep with the FlatAdamW update, clipping and accumulation inside its graph -- instead of train_step; see FastPath.
    None: the eager loop."""
    _check_accum(accum_steps)
    if fast is not None:
        fast.validate(model, criterion, optimizer, device, loss_scaler, teacher_model)
    kd_criterion = None
    if teacher_model is not None:                                 # engine.py:91-95: any module mapping images to logits
        kd_criterion = KnowledgeDistillationLoss(hard_distill=hard_distill)
        teacher_model.eval()
    model.train()
    criterion.train()
    print_out = logger.info if logger else print
    meters = defaultdict(Meter)
    arch_sample = arch_sample or None
    pending = []

    def drain():                                                  # device -> host sync (reference: every iteration)
        for v in (torch.stack(pending).tolist() if pending else []):
            if not math.isfinite(v):
                print_out('Loss is {}, stopping training'.format(v))
                sys.exit(1)
            meters['loss'].update(v)
        pending.clear()
    t0 = time.time()
    for step_i, (samples, targets) in enumerate(_full_windows(data_loader, accum_steps, print_out)):
        train_iter, micro_step = divmod(step_i, accum_steps)      # train_iter: the optimizer update's index
        samples = samples.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        patch_targets, patch_output_type = None, None
        if samples.dtype == torch.uint8 and not (getattr(patch_mixup_fn, "normalizes", False)
                                                 or getattr(mixup_fn, "normalizes", False)):
            raise TypeError(_U8_MESSAGE % "train_one_epoch")
        if mixup_fn is not None:
            into = _mix_destination(fast, model, mixup_fn, samples, max_norm, accum_steps, grad_sync)
            if into is not None:                                  # straight into the captured step's x / t: no copy at replay
                samples, targets = mixup_fn(samples, targets, out=into[0], targets_out=into[1])
            else:
                samples, targets = mixup_fn(samples, targets)
            assert patch_mixup_fn is None
        if patch_mixup_fn is not None:
            into = _mix_destination(fast, model, patch_mixup_fn, samples, max_norm, accum_steps, grad_sync)
            if into is not None:                                  # straight into the captured step's x / t / pt: no copy at replay
                samples, targets, patch_targets, patch_output_type = patch_mixup_fn(
                    samples, targets, out=into[0], targets_out=into[1], patch_targets_out=into[2])
            else:
                samples, targets, patch_targets, patch_output_type = patch_mixup_fn(samples, targets)
        teacher_output = None
        if teacher_model is not None:
            with torch.no_grad():
                teacher_output = teacher_model(samples)
        if grad_sync is not None:
            grad_sync.broadcast_buffers()                         # DDP broadcast_buffers=True (main.py:367): per forward
        if fast is not None:
            loss = fast.micro_step(model, criterion, optimizer, samples, targets, patch_targets, patch_output_type, epoch,
                                   train_iter, arch_sample, grad_sync, max_norm, accum_steps, micro_step)
        else:
            loss = train_step(model, criterion, optimizer, samples, targets, patch_targets, patch_output_type, epoch,
                              train_iter, arch_sample, grad_sync, loss_scaler, max_norm, teacher_output=teacher_output,
                              kd_criterion=kd_criterion, alpha=alpha, accum_steps=accum_steps, micro_step=micro_step)
        pending.append(loss)
        final = micro_step == accum_steps - 1
        if model_ema is not None and final:
            model_ema.update(model)
        if len(pending) >= sync_every:
            drain()
        if not final:
            continue
        meters['lr'].update(optimizer.param_groups[0]['lr'])
        if print_freq and train_iter % print_freq == 0:
            print_out('Epoch: [{}] [{}] loss: {:.4f} time: {:.1f}s'.format(epoch, train_iter, meters['loss'].global_avg,
                                                                          time.time() - t0))
    drain()
    for m in meters.values():
        m.synchronize_between_processes()
    print_out('Averaged stats: ' + '  '.join('{}: {:.6f}'.format(k, m.global_avg) for k, m in meters.items()))
    return {k: m.global_avg for k, m in meters.items()}


_U8_MESSAGE = ("%s got a uint8 image batch: nothing on this path normalises it.  Wrap the loader in "
               "vitres.data.DevicePrefetchLoader (evaluation), or train with SwitchTokenMix(..., input_norm=(mean, std)) "
               "or Mixup(..., input_norm=(mean, std))")


def _mix_destination(fast, model, mix, samples, max_norm, accum_steps, grad_sync):
    """Where a vitres SwitchTokenMix (x, t, pt) or Mixup (x, t; no patch targets) writes under fast=: the static inputs of the captured
    step this batch will replay -- every part of that step's key is known before the mix -- or None (first batch of a key, the eager
    loop, any other mix)."""
    if fast is None or samples.dim() != 4:
        return None
    B = samples.shape[0]
    if isinstance(mix, SwitchTokenMix):
        pt_shape, pot = (B, mix.patch_len * mix.patch_len, mix.num_classes), 'seq'
    elif isinstance(mix, Mixup):
        pt_shape, pot = None, None
    else:
        return None
    several = grad_sync is not None and grad_sync.world > 1
    return fast.static_inputs(model, samples.shape, (B, mix.num_classes), pt_shape, pot, max_norm, accum_steps, several)


def _full_windows(data_loader, k, print_out=print):
    """The loader's batches, minus a trailing window of fewer than k (k = 1: the loader itself)."""
    if k == 1:
        yield from data_loader
        return
    window = []
    for batch in data_loader:
        window.append(batch)
        if len(window) == k:
            yield from window
            window = []
    if window:
        print_out('Dropped a trailing window of {} micro-batch(es): accum_steps is {}'.format(len(window), k))


def accuracy(output, target, topk=(1,)):
    """timm.utils.accuracy: top-k accuracy in percent."""
    maxk = max(topk)
    pred = output.topk(maxk, 1, True, True)[1].t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[:k].reshape(-1).float().sum(0) * 100.0 / target.size(0) for k in topk]


@torch.no_grad()
def evaluate(data_loader, model, device, print_freq=100, logger=None, device_meters=None):
    """engine.evaluate (:194-261): eval forward, CE, top-1/5 weighted by batch size, global averages.
    device_meters: loss and hit counts accumulate in ONE vr_eval_state on the device (kernels.eval_metrics, one launch per batch, the
    distillation head and the joint softmax of two-token models included) and are read once, after the last batch -- no torch op and
    no device-to-host read inside the loop.  None: on when the logits are CUDA tensors; True: forced; False: the reference's torch
    statement with its three to seven `.item()` reads per batch.  Either way the meters hold the same totals and counts."""
    criterion = torch.nn.CrossEntropyLoss()
    print_out = logger.info if logger else print
    meters = defaultdict(Meter)
    model.eval()
    state, two_heads = None, False
    for images, target in data_loader:
        images = images.to(device, non_blocking=True)
        target = target.to(device, non_blocking=True)
        output = model(images)
        output_cls, output_dst = (output[0], output[1]) if isinstance(output, tuple) else (output, None)
        if device_meters or (device_meters is None and output_cls.is_cuda):
            if state is None:
                state = K.eval_state(output_cls.device)
            two_heads = two_heads or output_dst is not None
            K.eval_metrics(_fp32_rows(output_cls), target, state, None if output_dst is None else _fp32_rows(output_dst))
            continue
        loss = criterion(output_cls, target)
        acc1, acc5 = accuracy(output_cls, target, topk=(1, 5))
        n = images.shape[0]
        meters['loss'].update(loss.item())
        meters['acc1'].update(acc1.item(), n=n)
        meters['acc5'].update(acc5.item(), n=n)
        if output_dst is not None:                       # two-token variants: distillation head and joint softmax (:230-238)
            d1, d5 = accuracy(output_dst, target, topk=(1, 5))
            meters['dst_acc1'].update(d1.item(), n=n)
            meters['dst_acc5'].update(d5.item(), n=n)
            joint = torch.softmax(output_cls, dim=1) + torch.softmax(output_dst, dim=1)
            j1, j5 = accuracy(joint, target, topk=(1, 5))
            meters['jnt_acc1'].update(j1.item(), n=n)
            meters['jnt_acc5'].update(j5.item(), n=n)
    if state is not None:
        st = K.read_eval_state(state)                    # the evaluation's only device-to-host read
        # loss: the unweighted mean of batch means (the reference's meter); accuracies: weighted by batch size
        meters['loss'].total, meters['loss'].count = st['loss_sum'], st['calls']
        for head in ('', 'dst_', 'jnt_') if two_heads else ('',):
            for k in ('1', '5'):
                m = meters[head + 'acc' + k]
                m.total, m.count = 100.0 * st[head + 'top' + k], st['rows']
    for m in meters.values():
        m.synchronize_between_processes()
    info = 'Acc@1: {:.2f}, Acc@5: {:.2f}, loss: {:.2f}'.format(meters['acc1'].global_avg, meters['acc5'].global_avg,
                                                             meters['loss'].global_avg)
    if 'dst_acc1' in meters:
        info += ', Distill Acc@1: {:.2f}, Distill Acc@5: {:.2f}, Joint Acc@1: {:.2f}, Joint Acc@5: {:.2f}'.format(
            meters['dst_acc1'].global_avg, meters['dst_acc5'].global_avg, meters['jnt_acc1'].global_avg,
            meters['jnt_acc5'].global_avg)
    print_out(info + '\n')
    return {k: m.global_avg for k, m in meters.items()}


def _fp32_rows(logits):
    """Logits as vr_eval_metrics reads them (fp32 rows; the models' heads already return these)."""
    return logits if logits.dtype == torch.float32 else logits.float()


def param_groups_weight_decay(model, weight_decay=0.05):
    """timm 0.3.2 optim_factory.add_weight_decay as used by create_optimizer (main.py:385): 1-D parameters,
    `.bias` and names returned by model.no_weight_decay() get no weight decay."""
    skip = model.no_weight_decay() if hasattr(model, 'no_weight_decay') else set()
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if (p.ndim == 1 or name.endswith('.bias') or name in skip) else decay).append(p)
    return [{'params': no_decay, 'weight_decay': 0.}, {'params': decay, 'weight_decay': weight_decay}]
