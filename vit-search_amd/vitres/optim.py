"""Step tail on the flat parameter arena: AdamW (+ bf16 shadow, gradient averaging, EMA) in ONE HIP pass.

Reference: timm 0.3.2 `create_optimizer(args, model)` -> torch.optim.AdamW(lr, weight_decay=0.05) over the two groups of
`add_weight_decay` (main.py:385; engine.param_groups_weight_decay restates the grouping), `ModelEmaV2` (main.py:357-363).
`FlatAdamW` keeps torch.optim.Optimizer's interface (param_groups with mutable 'lr' for the cosine scheduler,
state_dict / load_state_dict, zero_grad) but its state is two flat fp32 buffers shaped like the model's arena, and step()
is one `vr_adamw_flat` launch that also refreshes the bf16 weight shadow the next forward reads.

Gradient-norm clipping (the reference's `--clip-grad`: loss_scaler(loss, optimizer, clip_grad=max_norm, ...), engine.py:178-180, i.e.
torch.nn.utils.clip_grad_norm_) is part of the same tail when `max_norm` is set: vr_grad_sumsq over the gradient arena ->
vr_clip_finish (norm, coefficient, skip flag in a device-resident vr_clip_state) -> vr_adamw_flat_clip, which multiplies every
gradient by the coefficient.  All three are capturable (engine.GraphedTrainStep).
"""
import ctypes
import math

import torch

from . import _lib, stem
from .kernels import _p, _stream

MAX_GROUPS = 16
# vr_grad_sumsq: partial sums per arena range (one per workgroup) and ranges per step.  2048 workgroups of 256 threads at 8 elements
# per trip keep every thread's fp32 chains at 144 M / (2048 * 2048) = 35 terms for the largest shipped arena (bound: 256).
NORM_PARTIALS = 2048
NORM_MAX_RANGES = 8


class _Group(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_c1", "sqrt_bias_c2",
                                              "grad_scale")]


class _ClipState(ctypes.Structure):            # vr_clip_state (include/vitres_hip.h): 8 dwords
    _fields_ = [("max_norm", ctypes.c_float), ("grad_scale", ctypes.c_float), ("norm", ctypes.c_float), ("coef", ctypes.c_float),
                ("skip", ctypes.c_int32), ("skipped", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


def _check_accum_steps(v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError("accum_steps must be an int >= 1, got %r" % (v,))
    return v


def _check_max_norm(v):
    if v is None:
        return None
    v = float(v)
    if math.isnan(v) or v < 0:
        raise ValueError("max_norm must be None, 0 (both: no clipping), a positive number or inf (measure only), got %r" % v)
    return v


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, model, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, ema_decay=None, max_norm=None,
                 accum_steps=1):
        """params: iterable of parameters or of param-group dicts (as torch.optim.AdamW); every parameter must belong to
        `model`, whose arena they live in.  ema_decay: keep an exponential moving average of the parameters
        (`ema_state_dict()` returns it under the model's state_dict keys).
        max_norm: clip the global L2 norm of the gradients (of all groups together, after grad_scale) to this value before the
        update, as torch.nn.utils.clip_grad_norm_ does: every gradient is multiplied by min(1, max_norm / (norm + 1e-6)).  A plain
        attribute that may change between steps.  None or 0: off -- no extra launch, no extra allocation.  float("inf"): the norm
        is measured (grad_norm()) and non-finite steps are skipped, nothing is clipped.  While it is on, a step whose gradient
        norm is inf or NaN changes NOTHING on the device -- parameters, moments, EMA and bf16 shadow keep their values
        (skipped_steps() counts them) -- where torch's formula would turn every parameter into NaN.  The host step count still
        advances on such a step: the host runs ahead of the device and cannot know.  Against torch.cuda.amp.GradScaler, which does
        not count a skipped step, only the bias corrections of the later steps differ (they are one step further along).
        accum_steps (an int >= 1, a plain attribute like grad_scale): the arena holds the SUM of the gradients of that many
        micro-batches (loss_and_grad(accumulate=True), engine.GraphedTrainStep(accum_steps=k)); the update uses their mean: every
        gradient is multiplied by grad_scale / accum_steps, so grad_norm(), clipping and the skip rule see the averaged gradient.
        The step count and the bias corrections count optimizer updates, not micro-batches."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError("at most %d parameter groups" % MAX_GROUPS)
        self.model = model
        self.ema_decay = ema_decay
        self._step = 0
        self._arena_id = None
        self.grad_scale = 1.0              # e.g. 1/world when the all-reduce leaves a SUM in the gradient arena
        self.max_norm = _check_max_norm(max_norm)
        self.accum_steps = _check_accum_steps(accum_steps)
        self._clip = None                  # device state of the clipping launches: allocated by the first step that clips
        self._graph_clip = None            # engine.GraphedTrainStep: whether its captured graph holds the clipping launches

    # ---- gradient-norm clipping ---------------------------------------------------------------------------------
    def clip_enabled(self):
        return bool(_check_max_norm(self.max_norm))

    def serve_graph(self, clip):
        """Declare which captured graph the next prepare_step() / replay belongs to, for a caller that keeps several graphs of this
        optimizer (engine.FastPath): clip = whether that graph holds the clipping launches -- prepare_step() and the replay raise
        when max_norm disagrees with it; None = no captured graph holds the update (step() runs it after the replay)."""
        self._graph_clip = None if clip is None else bool(clip)

    def check_graph_clip(self):
        """A graph holds the clipping launches or not from its capture on: raises once max_norm was switched between on and off
        after it (prepare_step() and every replay ask; on <-> float("inf") is the switch a captured graph follows)."""
        if self._graph_clip is not None and self.clip_enabled() != self._graph_clip:
            raise RuntimeError("FlatAdamW.max_norm was %s after the step's graph was captured %s the clipping launches: a replay "
                               "would ignore it.  Capture with max_norm set (float('inf') measures without clipping) and switch "
                               "between values, or capture a new GraphedTrainStep."
                               % (("set", "without") if self.clip_enabled() else ("cleared", "with")))

    def prepare_capture(self):
        """Before a capture of step_device() / norm_range_device() launches (engine.GraphedTrainStep): fills the device blocks they read
        WITHOUT counting a step, hands the partial-sum slices out from the first again; returns whether the graph is to clip."""
        clip = self._graph_clip = self.clip_enabled()      # (a graph captured earlier with the other setting has no say any more)
        self.prepare_step()
        self._step -= 1
        if clip:
            self._clip["used"] = 0
        return clip

    def _grad_factor(self):
        """What every gradient element is multiplied by: grad_scale (the caller's 1/world) / accum_steps (mean over the window)."""
        return float(self.grad_scale) / _check_accum_steps(self.accum_steps)

    def _clip_bind(self, dev):
        c = self._clip
        if c is None or c["state"].device != dev:
            old = c
            c = self._clip = {"state": torch.zeros(8, dtype=torch.float32, device=dev),
                              "partials": torch.zeros(NORM_PARTIALS * NORM_MAX_RANGES, dtype=torch.float32, device=dev), "used": 0}
            c["state"][2:4] = torch.tensor([0.0, 1.0])     # (norm, coef) before the first measured step
            if old is not None:
                c["state"].copy_(old["state"])
        return c

    def _clip_upload(self, dev, pinned=False):
        """max_norm and grad_scale -> the input half of the device's vr_clip_state (the output half is the device's own)."""
        c = self._clip_bind(dev)
        host = torch.tensor([_check_max_norm(self.max_norm), self._grad_factor()], dtype=torch.float32)
        if pinned and dev.type == "cuda":
            host = host.pin_memory()       # (a fresh block per step, as for the hyper-parameters in prepare_step)
        c["state"][:2].copy_(host, non_blocking=pinned)
        return c

    def reserve_norm_slice(self, lo, hi):
        """The slice of the partial-sum buffer norm_range_device(lo, hi) will fill: (first, count).  Slices are handed out in
        call order and given back by clip_finish_device()."""
        c = self._clip_bind(self._bind()["flat"].device)
        count = min(((hi - lo) // 8 + 255) // 256, NORM_PARTIALS)
        if c["used"] + count > c["partials"].numel():
            raise RuntimeError("more than %d arena ranges in one gradient norm" % NORM_MAX_RANGES)
        first, c["used"] = c["used"], c["used"] + count
        return first, count

    @torch.no_grad()
    def norm_range_device(self, lo, hi, piece, max_blocks=0, gate=None):
        """Sum of squares of the gradient arena range [lo, hi) (multiples of 8) into the slice `piece` = reserve_norm_slice(lo,
        hi) of the partial sums: capturable.  max_blocks as for step_device.  gate: a device int32 word read at run time; 0 makes
        the launch a no-op that leaves the slice untouched (vr_grad_sumsq_gated: non-final micro-steps of an accumulation window)."""
        a = self._bind()
        g = a.get("gcur")
        n = a["flat"].numel()
        if g is None:
            raise RuntimeError("norm_range_device needs gradients in the arena")
        if lo % 8 or hi % 8 or not (0 <= lo < hi <= n):
            raise ValueError("range must be non-empty and aligned to 8 elements")
        c = self._clip_bind(a["flat"].device)
        first, count = piece
        if not (0 <= first and count > 0 and first + count <= c["partials"].numel()):
            raise ValueError("piece is not a slice of the partial-sum buffer")
        if gate is not None:
            _lib.check(_lib.lib().vr_grad_sumsq_gated(g.data_ptr() + 4 * lo, self._flat_state["gid"].data_ptr() + lo // 8, hi - lo,
                                                      c["partials"].data_ptr() + 4 * first, count, int(max_blocks), _p(gate),
                                                      _stream()), "vr_grad_sumsq_gated")
            return
        _lib.check(_lib.lib().vr_grad_sumsq(g.data_ptr() + 4 * lo, self._flat_state["gid"].data_ptr() + lo // 8, hi - lo,
                                            c["partials"].data_ptr() + 4 * first, count, int(max_blocks), _stream()),
                   "vr_grad_sumsq")

    @torch.no_grad()
    def clip_finish_device(self, gate=None):
        """Partial sums of every norm_range_device since the last call -> norm, clip coefficient and skip flag on the device.
        gate: as for norm_range_device; gate 0 leaves every field of the device state untouched (vr_clip_finish_gated)."""
        c = self._clip
        if c is None or c["used"] == 0:
            raise RuntimeError("clip_finish_device needs norm_range_device launches before it")
        if gate is not None:
            _lib.check(_lib.lib().vr_clip_finish_gated(_p(c["partials"]), c["used"], _p(c["state"]), _p(gate), _stream()),
                       "vr_clip_finish_gated")
        else:
            _lib.check(_lib.lib().vr_clip_finish(_p(c["partials"]), c["used"], _p(c["state"]), _stream()), "vr_clip_finish")
        c["used"] = 0

    def grad_norm(self):
        """L2 norm of the last step's gradient as the optimizer used it (after grad_scale, before clipping), as clip_grad_norm_
        returns it: a 0-dim device tensor, not synchronised.  Needs max_norm (float("inf") measures without clipping)."""
        if self._clip is None:
            raise RuntimeError("grad_norm() needs max_norm set (float('inf') measures without clipping) and one step taken")
        return self._clip["state"][2]

    def skipped_steps(self):
        """Number of steps skipped so far because their gradient norm was inf or NaN (synchronises)."""
        return 0 if self._clip is None else int(self._clip["state"].view(torch.int32)[5].item())

    # ---- arena-shaped state -------------------------------------------------------------------------------
    def _bind(self):
        dev = next(self.model.parameters()).device
        a = self.model._ensure_arena(dev)
        if self._arena_id == id(a):
            return a
        flat = a["flat"]
        if flat.numel() % 8:
            raise RuntimeError("arena length must be a multiple of 8")
        gid = torch.full((flat.numel() // 8,), 255, dtype=torch.uint8)
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if id(p) not in a["index"]:
                    raise ValueError("FlatAdamW: parameter does not belong to the model's arena")
                off, n = a["offsets"][a["index"][id(p)]]
                gid[off // 8:(off + n + 7) // 8] = gi
        old = getattr(self, "_flat_state", None)
        self._flat_state = {"m": torch.zeros_like(flat), "v": torch.zeros_like(flat), "gid": gid.to(flat.device),
                            "ema": flat.clone() if self.ema_decay is not None else None}
        if old is not None and old["m"].numel() == flat.numel():      # arena rebuilt (e.g. .to(device)): carry the state
            for k in ("m", "v", "ema"):
                if old[k] is not None and self._flat_state[k] is not None:
                    self._flat_state[k].copy_(old[k])
        self._arena_id = id(a)
        return a

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        a = self._bind()
        g = a.get("gcur")
        p0 = a["params"][0]
        if g is None or p0.grad is None or p0.grad.data_ptr() != g.data_ptr() + 4 * a["offsets"][0][0]:
            raise RuntimeError("FlatAdamW needs the gradients in the model's flat arena (one backward since zero_grad)")
        self._step += 1
        stem.drop_fold(self.model)             # parameters change through raw pointers: no Tensor._version moves
        arr = self._group_structs(self._step)
        st = self._flat_state
        shadow = a["shadow"] if self.model.compute_dtype == torch.bfloat16 else None
        if self.clip_enabled():            # sum of squares -> norm / coefficient -> AdamW on the clipped gradient: three launches
            n = a["flat"].numel()
            c = self._clip_upload(a["flat"].device)
            self.norm_range_device(0, n, self.reserve_norm_slice(0, n))
            self.clip_finish_device()
            _lib.check(_lib.lib().vr_adamw_flat_clip(_p(a["flat"]), _p(g), _p(st["m"]), _p(st["v"]), _p(shadow), _p(st["ema"]),
                                                     float(self.ema_decay or 0.0), _p(st["gid"]), ctypes.byref(arr), 0,
                                                     len(self.param_groups), n, _p(c["state"]), 0, _stream()), "vr_adamw_flat_clip")
        else:
            _lib.check(_lib.lib().vr_adamw_flat(_p(a["flat"]), _p(g), _p(st["m"]), _p(st["v"]), _p(shadow), _p(st["ema"]),
                                                float(self.ema_decay or 0.0), _p(st["gid"]), ctypes.byref(arr),
                                                len(self.param_groups), a["flat"].numel(), _stream()), "vr_adamw_flat")
        if shadow is not None:
            a["shadow_ok"] = True              # forwards skip their own vr_cast_f32_bf16 from now on (model.invalidate_shadow)
        return loss

    # ---- the update as part of a captured hipGraph ---------------------------------------------------------------------
    @staticmethod
    def _bias_corrections(b1, b2, t):
        """(bias_c1, sqrt_bias_c2) of step t in double, before vr_adamw_group rounds them to fp32"""
        return 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)

    def _group_structs(self, t):
        arr = (_Group * len(self.param_groups))()
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            bias_c1, sqrt_bias_c2 = self._bias_corrections(b1, b2, t)
            arr[gi] = _Group(group["lr"], b1, b2, group["eps"], group["weight_decay"], bias_c1, sqrt_bias_c2, self._grad_factor())
        return arr

    def prepare_step(self, apply=True):
        """apply=False (a non-final micro-step of an accumulation window: engine.GraphedTrainStep(accum_steps=k), k > 1): the step
        count stays and an ALL-ZERO hyper-parameter block is uploaded -- the captured AdamW launches skip every group whose bias_c1
        is 0, so the replay changes no parameter, moment, EMA or shadow element.  apply=True:
        Advance the step count and upload this step's per-group hyper-parameters (learning rates written by the scheduler,
        bias corrections) to the device buffer step_device() launches read -- call once before every replay of a graph that
        contains step_device() launches (engine.GraphedTrainStep(optimizer=...)).  With max_norm set, max_norm and grad_scale
        are uploaded too; a graph holds the clipping launches or not from its capture on, so switching max_norm between on and
        off after the capture raises here (on <-> float("inf") is the switch a captured graph follows)."""
        self.check_graph_clip()
        a = self._bind()
        dev = a["flat"].device
        if getattr(self, "_hp_dev", None) is None or self._hp_dev.device != dev:
            self._hp_dev = torch.zeros(MAX_GROUPS * 8, dtype=torch.float32, device=dev)
        host = torch.zeros(MAX_GROUPS * 8, dtype=torch.float32)
        if apply:
            self._step += 1
            stem.drop_fold(self.model)         # parameters change through raw pointers: no Tensor._version moves
            arr = self._group_structs(self._step)
            vals = [getattr(arr[gi], n) for gi in range(len(self.param_groups)) for n, _ in _Group._fields_]
            host[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
        if dev.type == "cuda":
            host = host.pin_memory()       # a fresh pinned block per step: the host runs several replays ahead of the device, a
                                           # reused staging buffer would be overwritten before its copy has executed
        self._hp_dev.copy_(host, non_blocking=True)
        if apply and self.clip_enabled():
            self._clip_upload(dev, pinned=True)

    @torch.no_grad()
    def step_device(self, lo=0, hi=None, max_blocks=0, clip=False):
        """AdamW over the arena range [lo, hi) (multiples of 8) with the hyper-parameters prepare_step() uploaded: capturable.
        max_blocks > 0: launched with at most that many workgroups (an update that runs beside other work).
        clip: the gradient is also multiplied by the coefficient clip_finish_device() left on the device (and nothing is written
        on a skipped step) -- the launch must follow the finish of the WHOLE arena's norm."""
        a = self._bind()
        g = a.get("gcur")
        if g is None or getattr(self, "_hp_dev", None) is None:
            raise RuntimeError("step_device needs gradients in the arena and a prepare_step() before it")
        n = a["flat"].numel()
        hi = n if hi is None else hi
        if lo % 8 or hi % 8 or not (0 <= lo < hi <= n):
            raise ValueError("range must be non-empty and aligned to 8 elements")
        st = self._flat_state
        shadow = a["shadow"] if self.model.compute_dtype == torch.bfloat16 else None
        stem.drop_fold(self.model)

        def at(t, esz):
            return None if t is None else t.data_ptr() + lo * esz
        if clip:
            if self._clip is None:
                raise RuntimeError("step_device(clip=True) needs clip_finish_device() before it")
            _lib.check(_lib.lib().vr_adamw_flat_clip(at(a["flat"], 4), at(g, 4), at(st["m"], 4), at(st["v"], 4), at(shadow, 2),
                                                     at(st["ema"], 4), float(self.ema_decay or 0.0), st["gid"].data_ptr() + lo // 8,
                                                     _p(self._hp_dev), 1, len(self.param_groups), hi - lo, _p(self._clip["state"]),
                                                     int(max_blocks), _stream()), "vr_adamw_flat_clip")
        else:
            _lib.check(_lib.lib().vr_adamw_flat_dev_capped(
                at(a["flat"], 4), at(g, 4), at(st["m"], 4), at(st["v"], 4), at(shadow, 2), at(st["ema"], 4), float(self.ema_decay or 0.0),
                st["gid"].data_ptr() + lo // 8, _p(self._hp_dev), len(self.param_groups), hi - lo, int(max_blocks), _stream()),
                "vr_adamw_flat_dev_capped")
        if shadow is not None:
            a["shadow_ok"] = True

    def own_shadow(self):
        """Declare before capturing a hipGraph that this optimizer keeps the bf16 weight shadow up to date: casts it once
        now; forwards (and graphs captured from now on) contain no cast of their own."""
        a = self._bind()
        if self.model.compute_dtype == torch.bfloat16:
            from . import kernels as K
            K.cast_bf16(a["flat"], a["shadow"])
            a["shadow_ok"] = True

    # ---- checkpoint / EMA views -------------------------------------------------------------------------------
    def state_dict(self):
        self._bind()
        st = self._flat_state
        return {"step": self._step, "exp_avg": st["m"].clone(), "exp_avg_sq": st["v"].clone(),
                "ema": None if st["ema"] is None else st["ema"].clone(),
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                "max_norm": _check_max_norm(self.max_norm)}

    def load_state_dict(self, sd):
        """Accepts its own flat layout or torch.optim.AdamW's (the 'optimizer' entry of a reference checkpoint.pth.tar,
        main.py:506-512): per-parameter exp_avg / exp_avg_sq are scattered into the arena-shaped moments."""
        if "state" in sd:
            return self.load_torch_state_dict(sd)
        self._bind()
        st = self._flat_state
        self._step = int(sd["step"])
        st["m"].copy_(sd["exp_avg"])
        st["v"].copy_(sd["exp_avg_sq"])
        if st["ema"] is not None and sd.get("ema") is not None:
            st["ema"].copy_(sd["ema"])
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if "max_norm" in sd:                   # (a state dict written before max_norm existed leaves the constructor's value)
            self.max_norm = _check_max_norm(sd["max_norm"])

    def _ordered_params(self):
        return [p for g in self.param_groups for p in g["params"]]      # torch numbers parameters in this order

    def torch_state_dict(self):
        """The state in torch.optim.AdamW.state_dict() layout ({'state': {i: {step, exp_avg, exp_avg_sq}}, 'param_groups'}),
        i.e. what the reference writes under 'optimizer' -- a checkpoint saved here resumes in the reference and vice versa."""
        a = self._bind()
        st = self._flat_state
        state, groups, i = {}, [], 0
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                off, n = a["offsets"][a["index"][id(p)]]
                if self._step > 0:
                    state[i] = {"step": torch.tensor(float(self._step)), "exp_avg": st["m"][off:off + n].view(p.shape).clone(),
                                "exp_avg_sq": st["v"][off:off + n].view(p.shape).clone()}
                ids.append(i)
                i += 1
            pg = {k: v for k, v in g.items() if k != "params"}
            pg.setdefault("amsgrad", False)
            pg["params"] = ids
            groups.append(pg)
        return {"state": state, "param_groups": groups}

    def load_torch_state_dict(self, sd):
        a = self._bind()
        st = self._flat_state
        params = self._ordered_params()
        n_saved = sum(len(g["params"]) for g in sd["param_groups"])
        if n_saved != len(params) or len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups / parameters")
        steps = set()
        st["m"].zero_()
        st["v"].zero_()
        saved_ids = [i for g in sd["param_groups"] for i in g["params"]]
        for p, i in zip(params, saved_ids):
            ps = sd["state"].get(i)
            if ps is None:
                continue
            if tuple(ps["exp_avg"].shape) != tuple(p.shape):
                raise ValueError("optimizer state of parameter %d has shape %s, expected %s" % (i, tuple(ps["exp_avg"].shape),
                                                                                                tuple(p.shape)))
            off, n = a["offsets"][a["index"][id(p)]]
            st["m"][off:off + n].copy_(ps["exp_avg"].reshape(-1))
            st["v"][off:off + n].copy_(ps["exp_avg_sq"].reshape(-1))
            steps.add(int(ps["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ (%s): not an AdamW state this optimizer can continue" % sorted(steps))
        self._step = steps.pop() if steps else 0
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in s.items() if k not in ("params", "amsgrad", "foreach", "maximize", "capturable",
                                                               "differentiable", "fused", "decoupled_weight_decay")})

    def ema_state_dict(self):
        """EMA parameters under the model's state_dict keys (buffers are taken from the live model, as ModelEmaV2's
        deepcopy shares nothing but is updated from them every step)."""
        a = self._bind()
        if self._flat_state["ema"] is None:
            raise RuntimeError("constructed without ema_decay")
        ema = self._flat_state["ema"]
        byid = {id(p): ema[off:off + n].view(p.shape) for p, (off, n) in zip(a["params"], a["offsets"])}
        out = {}
        for k, v in self.model.state_dict(keep_vars=True).items():
            out[k] = byid[id(v)].clone() if id(v) in byid else v.detach().clone()
        return out

    def load_ema_state_dict(self, sd):
        """Inverse of ema_state_dict(): scatter a model-keyed state dict (the 'model_ema' entry of a checkpoint, reference
        utils._load_checkpoint_for_ema / main.py:413-414) into the arena-shaped EMA.  Buffers in `sd` are ignored (the EMA tracks
        parameters only; buffers come from the live model)."""
        a = self._bind()
        if self._flat_state["ema"] is None:
            raise RuntimeError("constructed without ema_decay")
        ema = self._flat_state["ema"]
        where = {id(p): (off, n) for p, (off, n) in zip(a["params"], a["offsets"])}
        missing = []
        with torch.no_grad():
            for k, v in self.model.state_dict(keep_vars=True).items():
                if id(v) not in where:
                    continue
                if k not in sd:
                    missing.append(k)
                    continue
                off, n = where[id(v)]
                if tuple(sd[k].shape) != tuple(v.shape):
                    raise ValueError("model_ema[%s] has shape %s, expected %s" % (k, tuple(sd[k].shape), tuple(v.shape)))
                ema[off:off + n].copy_(sd[k].reshape(-1).to(ema.device, torch.float32))
        if missing:
            raise KeyError("model_ema lacks parameters: %s" % ", ".join(missing[:5]))

