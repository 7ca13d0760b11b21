"""Tensor-level wrappers over the C ABI (include/vitres_hip.h).

Each function takes torch CUDA tensors, passes raw device pointers + sizes to libvitres_hip.so on
torch's current stream, and returns torch tensors it allocated for the outputs.  PyTorch is used
for device memory and streams only.  Non-CUDA tensors raise: there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GemmArgs, LnEpilogue, RowMap, VR_BF16, VR_F16, VR_F32

IDENT = (0, 0, 0)

# bench.py instrumentation: when a list, every vr_gemm launch is bracketed by HIP events on torch's current stream
# (the stream the kernel is launched on) and (kind, flops, bytes, ev0, ev1) is appended.
PROFILE = None
PROFILE_ATTN = None       # with PROFILE: (kept FLOPs, event, event) per attention launch
PROFILE_DESC = None       # with PROFILE: one description per entry (tools/gemm_launches.py)


_DTCODES = {torch.float32: VR_F32, torch.bfloat16: VR_BF16, torch.float16: VR_F16}
_DTNAMES = {VR_F32: "f32", VR_BF16: "bf16", VR_F16: "f16"}


def _dtcode(dtype):
    code = _DTCODES.get(dtype)
    if code is None:
        raise TypeError("unsupported dtype %s (the kernels take float32, bfloat16 or float16)" % dtype)
    return code


def _dt(t):
    return _dtcode(t.dtype)


def is_fast16(dtype):
    """The 16-bit MFMA modes (bf16; fp16 for evaluation): the dtypes whose forward takes the 16-bit kernels and their fused forms."""
    return dtype == torch.bfloat16 or dtype == torch.float16


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("vitres kernels run on the GPU and need CUDA/HIP tensors (got %s); there is no CPU fallback" % t.device)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rm(m):
    return RowMap(*(m or IDENT))


# Workspaces of the split-K GEMM form (vr_gemm_args.ws): one per (device, role).  A role is a chain of launches that never overlap
# one another: 0 = the main stream, 1 = the side stream of vitres.functional, 8.. = its auxiliary streams (it switches the role
# around what it runs there).  Created zeroed on first use -- outside graph capture (engine.GraphedTrainStep calls ensure_workspaces first): a launch
# that finds none while capturing simply runs without tile sharing.
_WS = {}
_WS_ROLE = [0]
# test / tool aid: k_shares of every forward / data-gradient launch that does not pass its own (0: the library's rule)
K_SHARES = 0


class ws_role:
    def __init__(self, role):
        self.role = role

    def __enter__(self):
        self.prev, _WS_ROLE[0] = _WS_ROLE[0], self.role

    def __exit__(self, *exc):
        _WS_ROLE[0] = self.prev


def _workspace(dev, role=None):
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), _WS_ROLE[0] if role is None else role)
    ws = _WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        ws = _WS[key] = torch.zeros(int(_lib.lib().vr_gemm_ws_bytes()), dtype=torch.uint8, device=dev)
    return ws


def ensure_workspaces(dev, roles=(0, 1)):
    for r in roles:
        _workspace(torch.device(dev), r)


# Architecture groups of the batch being processed (vr_gemm_args.m_groups): the model sets it from its plan at the start of a
# forward / backward (G = B / example_per_arch contiguous groups of samples in the arch-grouped execution order, each with its own
# keep rows); every GEMM that carries keep arrays passes it on, so that the kernels deal every group to every XCD.
M_GROUPS = [1]
# The model vouches (vit_sr_supernet.sample_plan -> plan.skip_writes) that every tile / token split of the bf16 kernels sees ONE
# architecture of the batch being processed and that every masked Linear of the network is one the group-pure kernels cover: the
# masked GEMMs then carry sched bit 0x40000 -- producers leave fully masked output tiles unwritten, and a launch that would have
# to read such an operand through a kernel that tiles across groups fails (VR_EUNSUPPORTED) instead of reading them.
WRITE_SKIP = [False]
SKIP_WRITES_BIT = 0x40000
READS_SKIPPED_BIT = 0x80000


def reads_skipped():
    """sched bit for a GEMM whose operand (the MLP's hidden activation or its gradient) was produced under WRITE_SKIP: the launch
    must go to a kernel that tiles group by group, or fail."""
    return READS_SKIPPED_BIT if WRITE_SKIP[0] else 0


# test aid (tests/test_gpu_fullsize.py): fill the output of every launch that may leave tiles unwritten with NaN first -- a reader of
# an unwritten tile then changes the loss / gradients instead of quietly reading whatever the arena held
DBG_POISON = False


def _gemm_args(a, b, out, *, M, N, K, lda, ldb, ldc, a_trans=False, b_trans=False, out2=None, bias=None, pos=None,
               scale=None, keep_n=None, resid=None, dact_u=None, ldu=0, act=0, atomic=False, split_k=1, rows_in=0,
               a_map=None, b_map=None, c_map=None, bias_grad=None, keep_k=None, n_period=0, k_period=0, sched=0, ws="auto",
               ring=0, k_shares=0, m_groups=None, sr_pool=None, keep_out=None, tok_rows=None):
    """sr_pool = (x [B, T + g*g, Cin] fp32, g, T): the pooled shortcut of a spatial-reduction block added where resid would be;
    keep_out: the outer prefix mask, applied last; tok_rows = (src, pos or None, T, ld, rows per sample or 0, cols): the launch also
    writes the T token rows of every sample (vr_gemm_args.sr_x / keep_out / tok_src)."""
    args = GemmArgs()
    if sr_pool is not None:
        sx, sg, st = sr_pool
        assert sx.dtype == torch.float32 and sx.is_contiguous() and sx.shape[1] == st + sg * sg
        args.sr_x, args.sr_g, args.sr_cin, args.sr_tokens = _p(sx), sg, sx.shape[-1], st
    args.keep_out = _p(keep_out)
    if tok_rows is not None:
        src, tpos, tn, tld, trps, tcols = tok_rows
        assert src.dtype == torch.float32 and (tpos is None or tpos.dtype == torch.float32)
        args.tok_src, args.tok_pos, args.tok_rows, args.tok_ld, args.tok_rps, args.tok_cols = _p(src), _p(tpos), tn, tld, trps, tcols
    if isinstance(ws, str):         # "auto": the role's workspace wherever the K-split kernels (gemm_ntk.hip) could be chosen
        ws = _workspace(a.device) if (not a_trans and is_fast16(a.dtype) and a.is_cuda and K >= 512 and k_shares != 1) else None
    if ws is not None:
        args.ws, args.ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    args.ring, args.k_shares = ring, (k_shares or (K_SHARES if not a_trans else 0))
    args.A, args.B, args.C, args.C2 = _p(a), _p(b), _p(out), _p(out2)
    args.bias, args.pos, args.scale, args.keep_n = _p(bias), _p(pos), _p(scale), _p(keep_n)
    args.resid, args.dact_u, args.bias_grad, args.keep_k = _p(resid), _p(dact_u), _p(bias_grad), _p(keep_k)
    args.n_period, args.k_period, args.sched = n_period, k_period, sched
    mg = M_GROUPS[0] if m_groups is None else m_groups      # (closures launched later pass the value of their own forward / backward)
    args.m_groups = mg if ((keep_k is not None or keep_n is not None) and rows_in > 0) else 0
    if WRITE_SKIP[0] and (keep_k is not None or keep_n is not None) and rows_in > 0 and (mg <= 1 or args.m_groups > 1):
        args.sched |= SKIP_WRITES_BIT
    args.M, args.N, args.K = M, N, K
    args.lda, args.ldb, args.ldc, args.ldu = lda, ldb, ldc, ldu
    args.a_trans, args.b_trans = int(a_trans), int(b_trans)
    args.in_dtype, args.out_dtype = _dt(a), _dt(out)
    assert b.dtype == a.dtype, "A and B must share a dtype"
    args.act, args.atomic, args.split_k, args.rows_in = act, int(atomic), split_k, rows_in
    args.a_map, args.b_map, args.c_map = _rm(a_map), _rm(b_map), _rm(c_map)
    return args


def gemm_ln_supported(a, N, ldc):
    """vr_gemm_ln covers this Linear (16-bit operands, whole rows in one tile)."""
    return is_fast16(a.dtype) and N == ldc and bool(_lib.lib().vr_gemm_ln_supported(N))


def _kept_flops(M, N, K, rows_in, keep_k, keep_n, k_period=0):
    def kept(keep, dim, period):
        if keep is None:
            return None
        k = keep.detach().to("cpu", torch.float64)
        return torch.clamp(k, min=0, max=period) * (dim // period) if period else torch.clamp(k, min=0, max=dim)
    kk, kn = kept(keep_k, K, k_period), kept(keep_n, N, 0)
    if kk is None and kn is None:
        return 2.0 * M * N * K
    nb = len(kk if kk is not None else kn)
    kk = kk if kk is not None else torch.full((nb,), float(K), dtype=torch.float64)
    kn = kn if kn is not None else torch.full((nb,), float(N), dtype=torch.float64)
    return float((2.0 * rows_in * kk * kn).sum())


def _launch_gemm_ln(args, ln, a, M, N, K, rows_in, keep_k, keep_n, k_period, extra_bytes):
    if PROFILE is None:
        _lib.check(_lib.lib().vr_gemm_ln(ctypes.byref(args), ctypes.byref(ln), _stream()), "vr_gemm_ln")
        return
    flops = _kept_flops(M, N, K, rows_in, keep_k, keep_n, k_period)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_lib.lib().vr_gemm_ln(ctypes.byref(args), ctypes.byref(ln), _stream()), "vr_gemm_ln")
    e1.record()
    # algorithmic bytes from the KEPT widths, like _gemm_work: sample b reads rows x kept K of A; the weights once for the widest
    # sample; the row-wide side tensors (residual stream, LayerNorm output ...) in full
    if keep_k is not None and rows_in > 0:
        kk = torch.clamp(keep_k.detach().to("cpu", torch.float64), min=0, max=k_period) * (K // k_period) if k_period else \
            torch.clamp(keep_k.detach().to("cpu", torch.float64), min=0, max=K)
        a_bytes, k_w = float((rows_in * kk).sum()) * 2, float(kk.max())
    else:
        a_bytes, k_w = float(M) * K * 2, float(K)
    PROFILE.append(((_DTNAMES[args.in_dtype], 0, 0, 2), flops, 2.0 * M * N * K, a_bytes + N * k_w * 2 + extra_bytes, e0, e1))
    if PROFILE_DESC is not None:
        PROFILE_DESC.append("ln%d M%d N%d K%d" % (ln.mode, M, N, K))


def gemm_ln_fwd(a, b, out, ln_w, ln_b, ln_keep, eps, *, M, N, K, lda, ldb, ldc, bias=None, scale=None, keep_n=None,
                resid=None, rows_in=0, keep_k=None, k_period=0, sched=0):
    """out = resid + scale * mask(a @ b^T + bias) (fp32) and (y, mean, rstd) = masked LayerNorm(out) -- vr_gemm_ln mode 0; y in a's
    (16-bit) dtype."""
    args = _gemm_args(a, b, out, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, bias=bias, scale=scale, keep_n=keep_n, resid=resid,
                      rows_in=rows_in, keep_k=keep_k, k_period=k_period, sched=sched)
    y = torch.empty(out.shape, dtype=a.dtype, device=out.device)
    mean = torch.empty(M, dtype=torch.float32, device=out.device)
    rstd = torch.empty(M, dtype=torch.float32, device=out.device)
    ln = LnEpilogue()
    ln.mode, ln.eps = 0, eps
    ln.w, ln.b, ln.keep, ln.y, ln.mean, ln.rstd = _p(ln_w), _p(ln_b), _p(ln_keep), _p(y), _p(mean), _p(rstd)
    _launch_gemm_ln(args, ln, a, M, N, K, rows_in, keep_k, keep_n, k_period, M * N * (4 + 4 + 2))
    return y, mean, rstd


# vr_gemm_ln_fold (rows of several 128-column tiles; narrower rows go to vr_gemm_ln) is OPT-IN: measured round 6 inside the sr_tiny step
# 7.51 against 6.97 ms (52 - 73 us per folded launch against 22 - 35 + 5 - 8 for the two kernels, profiles/r06_ln_fold.txt): the tiles'
# fp32 rows must be visible to a workgroup on ANOTHER XCD inside the launch, i.e. stored write-through (partial-line writes to
# memory) and waited for, and the last arriver's row loop is a tail nothing runs beside.  Set True by tests (the model-level
# parity of the form).
LN_FOLD = False


def gemm_ln_fold_fwd(a, b, out, ln_w, ln_b, ln_keep, eps, *, M, N, K, lda, ldb, ldc, bias=None, scale=None, keep_n=None,
                     resid=None, rows_in=0, keep_k=None, k_period=0, sched=0):
    """gemm_ln_fwd for rows that span several tiles (vr_gemm_ln_fold): out = resid + scale * mask(a @ b^T + bias) (fp32) and
    (y, mean, rstd) = masked LayerNorm(out), one launch of the tiled kernel -- or None (nothing launched) when the form is not
    covered: the caller then issues the Linear and the LayerNorm separately."""
    if not (LN_FOLD and a.is_cuda and a.dtype == torch.bfloat16 and out.dtype == torch.float32 and N == ldc and 256 < N <= 2048 and
            bias is not None and resid is not None and K % 64 == 0):
        return None
    args = _gemm_args(a, b, out, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, bias=bias, scale=scale, keep_n=keep_n, resid=resid,
                      rows_in=rows_in, keep_k=keep_k, k_period=k_period, sched=sched, k_shares=0,
                      ws=_workspace(a.device))
    if not args.ws:
        return None
    y = torch.empty(out.shape, dtype=torch.bfloat16, device=out.device)
    mean = torch.empty(M, dtype=torch.float32, device=out.device)
    rstd = torch.empty(M, dtype=torch.float32, device=out.device)
    ln = LnEpilogue()
    ln.mode, ln.eps = 0, eps
    ln.w, ln.b, ln.keep, ln.y, ln.mean, ln.rstd = _p(ln_w), _p(ln_b), _p(ln_keep), _p(y), _p(mean), _p(rstd)
    if PROFILE is not None:
        flops, alg_bytes = _gemm_work(a, out, M, N, K, False, rows_in, keep_k, keep_n, k_period, 0, resid=resid, bias=bias)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = _lib.lib().vr_gemm_ln_fold(ctypes.byref(args), ctypes.byref(ln), _stream())
    if rc == -3:                                   # VR_EUNSUPPORTED: nothing was launched
        return None
    _lib.check(rc, "vr_gemm_ln_fold")
    if PROFILE is not None:
        e1.record()
        PROFILE.append((("bf16", 0, 0, 0), flops, 2.0 * M * N * K, alg_bytes + M * N * 2, e0, e1))       # (+ the LayerNorm's output)
        if PROFILE_DESC is not None:
            PROFILE_DESC.append("nt+ln M%d N%d K%d bias res%s f32out" % (M, N, K, " scale" if scale is not None else ""))
    return y, mean, rstd


def gemm_ln_bwd(du, wt, x, ln_w, mean, rstd, ln_keep, dx_in, dw, db, next_cast=None, *, M, N, K, lda, ldb, rows_in=0,
                keep_k=None, k_period=0, copies=1, sched=0):
    """LayerNorm backward of dy = du @ wt^T without writing dy -- vr_gemm_ln mode 1; returns dx or (dx, gt) like ln_bwd
    (copies: dw / db are [copies, N] partial rows, see ln_bwd)."""
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    gt = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if next_cast is not None else None
    sc, kp = next_cast if next_cast is not None else (None, None)
    args = _gemm_args(du, wt, dx, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=N, resid=dx_in, rows_in=rows_in, keep_k=keep_k,
                      k_period=k_period, sched=sched)
    ln = LnEpilogue()
    ln.mode, ln.eps = 1, 0.0
    ln.w, ln.keep, ln.mean, ln.rstd, ln.x = _p(ln_w), _p(ln_keep), _p(mean), _p(rstd), _p(x)
    ln.dw, ln.db, ln.gt_out, ln.gt_scale, ln.gt_keep = _p(dw), _p(db), _p(gt), _p(sc), _p(kp)
    ln.grad_copies = copies
    _launch_gemm_ln(args, ln, du, M, N, K, rows_in, keep_k, ln_keep, k_period, M * N * (4 + 4 + 4 + 2))
    return dx if next_cast is None else (dx, gt)


def gemm(a, b, out, *, M, N, K, lda, ldb, ldc, a_trans=False, b_trans=False, out2=None, bias=None, pos=None,
         scale=None, keep_n=None, resid=None, dact_u=None, ldu=0, act=0, atomic=False, split_k=1, rows_in=0,
         a_map=None, b_map=None, c_map=None, bias_grad=None, keep_k=None, n_period=0, k_period=0, sched=0, ws="auto",
         ring=0, k_shares=0, m_groups=None, sr_pool=None, keep_out=None, tok_rows=None):
    """out[M,N] = epilogue(a[M,K] @ b[N,K]^T) -- see vr_gemm in include/vitres_hip.h.  ws: K-split workspace (a uint8 tensor),
    None, or "auto" = the current role's (see _workspace).  sr_pool / keep_out / tok_rows: see _gemm_args."""
    args = _gemm_args(a, b, out, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, a_trans=a_trans, b_trans=b_trans, out2=out2,
                      bias=bias, pos=pos, scale=scale, keep_n=keep_n, resid=resid, dact_u=dact_u, ldu=ldu, act=act,
                      atomic=atomic, split_k=split_k, rows_in=rows_in, a_map=a_map, b_map=b_map, c_map=c_map,
                      bias_grad=bias_grad, keep_k=keep_k, n_period=n_period, k_period=k_period, sched=sched, ws=ws,
                      ring=ring, k_shares=k_shares, m_groups=m_groups, sr_pool=sr_pool, keep_out=keep_out, tok_rows=tok_rows)
    if DBG_POISON and (args.sched & SKIP_WRITES_BIT) and keep_n is not None and not a_trans and resid is None and \
            is_fast16(out.dtype):
        out.fill_(float("nan"))
        if out2 is not None:
            out2.fill_(float("nan"))
    if PROFILE is None:
        _lib.check(_lib.lib().vr_gemm(ctypes.byref(args), _stream()), "vr_gemm")
        return out
    flops, alg_bytes = _gemm_work(a, out, M, N, K, a_trans, rows_in, keep_k, keep_n, k_period, n_period, out2=out2, resid=resid,
                                  dact_u=dact_u, pos=pos, bias=bias, atomic=atomic,
                                  skip_writes=bool(args.sched & SKIP_WRITES_BIT))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_lib.lib().vr_gemm(ctypes.byref(args), _stream()), "vr_gemm")
    e1.record()
    PROFILE.append(((_DTNAMES[args.in_dtype], int(a_trans), int(b_trans),
                     int(a_map is not None or b_map is not None)), flops, 2.0 * M * N * K, alg_bytes, e0, e1))
    if PROFILE_DESC is not None:
        PROFILE_DESC.append("%s M%d N%d K%d%s%s%s%s%s%s%s" % (
            "tn" if a_trans else ("nn" if b_trans else "nt"), M, N, K, " act%d" % act if act else "", " bias" if bias is not None else "",
            " res" if resid is not None else "", " scale" if scale is not None else "", " dact" if dact_u is not None else "",
            " map" if (a_map or b_map or c_map) else "", " f32out" if out.dtype == torch.float32 and not a_trans else ""))
    return out


def gemm_group(calls):
    """calls: [(a, b, out, kwargs)] -- the arguments of gemm() for each problem.  One vr_gemm_group launch (weight gradients of
    a transformer block share the CUs); semantics are exactly those of issuing the calls one after the other."""
    if len(calls) == 1:
        a, b, out, kw = calls[0]
        return gemm(a, b, out, **kw)
    arr = (GemmArgs * len(calls))()
    for i, (a, b, out, kw) in enumerate(calls):
        arr[i] = _gemm_args(a, b, out, **kw)
    if PROFILE is None:
        _lib.check(_lib.lib().vr_gemm_group(arr, len(calls), _stream()), "vr_gemm_group")
        return
    flops = dense = alg = 0.0
    for a, b, out, kw in calls:
        f, by = _gemm_work(a, out, kw["M"], kw["N"], kw["K"], kw.get("a_trans", False), kw.get("rows_in", 0), kw.get("keep_k"),
                           kw.get("keep_n"), kw.get("k_period", 0), kw.get("n_period", 0), atomic=kw.get("atomic", False))
        flops, dense, alg = flops + f, dense + 2.0 * kw["M"] * kw["N"] * kw["K"], alg + by
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_lib.lib().vr_gemm_group(arr, len(calls), _stream()), "vr_gemm_group")
    e1.record()
    a0, kw0 = calls[0][0], calls[0][3]
    PROFILE.append(((_DTNAMES[_dt(a0)], int(kw0.get("a_trans", False)),
                     int(kw0.get("b_trans", False)), 0), flops, dense, alg, e0, e1))
    if PROFILE_DESC is not None:
        PROFILE_DESC.append("group " + " + ".join("M%d N%d K%d" % (kw["M"], kw["N"], kw["K"]) for _, _, _, kw in calls))


def _written_cols(keep_n, N, n_period, BN=128):
    """Per sample: the output columns a launch under SKIP_WRITES_BIT actually stores -- the BN-wide column tiles that hold a kept
    column for the sample's architecture GROUP (gemm_ntk.hip: a tile beyond the group's width is not written; a DropPath-dropped
    sample, marked -(k + 2), still gets its group's width k: its zeros below k are stored)."""
    gw = keep_n.detach().to("cpu", torch.int64)
    gw = torch.where(gw < 0, -gw - 2, gw)
    out = torch.zeros(gw.shape, dtype=torch.float64)
    for w in set(gw.tolist()):
        cols = 0
        for n0 in range(0, N, BN):
            ln = min(BN, N - n0)
            if w <= 0:
                live = False
            elif n_period <= 0:
                live = n0 < w
            else:
                r = n0 % n_period
                live = r < w or r + ln > n_period
            cols += ln if live else 0
        out[gw == w] = cols
    return out


def _gemm_work(a, out, M, N, K, a_trans, rows_in, keep_k, keep_n, k_period, n_period, out2=None, resid=None, dact_u=None,
               pos=None, bias=None, atomic=False, skip_writes=False):
    """(kept FLOPs, algorithmic HBM bytes) of one vr_gemm launch, both from the KEPT (un-masked) widths of the samples it
    touches -- skipped work is never counted, and neither are operand bytes the masks let the kernel skip.
      forward / dgrad (C[M,N] = A[M,K] B[N,K]^T): sample b reads rows_in x kk[b] of A; the weights are read once for the widest
        sample: max(kk) x max(kn).  Outputs and epilogue side tensors (fp32 residual, saved gelu', second output): a launch that
        stores zeros in masked columns (downstream kernels read whole rows) counts rows_in x N per sample; a launch under
        SKIP_WRITES_BIT (skip_writes: bf16 result, no residual) counts only the 128-column tiles its architecture group keeps
        (_written_cols) -- a fully masked tile is neither written nor is its saved gelu' read, a dropped layer counts nothing;
      wgrad (C[M,N] += A[T,M]^T B[T,N], a_trans): sample b reads rows_in x (kr[b] + kc[b]) channels; C (fp32) is read-modified-
        written once over its widest kept block."""
    esz, osz = a.element_size(), out.element_size()

    def kept(keep, dim, period):
        if keep is None:
            return None
        k = keep.detach().to("cpu", torch.float64)
        return torch.clamp(k, min=0, max=period) * (dim // period) if period else torch.clamp(k, min=0, max=dim)
    if a_trans:                                   # wgrad: keep_k bounds output rows (M), keep_n output columns (N); K = tokens
        kr, kc = kept(keep_k, M, k_period), kept(keep_n, N, n_period)
        if kr is None and kc is None:
            return 2.0 * M * N * K, float(K * (M + N) * esz + 2 * M * N * 4)
        nb = len(kr if kr is not None else kc)
        kr = kr if kr is not None else torch.full((nb,), float(M), dtype=torch.float64)
        kc = kc if kc is not None else torch.full((nb,), float(N), dtype=torch.float64)
        flops = float((2.0 * rows_in * kr * kc).sum())
        return flops, float((rows_in * (kr + kc)).sum() * esz + 2 * float(kr.max()) * float(kc.max()) * 4)
    kk, kn = kept(keep_k, K, k_period), kept(keep_n, N, n_period)
    per_elem = osz + (osz if out2 is not None else 0) + (4 if resid is not None else 0) + (esz if dact_u is not None else 0)
    if kk is None and kn is None:
        return 2.0 * M * N * K, float((M * K + N * K) * esz + M * N * per_elem)
    nb = len(kk if kk is not None else kn)
    kk = kk if kk is not None else torch.full((nb,), float(K), dtype=torch.float64)
    kn = kn if kn is not None else torch.full((nb,), float(N), dtype=torch.float64)
    flops = float((2.0 * rows_in * kk * kn).sum())
    if skip_writes and keep_n is not None and rows_in > 0 and resid is None and osz == 2:
        out_bytes = float((rows_in * _written_cols(keep_n, N, n_period)).sum()) * per_elem
    else:
        out_bytes = float(M) * N * per_elem
    return flops, float((rows_in * kk).sum() * esz + float(kk.max()) * float(kn.max()) * esz + out_bytes)


def zero_ranges(buf, ranges, gate=None):
    """buf[lo:hi] = 0 for every (lo, hi) of `ranges` (fp32 buffer; one launch per 24 ranges) -- vr_zero_ranges.
    gate: a device int32 tensor whose first element decides at run time whether the launch does anything (0: the buffer keeps its
    contents) -- vr_zero_ranges_gated, for a captured graph that serves every micro-step of a gradient-accumulation window."""
    ranges = [(int(lo), int(hi)) for lo, hi in ranges if hi > lo]
    if gate is not None:
        assert gate.dtype == torch.int32 and gate.device == buf.device and gate.numel() >= 1
    for i in range(0, len(ranges), _lib.MAX_ZERO_RANGES):
        chunk = ranges[i:i + _lib.MAX_ZERO_RANGES]
        zr = _lib.ZeroRanges()
        zr.n = len(chunk)
        for j, (lo, hi) in enumerate(chunk):
            zr.lo[j], zr.count[j] = lo, hi - lo
        if gate is not None:
            _lib.check(_lib.lib().vr_zero_ranges_gated(_p(buf), ctypes.byref(zr), _p(gate), _stream()), "vr_zero_ranges_gated")
        else:
            _lib.check(_lib.lib().vr_zero_ranges(_p(buf), ctypes.byref(zr), _stream()), "vr_zero_ranges")
    return buf


def zero_(t):
    """t[...] = 0 for a contiguous fp32 / bf16 tensor (vr_zero_ranges on its storage viewed as fp32 words)."""
    if t.numel() == 0:
        return t
    nbytes = t.numel() * t.element_size()
    if not t.is_contiguous() or nbytes % 4 or t.data_ptr() % 4:
        raise ValueError("zero_: contiguous, 4-byte sized and aligned tensors only")
    zr = _lib.ZeroRanges()
    zr.n, zr.lo[0], zr.count[0] = 1, 0, nbytes // 4
    _lib.check(_lib.lib().vr_zero_ranges(_p(t), ctypes.byref(zr), _stream()), "vr_zero_ranges")
    return t


def relayout(src, dst, A, B, C, dst_ld=None, src_ld=None):
    """dst[a, c, b] = src[a, b, c] (flat: dst[a * dst_ld + c * B + b] = src[a * src_ld + b * C + c]); fp32 / bf16 either side --
    vr_relayout.  Pad columns (dst_ld > B * C) keep their contents."""
    dst_ld = B * C if dst_ld is None else dst_ld
    src_ld = B * C if src_ld is None else src_ld
    _lib.check(_lib.lib().vr_relayout(_p(src), _p(dst), A, B, C, src_ld, dst_ld, _dt(src), _dt(dst), _stream()), "vr_relayout")
    return dst


def relayout_add(src, dst, A, B, C, dst_ld=None, src_ld=None):
    """dst[a, c, b] += src[a, b, c], fp32 both sides, relayout()'s index map -- vr_relayout_add.  A = B = 1: dst += src (flat)."""
    if src.dtype != torch.float32 or dst.dtype != torch.float32:
        raise ValueError("relayout_add: fp32 tensors only")
    dst_ld = B * C if dst_ld is None else dst_ld
    src_ld = B * C if src_ld is None else src_ld
    _lib.check(_lib.lib().vr_relayout_add(_p(src), _p(dst), A, B, C, src_ld, dst_ld, _stream()), "vr_relayout_add")
    return dst


def put_grad(src, dst, A, B, C, src_ld=None, add=False):
    """A gradient that was formed in a temporary goes to its place in the arena: stored (relayout) when the arena was cleared for
    this backward, added (relayout_add) when it holds the sum of earlier micro-steps."""
    return relayout_add(src, dst, A, B, C, src_ld=src_ld) if add else relayout(src, dst, A, B, C, src_ld=src_ld)


def copy_i32_from_pinned(host, dst):
    """dst (device int32) = host (pinned int32) by a KERNEL on the current stream -- vr_relayout reading the mapped host pages -- instead
    of a hipMemcpyAsync: the copy engine's hand-off to and from the compute queue cost ~25 us of idle GPU per training step."""
    assert host.is_pinned() and host.dtype == torch.int32 and dst.dtype == torch.int32 and dst.is_cuda and host.numel() == dst.numel()
    n = host.numel()
    _lib.check(_lib.lib().vr_relayout(host.data_ptr(), dst.data_ptr(), 1, 1, n, n, n, VR_F32, VR_F32, _stream()), "vr_relayout")
    return dst


def cast_bf16(src, dst):
    _lib.check(_lib.lib().vr_cast_f32_bf16(_p(src), _p(dst), src.numel(), _stream()), "vr_cast_f32_bf16")
    return dst


def cast_f16(src, dst):
    _lib.check(_lib.lib().vr_cast_f32_f16(_p(src), _p(dst), src.numel(), _stream()), "vr_cast_f32_f16")
    return dst


def cast16(src, dst):
    """fp32 -> dst's 16-bit dtype (bf16 or fp16), round to nearest even."""
    return cast_f16(src, dst) if dst.dtype == torch.float16 else cast_bf16(src, dst)


def tr_descs(entries, device):
    """entries: [(src_off, dst_off, rows, cols, ld_dst)] -> (device descriptor array for cast_transpose_batch, max tiles)."""
    import numpy as np
    arr = np.zeros(len(entries), dtype=np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("rows", "<i4"), ("cols", "<i4"),
                                                 ("ld_dst", "<i4"), ("reserved", "<i4")]))
    for i, (so, do, r, c, ld) in enumerate(entries):
        arr[i] = (so, do, r, c, ld, 0)
    max_tiles = max(((r + 63) // 64) * ((c + 63) // 64) for _, _, r, c, _ in entries)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), max_tiles, list(entries)


def cast_transpose_batch(src, dst, descs):
    """dst (bf16, pre-zeroed pads) <- transposed bf16 copies of the fp32 matrices described by tr_descs()."""
    dev, max_tiles, entries = descs
    _lib.check(_lib.lib().vr_cast_transpose_batch(_p(src), _p(dst), _p(dev), len(entries), max_tiles, _stream()),
               "vr_cast_transpose_batch")
    return dst


def ln_fwd(x, w, b, keep, rows_per_sample, eps, out_dtype):
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().vr_ln_fwd(_p(x), _p(w), _p(b), _p(y), _p(mean), _p(rstd), _p(keep), M, C, rows_per_sample,
                                    eps, _dtcode(out_dtype), _stream()), "vr_ln_fwd")
    return y, mean, rstd


def ln_bwd(dy, x, w, mean, rstd, keep, rows_per_sample, dx_in, dw, db, next_cast=None, copies=1):
    """next_cast = (scale or None, keep or None): also return scale_mask_cast(dx, scale, keep) in dy's dtype (the gradient
    entering the next backward branch), produced in the same pass.
    copies > 1: dw / db are [copies, C] rows of partial sums that ln_grad_reduce folds into the parameter gradients."""
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    gt = torch.empty(x.shape, dtype=dy.dtype, device=x.device) if next_cast is not None else None
    sc, kp = next_cast if next_cast is not None else (None, None)
    _lib.check(_lib.lib().vr_ln_bwd(_p(dy), _p(x), _p(w), _p(mean), _p(rstd), _p(keep), _p(dx_in), _p(dx), _p(dw), _p(db),
                                    _p(gt), _p(sc), _p(kp), M, C, rows_per_sample, _dt(dy), copies, _stream()), "vr_ln_bwd")
    return dx if next_cast is None else (dx, gt)


def ln_bwd_sr(dcol, dy_tok, gout, x, w, mean, rstd, keep, g, num_tokens, dw, db, next_cast=None, copies=1):
    """ln_bwd of a spatial-reduction block's LayerNorm with col2im (patch rows of dy from dcol), the token rows of dy (dy_tok
    [B * num_tokens, C]) and the pooled shortcut's gradient (dx_in from gout [B, No, Cout]) read in place (vr_ln_bwd_sr; bf16)."""
    B, Ni, C = x.shape
    assert Ni == num_tokens + g * g and dcol.dtype == torch.bfloat16 and dy_tok.dtype == torch.bfloat16
    assert dcol.numel() == B * (g // 2) ** 2 * 9 * C and dy_tok.numel() == B * num_tokens * C and gout.shape[0] == B
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    gt = torch.empty(x.shape, dtype=dcol.dtype, device=x.device) if next_cast is not None else None
    sc, kp = next_cast if next_cast is not None else (None, None)
    _lib.check(_lib.lib().vr_ln_bwd_sr(_p(dcol), _p(dy_tok), _p(gout), _p(x), _p(w), _p(mean), _p(rstd), _p(keep), _p(dx), _p(dw),
                                       _p(db), _p(gt), _p(sc), _p(kp), B, g, C, gout.shape[-1], num_tokens, copies, _stream()),
               "vr_ln_bwd_sr")
    return dx if next_cast is None else (dx, gt)


def ln_grad_reduce(slots, copies):
    """slots: (part_w [copies, C], part_b [copies, C], dw [C], db [C]) per LayerNorm -- dw += part_w.sum(0), db likewise, and
    the partial rows are zero again (vr_ln_grad_reduce)."""
    if not slots:
        return
    arr = (_lib.LnGradSlot * len(slots))()
    for i, (pw, pb, dw, db) in enumerate(slots):
        C = dw.numel()
        assert pw.numel() == copies * C and pb.numel() == copies * C and db.numel() == C
        assert pw.is_contiguous() and pb.is_contiguous() and dw.is_contiguous() and db.is_contiguous()
        arr[i].part_w, arr[i].part_b, arr[i].dw, arr[i].db, arr[i].C = _p(pw), _p(pb), _p(dw), _p(db), C
    _lib.check(_lib.lib().vr_ln_grad_reduce(arr, len(slots), copies, _stream()), "vr_ln_grad_reduce")


def _attn_profiled(call, keep_hd, B, N, H, D, passes):
    """bench.py's `roofline.blocks_mfma_util`: kept FLOPs (4 N^2 per kept head channel and pass pair) and HIP events of one launch."""
    kept = float(keep_hd.clamp(min=0).sum().item()) if keep_hd is not None else float(B * H * D)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    PROFILE_ATTN.append((passes * 2.0 * N * N * kept, e0, e1))


def attn_fwd(qkv, keep_hd, B, N, H, D, scale):
    o = torch.empty((B, N, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    call = lambda: _lib.check(_lib.lib().vr_attn_fwd(_p(qkv), _p(o), _p(lse), _p(keep_hd), B, N, H, D, scale, _dt(qkv), _stream()),
                              "vr_attn_fwd")
    if PROFILE_ATTN is None:
        call()
    else:
        _attn_profiled(call, keep_hd, B, N, H, D, 2)                # Q K^T and P V
    return o, lse


def attn_bwd(qkv, o, d_o, lse, keep_hd, B, N, H, D, scale):
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    call = lambda: _lib.check(_lib.lib().vr_attn_bwd(_p(qkv), _p(o), _p(d_o), _p(lse), _p(delta), _p(dqkv), _p(keep_hd), B, N, H, D,
                                                     scale, _dt(qkv), _stream()), "vr_attn_bwd")
    if PROFILE_ATTN is None:
        call()
    else:
        _attn_profiled(call, keep_hd, B, N, H, D, 5)                # S recomputed, dP, dV, dQ, dK
    return dqkv


def softce(logits, target, gscale, want_grad=True):
    K = logits.shape[-1]
    R = logits.numel() // K
    loss_rows = torch.empty(R, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    _lib.check(_lib.lib().vr_softce(_p(logits), _p(target), _p(loss_rows), _p(dlogits), R, K, gscale, _stream()),
               "vr_softce")
    return loss_rows, dlogits


def softce_train(logits, target, sample_map, rows_per_sample, loss_acc, grad_dtype):
    """dlogits (grad_dtype, row pitch = classes rounded up to 8, pad zeroed) of mean soft-target CE; loss_acc += the mean."""
    K = logits.shape[-1]
    R = logits.numel() // K
    ld = (K + 7) // 8 * 8
    d = torch.empty((R, ld), dtype=grad_dtype, device=logits.device)
    _lib.check(_lib.lib().vr_softce_train(_p(logits), _p(target), _p(sample_map), rows_per_sample, _p(loss_acc), _p(d), ld,
                                          _dtcode(grad_dtype), R, K, 1.0 / R, 1.0 / R, _stream()), "vr_softce_train")
    return d


# vr_eval_state as int64 words: word 0 holds the bits of the double loss_sum
EVAL_STATE_FIELDS = ("loss_sum", "calls", "rows", "top1", "top5", "dst_top1", "dst_top5", "jnt_top1", "jnt_top5", "reserved")


def eval_state(device):
    """A zeroed vr_eval_state in device memory (one per evaluation)."""
    return torch.zeros(len(EVAL_STATE_FIELDS), dtype=torch.int64, device=device)


def read_eval_state(state):
    """The fields of a vr_eval_state as Python numbers: ONE device-to-host copy (which waits for every eval_metrics queued before it)."""
    host = state.cpu()
    out = dict(zip(EVAL_STATE_FIELDS, host.numpy().tolist()))
    out["loss_sum"] = float(host[:1].view(torch.float64).numpy()[0])
    return out


def eval_metrics(logits, labels, state, logits2=None):
    """vr_eval_metrics: state += {mean CE, top-1 / top-5 hits} of fp32 logits [R, K] against int64 labels [R]; with logits2 (the
    distillation head) also its hits and those of softmax(logits) + softmax(logits2).  Nothing is read back."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError("eval_metrics: logits [R, K] and labels [R] expected, got %s and %s" % (tuple(logits.shape), tuple(labels.shape)))
    if logits.dtype != torch.float32 or labels.dtype != torch.int64 or state.dtype != torch.int64:
        raise TypeError("eval_metrics: fp32 logits, int64 labels and an int64 state (kernels.eval_state) expected")
    if state.numel() != len(EVAL_STATE_FIELDS) or not state.is_contiguous():
        raise ValueError("eval_metrics: state must come from kernels.eval_state()")
    R, K = logits.shape
    if logits.stride(1) != 1 and K > 1:
        logits = logits.contiguous()
    ld = logits.stride(0) if R > 1 else max(logits.stride(0), K)
    if logits2 is not None:
        if logits2.shape != logits.shape or logits2.dtype != torch.float32:
            raise ValueError("eval_metrics: logits2 must have the shape and dtype of logits")
        if (logits2.stride(1) != 1 and K > 1) or (R > 1 and logits2.stride(0) != ld):
            logits2 = logits2.contiguous()
            if ld != K:
                logits, ld = logits.contiguous(), K
    _lib.check(_lib.lib().vr_eval_metrics(_p(logits), _p(logits2), _p(labels.contiguous()), R, K, ld, _p(state), _stream()),
               "vr_eval_metrics")
    return state


def colsum(x, out, M, N, ld, row_map=None):
    _lib.check(_lib.lib().vr_colsum(_p(x), _p(out), M, N, ld, _dt(x), _rm(row_map), _stream()), "vr_colsum")
    return out


def scale_mask_cast(x, scale, keep, rows_per_sample, out_dtype):
    C = x.shape[-1]
    M = x.numel() // C
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _lib.check(_lib.lib().vr_scale_mask_cast(_p(x), _p(out), _p(scale), _p(keep), M, C, rows_per_sample,
                                             _dtcode(out_dtype), _stream()), "vr_scale_mask_cast")
    return out


def token_mean(y, first):
    """[B, N, C] -> [B, C]: mean over tokens first.. (patch_output_type='avg')."""
    B, N, C = y.shape
    out = torch.empty((B, C), dtype=y.dtype, device=y.device)
    _lib.check(_lib.lib().vr_token_mean(_p(y), _p(out), B, N, C, first, _dt(y), _stream()), "vr_token_mean")
    return out


def token_mean_bwd(dmean, dy, first):
    B, N, C = dy.shape
    _lib.check(_lib.lib().vr_token_mean_bwd(_p(dmean), _p(dy), B, N, C, first, _dt(dy), _stream()), "vr_token_mean_bwd")
    return dy


def batchsum(x, out):
    B = x.shape[0]
    inner = x.numel() // B
    _lib.check(_lib.lib().vr_batchsum(_p(x), _p(out), B, inner, _stream()), "vr_batchsum")
    return out


def im2col_patch(img, P, ldk, out_dtype, sample_map=None, out=None):
    """sample_map (int64 [B], device): output sample b is image sample_map[b]; out: a preallocated col matrix."""
    B, Cin, H, W = img.shape
    col = out if out is not None else torch.empty((B * (H // P) * (W // P), ldk), dtype=out_dtype, device=img.device)
    _lib.check(_lib.lib().vr_im2col_patch_map(_p(img), _p(col), _p(sample_map), B, Cin, H, W, P, ldk, _dtcode(out_dtype),
                                              _stream()), "vr_im2col_patch_map")
    return col


def embed_cls(tokens, pos, x, keep, num_tokens=1):
    """token rows 0..num_tokens-1 of x [B, N, C] <- tokens + pos (masked)."""
    B, N, C = x.shape
    _lib.check(_lib.lib().vr_embed_cls(_p(tokens), _p(pos), _p(x), _p(keep), B, N, C, num_tokens, _stream()), "vr_embed_cls")
    return x


def sr_im2col(y, B, g, C, num_tokens=1):
    col = torch.empty((B * (g // 2) ** 2, 9 * C), dtype=y.dtype, device=y.device)
    _lib.check(_lib.lib().vr_sr_im2col(_p(y), _p(col), B, g, C, num_tokens, _dt(y), _stream()), "vr_sr_im2col")
    return col


def sr_col2im(dcol, dy, B, g, C, num_tokens=1):
    _lib.check(_lib.lib().vr_sr_col2im(_p(dcol), _p(dy), B, g, C, num_tokens, _dt(dcol), _stream()), "vr_sr_col2im")
    return dy


def sr_resid(x, B, g, cin, cout, num_tokens=1):
    out = torch.empty((B, num_tokens + (g // 2) ** 2, cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().vr_sr_resid(_p(x), _p(out), B, g, cin, cout, num_tokens, _stream()), "vr_sr_resid")
    return out


def sr_resid_bwd(dout, B, g, cin, cout, num_tokens=1):
    dx = torch.empty((B, num_tokens + g * g, cin), dtype=torch.float32, device=dout.device)
    _lib.check(_lib.lib().vr_sr_resid_bwd(_p(dout), _p(dx), B, g, cin, cout, 0, num_tokens, _stream()), "vr_sr_resid_bwd")
    return dx


def mask_rows(x, keep, rows_per_sample):
    C = x.shape[-1]
    M = x.numel() // C
    _lib.check(_lib.lib().vr_mask_rows(_p(x), _p(keep), M, C, rows_per_sample, _stream()), "vr_mask_rows")
    return x


# ---- convolutional patch embedding (stem.hip) ---------------------------------------------------------------
def im2col3x3_image(img, stride, ld, out_dtype):
    B, C, H, W = img.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    col = torch.empty((B * Ho * Wo, ld), dtype=out_dtype, device=img.device)
    _lib.check(_lib.lib().vr_im2col3x3(_p(img), _p(col), B, H, W, C, stride, 1, ld, _dtcode(out_dtype), _stream()),
               "vr_im2col3x3")
    return col


def im2col3x3(a, B, H, W, C):
    col = torch.empty((B * H * W, 9 * C), dtype=a.dtype, device=a.device)
    _lib.check(_lib.lib().vr_im2col3x3(_p(a), _p(col), B, H, W, C, 1, 0, 9 * C, _dt(a), _stream()), "vr_im2col3x3")
    return col


def conv3x3_supported(a, Cin, Cout):
    return is_fast16(a.dtype) and Cin in (16, 24, 32) and Cout <= 32 and Cout % 4 == 0


def conv3x3(a, w, B, H, W, Cin, Cout, out_dtype):
    """Direct 3x3 / stride 1 / pad 1 convolution: a bf16 NHWC [B*H*W, Cin], w bf16 [Cout, 9*Cin] (kh, kw, ci) -> [B*H*W, Cout]."""
    out = torch.empty((B * H * W, Cout), dtype=out_dtype, device=a.device)
    _lib.check(_lib.lib().vr_conv3x3(_p(a), _p(w), _p(out), B, H, W, Cin, Cout, _dtcode(out_dtype), _stream()), "vr_conv3x3")
    return out


def conv3x3_res(a, w, res, B, H, W, Cin, Cout, out_dtype):
    """conv3x3(a, w) + res (bf16 [B*H*W, Cout]) in one pass -- vr_conv3x3_res."""
    out = torch.empty((B * H * W, Cout), dtype=out_dtype, device=a.device)
    _lib.check(_lib.lib().vr_conv3x3_res(_p(a), _p(w), _p(res), _p(out), B, H, W, Cin, Cout, _dtcode(out_dtype), _stream()),
               "vr_conv3x3_res")
    return out


def conv3x3_res_patch(a, w, res_col, B, H, W, Cin, Cout, res_patch, out_dtype):
    """conv3x3_res with `res` in patch order ([B*(H/p)*(W/p), p*p*Cout], patch_unfold's layout) -- vr_conv3x3_res_patch."""
    out = torch.empty((B * H * W, Cout), dtype=out_dtype, device=a.device)
    _lib.check(_lib.lib().vr_conv3x3_res_patch(_p(a), _p(w), _p(res_col), _p(out), B, H, W, Cin, Cout, _dtcode(out_dtype), res_patch,
                                               _stream()), "vr_conv3x3_res_patch")
    return out


def conv_w_flip(w, out_dtype):
    """Weights of the data-gradient convolution of a 3x3 / stride 1 / pad 1 Conv2d: [Ci, (kh, kw, co)] = w[co, ci, 2-kh, 2-kw]."""
    Co, Ci = w.shape[0], w.shape[1]
    out = torch.empty((Ci, 9 * Co), dtype=out_dtype, device=w.device)
    _lib.check(_lib.lib().vr_conv_w_flip(_p(w), _p(out), Co, Ci, _dtcode(out_dtype), _stream()), "vr_conv_w_flip")
    return out


def bn_finalize(sq, n, bn, momentum, update_running):
    """(scale, shift, mean, rstd) fp32 [C] of a train-mode BatchNorm2d from its (sum, sum of squares) [2, C]; updates the module's
    running statistics and batch counter in place (vr_bn_finalize)."""
    C = sq.shape[1]
    out = torch.empty((4, C), dtype=torch.float32, device=sq.device)
    rm, rv, nbt = (bn.running_mean, bn.running_var, bn.num_batches_tracked) if update_running else (None, None, None)
    _lib.check(_lib.lib().vr_bn_finalize(_p(sq[0]), _p(sq[1]), int(n), _p(bn.weight.detach()), _p(bn.bias.detach()), float(bn.eps),
                                         float(momentum), _p(rm), _p(rv), _p(nbt), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
                                         C, _stream()), "vr_bn_finalize")
    return out[0], out[1], out[2], out[3]


def conv1_direct_supported(img, w, Cout):
    return img.dtype == torch.float32 and img.shape[1] == 3 and is_fast16(w.dtype) and w.shape[1] == 32 and \
        Cout <= 32 and Cout % 4 == 0


def conv1_direct(img, w, bias, relu, out_dtype):
    """3x3 / stride 2 / pad 1 convolution of the fp32 NCHW image (3 channels): w bf16 [Cout, 32] (kh, kw, c; zero padded)
    -> NHWC [B*Ho*Wo, Cout], optionally relu(. + bias) (vr_conv1_direct)."""
    B, _, H, W = img.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((B * Ho * Wo, Cout), dtype=out_dtype, device=img.device)
    _lib.check(_lib.lib().vr_conv1_direct(_p(img), _p(w), _p(bias), _p(out), B, H, W, Cout, int(bool(relu)), _dtcode(out_dtype),
                                          _stream()), "vr_conv1_direct")
    return out


def conv3x3_bias_relu(a, w, bias, res, B, H, W, Cin, Cout, out_dtype):
    """relu(conv3x3(a, w) + bias[co]) (+ res): the evaluation form with BatchNorm folded into w / bias (vr_conv3x3_bias_relu)."""
    out = torch.empty((B * H * W, Cout), dtype=out_dtype, device=a.device)
    _lib.check(_lib.lib().vr_conv3x3_bias_relu(_p(a), _p(w), _p(bias), _p(res), _p(out), B, H, W, Cin, Cout, _dtcode(out_dtype),
                                               _stream()), "vr_conv3x3_bias_relu")
    return out


def conv3x3_bias_relu_patch(a, w, bias, res, B, H, W, Cin, Cout, patch, out_dtype):
    """conv3x3_bias_relu with the result laid out as patch_unfold would: [B*(H/patch)*(W/patch), patch*patch*Cout]."""
    out = torch.empty((B * (H // patch) * (W // patch), patch * patch * Cout), dtype=out_dtype, device=a.device)
    _lib.check(_lib.lib().vr_conv3x3_bias_relu_patch(_p(a), _p(w), _p(bias), _p(res), _p(out), B, H, W, Cin, Cout, patch,
                                                     _dtcode(out_dtype), _stream()), "vr_conv3x3_bias_relu_patch")
    return out


def conv3x3_wgrad_supported(a, Cin, Cout):
    return a.dtype == torch.bfloat16 and Cin == Cout and Cin in (16, 24, 32)


def conv3x3_wgrad(a, dz, dw, B, H, W, Cin, Cout):
    """dw fp32 [Cout, 9*Cin] (kh, kw, ci) += weight gradient of the 3x3 / stride 1 / pad 1 convolution (a, dz bf16 NHWC)."""
    _lib.check(_lib.lib().vr_conv3x3_wgrad(_p(a), _p(dz), _p(dw), B, H, W, Cin, Cout, _stream()), "vr_conv3x3_wgrad")
    return dw


def col2im3x3(dcol, B, H, W, C):
    d = torch.empty((B * H * W, C), dtype=dcol.dtype, device=dcol.device)
    _lib.check(_lib.lib().vr_col2im3x3(_p(dcol), _p(d), B, H, W, C, _dt(dcol), _stream()), "vr_col2im3x3")
    return d


def bn_stats(z, s, q):
    R, C = z.shape
    _lib.check(_lib.lib().vr_bn_stats(_p(z), _p(s), _p(q), R, C, _dt(z), _stream()), "vr_bn_stats")


def bn_relu(z, scale, shift, res, out_dtype):
    R, C = z.shape
    out = torch.empty((R, C), dtype=out_dtype, device=z.device)
    _lib.check(_lib.lib().vr_bn_relu(_p(z), _p(scale), _p(shift), _p(res), _p(out), R, C, _dtcode(out_dtype), _dt(z), _stream()),
               "vr_bn_relu")
    return out


def bn_bwd(da, z, scale, shift, mean, rstd, sg, sgz, training):
    R, C = z.shape
    dz = torch.empty((R, C), dtype=da.dtype, device=z.device)
    _lib.check(_lib.lib().vr_bn_bwd(_p(da), _p(z), _p(scale), _p(shift), _p(mean), _p(rstd), _p(sg), _p(sgz), _p(dz), R, C,
                                    int(training), _dt(da), _dt(z), _stream()), "vr_bn_bwd")
    return dz


def bn_relu_patch(z, scale, shift, res, B, H, W, patch, out_dtype):
    """bn_relu with the result written as the patchify operand [B*(H/patch)*(W/patch), patch*patch*C] (patch_unfold's layout)."""
    C = z.shape[-1]
    col = torch.empty((B * (H // patch) * (W // patch), patch * patch * C), dtype=out_dtype, device=z.device)
    _lib.check(_lib.lib().vr_bn_relu_patch(_p(z), _p(scale), _p(shift), _p(res), _p(col), B, H, W, patch, C, _dtcode(out_dtype),
                                           _dt(z), _stream()), "vr_bn_relu_patch")
    return col


def bn_bwd_patch(dcol, z, scale, shift, mean, rstd, sg, sgz, training, B, H, W, patch):
    """bn_bwd whose incoming gradient is in patch order (the projection's data gradient as its GEMM leaves it); dz is NHWC."""
    R, C = z.shape
    dz = torch.empty((R, C), dtype=dcol.dtype, device=z.device)
    _lib.check(_lib.lib().vr_bn_bwd_patch(_p(dcol), _p(z), _p(scale), _p(shift), _p(mean), _p(rstd), _p(sg), _p(sgz), _p(dz), B, H, W,
                                          patch, C, int(training), _dt(dcol), _dt(z), _stream()), "vr_bn_bwd_patch")
    return dz


def patch_unfold(a, B, gh, gw, P, C):
    col = torch.empty((B * gh * gw, P * P * C), dtype=a.dtype, device=a.device)
    _lib.check(_lib.lib().vr_patch_unfold(_p(a), _p(col), B, gh, gw, P, C, 0, _dt(a), _stream()), "vr_patch_unfold")
    return col


def patch_fold(col, B, gh, gw, P, C):
    a = torch.empty((B * gh * P * gw * P, C), dtype=col.dtype, device=col.device)
    _lib.check(_lib.lib().vr_patch_unfold(_p(a), _p(col), B, gh, gw, P, C, 1, _dt(col), _stream()), "vr_patch_unfold")
    return a


IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def norm_constants(mean, std):
    """(mean, std) in 0..1 units -> two ctypes float arrays in uint8 units: x * 255 in Python doubles, then rounded to fp32
    (timm's PrefetchLoader: torch.tensor([x * 255 for x in mean])).  Host memory: the kernels take them by value."""
    mean, std = [float(m) * 255 for m in mean], [float(s) * 255 for s in std]
    if len(mean) != len(std) or not 1 <= len(mean) <= 4:
        raise ValueError("mean and std need one entry per channel, at most 4 (got %d and %d)" % (len(mean), len(std)))
    arr = ctypes.c_float * len(mean)
    return arr(*mean), arr(*std)


# ---- what every wrapper of the input route does before it launches, each paragraph once ------------------------------------------------
def _out(what, out, shape, dtype, dev, name="out"):
    """The result tensor: a fresh one, or the caller's `name`= once it is contiguous, of that dtype and shape, on dev."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != dev:
        raise ValueError("%s: %s must be a contiguous %s tensor of shape %s on %s" % (what, name, dtype, tuple(shape), dev))
    return out


def _upload_i32(array, dev):
    host = torch.empty(array.shape, dtype=torch.int32, pin_memory=torch.device(dev).type == "cuda")
    host.numpy()[...] = array
    return host.to(dev, non_blocking=True)


def _dev_table(what, name, table, shape, dev):
    """A table the caller keeps on the device (and has checked): contiguous int32 of `shape` on dev; None in shape: any extent."""
    if table.dtype != torch.int32 or table.dim() != len(shape) or any(n is not None and n != m for n, m in zip(shape, table.shape)) \
            or not table.is_contiguous() or table.device != dev:
        raise ValueError("%s: a device %s must be a contiguous int32 %s tensor on %s" % (
            what, name, list("any" if n is None else n for n in shape), dev))
    return table


def _table(what, name, table, shape, dev, check):
    """A device table as it is (_dev_table), a host table through check() -- the function that returns it as the int32 array the
    device reads, or raises -- and then from pinned memory on the current stream without a host wait."""
    if isinstance(table, torch.Tensor):
        return _dev_table(what, name, table, shape, dev)
    return _upload_i32(check(table), dev)


def _u8_workspace(what, workspace, need, dev):
    """A launch's scratch bytes: `need` of them from torch's allocator, or the caller's uint8 tensor (the entry checks its size)."""
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != dev:
        raise ValueError("%s: the workspace is a contiguous uint8 tensor on %s" % (what, dev))
    return workspace


def _labels(labels, dev):
    return labels.to(dev).long().contiguous()


def _f32(v):
    return float(np.float32(v))               # torch rounds python scalars to fp32


def normalize_u8(u8, mean, std, out=None):
    """vr_normalize_u8: uint8 [B,C,H,W] -> fp32 (float(u) - mean[c] * 255) / (std[c] * 255), timm's PrefetchLoader statement bit
    for bit.  mean / std: per-channel sequences in 0..1 units, or the pair norm_constants() made of them; out: a preallocated
    contiguous fp32 tensor of the same shape."""
    return _normalize_u8(u8, mean, std, None, out)


def normalize_u8_erase(u8, mean, std, erase, out=None):
    """vr_normalize_u8_erase: normalize_u8 with the erase folded into the pass -- the bits of normalize_u8 then random_erase."""
    return _normalize_u8(u8, mean, std, erase, out)


def _normalize_u8(u8, mean, std, erase, out):
    what = "normalize_u8" if erase is None else "normalize_u8_erase"
    if u8.dtype != torch.uint8 or u8.dim() != 4:
        raise TypeError("%s: a uint8 [B,C,H,W] tensor expected, got %s %s" % (what, u8.dtype, tuple(u8.shape)))
    if not isinstance(mean, ctypes.Array):
        mean, std = norm_constants(mean, std)
    B, C, H, W = u8.shape
    if len(mean) != C:
        raise ValueError("%s: %d channels but %d normalisation constants" % (what, C, len(mean)))
    if erase is not None:
        check_erase_rects(erase["rects"], B, H, W, "vr_" + what)
    _p(u8)                                                         # (a CPU tensor is refused before anything is allocated)
    u8 = u8.contiguous()
    out = _out(what, out, (B, C, H, W), torch.float32, u8.device)
    args = (_p(u8), _p(out), B, C, H, W, mean, std)
    if erase is None:
        _lib.check(_lib.lib().vr_normalize_u8(*args, _stream()), "vr_" + what)
    else:
        ea, _keep = _erase_struct(erase, u8.device, "vr_" + what)
        _lib.check(_lib.lib().vr_normalize_u8_erase(*args, ctypes.byref(ea), _stream()), "vr_" + what)
    return out


# one row of the device table of vr_mixup / vr_mixup_u8 (vr_mixup_param of include/vitres_hip.h, 32 bytes)
MIXUP_PARAM = np.dtype([("lam", "<f4"), ("oml", "<f4"), ("y0", "<i4"), ("y1", "<i4"), ("x0", "<i4"), ("x1", "<i4"),
                        ("cutmix", "<i4"), ("pad", "<i4")])
assert MIXUP_PARAM.itemsize == ctypes.sizeof(_lib.MixupParam) == 32


def check_mixup_params(params, B, H, W, what="vr_mixup"):
    """params as a contiguous MIXUP_PARAM array of B rows whose boxes lie inside H x W (an empty box is legal); the device kernel
    cannot report a bad row, so the host copy is what is checked: RuntimeError VR_EINVAL, before anything is launched."""
    params = np.ascontiguousarray(params, dtype=MIXUP_PARAM)
    if params.shape != (B,):
        raise ValueError("%s: the parameter table has shape %s, the batch %d samples" % (what, params.shape, B))
    bad = ((params["y0"] < 0) | (params["y0"] > params["y1"]) | (params["y1"] > H)
           | (params["x0"] < 0) | (params["x0"] > params["x1"]) | (params["x1"] > W))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise RuntimeError("%s failed: %s: the box [%d,%d) x [%d,%d) of sample %d is not inside the %d x %d image" % (
            what, _lib._ERR[-1], params["y0"][i], params["y1"][i], params["x0"][i], params["x1"][i], i, H, W))
    return params


def mixup(x, labels, params, num_classes, on, off, norm=None, out=None, targets_out=None):
    """vr_mixup (fp32 x) / vr_mixup_u8 (uint8 x, norm = the pair norm_constants() made): timm's Mixup / CutMix of sample i with
    sample B-1-i by row i of `params` (a MIXUP_PARAM array: lam and 1 - lam already rounded to fp32 by the rule of the mode that drew
    them, a pixel box, the cutmix flag) and the mixed smoothed one-hot targets of the int64 `labels`; on / off: the one-hot values.
    The table is built in pinned host memory and uploaded on the current stream without a host wait.  Returns (out, targets):
    fresh fp32 tensors, or the contiguous fp32 out= [B,C,H,W] / targets_out= [B,num_classes] written in place; x is not modified."""
    return _mixup(x, labels, params, num_classes, on, off, norm, None, out, targets_out)


def mixup_u8_erase(x, labels, params, num_classes, on, off, norm, erase, out=None, targets_out=None):
    """vr_mixup_u8_erase: mixup() on uint8 x with every sample erased (normalised space, its own rectangles and noise) before it is
    mixed; erase: what erase_args() / RandomErasing.next_args() made.  The same bits as normalize_u8 -> random_erase -> mixup."""
    if norm is None:
        raise TypeError("vr_mixup_u8_erase normalises uint8 samples: norm = the pair norm_constants() made is required")
    return _mixup(x, labels, params, num_classes, on, off, norm, erase, out, targets_out)


def _mixup(x, labels, params, num_classes, on, off, norm, erase, out, targets_out):
    what = "vr_mixup" if norm is None else "vr_mixup_u8" if erase is None else "vr_mixup_u8_erase"
    want = torch.float32 if norm is None else torch.uint8
    if x.dim() != 4 or x.dtype != want:
        raise TypeError("%s: a %s [B,C,H,W] tensor expected, got %s %s" % (what, want, x.dtype, tuple(x.shape)))
    B, C, H, W = x.shape
    params = check_mixup_params(params, B, H, W, what)
    if erase is not None:
        check_erase_rects(erase["rects"], B, H, W, what)
    if norm is not None and len(norm[0]) != C:
        raise ValueError("%s: %d channels but %d normalisation constants" % (what, C, len(norm[0])))
    _p(x)                                                          # (a CPU tensor is refused before anything is allocated)
    x, dev = x.contiguous(), x.device
    out = _out(what, out, (B, C, H, W), torch.float32, dev)
    targets = _out(what, targets_out, (B, num_classes), torch.float32, dev, "targets_out")
    table = _upload_i32(params.view(np.int32).reshape(B, -1), dev)
    labels = _labels(labels, dev)
    args = (_p(x), _p(out), _p(labels), _p(targets), _p(table), B, C, H, W, num_classes, _f32(on), _f32(off))
    if norm is None:
        _lib.check(_lib.lib().vr_mixup(*args, _stream()), what)
    elif erase is None:
        _lib.check(_lib.lib().vr_mixup_u8(*args, norm[0], norm[1], _stream()), what)
    else:
        ea, _keep = _erase_struct(erase, dev, what)
        _lib.check(_lib.lib().vr_mixup_u8_erase(*args, norm[0], norm[1], ctypes.byref(ea), _stream()), what)
    return out, targets


# ---- timm's RandomErasing on the device (vr_random_erase and the *_erase forms of the uint8 entries; vitres/random_erasing.py draws)
ERASE_MODES = {"const": _lib.VR_ERASE_CONST, "rand": _lib.VR_ERASE_RAND, "pixel": _lib.VR_ERASE_PIXEL}
ERASE_MAX_RECTS = 4


def check_erase_rects(rects, B, H, W, what="vr_random_erase"):
    """rects as a contiguous int32 [B, R, 4] array of (y0, y1, x0, x1), 1 <= R <= 4, every rectangle inside H x W (empty ones are
    legal).  As for the Mixup boxes the device cannot report a bad row, so the host copy is what is checked: RuntimeError VR_EINVAL,
    before anything is launched."""
    rects = np.ascontiguousarray(rects, dtype=np.int32)
    if rects.ndim != 3 or rects.shape[0] != B or not 1 <= rects.shape[1] <= ERASE_MAX_RECTS or rects.shape[2] != 4:
        raise ValueError("%s: the rectangle table has shape %s, expected (%d, 1..%d, 4)" % (what, rects.shape, B, ERASE_MAX_RECTS))
    y0, y1, x0, x1 = (rects[..., i] for i in range(4))
    bad = (y0 < 0) | (y0 > y1) | (y1 > H) | (x0 < 0) | (x0 > x1) | (x1 > W)
    if bad.any():
        b, r = (int(v[0]) for v in np.nonzero(bad))
        raise RuntimeError("%s failed: %s: the rectangle [%d,%d) x [%d,%d) (number %d of sample %d) is not inside the %d x %d image"
                           % (what, _lib._ERR[-1], y0[b, r], y1[b, r], x0[b, r], x1[b, r], r, b, H, W))
    return rects


def erase_args(rects, mode, seed, call, device=None):
    """What the erase wrappers take: the host table int32 [B, R, 4] (kept for the check), the mode ('const', 'rand', 'pixel'), the
    64-bit seed and call of the noise contract, and -- with `device` -- the table already on the device, copied from pinned memory on
    the current stream without a host wait (otherwise the wrapper uploads it)."""
    if mode not in ERASE_MODES:
        raise ValueError("erase mode must be one of %s, got %r" % (sorted(ERASE_MODES), mode))
    rects = np.ascontiguousarray(rects, dtype=np.int32)
    args = dict(rects=rects, mode=mode, seed=int(seed) & (2 ** 64 - 1), call=int(call) & (2 ** 64 - 1), table=None)
    if device is not None:
        args["table"] = _upload_i32(rects, device)
    return args


def _erase_struct(erase, dev, what):
    """(the vr_erase_args struct, the device table it points to -- to be kept alive until the launch is issued)"""
    rects = erase["rects"]                                                # (checked by the caller, before it allocated anything)
    table = erase.get("table")
    if table is None or table.device != dev:
        table = _upload_i32(rects, dev)
    _dev_table(what, "rectangle table", table, rects.shape, dev)
    return _lib.EraseArgs(_p(table), rects.shape[1], ERASE_MODES[erase["mode"]], erase["seed"], erase["call"]), table


def random_erase(x, erase):
    """vr_random_erase: timm's RandomErasing on a normalised fp32 [B,C,H,W] batch, IN PLACE, by the rectangles, mode, seed and
    call of `erase` (erase_args() / RandomErasing.next_args()).  Returns x."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("random_erase: a contiguous fp32 [B,C,H,W] tensor expected, got %s %s" % (x.dtype, tuple(x.shape)))
    B, C, H, W = x.shape
    check_erase_rects(erase["rects"], B, H, W)
    _p(x)
    ea, _keep = _erase_struct(erase, x.device, "vr_random_erase")
    _lib.check(_lib.lib().vr_random_erase(_p(x), B, C, H, W, ea.rects, ea.R, ea.mode, ea.seed, ea.call, _stream()), "vr_random_erase")
    return x


def token_mix(x, labels, draw, patch_len, num_classes, on, off, norm=None, erase=None, out=None, targets_out=None,
              patch_targets_out=None):
    """vr_token_mix (fp32 x) / vr_token_mix_u8 (uint8 x, norm = the pair norm_constants() made) / vr_token_mix_u8_erase (erase =
    erase_args() / RandomErasing.next_args() as well): SwitchTokenMix of the batch x by `draw`
    (vitres.token_mixup.SwitchTokenMix.draw: half, partner, the box on the patch_len grid, lam_patch, lam_img); the uint8 forms
    normalise as normalize_u8 does, the erased one erases every sample, in normalised space, before it is mixed -- the bits of
    normalize_u8 -> random_erase -> vr_token_mix.  on / off: the smoothed one-hot values.  Returns (out, targets, patch_targets):
    fresh fp32 tensors, or the contiguous fp32 out= [B,C,H,W] / targets_out= [B,num_classes] / patch_targets_out=
    [B,patch_len^2,num_classes] written in place; x is not modified."""
    if erase is not None and norm is None:
        raise TypeError("vr_token_mix_u8_erase normalises uint8 samples: norm = the pair norm_constants() made is required")
    what = "vr_token_mix" if norm is None else "vr_token_mix_u8" if erase is None else "vr_token_mix_u8_erase"
    want = torch.float32 if norm is None else torch.uint8
    if x.dim() != 4 or x.dtype != want:
        raise TypeError("%s: a %s [B,C,H,W] tensor expected, got %s %s" % (what, want, x.dtype, tuple(x.shape)))
    B, C, H, W = x.shape
    if erase is not None:
        check_erase_rects(erase["rects"], B, H, W, what)
    if norm is not None and len(norm[0]) != C:
        raise ValueError("%s: input_norm has %d channels, the samples %d" % (what, len(norm[0]), C))
    _p(x)                                                          # (a CPU tensor is refused before anything is allocated)
    x, dev, pl = x.contiguous(), x.device, patch_len
    out = _out(what, out, (B, C, H, W), torch.float32, dev)
    targets = _out(what, targets_out, (B, num_classes), torch.float32, dev, "targets_out")
    patch_targets = _out(what, patch_targets_out, (B, pl * pl, num_classes), torch.float32, dev, "patch_targets_out")
    partner = draw["partner"].to(dev, non_blocking=True)
    labels = _labels(labels, dev)
    y0, y1, x0, x1 = draw["box"]
    args = (_p(x), _p(out), _p(labels), _p(partner), _p(targets), _p(patch_targets), B, C, H, W, num_classes, pl, draw["half"], y0, y1,
            x0, x1, _f32(draw["lam_patch"]), _f32(1. - draw["lam_patch"]), _f32(draw["lam_img"]), _f32(1. - draw["lam_img"]), _f32(on),
            _f32(off))
    if norm is None:
        _lib.check(_lib.lib().vr_token_mix(*args, _stream()), what)
    elif erase is None:
        _lib.check(_lib.lib().vr_token_mix_u8(*args, norm[0], norm[1], _stream()), what)
    else:
        ea, _keep = _erase_struct(erase, dev, what)
        _lib.check(_lib.lib().vr_token_mix_u8_erase(*args, norm[0], norm[1], ctypes.byref(ea), _stream()), what)
    return out, targets, patch_targets


def token_mix_u8_erase(x, labels, draw, patch_len, num_classes, on, off, norm, erase, out=None, targets_out=None,
                       patch_targets_out=None):
    """token_mix's erased form under its own name: norm and erase are required."""
    if erase is None:
        raise TypeError("vr_token_mix_u8_erase: erase = erase_args() / RandomErasing.next_args() is required")
    return token_mix(x, labels, draw, patch_len, num_classes, on, off, norm, erase, out, targets_out, patch_targets_out)


# ---- crop + resize + window + mirror of uint8 batches (vr_resample_u8; vitres/resized_crop.py draws the boxes) ---------------------------
RESAMPLE_FILTERS = {"bilinear": _lib.VR_BILINEAR, "bicubic": _lib.VR_BICUBIC, _lib.VR_BILINEAR: _lib.VR_BILINEAR,
                    _lib.VR_BICUBIC: _lib.VR_BICUBIC}
# one row of the device table (vr_resample_box of include/vitres_hip.h, 48 bytes = 12 int32)
RESAMPLE_BOX_FIELDS = ("x0", "y0", "w", "h", "ow", "oh", "wx", "wy", "flip")
RESAMPLE_BOX_INTS = ctypes.sizeof(_lib.ResampleBox) // 4
assert RESAMPLE_BOX_INTS == 12


def _out_size(out_size):
    So_h, So_w = (out_size, out_size) if isinstance(out_size, int) else out_size
    return int(So_h), int(So_w)


def _resample_filter(filter):
    if filter not in RESAMPLE_FILTERS:
        raise ValueError("resample filter must be 'bilinear' (2) or 'bicubic' (3), got %r" % (filter,))
    return RESAMPLE_FILTERS[filter]


def resample_boxes(B):
    """A zeroed host table int32 [B, 12]: columns RESAMPLE_BOX_FIELDS, then three reserved words."""
    return np.zeros((B, RESAMPLE_BOX_INTS), dtype=np.int32)


def check_resample_boxes(boxes, B, Hs, Ws, out_size, what="vr_resample_u8"):
    """boxes as a contiguous int32 [B, 12] array (9 columns are padded with the reserved words) with w, h >= 1, every box inside the
    Hs x Ws canvas and every window inside its (ow, oh).  The device cannot report a bad row, so the host copy is what is checked:
    RuntimeError VR_EINVAL, before anything is launched."""
    return _check_boxes(boxes, B, Hs, Ws, None, out_size, what, "the %d x %d canvas")


def _check_boxes(boxes, B, rows, pitch, max_side, out_size, what, where):
    """The box table of either route as the contiguous int32 [B, 12] array: w, h >= 1 (at most max_side, if given), every box inside
    rows x pitch -- two ints, or one of each per sample -- and every window inside its (ow, oh).  where: how the message names
    those limits."""
    So_h, So_w = _out_size(out_size)
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[0] != B or boxes.shape[1] not in (len(RESAMPLE_BOX_FIELDS), RESAMPLE_BOX_INTS):
        raise ValueError("%s: the box table has shape %s, expected (%d, %d)" % (what, boxes.shape, B, RESAMPLE_BOX_INTS))
    table = resample_boxes(B)
    table[:, :boxes.shape[1]] = boxes
    x0, y0, w, h, ow, oh, wx, wy = (table[:, i].astype(np.int64) for i in range(8))
    rows, pitch = (np.broadcast_to(np.asarray(v, dtype=np.int64), (B,)) for v in (rows, pitch))
    bad = ((w < 1) | (h < 1) | (x0 < 0) | (y0 < 0) | (x0 + w > pitch) | (y0 + h > rows)
           | (wx < 0) | (wy < 0) | (wx + So_w > ow) | (wy + So_h > oh))
    if max_side is not None:
        bad |= (w > max_side) | (h > max_side)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise RuntimeError("%s failed: %s: sample %d: the box x0=%d y0=%d w=%d h=%d must lie inside %s and the %d x %d window at "
                           "(%d, %d) inside the resized %d x %d image" % (what, _lib._ERR[-1], i, x0[i], y0[i], w[i], h[i],
                                                                         where % (rows[i], pitch[i]), So_h, So_w, wy[i], wx[i],
                                                                         oh[i], ow[i]))
    return table


def resample_band_rows(C, Hs, Ws, out_size, filter):
    """Output rows one workgroup of that vr_resample_u8 launch computes (vr_resample_band_rows); RuntimeError where the launch would
    be refused (VR_EUNSUPPORTED: not even a one-row band fits the LDS budget at the launch's worst scale)."""
    So_h, So_w = _out_size(out_size)
    rc = _lib.lib().vr_resample_band_rows(C, Hs, Ws, So_h, So_w, _resample_filter(filter))
    if rc <= 0:
        _lib.check(rc, "vr_resample_band_rows")
    return rc


def resample_u8(src, boxes, out_size, filter, out=None):
    """vr_resample_u8: per sample and channel, bit for bit,
        PIL crop((x0, y0, x0+w, y0+h)).resize((ow, oh), filter).crop((wx, wy, wx+So_w, wy+So_h)) [mirrored left-right if flip]
    of the uint8 canvas batch src [B,C,Hs,Ws] (Ws % 4 == 0) into uint8 [B,C,So_h,So_w] (So_w % 4 == 0).  boxes: a host int array
    [B, 9 or 12] (columns RESAMPLE_BOX_FIELDS) -- checked, then uploaded from pinned memory on the current stream without a host
    wait -- or an int32 [B, 12] DEVICE tensor the caller has checked (check_resample_boxes) and may rewrite in place between replays
    of a captured launch.  out_size: S or (So_h, So_w); filter: 'bilinear' / 'bicubic' or PIL's 2 / 3; out: a preallocated result."""
    if src.dtype != torch.uint8 or src.dim() != 4:
        raise TypeError("resample_u8: a uint8 [B,C,Hs,Ws] tensor expected, got %s %s" % (src.dtype, tuple(src.shape)))
    B, C, Hs, Ws = src.shape
    So_h, So_w = _out_size(out_size)
    code = _resample_filter(filter)
    _p(src)
    table = _table("resample_u8", "box table", boxes, (B, RESAMPLE_BOX_INTS), src.device,
                   lambda t: check_resample_boxes(t, B, Hs, Ws, (So_h, So_w)))
    src = src.contiguous()
    out = _out("resample_u8", out, (B, C, So_h, So_w), torch.uint8, src.device)
    _lib.check(_lib.lib().vr_resample_u8(_p(src), _p(table), _p(out), B, C, Hs, Ws, So_h, So_w, code, None, 0, _stream()),
               "vr_resample_u8")
    return out


# ---- RandAugment on uint8 batches (vr_rand_augment_u8; vitres/rand_augment.py draws the tables) -------------------------------------------
# op kinds of a record (VR_RA_* of include/vitres_hip.h): eleven kinds cover timm's fifteen ops, 'identity' is a drawn op not applied
RA_OPS = {"identity": _lib.VR_RA_IDENTITY, "invert": _lib.VR_RA_INVERT, "posterize": _lib.VR_RA_POSTERIZE,
          "solarize": _lib.VR_RA_SOLARIZE, "solarize_add": _lib.VR_RA_SOLARIZE_ADD, "autocontrast": _lib.VR_RA_AUTOCONTRAST,
          "equalize": _lib.VR_RA_EQUALIZE, "brightness": _lib.VR_RA_BRIGHTNESS, "color": _lib.VR_RA_COLOR,
          "contrast": _lib.VR_RA_CONTRAST, "sharpness": _lib.VR_RA_SHARPNESS, "affine": _lib.VR_RA_AFFINE}
# one record of the device table (vr_ra_op, 64 bytes = 16 int32)
RA_DTYPE = np.dtype([("op", "<i4"), ("filter", "<i4"), ("iarg", "<i4"), ("factor", "<f4"), ("m", "<f8", (6,))])
RA_OP_INTS = ctypes.sizeof(_lib.RaOp) // 4
assert RA_DTYPE.itemsize == ctypes.sizeof(_lib.RaOp) == 64 and RA_OP_INTS == 16
RA_MAX_LAYERS = 4
_RA_IARG = {_lib.VR_RA_POSTERIZE: (0, 8), _lib.VR_RA_SOLARIZE: (0, 256), _lib.VR_RA_SOLARIZE_ADD: (0, 255)}
_RA_BLENDS = (_lib.VR_RA_BRIGHTNESS, _lib.VR_RA_COLOR, _lib.VR_RA_CONTRAST, _lib.VR_RA_SHARPNESS)


def ra_table(B, layers):
    """A host table of B x layers records (RA_DTYPE: op, filter, iarg, factor, m[6]), every record 'identity'."""
    return np.zeros((B, layers), dtype=RA_DTYPE)


def ra_fill(fill):
    """(r, g, b) bytes -> the packed fill word r | g << 8 | b << 16"""
    given, fill = tuple(fill), tuple(int(v) for v in fill)
    if len(fill) != 3 or any(v < 0 or v > 255 or v != g for v, g in zip(fill, given)):
        raise ValueError("rand_augment_u8: fill must be three bytes (r, g, b), got %r" % (given,))
    return fill[0] | fill[1] << 8 | fill[2] << 16


def check_ra_table(table, B, layers=None, what="vr_rand_augment_u8"):
    """table (RA_DTYPE [B, layers]) as the contiguous int32 [B, layers, 16] array the device reads, with every record checked: a known
    op; filter 2 / 3 and a finite matrix for 'affine'; posterize bits 0..8, solarize threshold 0..256, solarize_add addend 0..255;
    a finite factor for the blends.  The device treats a bad record as identity and cannot report it, so the host copy is what is
    checked: RuntimeError VR_EINVAL, before anything is launched."""
    table = np.asarray(table)
    if table.dtype != RA_DTYPE or table.ndim != 2 or table.shape[0] != B or (layers is not None and table.shape[1] != layers) \
            or not 1 <= table.shape[1] <= RA_MAX_LAYERS:
        raise ValueError("%s: the op table must be a %s array of shape (%d, %s), 1..%d layers; got %s %s" % (
            what, "ra_table", B, "layers" if layers is None else layers, RA_MAX_LAYERS, table.dtype, table.shape))
    table = np.ascontiguousarray(table)
    op, filt, iarg = table["op"], table["filter"], table["iarg"]
    bad = (op < 0) | (op > _lib.VR_RA_AFFINE)
    bad |= (op == _lib.VR_RA_AFFINE) & (((filt != _lib.VR_BILINEAR) & (filt != _lib.VR_BICUBIC)) | ~np.isfinite(table["m"]).all(axis=-1))
    for code, (lo, hi) in _RA_IARG.items():
        bad |= (op == code) & ((iarg < lo) | (iarg > hi))
    bad |= np.isin(op, _RA_BLENDS) & ~np.isfinite(table["factor"])
    if bad.any():
        b, k = (int(v[0]) for v in np.nonzero(bad))
        r = table[b, k]
        raise RuntimeError("%s failed: %s: sample %d, layer %d: op=%d filter=%d iarg=%d factor=%r m=%s is not a record the kernel "
                           "applies" % (what, _lib._ERR[-1], b, k, r["op"], r["filter"], r["iarg"], float(r["factor"]), r["m"].tolist()))
    return table.view(np.int32).reshape(B, table.shape[1], RA_OP_INTS)


def rand_augment_u8(src, table, fill, out=None):
    """vr_rand_augment_u8: every sample's records applied in order to the uint8 [B,3,H,W] batch src (W % 4 == 0), bit for bit what PIL
    makes of the RGB image with timm's RandAugment ops (the header states each op).  table: a host RA_DTYPE array [B, layers]
    (ra_table; vitres.rand_augment.RandAugment.draw) -- checked, then uploaded from pinned memory on the current stream without a
    host wait -- or an int32 [B, layers, 16] DEVICE tensor the caller has checked (check_ra_table) and may rewrite in place between
    replays of a captured launch.  fill: the (r, g, b) bytes the affine ops put where they map outside the image; out: a
    preallocated result (not src).  With more than one layer a workspace of the batch's size is taken from torch's allocator."""
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[1] != 3:
        raise TypeError("rand_augment_u8: a uint8 [B,3,H,W] tensor expected, got %s %s" % (src.dtype, tuple(src.shape)))
    B, _, H, W = src.shape
    word = ra_fill(fill)
    _p(src)
    dev_table = _table("rand_augment_u8", "op table", table, (B, None, RA_OP_INTS), src.device, lambda t: check_ra_table(t, B))
    layers = int(dev_table.shape[1])
    src = src.contiguous()
    out = _out("rand_augment_u8", out, src.shape, torch.uint8, src.device)
    L = _lib.lib()
    need = int(L.vr_rand_augment_ws_bytes(B, H, W, layers)) if 1 <= layers <= RA_MAX_LAYERS else 0
    ws = torch.empty(need, dtype=torch.uint8, device=src.device) if need else None
    _lib.check(L.vr_rand_augment_u8(_p(src), _p(dev_table), _p(out), B, H, W, layers, word, _p(ws), need, _stream()),
               "vr_rand_augment_u8")
    return out


# ---- JPEG: the device half of decoding (vr_jpeg_reconstruct_u8; vitres/jpeg.py is the host half, vitres/data.py the loader) ---------------
# one record of the device table (vr_jpeg_desc, 64 bytes = 16 int32)
JPEG_DESC_DTYPE = np.dtype([("kind", "<i4"), ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"),
                            ("off", "<i4", (3,)), ("bw", "<i4", (3,)), ("bh", "<i4", (3,)), ("reserved", "<i4")])
JPEG_DESC_INTS = ctypes.sizeof(_lib.JpegDesc) // 4
assert JPEG_DESC_DTYPE.itemsize == ctypes.sizeof(_lib.JpegDesc) == 64 and JPEG_DESC_INTS == 16
JPEG_MAX_SIDE = 8192
JPEG_OFF_UNIT = 16                         # bytes per unit of vr_jpeg_desc.off


def jpeg_descs(B):
    """A zeroed host table of B records (JPEG_DESC_DTYPE: kind, width, height, ncomp, hs, vs, off[3], bw[3], bh[3])."""
    return np.zeros(B, dtype=JPEG_DESC_DTYPE)


def jpeg_ws_bytes(blob_bytes):
    """vr_jpeg_ws_bytes: the workspace a launch over a blob of that size needs (the component sample planes: half the blob)."""
    n = int(blob_bytes)
    return ((n + 1) // 2 + 15) & ~15 if n > 0 else 0


def check_jpeg_table(descs, blob_bytes, Hs, Ws, what="vr_jpeg_reconstruct_u8"):
    """descs (JPEG_DESC_DTYPE [B], or int32 [B, 16]) as the contiguous int32 [B, 16] array the device reads, with every record
    checked as the device checks it (the header lists the rules: kind, sides inside the canvas and 8192, sampling, block-plane sizes
    that follow from the sides, offsets inside the blob) and, beyond that, no two components overlapping.  The device zeroes the
    image of a bad record and cannot report it, so the host copy is what is checked: RuntimeError VR_EINVAL, before any launch."""
    descs = np.asarray(descs)
    if descs.dtype != JPEG_DESC_DTYPE:
        if descs.dtype != np.int32 or descs.ndim != 2 or descs.shape[1] != JPEG_DESC_INTS:
            raise ValueError("%s: the record table must be a jpeg_descs array or int32 [B, %d], got %s %s" % (
                what, JPEG_DESC_INTS, descs.dtype, descs.shape))
        descs = np.ascontiguousarray(descs).view(JPEG_DESC_DTYPE).reshape(-1)
    if descs.ndim != 1 or descs.shape[0] < 1:
        raise ValueError("%s: the record table must hold one record per image, got shape %s" % (what, descs.shape))
    descs = np.ascontiguousarray(descs)
    kind, W, H, nc, hs, vs = (descs[k].astype(np.int64) for k in ("kind", "width", "height", "ncomp", "hs", "vs"))
    off, bw, bh = (descs[k].astype(np.int64) for k in ("off", "bw", "bh"))
    raw = kind == _lib.VR_JPEG_RAW
    bad = ((kind != _lib.VR_JPEG_COEF) & ~raw) | (W < 1) | (W > min(Ws, JPEG_MAX_SIDE)) | (H < 1) | (H > min(Hs, JPEG_MAX_SIDE))
    samp = (hs == 1) & (vs == 1)
    bad |= raw & ~((nc == 3) & samp)
    bad |= ~raw & ~(((nc == 1) & samp) | ((nc == 3) & (samp | ((hs == 2) & ((vs == 1) | (vs == 2))))))
    hs_, vs_ = np.clip(hs, 1, 2), np.clip(vs, 1, 2)
    mx, my = -(-W // (8 * hs_)), -(-H // (8 * vs_))
    unit = np.where(raw, 64, 128)
    spans = []
    for c in range(3):
        live = c < nc
        size = bw[:, c] * bh[:, c] * unit
        bad |= live & ((bw[:, c] != mx * (hs_ if c == 0 else 1)) | (bh[:, c] != my * (vs_ if c == 0 else 1)) | (off[:, c] < 0)
                       | (off[:, c] * JPEG_OFF_UNIT + size > blob_bytes))
        spans += [(int(off[b, c]) * JPEG_OFF_UNIT, int(size[b]), b) for b in np.flatnonzero(live & ~bad)]
    if not bad.any():
        spans.sort()
        for (lo, n, _), (lo2, _, b2) in zip(spans, spans[1:]):
            if lo + n > lo2:
                bad[b2] = True
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        r = descs[i]
        raise RuntimeError("%s failed: %s: image %d: kind=%d %dx%d ncomp=%d sampling=%dx%d off=%s bw=%s bh=%s is not a record the "
                           "kernel takes for a %d-byte blob and a %d x %d canvas (or it overlaps another)" % (
                               what, _lib._ERR[-1], i, r["kind"], r["width"], r["height"], r["ncomp"], r["hs"], r["vs"],
                               r["off"].tolist(), r["bw"].tolist(), r["bh"].tolist(), blob_bytes, Hs, Ws))
    return descs.view(np.int32).reshape(descs.shape[0], JPEG_DESC_INTS)


def _qtabs(what, qtabs, B, dev):
    """The quantisation tables [B,3,64]: uint16 bits in a 16-bit integer tensor on dev, or a host uint16 array (copied there)."""
    if not isinstance(qtabs, torch.Tensor):
        qtabs = np.ascontiguousarray(qtabs)
        if qtabs.dtype != np.uint16:
            raise TypeError("%s: host quantisation tables are uint16, got %s" % (what, qtabs.dtype))
        qtabs = torch.from_numpy(qtabs.view(np.int16)).to(dev)
    if qtabs.dtype not in (torch.int16, torch.uint16) or tuple(qtabs.shape) != (B, 3, 64) or not qtabs.is_contiguous() \
            or qtabs.device != dev:
        raise ValueError("%s: qtabs must be a contiguous 16-bit integer [%d, 3, 64] tensor on %s" % (what, B, dev))
    return qtabs


def _jpeg_records(what, blob, descs, Hs, Ws):
    """The record table of either reconstruct entry on the device, and its checked host copy (None for a device table the caller
    has checked).  Hs, Ws: the bounds the records are held to."""
    host = None if isinstance(descs, torch.Tensor) else check_jpeg_table(descs, int(blob.numel()), Hs, Ws, "vr_" + what)
    if host is None:
        return _dev_table(what, "record table", descs, (None, JPEG_DESC_INTS), blob.device), None
    return _upload_i32(host, blob.device), host


def _jpeg_workspace(what, blob, workspace):
    return _u8_workspace(what, workspace, int(_lib.lib().vr_jpeg_ws_bytes(int(blob.numel()))), blob.device)


def jpeg_reconstruct_u8(blob, descs, qtabs, Hs, Ws, out=None, workspace=None):
    """vr_jpeg_reconstruct_u8: the batch's coefficient blob (uint8 device tensor, 1-D, as vitres.data.jpeg_collate lays it out) ->
    the uint8 canvas [B,3,Hs,Ws] pad_collate_u8 would have made of PIL's decoded images, bit for bit; every byte of it is written.
    descs: a host table (jpeg_descs / int32 [B, 16]) -- checked (check_jpeg_table), then uploaded from pinned memory on the current
    stream without a host wait -- or an int32 [B, 16] DEVICE tensor the caller has checked.  qtabs: the quantisation tables
    [B,3,64], uint16 bits in an int16 / uint16 tensor on the device, or a host uint16 array.  out: a preallocated canvas; workspace:
    a uint8 device tensor of at least jpeg_ws_bytes(blob.numel()) bytes (taken from torch's allocator when None)."""
    what = "jpeg_reconstruct_u8"
    _flat_u8(blob, what + ": blob")
    _p(blob)
    Hs, Ws = int(Hs), int(Ws)
    table, _host = _jpeg_records(what, blob, descs, Hs, Ws)
    B = int(table.shape[0])
    qtabs = _qtabs(what, qtabs, B, blob.device)
    out = _out(what, out, (B, 3, Hs, Ws), torch.uint8, blob.device)
    workspace = _jpeg_workspace(what, blob, workspace)
    _lib.check(_lib.lib().vr_jpeg_reconstruct_u8(_p(blob), int(blob.numel()), _p(table), _p(qtabs), _p(out), B, Hs, Ws, _p(workspace),
                                                 int(workspace.numel()), _stream()), "vr_" + what)
    return out


# ---- the ragged route: planes of every sample's own size in one flat buffer (vr_jpeg_reconstruct_ragged_u8, vr_resample_ragged_u8) -------
# one record of the device table (vr_ragged_plane, 32 bytes = 8 int32)
RAGGED_PLANE_DTYPE = np.dtype([("off", "<i8"), ("pitch", "<i4"), ("rows", "<i4"), ("ws_off", "<i8"), ("reserved", "<i4", (2,))])
RAGGED_PLANE_INTS = ctypes.sizeof(_lib.RaggedPlane) // 4
assert RAGGED_PLANE_DTYPE.itemsize == ctypes.sizeof(_lib.RaggedPlane) == 32 and RAGGED_PLANE_INTS == 8
RAGGED_MAX_SIDE = 8192
RAGGED_ALIGN = 16                          # a sample's offset in the flat buffer


def ragged_planes(B):
    """A zeroed host table of B records (RAGGED_PLANE_DTYPE: off, pitch, rows, ws_off)."""
    return np.zeros(B, dtype=RAGGED_PLANE_DTYPE)


def ragged_layout(sizes, C=3):
    """(planes, nbytes): the packed layout of images of `sizes` [B,2] (h, w) with C channels -- pitch = the width rounded up to 4,
    rows = the height, every sample on the next multiple of 16; nbytes = the flat buffer's size (a multiple of 16)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    if sizes.ndim != 2 or sizes.shape[1] != 2 or sizes.shape[0] < 1 or (sizes < 1).any():
        raise ValueError("ragged_layout: sizes must hold one positive (h, w) per sample, got shape %s" % (sizes.shape,))
    planes = ragged_planes(sizes.shape[0])
    pitch = (sizes[:, 1] + 3) // 4 * 4
    span = (int(C) * sizes[:, 0] * pitch + RAGGED_ALIGN - 1) // RAGGED_ALIGN * RAGGED_ALIGN
    ends = np.cumsum(span)
    planes["off"], planes["pitch"], planes["rows"] = ends - span, pitch, sizes[:, 0]
    return planes, int(ends[-1])


def _ragged_table(planes, what):
    planes = np.asarray(planes)
    if planes.dtype != RAGGED_PLANE_DTYPE:
        if planes.dtype != np.int32 or planes.ndim != 2 or planes.shape[1] != RAGGED_PLANE_INTS:
            raise ValueError("%s: the plane table must be a ragged_planes array or int32 [B, %d], got %s %s" % (
                what, RAGGED_PLANE_INTS, planes.dtype, planes.shape))
        planes = np.ascontiguousarray(planes).view(RAGGED_PLANE_DTYPE).reshape(-1)
    if planes.ndim != 1 or planes.shape[0] < 1:
        raise ValueError("%s: the plane table must hold one record per sample, got shape %s" % (what, planes.shape))
    return np.ascontiguousarray(planes)


def ragged_bounds(planes):
    """(Hs, Ws): the largest rows and pitch of a host plane table -- the bounds a launch over it declares."""
    planes = _ragged_table(planes, "ragged_bounds")
    return int(planes["rows"].max()), int(planes["pitch"].max())


def check_ragged_planes(planes, C, nbytes, sizes=None, what="vr_resample_ragged_u8"):
    """planes (RAGGED_PLANE_DTYPE [B], or int32 [B, 8]) as the contiguous int32 [B, 8] array the device reads, with every record
    checked as the device checks it -- off >= 0 and a multiple of 16, pitch a multiple of 4, 4 <= pitch, 1 <= rows, both at most
    8192, the C planes inside the nbytes of the flat buffer -- and, beyond that, no two samples overlapping and (sizes [B,2] of
    (h, w) given) every plane holding its image: pitch >= w, rows >= h.  The device writes zeros / nothing for a bad record and
    cannot report it, so the host copy is what is checked: RuntimeError VR_EINVAL, before any launch."""
    planes = _ragged_table(planes, what)
    B = planes.shape[0]
    off, pitch, rows = (planes[k].astype(np.int64) for k in ("off", "pitch", "rows"))
    bad = (off < 0) | (off % RAGGED_ALIGN != 0) | (pitch < 4) | (pitch % 4 != 0) | (pitch > RAGGED_MAX_SIDE) | (rows < 1) \
        | (rows > RAGGED_MAX_SIDE)
    size = int(C) * rows * pitch
    bad |= off + size > int(nbytes)
    if sizes is not None:
        sizes = np.asarray(sizes, dtype=np.int64)
        if sizes.shape != (B, 2):
            raise ValueError("%s: sizes must hold one (h, w) per plane record, got shape %s" % (what, sizes.shape))
        bad |= (sizes[:, 0] < 1) | (sizes[:, 1] < 1) | (sizes[:, 0] > rows) | (sizes[:, 1] > pitch)
    if not bad.any():
        order = np.argsort(off, kind="stable")
        over = off[order][:-1] + size[order][:-1] > off[order][1:]
        bad[order[1:][over]] = True
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise RuntimeError("%s failed: %s: sample %d: the plane record off=%d pitch=%d rows=%d is not one the kernel takes for %d "
                           "channels in a %d-byte buffer%s (or it overlaps another)" % (
                               what, _lib._ERR[-1], i, off[i], pitch[i], rows[i], C, nbytes,
                               "" if sizes is None else " and a %d x %d image" % (sizes[i, 0], sizes[i, 1])))
    return planes.view(np.int32).reshape(B, RAGGED_PLANE_INTS)


def check_ragged_boxes(boxes, planes, out_size, what="vr_resample_ragged_u8"):
    """check_resample_boxes against every sample's OWN plane: w, h >= 1 (at most 8192), the box inside pitch x rows of its record,
    the window inside (ow, oh).  Returns the contiguous int32 [B, 12] table; RuntimeError VR_EINVAL for the first bad row."""
    planes = _ragged_table(planes, what)
    return _check_boxes(boxes, planes.shape[0], planes["rows"], planes["pitch"], RAGGED_MAX_SIDE, out_size, what,
                        "its own %d x %d plane")


def resample_ragged_ws_bytes(C, total_rows, So_w):
    """vr_resample_ragged_ws_bytes: the workspace intermediates packed over heights that sum to total_rows need."""
    C, total_rows, So_w = int(C), int(total_rows), int(So_w)
    return (C * total_rows * So_w + 15) & ~15 if min(C, total_rows, So_w) > 0 else 0


def ragged_ws_offsets(planes, C, So_w, heights=None):
    """Fill the ws_off of a host plane table IN PLACE -- the samples' intermediates [C][height][So_w] packed one after another -- and
    return the workspace bytes they need (resample_ragged_ws_bytes of the heights' sum).  heights: the boxes' heights [B]; None: the
    planes' rows, which bound them (for tables rewritten under a captured launch)."""
    if planes.dtype != RAGGED_PLANE_DTYPE:
        raise ValueError("ragged_ws_offsets fills a ragged_planes array, got %s" % planes.dtype)
    heights = planes["rows"].astype(np.int64) if heights is None else np.asarray(heights, dtype=np.int64)
    if heights.shape != planes.shape or (heights < 1).any():
        raise ValueError("ragged_ws_offsets: one positive height per sample expected")
    span = int(C) * heights * int(So_w)
    planes["ws_off"] = np.cumsum(span) - span
    return resample_ragged_ws_bytes(C, int(heights.sum()), So_w)


def _flat_u8(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
        raise TypeError("%s: a contiguous 1-D uint8 tensor expected" % what)
    return t


def _declared_bytes(what, name, t, declared):
    """How much of the flat buffer t a launch declares to the kernel: all of it, or the caller's figure within it."""
    declared = int(t.numel()) if declared is None else int(declared)
    if not 0 < declared <= t.numel():
        raise ValueError("%s: %s_bytes must be within the %d bytes of %s" % (what, name, t.numel(), name))
    return declared


def jpeg_reconstruct_ragged_u8(blob, descs, qtabs, planes, dst=None, dst_bytes=None, workspace=None, bounds=None):
    """vr_jpeg_reconstruct_ragged_u8: jpeg_reconstruct_u8 into ragged planes -- every image's three planes (rows x pitch bytes each,
    zero outside the image) at its record's place in the flat uint8 buffer dst, bit for bit the bytes of the padded canvas inside
    the image; bytes of dst outside the planes keep their values.  planes: a host table (ragged_planes / ragged_layout; checked
    against the buffer and the records' sizes, then uploaded) or an int32 [B, 8] DEVICE tensor the caller has checked, with
    bounds=(Hs, Ws) >= every record's rows and pitch.  dst: None (a zeroed buffer just large enough is made) or a flat uint8 device
    tensor, of which dst_bytes (default: all) are declared to the kernel.  descs, qtabs, workspace: as jpeg_reconstruct_u8.
    Returns dst."""
    what = "jpeg_reconstruct_ragged_u8"
    _flat_u8(blob, what + ": blob")
    _p(blob)
    dev = blob.device
    host_planes = None if isinstance(planes, torch.Tensor) else _ragged_table(planes, "vr_" + what)
    if dst is None:
        if host_planes is None:
            raise ValueError("%s: with a device plane table the destination must be given" % what)
        end = (host_planes["off"].astype(np.int64) + 3 * host_planes["rows"].astype(np.int64) * host_planes["pitch"]).max()
        dst = torch.zeros(max(int(end), 1), dtype=torch.uint8, device=dev)
    _flat_u8(dst, what + ": dst")
    if dst.device != dev:
        raise ValueError("%s: dst must be on %s" % (what, dev))
    dst_bytes = _declared_bytes(what, "dst", dst, dst_bytes)
    if bounds is None and host_planes is None:
        raise ValueError("%s: a device plane table needs bounds=(Hs, Ws)" % what)
    Hs, Ws = ragged_bounds(host_planes) if bounds is None else (int(v) for v in bounds)
    table, host_descs = _jpeg_records(what, blob, descs, max(Hs, 1), max(Ws, 1))
    B = int(table.shape[0])
    if host_planes is None:
        ptable = _dev_table(what, "plane table", planes, (B, RAGGED_PLANE_INTS), dev)
    else:
        if host_planes.shape[0] != B:
            raise ValueError("%s: %d plane records for %d images" % (what, host_planes.shape[0], B))
        sizes = None if host_descs is None else host_descs[:, [2, 1]]           # (height, width)
        ptable = _upload_i32(check_ragged_planes(host_planes, 3, dst_bytes, sizes, "vr_" + what), dev)
    qtabs = _qtabs(what, qtabs, B, dev)
    workspace = _jpeg_workspace(what, blob, workspace)
    _lib.check(_lib.lib().vr_jpeg_reconstruct_ragged_u8(_p(blob), int(blob.numel()), _p(table), _p(qtabs), _p(dst), dst_bytes,
                                                        _p(ptable), B, Hs, Ws, _p(workspace), int(workspace.numel()), _stream()),
               "vr_" + what)
    return dst


def resample_ragged_u8(src, planes, boxes, C, out_size, filter, out=None, workspace=None, src_bytes=None, bounds=None):
    """vr_resample_ragged_u8: resample_u8 -- the same boxes, arithmetic, window and mirror, bit for bit PIL's -- from ragged planes of
    C channels in the flat uint8 device buffer src, with no limit on the scale: any box with sides up to 8192 inside its own plane,
    to any out_size (So_w % 4 == 0).  Returns uint8 [B,C,So_h,So_w].
    planes, boxes: host tables (ragged_planes / int arrays) -- checked (check_ragged_planes, check_ragged_boxes), the intermediates
    laid out over the boxes' heights (ragged_ws_offsets) and both uploaded from pinned memory without a host wait -- or int32 DEVICE
    tensors [B, 8] and [B, 12] the caller has checked and laid out, which may be rewritten in place between replays of a captured
    launch; then workspace and bounds=(Hs, Ws) >= every record's rows and pitch must be given.  Host and device tables do not mix.
    workspace: a uint8 device tensor (None: taken from torch's allocator; a host-table call raises ValueError if a given one is too
    small); src_bytes: how much of src is declared to the kernel (default: all)."""
    what = "resample_ragged_u8"
    _flat_u8(src, what + ": src")
    _p(src)
    dev, C = src.device, int(C)
    So_h, So_w = _out_size(out_size)
    code = _resample_filter(filter)
    src_bytes = _declared_bytes(what, "src", src, src_bytes)
    if isinstance(planes, torch.Tensor) != isinstance(boxes, torch.Tensor):
        raise ValueError("%s: planes and boxes are both host tables or both device tensors" % what)
    if isinstance(planes, torch.Tensor):
        ptable = _dev_table(what, "plane table", planes, (None, RAGGED_PLANE_INTS), dev)
        B = int(ptable.shape[0])
        btable = _dev_table(what, "box table", boxes, (B, RESAMPLE_BOX_INTS), dev)
        if workspace is None or bounds is None:
            raise ValueError("%s: device tables need workspace= and bounds=(Hs, Ws)" % what)
        (Hs, Ws), need = (int(v) for v in bounds), 0
    else:
        # (not _table: the plane table is uploaded only after the boxes' heights have laid the intermediates out in it)
        host = _ragged_table(planes, "vr_" + what).copy()
        B = host.shape[0]
        check_ragged_planes(host, C, src_bytes, None, "vr_" + what)
        hb = check_ragged_boxes(boxes, host, (So_h, So_w))
        need = ragged_ws_offsets(host, C, So_w, hb[:, 3]) if 1 <= C <= 4 and So_w > 0 else 16
        Hs, Ws = ragged_bounds(host) if bounds is None else (int(v) for v in bounds)
        if isinstance(workspace, torch.Tensor) and workspace.numel() < need:
            raise ValueError("%s: the workspace has %d bytes, the batch needs %d" % (what, workspace.numel(), need))
        ptable = _upload_i32(host.view(np.int32).reshape(B, RAGGED_PLANE_INTS), dev)
        btable = _upload_i32(hb, dev)
    workspace = _u8_workspace(what, workspace, need, dev)
    out = _out(what, out, (B, C, So_h, So_w), torch.uint8, dev)
    _lib.check(_lib.lib().vr_resample_ragged_u8(_p(src), src_bytes, _p(ptable), _p(btable), _p(out), B, C, Hs, Ws, So_h, So_w, code,
                                                _p(workspace), int(workspace.numel()), _stream()), "vr_" + what)
    return out
