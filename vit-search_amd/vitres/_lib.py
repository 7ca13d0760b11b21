"""ctypes loaders for libvitres_hip.so (the C ABI declared in include/vitres_hip.h) and for libvitres_jpeg.so (the host-only JPEG
entropy decoder of include/vitres_jpeg.h: `jpeg_lib()`, which never touches the HIP library -- DataLoader workers load only that).

The library is the product: there is no CPU / PyTorch fallback.  Importing this module never fails
(so that host-side logic can be unit-tested without a GPU), but the first kernel call raises
RuntimeError when the shared object is missing or does not export a declared symbol.
"""
import ctypes
import os
from ctypes import c_float, c_int32, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# VITRES_LIB: another build of the same ABI (A/B timing of kernel changes on one box: tools/ab.sh)
LIB_PATH = os.environ.get("VITRES_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libvitres_hip.so")

JPEG_LIB_PATH = os.environ.get("VITRES_JPEG_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libvitres_jpeg.so")

VR_F32, VR_BF16, VR_F16 = 0, 1, 2


class RowMap(ctypes.Structure):
    _fields_ = [("rpi", c_int32), ("rps", c_int32), ("off", c_int32)]


class GemmArgs(ctypes.Structure):
    _fields_ = [
        ("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("C2", c_void_p),
        ("bias", c_void_p), ("pos", c_void_p), ("scale", c_void_p), ("keep_n", c_void_p),
        ("resid", c_void_p), ("dact_u", c_void_p), ("keep_k", c_void_p), ("bias_grad", c_void_p),
        ("M", c_int32), ("N", c_int32), ("K", c_int32),
        ("lda", c_int32), ("ldb", c_int32), ("ldc", c_int32), ("ldu", c_int32),
        ("a_trans", c_int32), ("b_trans", c_int32),
        ("in_dtype", c_int32), ("out_dtype", c_int32),
        ("act", c_int32), ("atomic", c_int32), ("split_k", c_int32), ("rows_in", c_int32), ("n_period", c_int32), ("k_period", c_int32), ("sched", c_int32),
        ("a_map", RowMap), ("b_map", RowMap), ("c_map", RowMap), ("m_groups", c_int32),
        ("ws", c_void_p), ("ws_bytes", c_int64), ("ring", c_int32), ("k_shares", c_int32),
        ("sr_x", c_void_p), ("keep_out", c_void_p), ("tok_src", c_void_p), ("tok_pos", c_void_p),
        ("sr_g", c_int32), ("sr_cin", c_int32), ("sr_tokens", c_int32),
        ("tok_rows", c_int32), ("tok_ld", c_int32), ("tok_rps", c_int32), ("tok_cols", c_int32), ("reserved0", c_int32),
    ]


class LnEpilogue(ctypes.Structure):
    _fields_ = [("mode", c_int32), ("eps", c_float), ("w", c_void_p), ("b", c_void_p), ("keep", c_void_p), ("y", c_void_p),
                ("mean", c_void_p), ("rstd", c_void_p), ("x", c_void_p), ("dw", c_void_p), ("db", c_void_p),
                ("gt_out", c_void_p), ("gt_scale", c_void_p), ("gt_keep", c_void_p), ("grad_copies", c_int32)]


MAX_ZERO_RANGES = 24


class ZeroRanges(ctypes.Structure):
    _fields_ = [("lo", c_int64 * MAX_ZERO_RANGES), ("count", c_int64 * MAX_ZERO_RANGES), ("n", c_int32), ("reserved", c_int32)]


class LnGradSlot(ctypes.Structure):
    _fields_ = [("part_w", c_void_p), ("part_b", c_void_p), ("dw", c_void_p), ("db", c_void_p), ("C", c_int32),
                ("reserved", c_int32)]


class MixupParam(ctypes.Structure):
    _fields_ = [("lam", c_float), ("oml", c_float), ("y0", c_int32), ("y1", c_int32), ("x0", c_int32), ("x1", c_int32),
                ("cutmix", c_int32), ("pad", c_int32)]


class EraseArgs(ctypes.Structure):
    _fields_ = [("rects", c_void_p), ("R", c_int32), ("mode", c_int32), ("seed", c_uint64), ("call", c_uint64)]


VR_ERASE_CONST, VR_ERASE_RAND, VR_ERASE_PIXEL = 0, 1, 2


class ResampleBox(ctypes.Structure):
    _fields_ = [("x0", c_int32), ("y0", c_int32), ("w", c_int32), ("h", c_int32), ("ow", c_int32), ("oh", c_int32),
                ("wx", c_int32), ("wy", c_int32), ("flip", c_int32), ("reserved", c_int32 * 3)]


VR_BILINEAR, VR_BICUBIC = 2, 3            # PIL's filter numbers


class RaOp(ctypes.Structure):
    _fields_ = [("op", c_int32), ("filter", c_int32), ("iarg", c_int32), ("factor", c_float), ("m", ctypes.c_double * 6)]


(VR_RA_IDENTITY, VR_RA_INVERT, VR_RA_POSTERIZE, VR_RA_SOLARIZE, VR_RA_SOLARIZE_ADD, VR_RA_AUTOCONTRAST, VR_RA_EQUALIZE,
 VR_RA_BRIGHTNESS, VR_RA_COLOR, VR_RA_CONTRAST, VR_RA_SHARPNESS, VR_RA_AFFINE) = range(12)


class JpegDesc(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("width", c_int32), ("height", c_int32), ("ncomp", c_int32), ("hs", c_int32), ("vs", c_int32),
                ("off", c_int32 * 3), ("bw", c_int32 * 3), ("bh", c_int32 * 3), ("reserved", c_int32)]


VR_JPEG_COEF, VR_JPEG_RAW = 0, 1


class RaggedPlane(ctypes.Structure):
    _fields_ = [("off", c_int64), ("pitch", c_int32), ("rows", c_int32), ("ws_off", c_int64), ("reserved", c_int32 * 2)]


class JpegInfo(ctypes.Structure):                 # include/vitres_jpeg.h
    _fields_ = [("supported", c_int32), ("width", c_int32), ("height", c_int32), ("ncomp", c_int32), ("hs", c_int32), ("vs", c_int32),
                ("restart_interval", c_int32), ("blocks", c_int32 * 3), ("bw", c_int32 * 3), ("bh", c_int32 * 3)]


# name -> argtypes ; every entry point returns int.  Must list every symbol of include/vitres_hip.h
SYMBOLS = {
    "vr_version": [],
    "vr_gemm": [ctypes.POINTER(GemmArgs), c_void_p],
    "vr_gemm_group": [ctypes.POINTER(GemmArgs), ctypes.c_int32, c_void_p],
    "vr_gemm_ln": [ctypes.POINTER(GemmArgs), ctypes.POINTER(LnEpilogue), c_void_p],
    "vr_gemm_ln_supported": [c_int32],
    "vr_gemm_ln_fold": [ctypes.POINTER(GemmArgs), ctypes.POINTER(LnEpilogue), c_void_p],
    "vr_gemm_ws_bytes": [],
    "vr_cast_f32_bf16": [c_void_p, c_void_p, c_int64, c_void_p],
    "vr_cast_f32_f16": [c_void_p, c_void_p, c_int64, c_void_p],
    "vr_adamw_flat": [c_void_p] * 6 + [c_float, c_void_p, c_void_p, c_int32, c_int64, c_void_p],
    "vr_adamw_flat_dev": [c_void_p] * 6 + [c_float, c_void_p, c_void_p, c_int32, c_int64, c_void_p],
    "vr_adamw_flat_dev_capped": [c_void_p] * 6 + [c_float, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p],
    "vr_grad_sumsq": [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p],
    "vr_clip_finish": [c_void_p, c_int32, c_void_p, c_void_p],
    "vr_grad_sumsq_gated": [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    "vr_clip_finish_gated": [c_void_p, c_int32, c_void_p, c_void_p, c_void_p],
    "vr_adamw_flat_clip": [c_void_p] * 6 + [c_float, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_void_p],
    "vr_cast_transpose_batch": [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    "vr_ln_fwd": [c_void_p] * 7 + [c_int32, c_int32, c_int32, c_float, c_int32, c_void_p],
    "vr_ln_bwd": [c_void_p] * 13 + [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p],
    "vr_ln_bwd_sr": [c_void_p] * 14 + [c_int32] * 6 + [c_void_p],
    "vr_ln_grad_reduce": [ctypes.POINTER(LnGradSlot), c_int32, c_int32, c_void_p],
    "vr_attn_fwd": [c_void_p] * 4 + [c_int32] * 4 + [c_float, c_int32, c_void_p],
    "vr_attn_bwd": [c_void_p] * 7 + [c_int32] * 4 + [c_float, c_int32, c_void_p],
    "vr_softce": [c_void_p] * 4 + [c_int32, c_int32, c_float, c_void_p],
    "vr_softce_train": [c_void_p] * 3 + [c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_void_p],
    "vr_eval_metrics": [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p],
    "vr_colsum": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, RowMap, c_void_p],
    "vr_scale_mask_cast": [c_void_p] * 4 + [c_int32] * 4 + [c_void_p],
    "vr_conv3x3_wgrad": [c_void_p, c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p],
    "vr_conv3x3": [c_void_p, c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p],
    "vr_conv3x3_bias_relu": [c_void_p] * 5 + [c_int32] * 6 + [c_void_p],
    "vr_conv3x3_res": [c_void_p] * 4 + [c_int32] * 6 + [c_void_p],
    "vr_conv3x3_bias_relu_patch": [c_void_p] * 5 + [c_int32] * 7 + [c_void_p],
    "vr_conv_w_flip": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p],
    "vr_conv1_direct": [c_void_p] * 4 + [c_int32] * 6 + [c_void_p],
    "vr_token_mix": [c_void_p] * 6 + [c_int32] * 11 + [c_float] * 6 + [c_void_p],
    "vr_normalize_u8": [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p, c_void_p, c_void_p],
    "vr_token_mix_u8": [c_void_p] * 6 + [c_int32] * 11 + [c_float] * 6 + [c_void_p, c_void_p, c_void_p],
    "vr_mixup": [c_void_p] * 5 + [c_int32] * 5 + [c_float, c_float, c_void_p],
    "vr_mixup_u8": [c_void_p] * 5 + [c_int32] * 5 + [c_float, c_float, c_void_p, c_void_p, c_void_p],
    "vr_random_erase": [c_void_p] + [c_int32] * 4 + [c_void_p, c_int32, c_int32, c_uint64, c_uint64, c_void_p],
    "vr_normalize_u8_erase": [c_void_p, c_void_p] + [c_int32] * 4 + [c_void_p, c_void_p, ctypes.POINTER(EraseArgs), c_void_p],
    "vr_token_mix_u8_erase": [c_void_p] * 6 + [c_int32] * 11 + [c_float] * 6 + [c_void_p, c_void_p, ctypes.POINTER(EraseArgs),
                                                                               c_void_p],
    "vr_mixup_u8_erase": [c_void_p] * 5 + [c_int32] * 5 + [c_float, c_float, c_void_p, c_void_p, ctypes.POINTER(EraseArgs), c_void_p],
    "vr_resample_u8": [c_void_p, c_void_p, c_void_p] + [c_int32] * 7 + [c_void_p, ctypes.c_size_t, c_void_p],
    "vr_resample_band_rows": [c_int32] * 6,
    "vr_rand_augment_u8": [c_void_p, c_void_p, c_void_p] + [c_int32] * 4 + [ctypes.c_uint32, c_void_p, ctypes.c_size_t, c_void_p],
    "vr_jpeg_reconstruct_u8": [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, ctypes.c_size_t,
                               c_void_p],
    "vr_jpeg_reconstruct_ragged_u8": [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32,
                                      c_void_p, ctypes.c_size_t, c_void_p],
    "vr_resample_ragged_u8": [c_void_p, c_int64, c_void_p, c_void_p, c_void_p] + [c_int32] * 7 + [c_void_p, ctypes.c_size_t, c_void_p],
    "vr_token_mean": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p],
    "vr_token_mean_bwd": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p],
    "vr_batchsum": [c_void_p, c_void_p, c_int32, c_int64, c_void_p],
    "vr_im2col_patch": [c_void_p, c_void_p] + [c_int32] * 7 + [c_void_p],
    "vr_im2col_patch_map": [c_void_p, c_void_p, c_void_p] + [c_int32] * 7 + [c_void_p],
    "vr_embed_cls": [c_void_p] * 4 + [c_int32] * 4 + [c_void_p],
    "vr_sr_im2col": [c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p],
    "vr_sr_col2im": [c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p],
    "vr_sr_resid": [c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p],
    "vr_sr_resid_bwd": [c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p],
    "vr_mask_rows": [c_void_p, c_void_p] + [c_int32] * 3 + [c_void_p],
    "vr_zero_ranges": [c_void_p, ctypes.POINTER(ZeroRanges), c_void_p],
    "vr_zero_ranges_gated": [c_void_p, ctypes.POINTER(ZeroRanges), c_void_p, c_void_p],
    "vr_relayout": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, c_void_p],
    "vr_relayout_add": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_void_p],
    "vr_im2col3x3": [c_void_p, c_void_p] + [c_int32] * 8 + [c_void_p],
    "vr_col2im3x3": [c_void_p, c_void_p] + [c_int32] * 5 + [c_void_p],
    "vr_bn_stats": [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p],
    "vr_bn_finalize": [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_float] + [c_void_p] * 7 + [c_int32, c_void_p],
    "vr_bn_relu": [c_void_p] * 5 + [c_int64, c_int32, c_int32, c_int32, c_void_p],
    "vr_bn_bwd": [c_void_p] * 9 + [c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p],
    "vr_patch_unfold": [c_void_p, c_void_p] + [c_int32] * 7 + [c_void_p],
    "vr_bn_relu_patch": [c_void_p] * 5 + [c_int32] * 7 + [c_void_p],
    "vr_bn_bwd_patch": [c_void_p] * 9 + [c_int32] * 8 + [c_void_p],
    "vr_conv3x3_res_patch": [c_void_p] * 4 + [c_int32] * 7 + [c_void_p],
}

# the entry points that do not return int: name -> (argtypes, restype)
OTHER_SYMBOLS = {
    "vr_resample_ws_bytes": ([c_int32, c_int32, c_int32], ctypes.c_size_t),
    "vr_rand_augment_ws_bytes": ([c_int32] * 4, ctypes.c_size_t),
    "vr_jpeg_ws_bytes": ([c_int64], ctypes.c_size_t),
    "vr_resample_ragged_ws_bytes": ([c_int32, c_int64, c_int32], ctypes.c_size_t),
}

# the host-only library: name -> argtypes, every entry returns int
JPEG_SYMBOLS = {
    "vr_jpeg_probe": [c_void_p, c_int64, ctypes.POINTER(JpegInfo)],
    "vr_jpeg_entropy_decode": [c_void_p, c_int64, ctypes.POINTER(JpegInfo), c_void_p, c_int64, c_void_p],
}

_lib = None


def lib():
    """Load (once) and return the library; raise loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libvitres_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C vit-search_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
        # torch first: it ships its own HIP runtime, and the library must bind to that copy -- loaded ahead of torch it would bring
        # in the system's, and two runtimes in one process do not share devices, streams or memory
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SYMBOLS.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise RuntimeError("libvitres_hip.so does not export %s" % name) from e
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        for name, (argtypes, restype) in OTHER_SYMBOLS.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise RuntimeError("libvitres_hip.so does not export %s" % name) from e
            fn.argtypes, fn.restype = argtypes, restype
        _lib = L
    return _lib


_jpeg_lib = None


def jpeg_lib():
    """Load (once) and return libvitres_jpeg.so.  Plain host code: loading it pulls in neither libvitres_hip.so nor the HIP runtime."""
    global _jpeg_lib
    if _jpeg_lib is None:
        if not os.path.exists(JPEG_LIB_PATH):
            raise RuntimeError(
                "libvitres_jpeg.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C vit-search_amd/csrc`)." % JPEG_LIB_PATH)
        L = ctypes.CDLL(JPEG_LIB_PATH)
        for name, argtypes in JPEG_SYMBOLS.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise RuntimeError("libvitres_jpeg.so does not export %s" % name) from e
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        _jpeg_lib = L
    return _jpeg_lib


_ERR = {-1: "VR_EINVAL (bad argument)", -2: "VR_EALIGN (pointer / leading-dimension alignment)",
        -3: "VR_EUNSUPPORTED (shape or dtype not supported)"}


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, _ERR.get(rc, "hipError_t %d" % rc)))
