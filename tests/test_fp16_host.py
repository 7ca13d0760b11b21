"""Host side of the fp16 evaluation mode (no GPU): the dtype code of the C ABI, the dtype mapping of vitres.kernels, the GEMM
argument marshalling with fp16 operands, and the guard that keeps fp16 out of training -- it must fire before any launch."""
import os

import pytest
import torch

import recipe
import vitres
from vitres import _lib
from vitres import kernels as K

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitres_hip.h")


def test_f16_dtype_code_is_declared():
    assert _lib.VR_F16 == 2
    src = open(HDR).read()
    assert "#define VR_F16 2" in src and "VR_F16 = 2" in src
    assert "vr_cast_f32_f16" in src and "vr_cast_f32_f16" in _lib.SYMBOLS


def test_dtype_mapping():
    assert K._dtcode(torch.float16) == _lib.VR_F16 and K._dt(torch.zeros(1, dtype=torch.float16)) == _lib.VR_F16
    assert K._dtcode(torch.bfloat16) == _lib.VR_BF16 and K._dtcode(torch.float32) == _lib.VR_F32
    for bad in (torch.float64, torch.int32):
        with pytest.raises(TypeError):
            K._dtcode(bad)
        with pytest.raises(TypeError):
            K._dt(torch.zeros(1, dtype=bad))
    assert K.is_fast16(torch.float16) and K.is_fast16(torch.bfloat16) and not K.is_fast16(torch.float32)


def test_gemm_argument_marshalling_of_fp16_operands(monkeypatch):
    monkeypatch.setattr(K, "_p", lambda t: None if t is None else 0x1000)
    a, b = torch.zeros(8, 16, dtype=torch.float16), torch.zeros(4, 16, dtype=torch.float16)
    for out, code in ((torch.zeros(8, 4), _lib.VR_F32), (torch.zeros(8, 4, dtype=torch.float16), _lib.VR_F16)):
        args = K._gemm_args(a, b, out, M=8, N=4, K=16, lda=16, ldb=16, ldc=4, ws=None)
        assert (args.in_dtype, args.out_dtype, args.M, args.N, args.K) == (_lib.VR_F16, code, 8, 4, 16)
    with pytest.raises(AssertionError):            # bf16 and fp16 never mix
        K._gemm_args(a, b.to(torch.bfloat16), torch.zeros(8, 4), M=8, N=4, K=16, lda=16, ldb=16, ldc=4, ws=None)


def _micro():
    kw = dict(num_channels_to_keep=recipe.micro_keep_config(), example_per_arch=2, num_warmup_epochs=30)
    return vitres.create_model("flexible_vit_sr_patch14_224_patch_output_supernet", img_size=recipe.MICRO_IMG,
                               num_classes=recipe.MICRO_CLASSES, network_def=recipe.MICRO_DEFS[0], drop_path_rate=0.0, **kw)


def test_set_compute_dtype_accepts_fp16():
    m = _micro()
    assert m.set_compute_dtype(torch.float16) is m and m.compute_dtype == torch.float16
    m.set_compute_dtype(torch.bfloat16)
    assert m.compute_dtype == torch.bfloat16
    with pytest.raises(ValueError):
        m.set_compute_dtype(torch.float64)


def test_fp16_training_guard_fires_before_any_launch():
    """On a CPU tensor the forward would fail with the 'needs CUDA tensors' error at its first launch: NotImplementedError instead
    shows that the guard runs first."""
    m = _micro().set_compute_dtype(torch.float16)
    x = torch.zeros(4, 3, recipe.MICRO_IMG, recipe.MICRO_IMG)
    t = torch.zeros(4, recipe.MICRO_CLASSES)
    m.train()
    with pytest.raises(NotImplementedError, match="fp16 is eval-only"):
        m(x)
    with pytest.raises(NotImplementedError, match="fp16 is eval-only"):
        m.loss_and_grad(x, t)
    from vitres.engine import GraphedTrainStep
    with pytest.raises(NotImplementedError, match="fp16 is eval-only"):
        GraphedTrainStep(m, None, x, t)
    m.eval()                                       # evaluation passes the guard and reaches the device check
    with pytest.raises(RuntimeError, match="MI355X|CUDA|HIP"):
        m(x)
