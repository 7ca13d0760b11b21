"""vr_jpeg_reconstruct_u8 on the GPU: coefficient blobs made by the host library (vitres.data.jpeg_collate) -> canvases, bit for bit
against PIL's own pixels committed in tests/golden/f22_jpeg_pil.npz (written by tests/golden/make_jpeg_golden.py) -- every fixture
in batches that mix sizes, samplings, grayscale and raw (PIL-decoded) records, then alone; a reused workspace and an oversized
canvas; a bad record passed straight to the entry; argument rejections; and the loader chain against the pad_collate_u8 chain."""
import os
import random

import numpy as np
import pytest
import torch

import emu_jpeg as E
from vitres import _lib, data
from vitres import kernels as K
from vitres.resized_crop import RandomResizedCrop, ResizeCenterCrop

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f22_jpeg_pil.npz"))
RECORDS = E.golden_records(G)
GOOD = [r for r in RECORDS if r[1] == 0]
FALLBACK = [r for r in RECORDS if r[1] in (1, 3)]                 # files PIL reads and the fast path does not take
NBATCH = 13
_COLLATED = {}


def batch(i):
    """16 baseline fixtures of all sizes and samplings (every 13th of the size-major list) and one fallback file"""
    return GOOD[i::NBATCH] + [FALLBACK[i % len(FALLBACK)]]


def collated(key, records):
    """(jpeg_collate's tuple, pad_collate_u8 of PIL's pixels), made once and never written"""
    if key not in _COLLATED:
        _COLLATED[key] = (data.jpeg_collate([(r[2], k) for k, r in enumerate(records)]),
                          data.pad_collate_u8([(r[3], k) for k, r in enumerate(records)]))
    return _COLLATED[key]


def launch(blob, descs, qtabs, Hs, Ws, **kw):
    B = descs.shape[0]
    out = torch.full((B, 3, Hs, Ws), POISON, dtype=torch.uint8, device=DEV)
    got = K.jpeg_reconstruct_u8(blob.to(DEV), descs.to(DEV), qtabs.to(DEV), Hs, Ws, out=out, **kw)
    assert got is out
    return out.cpu()


@pytest.mark.parametrize("i", range(NBATCH))
def test_mixed_batches_equal_pil(i):
    records = batch(i)
    assert len({r[3].shape for r in records}) > 8 and len({r[0].split(".")[1] for r in records[:-1]}) == 4
    (blob, descs, qtabs, sizes, _), (want, want_sizes, _) = collated(("batch", i), records)
    assert sorted(descs[:, 0].tolist()) == [0] * 16 + [1] and torch.equal(sizes, want_sizes)
    got = launch(blob, descs, qtabs, *want.shape[2:])
    assert torch.equal(got, want), "differs from PIL in %d bytes" % int((got != want).sum())


@pytest.mark.parametrize("name", ["1x1.444.q85", "3x5.420.q30r2", "33x2.422.q95rr", "2x33.420.q100opt", "9x17.gray.q30r2",
                                  "37x53.420.q95rr", "31x64.422.q30r2", "48x40.444.q100opt", "fallback.png"])
def test_single_images_equal_pil(name):
    records = [r for r in RECORDS if r[0] == name]
    (blob, descs, qtabs, _, _), (want, _, _) = collated(("one", name), records)
    assert torch.equal(launch(blob, descs, qtabs, *want.shape[2:]), want)


def test_second_batch_through_the_same_workspace_and_a_larger_canvas():
    (b0, d0, q0, _, _), (w0, _, _) = collated(("batch", 0), batch(0))
    (b1, d1, q1, _, _), (w1, _, _) = collated(("batch", 1), batch(1))
    ws = torch.full((K.jpeg_ws_bytes(max(b0.numel(), b1.numel())) + 64,), POISON, dtype=torch.uint8, device=DEV)
    assert torch.equal(launch(b0, d0, q0, *w0.shape[2:], workspace=ws), w0)
    assert torch.equal(launch(b1, d1, q1, *w1.shape[2:], workspace=ws), w1)
    assert torch.equal(launch(b0, d0, q0, *w0.shape[2:], workspace=ws), w0)
    assert (ws[-64:] == POISON).all()
    Hs, Ws = w1.shape[2] + 5, w1.shape[3] + 12
    want = torch.zeros((w1.shape[0], 3, Hs, Ws), dtype=torch.uint8)
    want[:, :, :w1.shape[2], :w1.shape[3]] = w1
    assert torch.equal(launch(b1, d1, q1, Hs, Ws, workspace=ws), want)


@pytest.mark.parametrize("field,value", [("off", 1 << 27), ("off", -1), ("width", 4096), ("hs", 3), ("kind", 2), ("bw", 1 << 20),
                                         ("ncomp", 2)])
def test_an_invalid_record_zeroes_its_image_and_nothing_else(field, value):
    (blob, descs, qtabs, _, _), (want, _, _) = collated(("batch", 2), batch(2))
    bad = descs.clone()
    victim = 5
    rec = bad.numpy().view(K.JPEG_DESC_DTYPE).reshape(-1)
    if rec[field].ndim == 2:
        rec[field][victim, 1 if rec["ncomp"][victim] == 3 else 0] = value
    else:
        rec[field][victim] = value
    with pytest.raises(RuntimeError, match="VR_EINVAL"):
        K.check_jpeg_table(bad.numpy(), blob.numel(), *want.shape[2:])
    got = launch(blob, bad, qtabs, *want.shape[2:])                       # a device table is the caller's to check: not checked here
    expect = want.clone()
    expect[victim] = 0
    assert torch.equal(got, expect)


def test_argument_errors():
    (blob, descs, qtabs, _, _), (want, _, _) = collated(("batch", 3), batch(3))
    Hs, Ws = want.shape[2:]
    blob, descs, qtabs = blob.to(DEV), descs.to(DEV), qtabs.to(DEV)
    L = _lib.lib()
    B, n = descs.shape[0], blob.numel()
    out = torch.empty((B, 3, Hs, Ws + 4), dtype=torch.uint8, device=DEV)
    ws = torch.empty(K.jpeg_ws_bytes(n), dtype=torch.uint8, device=DEV)
    assert int(L.vr_jpeg_ws_bytes(n)) == ws.numel() == ((n + 1) // 2 + 15) // 16 * 16 and int(L.vr_jpeg_ws_bytes(0)) == 0

    def call(B=B, Hs=Hs, Ws=Ws, ws_bytes=ws.numel(), n=n):
        return L.vr_jpeg_reconstruct_u8(blob.data_ptr(), n, descs.data_ptr(), qtabs.data_ptr(), out.data_ptr(), B, Hs, Ws,
                                        ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert call(Ws=Ws + 2) == -3 and call(Ws=Ws + 1) == -3
    assert call(B=0) == -1 and call(Hs=0) == -1 and call(n=0) == -1
    assert call(ws_bytes=ws.numel() - 16) == -1 and call(ws_bytes=0) == -1
    assert call(Hs=8196) == -3 and call(B=65536) == -3
    assert call() == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="VR_EINVAL"):
        K.jpeg_reconstruct_u8(blob, descs, qtabs, Hs, Ws, workspace=ws[:ws.numel() - 16])
    with pytest.raises(ValueError):
        K.jpeg_reconstruct_u8(blob, descs, qtabs[:-1], Hs, Ws)


NAMES_E2E = ["37x53.420.q85", "48x40.444.q30r2", "31x64.422.q95rr", "17x23.gray.q100opt",
             "48x40.420.q95rr", "fallback.progressive", "37x53.422.q100opt", "31x64.444.q85"]


@pytest.mark.parametrize("kind", ["eval", "train"])
def test_loader_chain_equals_the_pad_collate_chain(kind):
    """DataLoader(jpeg_collate) -> DeviceJpegLoader -> DeviceCropLoader against pad_collate_u8 batches of PIL's pixels ->
    DeviceCropLoader: two batches of four files, the same transform and seeds; the crops are the same bytes."""
    S = 16
    records = [next(r for r in RECORDS if r[0] == n) for n in NAMES_E2E]
    files = [(r[2], k % 5) for k, r in enumerate(records)]
    loader = torch.utils.data.DataLoader(files, batch_size=4, collate_fn=data.jpeg_collate, pin_memory=True)
    ref = [data.pad_collate_u8([(r[3], k % 5) for k, r in list(enumerate(records))[lo:lo + 4]]) for lo in (0, 4)]
    if kind == "train":
        make = lambda: RandomResizedCrop(S, rng=random.Random(5), generator=torch.Generator().manual_seed(6))   # noqa: E731
    else:
        make = lambda: ResizeCenterCrop(S, crop_pct=0.8, interpolation="bilinear")                               # noqa: E731
    jl = data.DeviceJpegLoader(loader, DEV)
    assert len(jl) == 2 and jl.dataset is files and jl.sampler is loader.sampler
    got = [(x.cpu(), y.cpu()) for x, y in data.DeviceCropLoader(jl, make(), DEV)]
    want = [(x.cpu(), y.cpu()) for x, y in data.DeviceCropLoader(ref, make(), DEV)]
    assert len(got) == len(want) == 2
    for (x, y), (wx, wy) in zip(got, want):
        assert x.dtype == torch.uint8 and tuple(x.shape) == (4, 3, S, S) and torch.equal(x, wx) and torch.equal(y, wy)
    canvases = [(c.cpu(), s) for c, s, _ in data.DeviceJpegLoader(loader, DEV)]
    for (c, s), (wc, ws_, _) in zip(canvases, ref):
        assert torch.equal(c, wc) and torch.equal(torch.as_tensor(s), ws_)
