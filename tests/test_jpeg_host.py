"""The host half of JPEG decoding without a GPU: libvitres_jpeg.so (vitres.jpeg) against the portable restatement tests/emu_jpeg.py
(its own marker parser and a bit-at-a-time Huffman decoder) on every stream of tests/golden/f22_jpeg_pil.npz, the emulation's
reconstruction from the library's coefficients against PIL's committed pixels, the files the fast path leaves to PIL, damaged
streams, one stream cut at every byte, the layout jpeg_collate makes and check_jpeg_table's rejections, the emulated device entry
against pad_collate_u8, what a decoding process has mapped, and a two-worker DataLoader."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu_jpeg as E
from vitres import _lib, data
from vitres import jpeg as J
from vitres import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "f22_jpeg_pil.npz"))
RECORDS = E.golden_records(G)
GOOD = [r for r in RECORDS if r[1] == 0]
FALLBACK = [r for r in RECORDS if r[1] == 1]
DAMAGED = [r for r in RECORDS if r[1] in (2, 3)]
SAMPLING = {"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2), "gray": (1, 1, 1)}


def test_the_fixture_covers_what_it_should():
    assert len(GOOD) == 13 * 4 * 4 and [r[0] for r in FALLBACK] == ["fallback.progressive", "fallback.cmyk", "fallback.png"]
    assert [r[0] for r in DAMAGED] == ["damaged.cut_header", "damaged.cut_scan", "damaged.no_huffman_table"]
    widths = {E.probe(r[2])["bw"][1] for r in GOOD if ".420." in r[0]}
    assert min(widths) == 1 and max(widths) > 2                               # both sides of the chroma rule need dw <= 2 and dw > 2
    assert any(E.parse(r[2])["restart"] for r in GOOD) and any(len(r[2]) > 3000 for r in GOOD)


@pytest.mark.parametrize("group", range(13))
def test_coefficients_tables_and_pixels(group):
    """per fixture: probe's geometry, the library's coefficients and tables equal the emulation's, and the emulation's reconstruction
    from the LIBRARY's coefficients is PIL's image bit for bit"""
    for name, _, stream, pil in GOOD[16 * group:16 * group + 16]:
        H, W = (int(v) for v in name.split(".")[0].split("x"))
        info = J.probe(stream)
        nc, hs, vs = SAMPLING[name.split(".")[1]]
        assert info["supported"] and (info["height"], info["width"], info["ncomp"], info["hs"], info["vs"]) == (H, W, nc, hs, vs), name
        mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
        assert info["bw"][:nc] == (mx * hs, mx, mx)[:nc] and info["bh"][:nc] == (my * vs, my, my)[:nc]
        assert info["blocks"] == tuple(a * b for a, b in zip(info["bw"], info["bh"]))
        got_info, coef, qtab = J.entropy_decode(stream)
        assert got_info == info
        p, want, want_q = E.entropy_decode(stream)
        assert p["restart"] == info["restart_interval"] and np.array_equal(qtab, want_q) and qtab.dtype == np.uint16
        for c in range(nc):
            assert coef[c].dtype == np.int16 and np.array_equal(coef[c].reshape(-1, 64), want[c]), (name, c)
        planes = [E.idct_plane(coef[c].reshape(-1, 64), qtab[c], info["bw"][c], info["bh"][c]) for c in range(nc)]
        rgb = E.to_rgb(planes, W, H, hs, vs)
        assert np.array_equal(rgb, pil), "%s: %d bytes differ from PIL" % (name, int((rgb != pil).sum()))


def test_fallback_files_are_not_supported_and_no_error():
    for name, _, stream, _ in FALLBACK:
        info = J.probe(stream)
        assert info["supported"] is False and info["width"] == 0 and sum(info["blocks"]) == 0, name
        assert E.probe(stream) == dict(supported=False)
        with pytest.raises(J.JpegError) as e:
            J.entropy_decode(stream)
        assert e.value.code == -3
    assert J.probe(b"")["supported"] is False and J.probe(b"\xff\xd8")["supported"] is False


def test_damaged_streams_return_an_error():
    for name, _, stream, _ in DAMAGED:
        with pytest.raises(J.JpegError) as e:
            J.entropy_decode(stream)
        assert e.value.code == -1, name
        with pytest.raises(E.Damaged):
            E.entropy_decode(stream)
    good = next(r[2] for r in GOOD if r[0] == "17x23.420.q85")
    info = J.probe(good)
    coef = np.zeros(64 * sum(info["blocks"]) - 1, dtype=np.int16)             # a buffer one element short
    with pytest.raises(J.JpegError):
        J.entropy_decode(good, coef=coef)


def test_one_stream_cut_at_every_byte():
    """error or success, never a crash, and never a write past the capacity: success only with the end-of-image marker in"""
    stream = next(r[2] for r in GOOD if r[0] == "9x17.420.q30r2")
    info = J.probe(stream)
    n = 64 * sum(info["blocks"])
    guard = 64
    ok = 0
    for cut in range(len(stream)):
        coef = np.zeros(n + guard, dtype=np.int16)
        coef[n:] = 0x5A5A
        try:
            J.entropy_decode(stream[:cut], coef=coef[:n])
            ok += 1
        except J.JpegError:
            pass
        assert (coef[n:] == 0x5A5A).all(), cut
        assert J.probe(stream[:cut])["supported"] in (False, True)
    assert ok == 0                                                               # every proper prefix lacks the marker
    J.entropy_decode(stream)


def test_corrupted_scan_bytes_never_crash():
    stream = bytearray(next(r[2] for r in GOOD if r[0] == "17x23.422.q95rr"))
    info = J.probe(bytes(stream))
    n = 64 * sum(info["blocks"])
    rs = np.random.RandomState(3)
    for _ in range(300):
        bad = bytearray(stream)
        bad[rs.randint(2, len(bad))] = rs.randint(0, 256)
        coef = np.zeros(n, dtype=np.int16)
        try:
            J.entropy_decode(bytes(bad), coef=coef)
        except J.JpegError:
            pass


def _mixed():
    records = GOOD[5::13] + FALLBACK + [DAMAGED[2]]
    return records, data.jpeg_collate([(r[2], k % 7) for k, r in enumerate(records)])


def test_collate_layout():
    records, (blob, descs, qtabs, sizes, labels) = _mixed()
    B = len(records)
    assert blob.dtype == torch.uint8 and blob.dim() == 1 and descs.dtype == torch.int32 and tuple(descs.shape) == (B, 16)
    assert qtabs.dtype == torch.int16 and tuple(qtabs.shape) == (B, 3, 64) and sizes.dtype == torch.int32 and labels.dtype == torch.int64
    assert labels.tolist() == [k % 7 for k in range(B)]
    assert sizes.tolist() == [list(r[3].shape[:2]) for r in records]
    rec = descs.numpy().view(K.JPEG_DESC_DTYPE).reshape(-1)
    assert rec["kind"].tolist() == [0] * 16 + [1] * 4                          # the fallback files, and the stream the library refuses
    spans = []
    for b in range(B):
        unit = 64 if rec["kind"][b] else 128
        for c in range(rec["ncomp"][b]):
            lo = int(rec["off"][b, c]) * 16
            assert lo % unit == 0                                                # (the entry needs 16)
            spans.append((lo, lo + int(rec["bw"][b, c]) * int(rec["bh"][b, c]) * unit))
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] <= blob.numel()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    Hs, Ws = ((int(v) + 3) // 4 * 4 for v in sizes.numpy().max(axis=0))
    table = K.check_jpeg_table(descs.numpy(), blob.numel(), Hs, Ws)
    assert table.dtype == np.int32 and np.array_equal(table, descs.numpy())
    assert all(E.record_ok(d, blob.numel(), Hs, Ws) for d in descs.numpy())
    pinned = [t for t in (blob, descs, qtabs, sizes, labels) if isinstance(t, torch.Tensor)]
    assert len(pinned) == 5


@pytest.mark.parametrize("lo", range(0, 212, 53))
def test_emulated_entry_on_collated_batches_equals_pad_collate(lo):
    """the emulation standing in for the kernel: its canvas is pad_collate_u8 of PIL's images, padding included"""
    records = [r for r in RECORDS if r[1] != 2][lo:lo + 53]
    blob, descs, qtabs, sizes, _ = data.jpeg_collate([(r[2], 0) for r in records])
    want, want_sizes, _ = data.pad_collate_u8([(r[3], 0) for r in records])
    got = E.reconstruct_u8(blob.numpy(), descs.numpy(), qtabs.numpy(), *want.shape[2:])
    assert np.array_equal(got, want.numpy()) and torch.equal(sizes, want_sizes)


def test_collate_raises_what_pil_raises():
    with pytest.raises(Exception) as e:
        data.jpeg_collate([(DAMAGED[1][2], 0)])
    assert not isinstance(e.value, J.JpegError)
    with pytest.raises(ValueError):
        data.jpeg_collate([])


@pytest.mark.parametrize("field,c,value", [("off", 0, 1 << 26), ("off", 0, -8), ("width", None, 80), ("height", None, 0),
                                           ("hs", None, 3), ("vs", None, 2), ("ncomp", None, 4), ("kind", None, 2), ("bw", 0, 99),
                                           ("bh", 0, 0), ("off", 0, None)])
def test_check_jpeg_table_rejects(field, c, value):
    _, (blob, descs, _, sizes, _) = _mixed()
    Hs, Ws = ((int(v) + 3) // 4 * 4 for v in sizes.numpy().max(axis=0))
    table = descs.numpy().copy()
    rec = table.view(K.JPEG_DESC_DTYPE).reshape(-1)
    victim = next(b for b in range(len(rec)) if rec["kind"][b] == 0 and rec["hs"][b] == 1 and rec["ncomp"][b] == 3)
    if value is None:
        rec["off"][victim, 0] = rec["off"][victim + 1, 0]                       # two components on the same bytes
    elif c is None:
        rec[field][victim] = value
    else:
        rec[field][victim, c] = value
    with pytest.raises(RuntimeError, match="VR_EINVAL"):
        K.check_jpeg_table(table, blob.numel(), Hs, Ws)
    if value is not None:
        assert not E.record_ok(table[victim], blob.numel(), Hs, Ws)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                         # an image larger than the canvas
        K.check_jpeg_table(descs.numpy(), blob.numel(), Hs - 4, Ws)
    with pytest.raises(RuntimeError, match="VR_EINVAL"):                         # a blob shorter than the offsets say
        K.check_jpeg_table(descs.numpy(), blob.numel() - 128, Hs, Ws)


def test_abi_of_the_host_library():
    hdr = open(os.path.join(ROOT, "include", "vitres_jpeg.h")).read()
    import re
    assert set(re.findall(r"^int\s+(vr_\w+)\s*\(", hdr, flags=re.M)) == set(_lib.JPEG_SYMBOLS)
    assert not set(_lib.JPEG_SYMBOLS) & set(_lib.SYMBOLS)
    src = open(os.path.join(ROOT, "vit-search_amd", "csrc", "jpeg_host.cpp")).read()
    includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', src, flags=re.M)
    assert includes and all("hip" not in i.lower() for i in includes), includes
    import ctypes
    assert ctypes.sizeof(_lib.JpegInfo) == 64 and ctypes.sizeof(_lib.JpegDesc) == 64


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import emu_jpeg as E
import vitres.jpeg as J
G = np.load(sys.argv[3])
name, kind, stream, pil = E.golden_records(G)[100]
info, coef, qtab = J.entropy_decode(stream)
assert info["supported"] and coef[0].any()
maps = open("/proc/self/maps").read()
assert "libvitres_jpeg" in maps
for lib in ("libvitres_hip", "libamdhip64"):
    assert lib not in maps, lib
assert "torch" not in sys.modules
print("clean")
"""


def test_a_decoding_process_maps_no_hip_library():
    """a fresh process that imports vitres.jpeg and decodes has libvitres_jpeg.so mapped, and neither libvitres_hip.so nor the HIP
    runtime (nor torch, which would bring the runtime in); the library itself links against neither"""
    out = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "vit-search_amd"), os.path.join(ROOT, "tests"),
                          os.path.join(ROOT, "tests", "golden", "f22_jpeg_pil.npz")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "clean", out.stderr
    needed = subprocess.run(["readelf", "-d", _lib.JPEG_LIB_PATH], capture_output=True, text=True)
    if needed.returncode == 0:
        assert "NEEDED" in needed.stdout and "hip" not in needed.stdout.lower()


def test_two_worker_dataloader_yields_what_the_call_yields():
    records = GOOD[7::30] + FALLBACK[:1]
    files = [(r[2], k) for k, r in enumerate(records)][:8]
    assert len(files) == 8
    loader = torch.utils.data.DataLoader(files, batch_size=4, num_workers=2, collate_fn=data.jpeg_collate)
    got = list(loader)
    assert len(got) == 2
    for i, batch in enumerate(got):
        want = data.jpeg_collate(files[4 * i:4 * i + 4])
        assert len(batch) == 5 and all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(batch, want))
