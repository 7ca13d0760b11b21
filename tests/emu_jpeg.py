"""Portable numpy restatement of the JPEG path (include/vitres_jpeg.h, vr_jpeg_reconstruct_u8 of include/vitres_hip.h): the marker
parser and a bit-at-a-time Huffman decoder (the cross-check of the host library's coefficients), and the integer reconstruction --
dequantise, libjpeg's ISLOW inverse DCT, libjpeg's "fancy" chroma upsampling, YCbCr -> RGB, placement into the zero-padded canvas --
that stands in for the device entry on machines without a GPU.  Written for clarity, not speed: use it on small images."""
import numpy as np

# natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)

# one record of the device table: 16 int32 (vr_jpeg_desc)
D_KIND, D_W, D_H, D_NC, D_HS, D_VS, D_OFF, D_BW, D_BH, D_WORDS = 0, 1, 2, 3, 4, 5, 6, 9, 12, 16
MAX_SIDE = 8192


class Unsupported(Exception):
    """a stream the fast path does not take (the loader decodes it with PIL)"""


class Damaged(Exception):
    """a stream the host library answers with an error"""


def _ceil_div(a, b):
    return -(-a // b)


def parse(data):
    """Markers up to the first scan -> dict(width, height, ncomp, hs, vs, restart, bw[], bh[], qtab [ncomp, 64] natural order,
    dc / ac Huffman tables per component, scan = offset of the entropy-coded bytes).  Raises Unsupported / Damaged."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Unsupported("not a JPEG")
    pos = 2
    quant, huff, frame, restart = {}, {}, None, 0
    jfif, adobe = False, None
    while True:
        if pos >= n:
            raise Damaged("truncated before the scan")
        if data[pos] != 0xFF:
            raise Damaged("no marker where one is due")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise Damaged("truncated in a marker")
        m = data[pos]
        pos += 1
        if m == 0xD8 or m == 0xD9 or 0xD0 <= m <= 0xD7 or m == 0x01 or m == 0x00:
            raise Unsupported("marker %02x before the scan" % m)
        if pos + 2 > n:
            raise Damaged("truncated in a marker length")
        L = data[pos] << 8 | data[pos + 1]
        if L < 2 or pos + L > n:
            raise Damaged("bad marker length")
        seg = data[pos + 2:pos + L]
        pos += L
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                i += 1
                if pq > 1 or tq > 3 or i + 64 * (pq + 1) > len(seg):
                    raise Damaged("bad quantisation table")
                t = np.zeros(64, dtype=np.uint16)
                for k in range(64):
                    t[ZIGZAG[k]] = (seg[i] << 8 | seg[i + 1]) if pq else seg[i]
                    i += 1 + pq
                quant[tq] = t
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise Damaged("bad Huffman table")
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                i += 17
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or i + total > len(seg):
                    raise Damaged("bad Huffman table")
                codes, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        if code >= 1 << length:
                            raise Damaged("Huffman table with too many codes")
                        codes[(length, code)] = seg[i + k]
                        code += 1
                        k += 1
                    code <<= 1
                i += total
                huff[(tc, th)] = codes
        elif m == 0xDD:
            if len(seg) != 2:
                raise Damaged("bad restart interval")
            restart = seg[0] << 8 | seg[1]
        elif m == 0xE0:
            if len(seg) >= 14 and seg[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xC0:
            if frame is not None:
                raise Unsupported("two frames")
            if len(seg) < 6:
                raise Damaged("bad frame header")
            prec, H, W, nc = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if len(seg) != 6 + 3 * nc:
                raise Damaged("bad frame header")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
            frame = (prec, H, W, comps)
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Unsupported("SOF%d" % (m - 0xC0))
        elif m == 0xCC or m == 0xDC or m == 0xC8:
            raise Unsupported("marker %02x" % m)
        elif m == 0xDA:
            if frame is None:
                raise Damaged("scan before frame")
            break
    prec, H, W, comps = frame
    nc = len(comps)
    if prec != 8 or H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE or nc not in (1, 3):
        raise Unsupported("frame")
    samp = [(h, v) for _, h, v, _ in comps]
    if nc == 1:
        if samp[0] != (1, 1):
            raise Unsupported("sampling")
    else:
        if samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise Unsupported("sampling")
        if not jfif:
            if adobe is not None:
                if adobe != 1:
                    raise Unsupported("Adobe transform %d" % adobe)
            elif [c[0] for c in comps] == [0x52, 0x47, 0x42]:
                raise Unsupported("RGB component ids")
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise Damaged("bad scan header")
    if seg[0] != nc:
        raise Unsupported("more than one scan")
    sel = []
    for c in range(nc):
        if seg[1 + 2 * c] != comps[c][0]:
            raise Unsupported("scan component order")
        sel.append((seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15))
    if tuple(seg[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
        raise Unsupported("spectral selection")
    hs, vs = samp[0]
    mx, my = _ceil_div(W, 8 * hs), _ceil_div(H, 8 * vs)
    out = dict(width=W, height=H, ncomp=nc, hs=hs, vs=vs, restart=restart, mcus=mx * my, mx=mx,
               bw=[mx * h for h, _ in samp], bh=[my * v for _, v in samp], scan=pos)
    qt, dc, ac = [], [], []
    for c in range(nc):
        if comps[c][3] > 3 or comps[c][3] not in quant or sel[c][0] > 3 or sel[c][1] > 3 \
                or (0, sel[c][0]) not in huff or (1, sel[c][1]) not in huff:
            raise Damaged("a missing table")
        qt.append(quant[comps[c][3]])
        dc.append(huff[(0, sel[c][0])])
        ac.append(huff[(1, sel[c][1])])
    out.update(qtab=np.stack(qt), dc=dc, ac=ac)
    return out


def probe(data):
    """dict of the frame's geometry with supported = True, or dict(supported=False)"""
    try:
        p = parse(data)
    except (Unsupported, Damaged):
        return dict(supported=False)
    return dict(supported=True, width=p["width"], height=p["height"], ncomp=p["ncomp"], hs=p["hs"], vs=p["vs"],
                restart=p["restart"], bw=p["bw"], bh=p["bh"])


class _Bits:
    """the entropy-coded segment one bit at a time: FF 00 is a data FF, anything else after FF ends the data"""

    def __init__(self, data, pos):
        self.d, self.pos, self.cur, self.left = data, pos, 0, 0

    def bit(self):
        if self.left == 0:
            d = self.d
            if self.pos >= len(d):
                raise Damaged("truncated scan")
            b = d[self.pos]
            if b == 0xFF:
                if self.pos + 1 >= len(d):
                    raise Damaged("truncated scan")
                if d[self.pos + 1] != 0:
                    raise Damaged("marker inside an MCU")
                self.pos += 2
            else:
                self.pos += 1
            self.cur, self.left = b, 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v

    def symbol(self, codes):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bit()
            s = codes.get((length, code))
            if s is not None:
                return s
        raise Damaged("a code that is not in the table")

    def marker(self):
        """drop the rest of the byte, skip fill bytes, return the marker that follows"""
        if self.left >= 8:
            raise Damaged("whole bytes left before a marker")
        self.left = 0
        d = self.d
        if self.pos >= len(d) or d[self.pos] != 0xFF:
            raise Damaged("no marker where one is due")
        while self.pos < len(d) and d[self.pos] == 0xFF:
            self.pos += 1
        if self.pos >= len(d):
            raise Damaged("truncated scan")
        self.pos += 1
        return d[self.pos - 1]


def _extend(v, s):
    return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def entropy_decode(data):
    """-> (parse() dict, [per component int16 [bh * bw, 64] in natural order], qtab uint16 [3, 64] (unused rows zero))"""
    data = bytes(data)
    p = parse(data)
    nc, hs, vs = p["ncomp"], p["hs"], p["vs"]
    coef = [np.zeros((p["bh"][c] * p["bw"][c], 64), dtype=np.int16) for c in range(nc)]
    bits = _Bits(data, p["scan"])
    pred = [0] * nc
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    for mcu in range(p["mcus"]):
        if p["restart"] and mcu and mcu % p["restart"] == 0:
            if bits.marker() != 0xD0 + (mcu // p["restart"] - 1) % 8:
                raise Damaged("restart marker out of order")
            pred = [0] * nc
        my, mx = divmod(mcu, p["mx"])
        for c in range(nc):
            h, v = samp[c]
            q = p["qtab"][c].astype(np.int64)
            for by in range(v):
                for bx in range(h):
                    blk = coef[c][(my * v + by) * p["bw"][c] + mx * h + bx]
                    s = bits.symbol(p["dc"][c])
                    if s > 11:
                        raise Damaged("DC size")
                    pred[c] += _extend(bits.bits(s), s) if s else 0
                    if not -32768 <= pred[c] <= 32767 or abs(pred[c] * q[0]) > 32767:
                        raise Damaged("DC range")
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(p["ac"][c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            if k > 63:
                                raise Damaged("run past coefficient 63")
                            continue
                        k += r
                        if k > 63:
                            raise Damaged("run past coefficient 63")
                        if s > 10:
                            raise Damaged("AC size")
                        val = _extend(bits.bits(s), s)
                        if abs(val * q[ZIGZAG[k]]) > 32767:
                            raise Damaged("coefficient range")
                        blk[ZIGZAG[k]] = val
                        k += 1
    if bits.marker() != 0xD9:
        raise Damaged("no end-of-image marker behind the scan")
    qtab = np.zeros((3, 64), dtype=np.uint16)
    qtab[:nc] = p["qtab"]
    return p, coef, qtab


def golden_records(G):
    """records of tests/golden/f22_jpeg_pil.npz: [(name, kind, stream bytes, PIL's RGB pixels [H, W, 3] or None)]"""
    so, po = G["stream_off"], G["pixel_off"]
    out = []
    for i, name in enumerate(G["names"]):
        kind = int(G["kinds"][i])
        H, W = (int(v) for v in G["shapes"][i])
        pix = G["pixels"][po[i]:po[i + 1]].reshape(H, W, 3) if kind != 2 else None
        out.append((str(name), kind, G["streams"][so[i]:so[i + 1]].tobytes(), pix))
    return out


# ---- reconstruction: the arithmetic of vr_jpeg_reconstruct_u8 -------------------------------------------------------------------------
def _sra(x, n):
    return x >> n                                           # numpy's >> on signed integers is arithmetic


def _idct_pass(x, shift):
    """libjpeg jidctint (ISLOW) butterfly along the last axis of x [..., 8] (int64), descaled by `shift` with rounding"""
    c0, c1, c2, c3, c4, c5, c6, c7 = (x[..., i] for i in range(8))
    z1 = (c2 + c6) * 4433
    t2 = z1 - c6 * 15137
    t3 = z1 + c2 * 6270
    t0 = (c0 + c4) << 13
    t1 = (c0 - c4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = c7, c5, c3, c1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([_sra(t10 + o3 + r, shift), _sra(t11 + o2 + r, shift), _sra(t12 + o1 + r, shift), _sra(t13 + o0 + r, shift),
                     _sra(t13 - o0 + r, shift), _sra(t12 - o1 + r, shift), _sra(t11 - o2 + r, shift), _sra(t10 - o3 + r, shift)],
                    axis=-1)


def idct_plane(coef, qtab, bw, bh):
    """coef int16 [bh * bw, 64], qtab [64] -> the block-padded sample plane uint8 [bh * 8, bw * 8]"""
    x = coef.astype(np.int64).reshape(bh * bw, 8, 8) * qtab.astype(np.int64).reshape(1, 8, 8)
    x = _idct_pass(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)                     # columns first
    x = _idct_pass(x, 18)
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2(t, half_lo, half_hi, shift):
    """out[2i] = (3 t[i] + t[i-1] + half_lo) >> shift, out[2i+1] = (3 t[i] + t[i+1] + half_hi) >> shift, edges replicated"""
    left = np.concatenate([t[:, :1], t[:, :-1]], axis=1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * t + left + half_lo) >> shift
    out[:, 1::2] = (3 * t + right + half_hi) >> shift
    return out


def upsample(p, hs, vs):
    """a chroma plane [dh, dw] of a frame whose luma is sampled hs x vs -> [dh * vs, dw * hs]"""
    p = p.astype(np.int64)
    dh, dw = p.shape
    if hs == 1 and vs == 1:
        return p
    if dw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)
    if vs == 1:
        return _h2(p, 1, 2, 2)
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * dh, 2 * dw), dtype=np.int64)
    out[0::2] = _h2(3 * p + up, 8, 7, 4)
    out[1::2] = _h2(3 * p + down, 8, 7, 4)
    return out


def to_rgb(planes, W, H, hs, vs):
    """the component sample planes (block-padded) -> RGB uint8 [H, W, 3]"""
    y = planes[0][:H, :W].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    dw, dh = _ceil_div(W, hs), _ceil_div(H, vs)
    cb, cr = (upsample(planes[c][:dh, :dw], hs, vs)[:H, :W] - 128 for c in (1, 2))
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    """encoded baseline stream -> RGB uint8 [H, W, 3] (what Image.open(...).convert('RGB') gives)"""
    p, coef, qtab = entropy_decode(data)
    planes = [idct_plane(coef[c], qtab[c], p["bw"][c], p["bh"][c]) for c in range(p["ncomp"])]
    return to_rgb(planes, p["width"], p["height"], p["hs"], p["vs"])


def record_ok(d, blob_bytes, Hs, Ws):
    """the device's own test of one vr_jpeg_desc (16 int32)"""
    kind, W, H, nc, hs, vs = (int(v) for v in d[:6])
    if kind not in (0, 1) or not 1 <= W <= min(Ws, MAX_SIDE) or not 1 <= H <= min(Hs, MAX_SIDE):
        return False
    if kind == 1:
        if (nc, hs, vs) != (3, 1, 1):
            return False
    elif not ((nc == 1 and (hs, vs) == (1, 1)) or (nc == 3 and (hs, vs) in ((1, 1), (2, 1), (2, 2)))):
        return False
    mx, my = _ceil_div(W, 8 * hs), _ceil_div(H, 8 * vs)
    for c in range(nc):
        off, bw, bh = int(d[D_OFF + c]), int(d[D_BW + c]), int(d[D_BH + c])
        if bw != mx * (hs if c == 0 else 1) or bh != my * (vs if c == 0 else 1):
            return False
        if off < 0 or off * 16 + bw * bh * (64 if kind else 128) > blob_bytes:
            return False
    return True


def reconstruct_u8(blob, descs, qtabs, Hs, Ws):
    """The device entry on the CPU: blob uint8 [n], descs int32 [B, 16], qtabs uint16 [B, 3, 64] -> canvas uint8 [B, 3, Hs, Ws]"""
    blob, descs = np.asarray(blob, dtype=np.uint8), np.asarray(descs, dtype=np.int32)
    qtabs = np.asarray(qtabs).view(np.uint16)
    B = descs.shape[0]
    canvas = np.zeros((B, 3, Hs, Ws), dtype=np.uint8)
    for b in range(B):
        d = descs[b]
        if not record_ok(d, blob.size, Hs, Ws):
            continue
        kind, W, H, nc, hs, vs = (int(v) for v in d[:6])
        planes = []
        for c in range(nc):
            off, bw, bh = int(d[D_OFF + c]) * 16, int(d[D_BW + c]), int(d[D_BH + c])
            if kind == 1:
                planes.append(blob[off:off + bw * bh * 64].reshape(bh * 8, bw * 8))
            else:
                coef = blob[off:off + bw * bh * 128].view(np.int16).reshape(bw * bh, 64)
                planes.append(idct_plane(coef, qtabs[b, c], bw, bh))
        if kind == 1:
            rgb = np.stack([pl[:H, :W] for pl in planes], axis=2)
        else:
            rgb = to_rgb(planes, W, H, hs, vs)
        canvas[b, :, :H, :W] = rgb.transpose(2, 0, 1)
    return canvas
