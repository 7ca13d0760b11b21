// libvitres_jpeg.so: markers and Huffman decoding of baseline JPEG on the host, up to the quantised coefficients
// (include/vitres_jpeg.h).  No HIP here: DataLoader workers load this library and nothing of libvitres_hip.so.
//
// The decoder is table driven: a 64-bit bit buffer topped up eight bytes at a time where no FF is near, else a byte at a time
// (FF 00 unstuffed, a marker stops the feed); a 9-bit lookahead table per Huffman table that resolves every code of up to 9 bits in
// one probe, and libjpeg's maxcode / valoffset walk for the longer ones.  The two data-dependent branches a bit-serial decoder
// mispredicts -- "refill now?" on every byte and the sign of every coefficient -- are written without a branch.  All state lives
// on the caller's stack.
#include "../../include/vitres_jpeg.h"

#include <string.h>

#define VR_OK 0
#define VR_EINVAL (-1)
#define VR_EUNSUPPORTED (-3)

namespace {

constexpr int LOOK_BITS = 9;
constexpr int MAX_SIDE = 8192;

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTab {
    bool present;
    uint16_t look[1 << LOOK_BITS];      // (length << 8) | symbol for codes of up to LOOK_BITS bits, 0: longer
    int32_t maxcode[18];                // largest code of each length, -1: none
    int32_t valoff[17];                 // index of a length's first symbol minus its first code
    uint8_t vals[256];
};

struct Parsed {
    vr_jpeg_info info;
    uint16_t quant[4][64];              // natural order
    bool quant_present[4];
    HuffTab huff[2][4];                 // [class: 0 DC, 1 AC][id]
    int tq[3], td[3], ta[3];
    int mcu_x, mcu_y;
    int64_t scan;                       // offset of the entropy-coded bytes
};

enum { P_OK = 0, P_UNSUPPORTED = 1, P_DAMAGED = 2 };

// counts[16], symbols -> the decoding tables; false when the counts do not describe a prefix code
bool build_huff(HuffTab& t, const uint8_t* counts, const uint8_t* vals, int total) {
    memset(&t, 0, sizeof(t));
    memcpy(t.vals, vals, (size_t)total);
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = counts[len - 1];
        if (n == 0) {
            t.maxcode[len] = -1;
        } else {
            if (code + (uint32_t)n > (1u << len)) return false;
            t.valoff[len] = k - (int32_t)code;
            if (len <= LOOK_BITS) {
                for (int i = 0; i < n; ++i) {
                    const uint32_t first = (code + (uint32_t)i) << (LOOK_BITS - len);
                    const uint16_t e = (uint16_t)((len << 8) | vals[k + i]);
                    for (uint32_t j = 0; j < (1u << (LOOK_BITS - len)); ++j) t.look[first + j] = e;
                }
            }
            code += (uint32_t)n;
            k += n;
            t.maxcode[len] = (int32_t)code - 1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.present = true;
    return true;
}

int parse_headers(const uint8_t* d, int64_t n, Parsed& P) {
    memset(&P.info, 0, sizeof(P.info));
    memset(P.quant_present, 0, sizeof(P.quant_present));
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 4; ++i) P.huff[c][i].present = false;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return P_UNSUPPORTED;
    int64_t pos = 2;
    bool jfif = false, have_adobe = false, have_frame = false;
    int adobe = 0, restart = 0, prec = 0, H = 0, W = 0, nc = 0;
    int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0};
    const uint8_t* seg = nullptr;
    int seglen = 0;
    for (;;) {
        if (pos >= n) return P_DAMAGED;
        if (d[pos] != 0xFF) return P_DAMAGED;
        while (pos < n && d[pos] == 0xFF) ++pos;
        if (pos >= n) return P_DAMAGED;
        const int m = d[pos++];
        if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0x00) return P_UNSUPPORTED;
        if (pos + 2 > n) return P_DAMAGED;
        const int L = d[pos] << 8 | d[pos + 1];
        if (L < 2 || pos + L > n) return P_DAMAGED;
        seg = d + pos + 2;
        seglen = L - 2;
        pos += L;
        if (m == 0xDB) {
            int i = 0;
            while (i < seglen) {
                const int pq = seg[i] >> 4, tq = seg[i] & 15;
                ++i;
                if (pq > 1 || tq > 3 || i + 64 * (pq + 1) > seglen) return P_DAMAGED;
                for (int k = 0; k < 64; ++k) {
                    P.quant[tq][kZigzag[k]] = pq ? (uint16_t)(seg[i] << 8 | seg[i + 1]) : seg[i];
                    i += 1 + pq;
                }
                P.quant_present[tq] = true;
            }
        } else if (m == 0xC4) {
            int i = 0;
            while (i < seglen) {
                if (i + 17 > seglen) return P_DAMAGED;
                const int tc = seg[i] >> 4, th = seg[i] & 15;
                int total = 0;
                for (int k = 1; k <= 16; ++k) total += seg[i + k];
                if (tc > 1 || th > 3 || total > 256 || i + 17 + total > seglen) return P_DAMAGED;
                if (!build_huff(P.huff[tc][th], seg + i + 1, seg + i + 17, total)) return P_DAMAGED;
                i += 17 + total;
            }
        } else if (m == 0xDD) {
            if (seglen != 2) return P_DAMAGED;
            restart = seg[0] << 8 | seg[1];
        } else if (m == 0xE0) {
            if (seglen >= 14 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (seglen >= 12 && memcmp(seg, "Adobe", 5) == 0) {
                have_adobe = true;
                adobe = seg[11];
            }
        } else if (m == 0xC0) {
            if (have_frame) return P_UNSUPPORTED;
            if (seglen < 6) return P_DAMAGED;
            prec = seg[0];
            H = seg[1] << 8 | seg[2];
            W = seg[3] << 8 | seg[4];
            nc = seg[5];
            if (seglen != 6 + 3 * nc) return P_DAMAGED;
            for (int c = 0; c < nc && c < 3; ++c) {
                cid[c] = seg[6 + 3 * c];
                ch[c] = seg[7 + 3 * c] >> 4;
                cv[c] = seg[7 + 3 * c] & 15;
                P.tq[c] = seg[8 + 3 * c];
            }
            have_frame = true;
        } else if (m >= 0xC1 && m <= 0xCF) {            // SOF1.., JPG, DAC (0xC4 was taken above)
            return P_UNSUPPORTED;
        } else if (m == 0xDC) {
            return P_UNSUPPORTED;
        } else if (m == 0xDA) {
            if (!have_frame) return P_DAMAGED;
            break;
        }
    }
    if (prec != 8 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || (nc != 1 && nc != 3)) return P_UNSUPPORTED;
    if (nc == 1) {
        if (ch[0] != 1 || cv[0] != 1) return P_UNSUPPORTED;
    } else {
        const bool luma = (ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2);
        if (!luma || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return P_UNSUPPORTED;
        if (!jfif) {
            if (have_adobe) {
                if (adobe != 1) return P_UNSUPPORTED;
            } else if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') {
                return P_UNSUPPORTED;
            }
        }
    }
    if (seglen < 1 || seglen != 4 + 2 * seg[0]) return P_DAMAGED;
    if (seg[0] != nc) return P_UNSUPPORTED;
    for (int c = 0; c < nc; ++c) {
        if (seg[1 + 2 * c] != cid[c]) return P_UNSUPPORTED;
        P.td[c] = seg[2 + 2 * c] >> 4;
        P.ta[c] = seg[2 + 2 * c] & 15;
    }
    if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0) return P_UNSUPPORTED;
    for (int c = 0; c < nc; ++c) {
        if (P.tq[c] > 3 || !P.quant_present[P.tq[c]] || P.td[c] > 3 || P.ta[c] > 3 || !P.huff[0][P.td[c]].present
            || !P.huff[1][P.ta[c]].present)
            return P_DAMAGED;
    }
    const int hs = ch[0], vs = cv[0];
    P.mcu_x = (W + 8 * hs - 1) / (8 * hs);
    P.mcu_y = (H + 8 * vs - 1) / (8 * vs);
    vr_jpeg_info& I = P.info;
    I.supported = 1;
    I.width = W;
    I.height = H;
    I.ncomp = nc;
    I.hs = hs;
    I.vs = vs;
    I.restart_interval = restart;
    for (int c = 0; c < nc; ++c) {
        I.bw[c] = P.mcu_x * (c == 0 ? hs : 1);
        I.bh[c] = P.mcu_y * (c == 0 ? vs : 1);
        I.blocks[c] = I.bw[c] * I.bh[c];
    }
    P.scan = pos;
    return P_OK;
}

// the entropy-coded bytes as a bit stream: valid bits sit at the top of `acc`
struct BitReader {
    const uint8_t* d;
    int64_t pos, n;
    uint64_t acc;
    int nbits;

    // Bits of `acc` below the top `nbits` are either zero or a preview of the bytes at `pos` (what the fast path leaves there):
    // nothing reads them as data, and ORing the same bytes in again later changes nothing.
    inline void fill() {
        // eight bytes at once while none of them is FF (nothing to unstuff, no marker): the common case, and without a branch on
        // the data
        if (pos + 8 <= n) {
            uint64_t w;
            memcpy(&w, d + pos, 8);
            w = __builtin_bswap64(w);
            const uint64_t inv = ~w;                                    // a zero byte of inv is an FF byte of w
            if (((inv - 0x0101010101010101ull) & ~inv & 0x8080808080808080ull) == 0) {
                acc |= w >> nbits;
                pos += (63 - nbits) >> 3;                               // whole bytes that fit
                nbits |= 56;
                return;
            }
        }
        acc = nbits ? acc & ~(~0ull >> nbits) : 0;                      // drop the preview: the byte loop ORs into zeros
        while (nbits <= 56) {
            if (pos >= n) return;
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n || d[pos + 1] != 0x00) return;    // a marker (or fill bytes before one), or the end: no more data bits
                pos += 2;
            } else {
                ++pos;
            }
            acc |= (uint64_t)b << (56 - nbits);
            nbits += 8;
        }
    }
    inline void drop(int k) {
        acc <<= k;
        nbits -= k;
    }
    // the next Huffman symbol, -1: the code is not in the table or the data ran out
    inline int symbol(const HuffTab& t) {
        if (nbits < 32) fill();                                         // (a code and the value bits behind it: at most 27)
        const uint16_t e = t.look[acc >> (64 - LOOK_BITS)];
        if (e) {
            const int len = e >> 8;
            if (len > nbits) return -1;
            drop(len);
            return e & 255;
        }
        const int32_t code16 = (int32_t)(acc >> 48);
        for (int len = LOOK_BITS + 1; len <= 16; ++len) {
            const int32_t code = code16 >> (16 - len);
            if (code <= t.maxcode[len]) {
                const int32_t idx = code + t.valoff[len];
                if (len > nbits || idx < 0 || idx > 255) return -1;
                drop(len);
                return t.vals[idx];
            }
        }
        return -1;
    }
    // s bits (1..16) as a JPEG-extended signed value; false when the data ran out
    inline bool receive(int s, int32_t& v) {
        if (nbits < s) {
            fill();
            if (nbits < s) return false;
        }
        const int32_t raw = (int32_t)(acc >> (64 - s));
        drop(s);
        v = raw + (((raw - (1 << (s - 1))) >> 31) & (1 - (1 << s)));      // JPEG's EXTEND, without a branch on the sign bit
        return true;
    }
    // drop the rest of the byte, skip fill bytes, return the marker that follows; -1: there is none
    inline int marker() {
        if (nbits >= 8) return -1;
        acc = 0;
        nbits = 0;
        if (pos >= n || d[pos] != 0xFF) return -1;
        while (pos < n && d[pos] == 0xFF) ++pos;
        if (pos >= n) return -1;
        return d[pos++];
    }
};

inline bool in_range(int32_t v, uint16_t q) {
    const int32_t p = v * (int32_t)q;                             // |v| <= 32768, q <= 65535: no overflow
    return p >= -32767 && p <= 32767;
}

// (works on a copy of the reader so that the bit buffer stays in registers across the block; written back on success only -- a
// failed block ends the decode)
bool decode_block(BitReader& reader, const HuffTab& dc, const HuffTab& ac, const uint16_t* q, int32_t& pred, int16_t* blk) {
    BitReader br = reader;
    int s = br.symbol(dc);
    if (s < 0 || s > 11) return false;
    if (s) {
        int32_t diff;
        if (!br.receive(s, diff)) return false;
        pred += diff;
    }
    if (pred < -32768 || pred > 32767 || !in_range(pred, q[0])) return false;
    if (pred) blk[0] = (int16_t)pred;
    int k = 1;
    while (k < 64) {
        const int rs = br.symbol(ac);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            if (k > 63) return false;
            continue;
        }
        k += r;
        if (k > 63 || s > 10) return false;
        int32_t v;
        if (!br.receive(s, v)) return false;
        const int nat = kZigzag[k];
        if (!in_range(v, q[nat])) return false;
        blk[nat] = (int16_t)v;
        ++k;
    }
    reader = br;
    return true;
}

}  // namespace

extern "C" int vr_jpeg_probe(const uint8_t* data, int64_t len, vr_jpeg_info* info) {
    if (!data || !info || len < 0) return VR_EINVAL;
    Parsed P;
    if (parse_headers(data, len, P) != P_OK) memset(&P.info, 0, sizeof(P.info));
    *info = P.info;
    return VR_OK;
}

extern "C" int vr_jpeg_entropy_decode(const uint8_t* data, int64_t len, vr_jpeg_info* info, int16_t* coef, int64_t coef_capacity,
                                      uint16_t* qtab) {
    if (!data || !info || !coef || !qtab || len < 0) return VR_EINVAL;
    Parsed P;
    const int st = parse_headers(data, len, P);
    if (st != P_OK) {
        memset(info, 0, sizeof(*info));
        return st == P_UNSUPPORTED ? VR_EUNSUPPORTED : VR_EINVAL;
    }
    *info = P.info;
    const vr_jpeg_info& I = P.info;
    const int nc = I.ncomp;
    int64_t base[3] = {0, 0, 0}, total = 0;
    for (int c = 0; c < nc; ++c) {
        base[c] = total;
        total += (int64_t)I.blocks[c] * 64;
    }
    if (coef_capacity < total) return VR_EINVAL;
    memset(qtab, 0, 3 * 64 * sizeof(uint16_t));
    for (int c = 0; c < nc; ++c) memcpy(qtab + 64 * c, P.quant[P.tq[c]], 64 * sizeof(uint16_t));

    BitReader br = {data, P.scan, len, 0, 0};
    int32_t pred[3] = {0, 0, 0};
    const int hb[3] = {I.hs, 1, 1}, vb[3] = {I.vs, 1, 1};
    const int64_t mcus = (int64_t)P.mcu_x * P.mcu_y;
    int64_t to_restart = I.restart_interval;
    int next_rst = 0, mx = 0, my = 0;
    for (int64_t mcu = 0; mcu < mcus; ++mcu) {
        if (I.restart_interval && mcu) {
            if (to_restart == 0) {
                if (br.marker() != 0xD0 + next_rst) return VR_EINVAL;
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
                to_restart = I.restart_interval;
            }
        }
        --to_restart;
        for (int c = 0; c < nc; ++c) {
            const HuffTab& dc = P.huff[0][P.td[c]];
            const HuffTab& ac = P.huff[1][P.ta[c]];
            const uint16_t* q = qtab + 64 * c;
            for (int by = 0; by < vb[c]; ++by) {
                for (int bx = 0; bx < hb[c]; ++bx) {
                    const int64_t blk = (int64_t)(my * vb[c] + by) * I.bw[c] + (mx * hb[c] + bx);
                    if (!decode_block(br, dc, ac, q, pred[c], coef + base[c] + blk * 64)) return VR_EINVAL;
                }
            }
        }
        if (++mx == P.mcu_x) {
            mx = 0;
            ++my;
        }
    }
    if (br.marker() != 0xD9) return VR_EINVAL;
    return VR_OK;
}
