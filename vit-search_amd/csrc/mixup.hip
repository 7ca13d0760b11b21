// SwitchTokenMix on the device (reference token_mixup.py:39-162): the input side of the training step.
// The random draws (two torch.randperm, the Beta samples and the box from numpy) stay on the host with the reference's
// generators and call order (vitres/token_mixup.py); what is heavy -- rewriting the 77 MB image batch and building the
// 8 MB of soft patch targets -- is two streaming kernels, one read and one write per element, bit-exact with the
// reference's fp32 arithmetic (products rounded separately, then added: no FMA contraction).
//   rows [0, half)  : out = partner's pixels inside the box, own pixels outside; patch targets follow the box
//   rows [half, B)  : out = x * lam + partner * (1 - lam); every patch target = the mixed image target
// Further down: the uint8 forms (normalise inside the pass), timm's Mixup / CutMix (vr_mixup, vr_mixup_u8; vitres/mixup.py) and timm's
// RandomErasing as a counter-based noise the uint8 forms substitute while they read (the *_erase entries; vitres/random_erasing.py).
#include "common.h"
#include "../../include/vitres_hip.h"

namespace {

// fl(fl(a * la) + fl(b * lb)): hipcc contracts a*b+c into an FMA by default (-ffp-contract=fast), also through __fmul_rn
__device__ __forceinline__ float mix2(float a, float la, float b, float lb) {
#pragma clang fp contract(off)
    const float p = a * la;
    const float q = b * lb;
    return p + q;
}

__global__ __launch_bounds__(256) void mix_samples_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          const int64_t* __restrict__ partner, int B, int C, int H, int W,
                                                          int half, int py0, int py1, int px0, int px1, float lam, float oml) {
    const int w4 = W / 4;
    const long long per = (long long)C * H * w4, total = (long long)B * per;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / per);
        const long long r = idx % per;
        const int x = (int)(r % w4) * 4, yrow = (int)((r / w4) % H);
        const long long off = (long long)b * C * H * W + r * 4;
        const long long poff = (long long)partner[b] * C * H * W + r * 4;
        const float4 a = *reinterpret_cast<const float4*>(in + off);
        float4 o = a;
        if (b < half) {
            if (yrow >= py0 && yrow < py1 && x + 3 >= px0 && x < px1) {
                const float4 p = *reinterpret_cast<const float4*>(in + poff);
                if (x + 0 >= px0 && x + 0 < px1) o.x = p.x;
                if (x + 1 >= px0 && x + 1 < px1) o.y = p.y;
                if (x + 2 >= px0 && x + 2 < px1) o.z = p.z;
                if (x + 3 >= px0 && x + 3 < px1) o.w = p.w;
            }
        } else {
            const float4 p = *reinterpret_cast<const float4*>(in + poff);
            o = make_float4(mix2(a.x, lam, p.x, oml), mix2(a.y, lam, p.y, oml), mix2(a.z, lam, p.z, oml), mix2(a.w, lam, p.w, oml));
        }
        *reinterpret_cast<float4*>(out + off) = o;
    }
}

// one workgroup per sample: targets[b, :] and patch_targets[b, p, :] for all p
__global__ __launch_bounds__(256) void mix_targets_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ partner,
                                                          float* __restrict__ targets, float* __restrict__ patch_targets, int K,
                                                          int PL, int half, int y0, int y1, int x0, int x1, float lam_p,
                                                          float oml_p, float lam_i, float oml_i, float on, float off) {
    const int b = blockIdx.x;
    const int la = (int)labels[b], lb = (int)labels[partner[b]];
    const bool patch = b < half;
    const float l = patch ? lam_p : lam_i, m = patch ? oml_p : oml_i;
    for (int c = threadIdx.x; c < K; c += blockDim.x) {
        const float ya = c == la ? on : off, yb = c == lb ? on : off;
        const float t = mix2(ya, l, yb, m);
        targets[(long long)b * K + c] = t;
        for (int p = 0; p < PL * PL; ++p) {
            const int i = p / PL, j = p % PL;
            const bool in = i >= y0 && i < y1 && j >= x0 && j < x1;
            patch_targets[((long long)b * PL * PL + p) * K + c] = patch ? (in ? yb : ya) : t;
        }
    }
}

// ---- uint8 input side: timm's fast_collate batches (uint8 NCHW), normalised on the device as its PrefetchLoader does
// (input.float().sub_(mean).div_(std), mean / std = the 0..1 constants * 255).  n(u, c) = (float(u) - mean[c]) / std[c] with
// the correctly rounded division hipcc emits by default (v_div_scale / v_div_fmas / v_div_fixup; no fast-math flag on this
// file): bit-identical with the CPU statement.  A lane takes V = 16 pixels (one 16-byte load, four 16-byte stores) when the
// row length and the pointer allow it, V = 4 otherwise; the 4x smaller read is why the normaliser rides in the mixer.
struct NormParams {
    float mean[4], std[4];
};

__device__ __forceinline__ float pick4(const float (&v)[4], int c) {      // (a per-lane index into kernel arguments: selects, no scratch)
    return c == 0 ? v[0] : c == 1 ? v[1] : c == 2 ? v[2] : v[3];
}

__device__ __forceinline__ float norm1(uint32_t u, float m, float s) { return ((float)u - m) / s; }

template <int V>
struct U8Vec;
template <>
struct U8Vec<4> {
    uint32_t w[1];
    __device__ __forceinline__ void load(const uint8_t* p) { w[0] = *reinterpret_cast<const uint32_t*>(p); }
};
template <>
struct U8Vec<16> {
    uint32_t w[4];
    __device__ __forceinline__ void load(const uint8_t* p) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
};
template <int V>
__device__ __forceinline__ uint32_t u8_at(const U8Vec<V>& v, int i) { return (v.w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// ---- timm's RandomErasing (timm/data/random_erasing.py; the reference's --reprob 0.25 --remode pixel --recount 1) on the device.
// The host draws up to R rectangles per sample (vitres/random_erasing.py); what fills them is a pure function of
// (seed, call, sample, channel, y, x, mode, rectangle index for 'rand'): Philox4x32-10 keyed by the seed, counter
// (quad or rectangle index, sample + (domain << 24), call lo, call hi), its four words turned into four N(0,1) values by two
// Box-Muller pairs with the accurate logf / sqrtf / sinf / cosf (include/vitres_hip.h has the contract).  So "erase, then mix" is no
// pass of its own: a lane about to use pixels of sample s -- its own or the partner's -- checks s's rectangles and substitutes.
struct EraseParams {
    const vr_erase_rect* rects;
    int R, mode;
    uint32_t k0, k1, call_lo, call_hi;
    int H, W;                                                              // (normalize_u8_kernel has no other source for them)
};
template <bool ERASE>
struct EraseArg {};
template <>
struct EraseArg<true> {
    EraseParams e;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// four N(0,1) values of counter word `w0` (domain 0: the quad index -> pixels x..x+3; domain 1: the rectangle index -> channels 0..3)
__device__ __forceinline__ void erase_noise4(const EraseParams& e, uint32_t w0, int s, uint32_t domain, float (&z)[4]) {
#pragma clang fp contract(off)
    uint32_t r[4];
    philox4x32_10(w0, (uint32_t)s + (domain << 24), e.call_lo, e.call_hi, e.k0, e.k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = (float)((r[2 * h] >> 8) + 1u) * 0x1p-24f;         // (0, 1]: exact
        const float u2 = (float)(r[2 * h + 1] >> 8) * 0x1p-24f;            // [0, 1): exact
        const float rad = sqrtf(-2.f * logf(u1));
        const float ang = 6.2831853071795864769f * u2;
        z[2 * h] = rad * cosf(ang);
        z[2 * h + 1] = rad * sinf(ang);
    }
}

// does a rectangle of sample s meet pixels [x, x + n) of row y?  (rectangles are device data: compared with, never indexed by)
__device__ __forceinline__ bool erase_meets(const vr_erase_rect& rc, int y, int x, int n) {
    return y >= rc.y0 && y < rc.y1 && x + n > rc.x0 && x < rc.x1;
}

// o[0..V): the normalised pixels (c, y, x .. x+V) of sample s; those inside a rectangle of s get its fill, the later rectangle winning
template <int V>
__device__ __forceinline__ void erase_lane(float (&o)[V], const EraseParams& e, int s, int c, int H, int W, int y, int x) {
    const vr_erase_rect* rs = e.rects + (long long)s * e.R;
    for (int r = 0; r < e.R; ++r) {
        const vr_erase_rect rc = rs[r];
        if (!erase_meets(rc, y, x, V)) continue;
        if (e.mode == VR_ERASE_PIXEL) {
            const uint32_t q0 = (uint32_t)((((long long)c * H + y) * W + x) >> 2);
#pragma unroll
            for (int q = 0; q < V / 4; ++q) {
                if (!erase_meets(rc, y, x + 4 * q, 4)) continue;
                float z[4];
                erase_noise4(e, q0 + q, s, 0u, z);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + 4 * q + k >= rc.x0 && x + 4 * q + k < rc.x1) o[4 * q + k] = z[k];
            }
        } else {
            float v = 0.f;
            if (e.mode == VR_ERASE_RAND) {
                float z[4];
                erase_noise4(e, (uint32_t)r, s, 1u, z);
                v = pick4(z, c);
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (x + i >= rc.x0 && x + i < rc.x1) o[i] = v;
        }
    }
}

// does any rectangle of sample s meet pixels [x, x + n) of row y?
__device__ __forceinline__ bool erase_hits(const EraseParams& e, int s, int y, int x, int n) {
    bool hit = false;
    for (int r = 0; r < e.R; ++r) hit = hit || erase_meets(e.rects[(long long)s * e.R + r], y, x, n);
    return hit;
}

// A lane of a uint8 kernel whose pixels meet a rectangle of a sample it reads leaves the kernel's own path (which stays the code
// it is without ERASE -- few registers, many waves in flight) for this one: quad by quad, not unrolled, so that Philox and the
// Box-Muller functions exist once per sample role and their registers are not added to sixteen live pixels.  Per quad: the own
// bytes again (they are in cache), normalised, erased under sample b; where the mix takes the partner -- MIX_BOX: pixels of
// [px0, px1), MIX_BLEND: all -- the partner's bytes, normalised, erased under sample pb; then the choice / mix2 on the fp32 values.
enum { MIX_NONE = 0, MIX_BOX = 1, MIX_BLEND = 2 };

template <int V>
__device__ __forceinline__ void erased_lane(const uint8_t* __restrict__ in, float* __restrict__ out, long long off, long long poff,
                                            int mix, int px0, int px1, float lam, float oml, float m, float s, const EraseParams& e,
                                            int b, int pb, int c, int H, int W, int y, int x) {
#pragma unroll 1
    for (int q = 0; q < V / 4; ++q) {
        const int xq = x + 4 * q;
        U8Vec<4> a;
        a.load(in + off + 4 * q);
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = norm1(u8_at(a, k), m, s);
        erase_lane<4>(o, e, b, c, H, W, y, xq);
        if (mix == MIX_BLEND || (mix == MIX_BOX && xq + 3 >= px0 && xq < px1)) {
            U8Vec<4> p;
            p.load(in + poff + 4 * q);
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = norm1(u8_at(p, k), m, s);
            erase_lane<4>(t, e, pb, c, H, W, y, xq);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (mix == MIX_BLEND) o[k] = mix2(o[k], lam, t[k], oml);
                else if (xq + k >= px0 && xq + k < px1) o[k] = t[k];
            }
        }
        *reinterpret_cast<float4*>(out + off + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// in place on normalised fp32: a lane owns one quad and touches memory only when a rectangle of its sample meets it
__global__ __launch_bounds__(256) void random_erase_kernel(float* __restrict__ x, int B, int C, int H, int W, EraseParams e) {
    const int w4 = W / 4;
    const long long per = (long long)C * H * w4, total = (long long)B * per;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / per);
        const long long r = idx % per;
        const int xx = (int)(r % w4) * 4, y = (int)((r / w4) % H), c = (int)(r / ((long long)w4 * H));
        if (!erase_hits(e, b, y, xx, 4)) continue;
        float4* p = reinterpret_cast<float4*>(x + (long long)b * C * H * W + r * 4);
        const float4 a = *p;
        float o[4] = {a.x, a.y, a.z, a.w};
        erase_lane<4>(o, e, b, c, H, W, y, xx);
        *p = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ERASE (here and in the two mixers below): the *_erase entry points' form; ERASE = false is the kernel as it was
template <int V, bool ERASE>
__global__ __launch_bounds__(256) void normalize_u8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, long long total,
                                                           int hwv, int C, NormParams np, EraseArg<ERASE> ea) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c = (int)((idx / hwv) % C);
        const float m = pick4(np.mean, c), s = pick4(np.std, c);
        U8Vec<V> a;
        if constexpr (ERASE) {
            const int wv = ea.e.W / V, within = (int)(idx % hwv), b = (int)(idx / ((long long)hwv * C));
            const int y = within / wv, x = (within % wv) * V;
            if (erase_hits(ea.e, b, y, x, V)) {
                erased_lane<V>(in, out, idx * V, 0, MIX_NONE, 0, 0, 0.f, 0.f, m, s, ea.e, b, b, c, ea.e.H, ea.e.W, y, x);
                continue;
            }
        }
        a.load(in + idx * V);
#pragma unroll
        for (int q = 0; q < V / 4; ++q)
            *reinterpret_cast<float4*>(out + idx * V + 4 * q) =
                make_float4(norm1(u8_at(a, 4 * q), m, s), norm1(u8_at(a, 4 * q + 1), m, s), norm1(u8_at(a, 4 * q + 2), m, s),
                            norm1(u8_at(a, 4 * q + 3), m, s));
    }
}

// mix_samples_kernel on uint8 pixels: the choice partner / own is made on the bytes (n(chosen) == chosen n), the second half
// normalises both and mixes them as mix2 does.  The partner is read only where it is used.
// With ERASE every sample is erased before it is mixed (timm erases per sample, before collation): the own pixels under the own
// sample's rectangles, a partner pixel under the PARTNER's rectangles and noise, then the choice / the blend on the fp32 values.
template <int V, bool ERASE>
__global__ __launch_bounds__(256) void mix_samples_u8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                             const int64_t* __restrict__ partner, int B, int C, int H, int W,
                                                             int half, int py0, int py1, int px0, int px1, float lam, float oml,
                                                             NormParams np, EraseArg<ERASE> ea) {
    const int wv = W / V;
    const long long per = (long long)C * H * wv, total = (long long)B * per;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / per);
        const long long r = idx % per;
        const int x = (int)(r % wv) * V, yrow = (int)((r / wv) % H), c = (int)(r / ((long long)wv * H));
        const long long off = (long long)b * C * H * W + r * V;
        const long long poff = (long long)partner[b] * C * H * W + r * V;
        const float m = pick4(np.mean, c), s = pick4(np.std, c);
        if constexpr (ERASE) {
            const int pb = (int)partner[b];
            const int mix = b >= half ? MIX_BLEND : yrow >= py0 && yrow < py1 && x + V - 1 >= px0 && x < px1 ? MIX_BOX : MIX_NONE;
            if (erase_hits(ea.e, b, yrow, x, V) || (mix != MIX_NONE && erase_hits(ea.e, pb, yrow, x, V))) {
                erased_lane<V>(in, out, off, poff, mix, px0, px1, lam, oml, m, s, ea.e, b, pb, c, H, W, yrow, x);
                continue;
            }
        }
        U8Vec<V> a, p;
        a.load(in + off);
        p = a;
        float o[V];
        if (b < half) {
            const bool box = yrow >= py0 && yrow < py1 && x + V - 1 >= px0 && x < px1;
            if (box) p.load(in + poff);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const bool take = box && x + i >= px0 && x + i < px1;
                o[i] = norm1(take ? u8_at(p, i) : u8_at(a, i), m, s);
            }
        } else {
            p.load(in + poff);
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = mix2(norm1(u8_at(a, i), m, s), lam, norm1(u8_at(p, i), m, s), oml);
        }
#pragma unroll
        for (int q = 0; q < V / 4; ++q)
            *reinterpret_cast<float4*>(out + off + 4 * q) = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}

// ---- timm's Mixup / CutMix (timm/data/mixup.py, the reference's default input mix: main.py:308-314).  Sample b is mixed with sample
// B-1-b (x.flip(0)) by its own entry of a device table: a pixel box copied from the partner (cutmix), or x * lam + partner * oml
// with separately rounded products (mix2), or -- lam == 1, the samples timm leaves alone -- a copy that never reads the partner.
// One table serves timm's batch, elem and pair modes; the host (vitres/mixup.py) draws it.  The box is in pixels and aligned to
// nothing: a lane's V pixels may straddle an edge, lie inside the box or contain it, so the choice is made per pixel.
// lam == 1 in timm's own comparison: there lam is a double in batch mode, and one just below 1 that rounds to 1.f is still blended
// (x * 1.f + partner * oml); its oml is not 0, which tells it from a true 1 (oml == 0 by either of the host's rounding rules)
__device__ __forceinline__ bool untouched(const vr_mixup_param& m) { return m.lam == 1.f && m.oml == 0.f; }

__global__ __launch_bounds__(256) void mixup_samples_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            const vr_mixup_param* __restrict__ params, int B, int C, int H, int W) {
    const int w4 = W / 4;
    const long long per = (long long)C * H * w4, total = (long long)B * per;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / per);
        const long long r = idx % per;
        const int x = (int)(r % w4) * 4, yrow = (int)((r / w4) % H);
        const long long off = (long long)b * C * H * W + r * 4;
        const long long poff = (long long)(B - 1 - b) * C * H * W + r * 4;
        const vr_mixup_param m = params[b];
        const float4 a = *reinterpret_cast<const float4*>(in + off);
        float4 o = a;
        if (m.cutmix) {
            if (yrow >= m.y0 && yrow < m.y1 && x + 3 >= m.x0 && x < m.x1) {
                const float4 p = *reinterpret_cast<const float4*>(in + poff);
                if (x + 0 >= m.x0 && x + 0 < m.x1) o.x = p.x;
                if (x + 1 >= m.x0 && x + 1 < m.x1) o.y = p.y;
                if (x + 2 >= m.x0 && x + 2 < m.x1) o.z = p.z;
                if (x + 3 >= m.x0 && x + 3 < m.x1) o.w = p.w;
            }
        } else if (!untouched(m)) {
            const float4 p = *reinterpret_cast<const float4*>(in + poff);
            o = make_float4(mix2(a.x, m.lam, p.x, m.oml), mix2(a.y, m.lam, p.y, m.oml), mix2(a.z, m.lam, p.z, m.oml),
                            mix2(a.w, m.lam, p.w, m.oml));
        }
        *reinterpret_cast<float4*>(out + off) = o;
    }
}

// the same on uint8 pixels: own / partner is chosen on the bytes, the blend normalises both and mixes as mix2 does
template <int V, bool ERASE>
__global__ __launch_bounds__(256) void mixup_samples_u8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                               const vr_mixup_param* __restrict__ params, int B, int C, int H, int W,
                                                               NormParams np, EraseArg<ERASE> ea) {
    const int wv = W / V;
    const long long per = (long long)C * H * wv, total = (long long)B * per;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / per);
        const long long r = idx % per;
        const int x = (int)(r % wv) * V, yrow = (int)((r / wv) % H), c = (int)(r / ((long long)wv * H));
        const long long off = (long long)b * C * H * W + r * V;
        const long long poff = (long long)(B - 1 - b) * C * H * W + r * V;
        const vr_mixup_param m = params[b];
        const float mu = pick4(np.mean, c), s = pick4(np.std, c);
        if constexpr (ERASE) {                                    // (the lam == 1 copy still carries the sample's own erase)
            const int mix = !m.cutmix ? (untouched(m) ? MIX_NONE : MIX_BLEND)
                                      : yrow >= m.y0 && yrow < m.y1 && x + V - 1 >= m.x0 && x < m.x1 ? MIX_BOX : MIX_NONE;
            if (erase_hits(ea.e, b, yrow, x, V) || (mix != MIX_NONE && erase_hits(ea.e, B - 1 - b, yrow, x, V))) {
                erased_lane<V>(in, out, off, poff, mix, m.x0, m.x1, m.lam, m.oml, mu, s, ea.e, b, B - 1 - b, c, H, W, yrow, x);
                continue;
            }
        }
        U8Vec<V> a, p;
        a.load(in + off);
        p = a;
        float o[V];
        if (m.cutmix || untouched(m)) {
            const bool box = m.cutmix && yrow >= m.y0 && yrow < m.y1 && x + V - 1 >= m.x0 && x < m.x1;
            if (box) p.load(in + poff);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const bool take = box && x + i >= m.x0 && x + i < m.x1;
                o[i] = norm1(take ? u8_at(p, i) : u8_at(a, i), mu, s);
            }
        } else {
            p.load(in + poff);
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = mix2(norm1(u8_at(a, i), mu, s), m.lam, norm1(u8_at(p, i), mu, s), m.oml);
        }
#pragma unroll
        for (int q = 0; q < V / 4; ++q)
            *reinterpret_cast<float4*>(out + off + 4 * q) = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}

// one workgroup per sample: targets[b, :] = y_b * lam + y_(B-1-b) * oml on the smoothed one-hots, always (timm's mixup_target)
__global__ __launch_bounds__(256) void mixup_targets_kernel(const int64_t* __restrict__ labels, float* __restrict__ targets,
                                                            const vr_mixup_param* __restrict__ params, int B, int K, float on,
                                                            float off) {
    const int b = blockIdx.x;
    const int la = (int)labels[b], lb = (int)labels[B - 1 - b];
    const float l = params[b].lam, m = params[b].oml;
    for (int c = threadIdx.x; c < K; c += blockDim.x)
        targets[(long long)b * K + c] = mix2(c == la ? on : off, l, c == lb ? on : off, m);
}

inline unsigned stream_blocks(long long total) {
    const long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

inline NormParams norm_params(const float* mean, const float* std, int C) {
    NormParams np;
    for (int c = 0; c < 4; ++c) {
        np.mean[c] = c < C ? mean[c] : 0.f;
        np.std[c] = c < C ? std[c] : 1.f;
    }
    return np;
}

// The erase arguments' share of an entry point's checks, one per class of error and each in that class's turn.  ERASE = false: none.
constexpr int32_t ERASE_MAX_B = 1 << 24;                                  // (the sample index shares counter word 1 with the domain)
template <bool ERASE>
inline bool erase_einval(const vr_erase_args* er) {
    return ERASE && (!er || !er->rects || er->R < 1 || er->R > 4 || er->mode < VR_ERASE_CONST || er->mode > VR_ERASE_PIXEL);
}
template <bool ERASE>
inline bool erase_eunsupported(int B) { return ERASE && B > ERASE_MAX_B; }
template <bool ERASE>
inline bool erase_ealign(const vr_erase_args* er) { return ERASE && ((uintptr_t)er->rects & 3); }

inline EraseParams erase_params(const vr_erase_rect* rects, int R, int mode, uint64_t seed, uint64_t call, int H, int W) {
    return EraseParams{rects, R, mode, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), H, W};
}
template <bool ERASE>
inline EraseArg<ERASE> erase_arg(const vr_erase_args* er, int H, int W) {
    if constexpr (ERASE)
        return EraseArg<true>{erase_params(er->rects, er->R, er->mode, er->seed, er->call, H, W)};
    else
        return EraseArg<false>{};
}

template <bool ERASE>
int normalize_u8(const uint8_t* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mean, const float* std,
                 const vr_erase_args* er, vr_stream_t stream) {
    if (!in || !out || !mean || !std || erase_einval<ERASE>(er)) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VR_EINVAL;
    if (C > 4 || W % 4 || erase_eunsupported<ERASE>(B)) return VR_EUNSUPPORTED;
    if (((uintptr_t)in & 3) || ((uintptr_t)out & 15) || erase_ealign<ERASE>(er)) return VR_EALIGN;
    const NormParams np = norm_params(mean, std, C);
    const EraseArg<ERASE> ea = erase_arg<ERASE>(er, H, W);
    const long long n = (long long)B * C * H * W;
    if (W % 16 == 0 && !((uintptr_t)in & 15))
        hipLaunchKernelGGL((normalize_u8_kernel<16, ERASE>), dim3(stream_blocks(n / 16)), dim3(256), 0, (hipStream_t)stream, in, out,
                           n / 16, H * (W / 16), C, np, ea);
    else
        hipLaunchKernelGGL((normalize_u8_kernel<4, ERASE>), dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, in, out,
                           n / 4, H * (W / 4), C, np, ea);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

template <bool ERASE>
int token_mix_u8(const uint8_t* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                 float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes, int32_t patch_len,
                 int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch, float oml_patch, float lam_img,
                 float oml_img, float on_value, float off_value, const float* mean, const float* std, const vr_erase_args* er,
                 vr_stream_t stream) {
    if (!samples || !out || !labels || !partner || !targets || !patch_targets || !mean || !std || erase_einval<ERASE>(er))
        return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_classes <= 0 || patch_len <= 0 || half < 0 || half > B) return VR_EINVAL;
    if (C > 4 || W % 4 || H % patch_len || W % patch_len || erase_eunsupported<ERASE>(B)) return VR_EUNSUPPORTED;
    if (((uintptr_t)samples & 3) || ((uintptr_t)out & 15) || erase_ealign<ERASE>(er)) return VR_EALIGN;
    const NormParams np = norm_params(mean, std, C);
    const EraseArg<ERASE> ea = erase_arg<ERASE>(er, H, W);
    const int psy = H / patch_len, psx = W / patch_len;
    const long long n = (long long)B * C * H * W;
    if (W % 16 == 0 && !((uintptr_t)samples & 15))
        hipLaunchKernelGGL((mix_samples_u8_kernel<16, ERASE>), dim3(stream_blocks(n / 16)), dim3(256), 0, (hipStream_t)stream, samples,
                           out, partner, B, C, H, W, half, psy * y0, psy * y1, psx * x0, psx * x1, lam_img, oml_img, np, ea);
    else
        hipLaunchKernelGGL((mix_samples_u8_kernel<4, ERASE>), dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, samples,
                           out, partner, B, C, H, W, half, psy * y0, psy * y1, psx * x0, psx * x1, lam_img, oml_img, np, ea);
    hipLaunchKernelGGL(mix_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, partner, targets, patch_targets,
                       num_classes, patch_len, half, y0, y1, x0, x1, lam_patch, oml_patch, lam_img, oml_img, on_value, off_value);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

template <bool ERASE>
int mixup_u8(const uint8_t* samples, float* out, const int64_t* labels, float* targets, const vr_mixup_param* params, int32_t B,
             int32_t C, int32_t H, int32_t W, int32_t num_classes, float on_value, float off_value, const float* mean,
             const float* std, const vr_erase_args* er, vr_stream_t stream) {
    if (!samples || !out || !labels || !targets || !params || !mean || !std || erase_einval<ERASE>(er)) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_classes <= 0) return VR_EINVAL;
    if (C > 4 || W % 4 || B % 2 || (const void*)samples == (const void*)out || erase_eunsupported<ERASE>(B)) return VR_EUNSUPPORTED;
    if (((uintptr_t)samples & 3) || ((uintptr_t)out & 15) || ((uintptr_t)params & 3) || erase_ealign<ERASE>(er)) return VR_EALIGN;
    const NormParams np = norm_params(mean, std, C);
    const EraseArg<ERASE> ea = erase_arg<ERASE>(er, H, W);
    const long long n = (long long)B * C * H * W;
    if (W % 16 == 0 && !((uintptr_t)samples & 15))
        hipLaunchKernelGGL((mixup_samples_u8_kernel<16, ERASE>), dim3(stream_blocks(n / 16)), dim3(256), 0, (hipStream_t)stream,
                           samples, out, params, B, C, H, W, np, ea);
    else
        hipLaunchKernelGGL((mixup_samples_u8_kernel<4, ERASE>), dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream,
                           samples, out, params, B, C, H, W, np, ea);
    hipLaunchKernelGGL(mixup_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, targets, params, B, num_classes,
                       on_value, off_value);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

}  // namespace

static_assert(sizeof(vr_erase_rect) == 16, "vr_erase_rect is 16 bytes: the host marshals the [B][R] table as int32 quadruples");
static_assert(sizeof(vr_erase_args) == 32, "vr_erase_args is 32 bytes: the host marshals it as such");

extern "C" int vr_random_erase(float* x, int32_t B, int32_t C, int32_t H, int32_t W, const vr_erase_rect* rects, int32_t R,
                               int32_t mode, uint64_t seed, uint64_t call, vr_stream_t stream) {
    const vr_erase_args er = {rects, R, mode, seed, call};
    if (!x || erase_einval<true>(&er)) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VR_EINVAL;
    if (C > 4 || W % 4 || erase_eunsupported<true>(B)) return VR_EUNSUPPORTED;
    if (((uintptr_t)x & 15) || erase_ealign<true>(&er)) return VR_EALIGN;
    const long long n = (long long)B * C * H * W;
    hipLaunchKernelGGL(random_erase_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, B, C, H, W,
                       erase_params(rects, R, mode, seed, call, H, W));
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_normalize_u8(const uint8_t* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mean,
                               const float* std, vr_stream_t stream) {
    return normalize_u8<false>(in, out, B, C, H, W, mean, std, nullptr, stream);
}

extern "C" int vr_normalize_u8_erase(const uint8_t* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mean,
                                     const float* std, const vr_erase_args* erase, vr_stream_t stream) {
    return normalize_u8<true>(in, out, B, C, H, W, mean, std, erase, stream);
}

extern "C" int vr_token_mix_u8(const uint8_t* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                               float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes,
                               int32_t patch_len, int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch,
                               float oml_patch, float lam_img, float oml_img, float on_value, float off_value, const float* mean,
                               const float* std, vr_stream_t stream) {
    return token_mix_u8<false>(samples, out, labels, partner, targets, patch_targets, B, C, H, W, num_classes, patch_len, half, y0, y1,
                               x0, x1, lam_patch, oml_patch, lam_img, oml_img, on_value, off_value, mean, std, nullptr, stream);
}

extern "C" int vr_token_mix_u8_erase(const uint8_t* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                                     float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes,
                                     int32_t patch_len, int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch,
                                     float oml_patch, float lam_img, float oml_img, float on_value, float off_value, const float* mean,
                                     const float* std, const vr_erase_args* erase, vr_stream_t stream) {
    return token_mix_u8<true>(samples, out, labels, partner, targets, patch_targets, B, C, H, W, num_classes, patch_len, half, y0, y1,
                              x0, x1, lam_patch, oml_patch, lam_img, oml_img, on_value, off_value, mean, std, erase, stream);
}

extern "C" int vr_token_mix(const float* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                            float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes,
                            int32_t patch_len, int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch,
                            float oml_patch, float lam_img, float oml_img, float on_value, float off_value, vr_stream_t stream) {
    if (!samples || !out || !labels || !partner || !targets || !patch_targets) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_classes <= 0 || patch_len <= 0 || half < 0 || half > B) return VR_EINVAL;
    if (W % 4 || H % patch_len || W % patch_len || samples == out) return VR_EUNSUPPORTED;
    if (((uintptr_t)samples & 15) || ((uintptr_t)out & 15)) return VR_EALIGN;
    const int psy = H / patch_len, psx = W / patch_len;
    const long long total = (long long)B * C * H * (W / 4);
    long long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(mix_samples_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, samples, out, partner, B, C, H,
                       W, half, psy * y0, psy * y1, psx * x0, psx * x1, lam_img, oml_img);
    hipLaunchKernelGGL(mix_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, partner, targets, patch_targets,
                       num_classes, patch_len, half, y0, y1, x0, x1, lam_patch, oml_patch, lam_img, oml_img, on_value, off_value);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

static_assert(sizeof(vr_mixup_param) == 32, "vr_mixup_param is 32 bytes: the host marshals it as such");

extern "C" int vr_mixup(const float* samples, float* out, const int64_t* labels, float* targets, const vr_mixup_param* params,
                        int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes, float on_value, float off_value,
                        vr_stream_t stream) {
    if (!samples || !out || !labels || !targets || !params) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_classes <= 0) return VR_EINVAL;
    if (W % 4 || B % 2 || samples == out) return VR_EUNSUPPORTED;
    if (((uintptr_t)samples & 15) || ((uintptr_t)out & 15) || ((uintptr_t)params & 3)) return VR_EALIGN;
    const long long n = (long long)B * C * H * W;
    hipLaunchKernelGGL(mixup_samples_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, samples, out, params, B, C,
                       H, W);
    hipLaunchKernelGGL(mixup_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, targets, params, B, num_classes,
                       on_value, off_value);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_mixup_u8(const uint8_t* samples, float* out, const int64_t* labels, float* targets, const vr_mixup_param* params,
                           int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes, float on_value, float off_value,
                           const float* mean, const float* std, vr_stream_t stream) {
    return mixup_u8<false>(samples, out, labels, targets, params, B, C, H, W, num_classes, on_value, off_value, mean, std, nullptr,
                           stream);
}

extern "C" int vr_mixup_u8_erase(const uint8_t* samples, float* out, const int64_t* labels, float* targets,
                                 const vr_mixup_param* params, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes,
                                 float on_value, float off_value, const float* mean, const float* std, const vr_erase_args* erase,
                                 vr_stream_t stream) {
    return mixup_u8<true>(samples, out, labels, targets, params, B, C, H, W, num_classes, on_value, off_value, mean, std, erase,
                          stream);
}
