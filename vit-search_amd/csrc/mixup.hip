// SwitchTokenMix on the device (reference token_mixup.py:39-162): the input side of the training step.
// The random draws (two torch.randperm, the Beta samples and the box from numpy) stay on the host with the reference's
// generators and call order (vitres/token_mixup.py); what is heavy -- rewriting the 77 MB image batch and building the
// 8 MB of soft patch targets -- is two streaming kernels, one read and one write per element, bit-exact with the
// reference's fp32 arithmetic (products rounded separately, then added: no FMA contraction).
//   rows [0, half)  : out = partner's pixels inside the box, own pixels outside; patch targets follow the box
//   rows [half, B)  : out = x * lam + partner * (1 - lam); every patch target = the mixed image target
// Further down: the uint8 forms (normalise inside the pass) and timm's Mixup / CutMix (vr_mixup, vr_mixup_u8; vitres/mixup.py).
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

template <int V>
__global__ __launch_bounds__(256) void normalize_u8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, long long total,
                                                           int hwv, int C, NormParams np) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c = (int)((idx / hwv) % C);
        const float m = pick4(np.mean, c), s = pick4(np.std, c);
        U8Vec<V> a;
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
template <int V>
__global__ __launch_bounds__(256) void mix_samples_u8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                             const int64_t* __restrict__ partner, int B, int C, int H, int W,
                                                             int half, int py0, int py1, int px0, int px1, float lam, float oml,
                                                             NormParams np) {
    const int wv = W / V;
    const long long per = (long long)C * H * wv, total = (long long)B * per;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / per);
        const long long r = idx % per;
        const int x = (int)(r % wv) * V, yrow = (int)((r / wv) % H), c = (int)(r / ((long long)wv * H));
        const long long off = (long long)b * C * H * W + r * V;
        const long long poff = (long long)partner[b] * C * H * W + r * V;
        const float m = pick4(np.mean, c), s = pick4(np.std, c);
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
template <int V>
__global__ __launch_bounds__(256) void mixup_samples_u8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                               const vr_mixup_param* __restrict__ params, int B, int C, int H, int W,
                                                               NormParams np) {
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

}  // namespace

extern "C" int vr_normalize_u8(const uint8_t* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mean,
                               const float* std, vr_stream_t stream) {
    if (!in || !out || !mean || !std) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VR_EINVAL;
    if (C > 4 || W % 4) return VR_EUNSUPPORTED;
    if (((uintptr_t)in & 3) || ((uintptr_t)out & 15)) return VR_EALIGN;
    const NormParams np = norm_params(mean, std, C);
    const long long n = (long long)B * C * H * W;
    if (W % 16 == 0 && !((uintptr_t)in & 15))
        hipLaunchKernelGGL(normalize_u8_kernel<16>, dim3(stream_blocks(n / 16)), dim3(256), 0, (hipStream_t)stream, in, out, n / 16,
                           H * (W / 16), C, np);
    else
        hipLaunchKernelGGL(normalize_u8_kernel<4>, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, in, out, n / 4,
                           H * (W / 4), C, np);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_token_mix_u8(const uint8_t* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                               float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes,
                               int32_t patch_len, int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch,
                               float oml_patch, float lam_img, float oml_img, float on_value, float off_value, const float* mean,
                               const float* std, vr_stream_t stream) {
    if (!samples || !out || !labels || !partner || !targets || !patch_targets || !mean || !std) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_classes <= 0 || patch_len <= 0 || half < 0 || half > B) return VR_EINVAL;
    if (C > 4 || W % 4 || H % patch_len || W % patch_len) return VR_EUNSUPPORTED;
    if (((uintptr_t)samples & 3) || ((uintptr_t)out & 15)) return VR_EALIGN;
    const NormParams np = norm_params(mean, std, C);
    const int psy = H / patch_len, psx = W / patch_len;
    const long long n = (long long)B * C * H * W;
    if (W % 16 == 0 && !((uintptr_t)samples & 15))
        hipLaunchKernelGGL(mix_samples_u8_kernel<16>, dim3(stream_blocks(n / 16)), dim3(256), 0, (hipStream_t)stream, samples, out,
                           partner, B, C, H, W, half, psy * y0, psy * y1, psx * x0, psx * x1, lam_img, oml_img, np);
    else
        hipLaunchKernelGGL(mix_samples_u8_kernel<4>, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, samples, out,
                           partner, B, C, H, W, half, psy * y0, psy * y1, psx * x0, psx * x1, lam_img, oml_img, np);
    hipLaunchKernelGGL(mix_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, partner, targets, patch_targets,
                       num_classes, patch_len, half, y0, y1, x0, x1, lam_patch, oml_patch, lam_img, oml_img, on_value, off_value);
    VR_CHECK_LAUNCH();
    return VR_OK;
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
    if (!samples || !out || !labels || !targets || !params || !mean || !std) return VR_EINVAL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_classes <= 0) return VR_EINVAL;
    if (C > 4 || W % 4 || B % 2 || (const void*)samples == (const void*)out) return VR_EUNSUPPORTED;
    if (((uintptr_t)samples & 3) || ((uintptr_t)out & 15) || ((uintptr_t)params & 3)) return VR_EALIGN;
    const NormParams np = norm_params(mean, std, C);
    const long long n = (long long)B * C * H * W;
    if (W % 16 == 0 && !((uintptr_t)samples & 15))
        hipLaunchKernelGGL(mixup_samples_u8_kernel<16>, dim3(stream_blocks(n / 16)), dim3(256), 0, (hipStream_t)stream, samples, out,
                           params, B, C, H, W, np);
    else
        hipLaunchKernelGGL(mixup_samples_u8_kernel<4>, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, samples, out,
                           params, B, C, H, W, np);
    hipLaunchKernelGGL(mixup_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, targets, params, B, num_classes,
                       on_value, off_value);
    VR_CHECK_LAUNCH();
    return VR_OK;
}
