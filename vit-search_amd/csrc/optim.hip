// Step tail on the flat parameter arena: AdamW as timm 0.3.2's create_optimizer builds it for the
// reference (main.py:385; torch.optim.AdamW semantics: decoupled weight decay, bias-corrected moments), fused with what
// otherwise are separate passes over the 70-144 M parameters: the bf16 shadow the next forward's GEMMs read
// (vr_cast_f32_bf16), the 1/world averaging of the all-reduced gradient, and the ModelEmaV2 update (main.py:357-363,
// ema = d * ema + (1 - d) * p).  One streaming pass, 16-byte accesses, HBM-bound: 28 B/param (+2 shadow, +8 EMA).
#include <cstdlib>

#include "common.h"
#include "../../include/vitres_hip.h"

namespace {

struct Groups {
    vr_adamw_group g[VR_ADAMW_MAX_GROUPS];
};

// DEV: the per-group hyper-parameters are read from device memory (groups_dev) instead of the launch arguments, so that a launch
// captured into a hipGraph follows the learning-rate schedule and the bias corrections of every replayed step.
// CLIP: the gradient is also multiplied by the clip coefficient vr_clip_finish left in device memory, and a step whose gradient norm
// is not finite writes nothing at all (the coefficient would turn every parameter into NaN).
template <bool DEV, bool CLIP>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16_t* __restrict__ shadow, float* __restrict__ ema,
                                                    float ema_decay, const uint8_t* __restrict__ group_of_8, Groups groups,
                                                    const vr_adamw_group* __restrict__ groups_dev, long long n8,
                                                    const vr_clip_state* __restrict__ clip) {
    float coef = 1.0f;
    if (CLIP) {
        if (clip->skip) return;
        coef = clip->coef;
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const int gi = group_of_8[i];
        if (gi == 255) continue;                                   // padding / frozen parameters
        const vr_adamw_group h = DEV ? groups_dev[gi] : groups.g[gi];
        if (DEV && h.bias_c1 == 0.f) continue;                     // (1 - beta1^t is never 0: an all-zero group = "no update this replay")
        const long long e = i * 8;
        float pv[8], gv[8], mv[8], vv[8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(p + e + 4 * q), b = *reinterpret_cast<const float4*>(g + e + 4 * q);
            const float4 c = *reinterpret_cast<const float4*>(m + e + 4 * q), d = *reinterpret_cast<const float4*>(v + e + 4 * q);
            pv[4 * q] = a.x; pv[4 * q + 1] = a.y; pv[4 * q + 2] = a.z; pv[4 * q + 3] = a.w;
            gv[4 * q] = b.x; gv[4 * q + 1] = b.y; gv[4 * q + 2] = b.z; gv[4 * q + 3] = b.w;
            mv[4 * q] = c.x; mv[4 * q + 1] = c.y; mv[4 * q + 2] = c.z; mv[4 * q + 3] = c.w;
            vv[4 * q] = d.x; vv[4 * q + 1] = d.y; vv[4 * q + 2] = d.z; vv[4 * q + 3] = d.w;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float gr = gv[k] * h.grad_scale;
            if (CLIP) gr *= coef;
            float x = pv[k] * (1.0f - h.lr * h.weight_decay);
            mv[k] = h.beta1 * mv[k] + (1.0f - h.beta1) * gr;
            vv[k] = h.beta2 * vv[k] + (1.0f - h.beta2) * gr * gr;
            const float denom = sqrtf(vv[k]) / h.sqrt_bias_c2 + h.eps;
            x -= (h.lr / h.bias_c1) * (mv[k] / denom);
            pv[k] = x;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<float4*>(p + e + 4 * q) = make_float4(pv[4 * q], pv[4 * q + 1], pv[4 * q + 2], pv[4 * q + 3]);
            *reinterpret_cast<float4*>(m + e + 4 * q) = make_float4(mv[4 * q], mv[4 * q + 1], mv[4 * q + 2], mv[4 * q + 3]);
            *reinterpret_cast<float4*>(v + e + 4 * q) = make_float4(vv[4 * q], vv[4 * q + 1], vv[4 * q + 2], vv[4 * q + 3]);
        }
        if (shadow)
            *reinterpret_cast<uint4*>(shadow + e) = make_uint4(pack_bf2(pv[0], pv[1]), pack_bf2(pv[2], pv[3]),
                                                              pack_bf2(pv[4], pv[5]), pack_bf2(pv[6], pv[7]));
        if (ema) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float4 a = *reinterpret_cast<const float4*>(ema + e + 4 * q);
                a.x = ema_decay * a.x + (1.0f - ema_decay) * pv[4 * q];
                a.y = ema_decay * a.y + (1.0f - ema_decay) * pv[4 * q + 1];
                a.z = ema_decay * a.z + (1.0f - ema_decay) * pv[4 * q + 2];
                a.w = ema_decay * a.w + (1.0f - ema_decay) * pv[4 * q + 3];
                *reinterpret_cast<float4*>(ema + e + 4 * q) = a;
            }
        }
    }
}

// Sum of squares of the gradient elements AdamW consumes (group byte != 255) -- the first half of torch's clip_grad_norm_.
// Workgroup b < active strides over the groups of 8 and writes partials[b] with a plain store; workgroups beyond `active` (a capped
// launch beside the backward) write 0.  Nothing is accumulated across launches: no zeroing, no atomics, the same bits every replay.
// Error: eight independent fp32 chains per thread (one per element of a group of 8), each n8 / (active * 256) terms long, then
// a tree: 3 levels in the thread, 6 in the wave, 2 across the waves.
__device__ __forceinline__ void sumsq_body(const float* __restrict__ g, const uint8_t* __restrict__ group_of_8, long long n8, int active,
                                           float* __restrict__ partials) {
    __shared__ float wave_part[4];
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if ((int)blockIdx.x < active) {
        const long long stride = (long long)active * blockDim.x;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
            if (group_of_8[i] == 255) continue;                    // padding / frozen parameters: AdamW never reads them
            const float4 a = *reinterpret_cast<const float4*>(g + i * 8), b = *reinterpret_cast<const float4*>(g + i * 8 + 4);
            acc[0] = fmaf(a.x, a.x, acc[0]); acc[1] = fmaf(a.y, a.y, acc[1]); acc[2] = fmaf(a.z, a.z, acc[2]); acc[3] = fmaf(a.w, a.w, acc[3]);
            acc[4] = fmaf(b.x, b.x, acc[4]); acc[5] = fmaf(b.y, b.y, acc[5]); acc[6] = fmaf(b.z, b.z, acc[6]); acc[7] = fmaf(b.w, b.w, acc[7]);
        }
    }
    const float s = wave_sum(((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])));
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, const uint8_t* __restrict__ group_of_8, long long n8,
                                                    int active, float* __restrict__ partials) {
    sumsq_body(g, group_of_8, n8, active, partials);
}

// Gated forms (gradient accumulation: one captured graph serves every micro-step of an update window).  Every thread of the grid reads
// the same gate word first and the whole launch returns when it is 0: the partial sums, or every field of the state, keep their bits.
__global__ __launch_bounds__(256) void sumsq_gated_kernel(const float* __restrict__ g, const uint8_t* __restrict__ group_of_8, long long n8,
                                                          int active, float* __restrict__ partials, const int32_t* __restrict__ gate) {
    if (*gate == 0) return;
    sumsq_body(g, group_of_8, n8, active, partials);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup: all partials in double -> norm, clip coefficient, skip flag (vr_clip_state).
__device__ __forceinline__ void clip_finish_body(const float* __restrict__ partials, int n, vr_clip_state* __restrict__ st) {
    __shared__ double wave_part[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partials[i];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double total = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
        const float norm = (float)((double)st->grad_scale * sqrt(total));
        const bool bad = !(fabsf(norm) <= 3.402823466e38f);        // inf or NaN
        st->norm = norm;
        st->coef = bad ? 0.f : fminf(1.0f, st->max_norm / (norm + 1e-6f));       // torch.nn.utils.clip_grad_norm_'s formula
        st->skip = bad ? 1 : 0;
        if (bad) st->skipped += 1;
    }
}

__global__ __launch_bounds__(256) void clip_finish_kernel(const float* __restrict__ partials, int n, vr_clip_state* __restrict__ st) {
    clip_finish_body(partials, n, st);
}

__global__ __launch_bounds__(256) void clip_finish_gated_kernel(const float* __restrict__ partials, int n, vr_clip_state* __restrict__ st,
                                                                const int32_t* __restrict__ gate) {
    if (*gate == 0) return;
    clip_finish_body(partials, n, st);
}

}  // namespace

static int adamw_launch(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                        const uint8_t* group_of_8, const vr_adamw_group* groups, bool on_device, int32_t n_groups, int64_t n,
                        vr_stream_t stream, int32_t max_blocks = 0, const vr_clip_state* clip = nullptr) {
    if (!p || !g || !m || !v || !group_of_8 || !groups || n <= 0 || n_groups <= 0) return VR_EINVAL;
    if (n_groups > VR_ADAMW_MAX_GROUPS) return VR_EUNSUPPORTED;
    if (n % 8 || ((uintptr_t)p & 15) || ((uintptr_t)g & 15) || ((uintptr_t)m & 15) || ((uintptr_t)v & 15) ||
        (shadow && ((uintptr_t)shadow & 15)) || (ema && ((uintptr_t)ema & 15)))
        return VR_EALIGN;
    Groups gs = {};
    if (!on_device)
        for (int i = 0; i < n_groups; ++i) gs.g[i] = groups[i];
    const long long n8 = n / 8;
    long long blocks = (n8 + 255) / 256;
    const long long cap = max_blocks > 0 ? max_blocks : 8192;
    if (blocks > cap) blocks = cap;
    const vr_adamw_group* gd = on_device ? groups : nullptr;
#define VR_ADAMW_GO(DEV_, CLIP_)                                                                                                   \
    hipLaunchKernelGGL((adamw_kernel<DEV_, CLIP_>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,         \
                       (bf16_t*)shadow, ema, ema_decay, group_of_8, gs, gd, n8, clip)
    if (clip) {
        if (on_device) VR_ADAMW_GO(true, true); else VR_ADAMW_GO(false, true);
    } else {
        if (on_device) VR_ADAMW_GO(true, false); else VR_ADAMW_GO(false, false);
    }
#undef VR_ADAMW_GO
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_adamw_flat(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                             const uint8_t* group_of_8, const vr_adamw_group* groups, int32_t n_groups, int64_t n,
                             vr_stream_t stream) {
    return adamw_launch(p, g, m, v, shadow, ema, ema_decay, group_of_8, groups, false, n_groups, n, stream);
}

extern "C" int vr_adamw_flat_dev(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                                 const uint8_t* group_of_8, const vr_adamw_group* groups_dev, int32_t n_groups, int64_t n,
                                 vr_stream_t stream) {
    return adamw_launch(p, g, m, v, shadow, ema, ema_decay, group_of_8, groups_dev, true, n_groups, n, stream);
}

// The same launch capped at `max_blocks` resident workgroups (grid-stride): an update of a finished arena range that runs on the
// weight gradients' stream beside the rest of the backward must not take the chip (engine.GraphedTrainStep, opt_overlap_blocks).
extern "C" int vr_adamw_flat_dev_capped(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                                        const uint8_t* group_of_8, const vr_adamw_group* groups_dev, int32_t n_groups, int64_t n,
                                        int32_t max_blocks, vr_stream_t stream) {
    if (max_blocks < 0) return VR_EINVAL;
    return adamw_launch(p, g, m, v, shadow, ema, ema_decay, group_of_8, groups_dev, true, n_groups, n, stream, max_blocks);
}

// ---- gradient-norm clipping on the device (vr_clip_state) ----------------------------------------------------------------------
static int sumsq_launch(const float* g, const uint8_t* group_of_8, int64_t n, float* partials, int32_t n_partials, int32_t max_blocks,
                        const int32_t* gate, bool gated, vr_stream_t stream) {
    if (!g || !group_of_8 || !partials || n <= 0 || n_partials <= 0 || max_blocks < 0 || (gated && !gate)) return VR_EINVAL;
    if (n % 8 || ((uintptr_t)g & 15) || (gated && ((uintptr_t)gate & 3))) return VR_EALIGN;
    const long long n8 = n / 8;
    long long active = (n8 + 255) / 256;                           // workgroups that have work: the rest write 0
    if (active > n_partials) active = n_partials;
    if (max_blocks > 0 && active > max_blocks) active = max_blocks;
    if (gated)
        hipLaunchKernelGGL(sumsq_gated_kernel, dim3((unsigned)n_partials), dim3(256), 0, (hipStream_t)stream, g, group_of_8, n8, (int)active,
                           partials, gate);
    else
        hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)n_partials), dim3(256), 0, (hipStream_t)stream, g, group_of_8, n8, (int)active,
                           partials);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_grad_sumsq(const float* g, const uint8_t* group_of_8, int64_t n, float* partials, int32_t n_partials,
                             int32_t max_blocks, vr_stream_t stream) {
    return sumsq_launch(g, group_of_8, n, partials, n_partials, max_blocks, nullptr, false, stream);
}

extern "C" int vr_grad_sumsq_gated(const float* g, const uint8_t* group_of_8, int64_t n, float* partials, int32_t n_partials,
                                   int32_t max_blocks, const int32_t* gate, vr_stream_t stream) {
    return sumsq_launch(g, group_of_8, n, partials, n_partials, max_blocks, gate, true, stream);
}

extern "C" int vr_clip_finish(const float* partials, int32_t n_partials, vr_clip_state* state, vr_stream_t stream) {
    if (!partials || !state || n_partials <= 0) return VR_EINVAL;
    if ((uintptr_t)state & 3) return VR_EALIGN;
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (int)n_partials, state);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_clip_finish_gated(const float* partials, int32_t n_partials, vr_clip_state* state, const int32_t* gate,
                                    vr_stream_t stream) {
    if (!partials || !state || !gate || n_partials <= 0) return VR_EINVAL;
    if (((uintptr_t)state & 3) || ((uintptr_t)gate & 3)) return VR_EALIGN;
    hipLaunchKernelGGL(clip_finish_gated_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (int)n_partials, state, gate);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_adamw_flat_clip(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                                  const uint8_t* group_of_8, const vr_adamw_group* groups, int32_t groups_on_device,
                                  int32_t n_groups, int64_t n, const vr_clip_state* clip, int32_t max_blocks, vr_stream_t stream) {
    if (!clip || max_blocks < 0) return VR_EINVAL;
    return adamw_launch(p, g, m, v, shadow, ema, ema_decay, group_of_8, groups, groups_on_device != 0, n_groups, n, stream, max_blocks,
                        clip);
}
