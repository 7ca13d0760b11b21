// vr_resample_u8: crop + resize (+ window, + mirror) of uint8 batches, bit for bit PIL's 8-bit two-pass resample (include/vitres_hip.h).
//
// One workgroup per (sample, band of output rows), all channels:
//   1. the band's coefficients, in fp64 exactly as PIL's precompute_coeffs / normalize_coeffs_8bpc evaluate them (one rounded
//      operation per operator: this file is compiled with floating-point contraction off), as 22-bit fixed point into LDS;
//   2. horizontal pass: each wave takes (source row, channel) pairs of the rows the band's vertical taps touch, stages the row's
//      crop as aligned dwords in its own LDS slice and writes the resampled row into the LDS intermediate as uint8;
//   3. vertical pass: a lane reads the intermediate a dword (4 pixels) per tap and stores 4 output bytes.
// The LDS layout is sized on the host from the launch's dimensions alone (the boxes live in device memory): a box inside the canvas
// has h <= Hs and a window inside the resized image has oh >= So_h, so Hs / So_h bounds every sample's vertical scale, likewise
// Ws / So_w.  The kernel clamps every box into that envelope, so a bad box selects other pixels and addresses nothing out of range.
#include "common.h"
#include "../../include/vitres_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_PRECISION_BITS = 32 - 8 - 2;
constexpr int RS_MAX_BAND = 32;
constexpr size_t RS_LDS_BUDGET = 64 * 1024 - 64;   // dynamic part (the kernel has 16 static bytes): at least two workgroups per CU of
                                                   // 160 KiB, and within what a launch gets without raising the dynamic-LDS limit

struct ResamplePlan {
    int band, ksh, ksv, nrows, stage;         // band height; taps per output column / row; intermediate rows; bytes of a wave's stage
    size_t lds;
};

// PIL's bilinear_filter / bicubic_filter (a = -0.5), operator by operator
__device__ inline double rs_filter(double x, int bicubic) {
    if (x < 0.0) x = -x;
    if (bicubic) {
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

// taps of one output index of one axis: PIL's bounds, and its weights as fixed point
struct RsAxis {
    double scale, support, ss;
    int in;
};
__device__ inline RsAxis rs_axis(int in, int out, int bicubic) {
    RsAxis a;
    a.in = in;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = (bicubic ? 2.0 : 1.0) * fs;
    a.ss = 1.0 / fs;
    return a;
}
// writes cnt <= ks coefficients to k[t * stride]; returns xmin, sets cnt
__device__ inline int rs_taps(const RsAxis& a, int xx, int bicubic, int ks, int* k, int stride, int& cnt) {
    const double center = (xx + 0.5) * a.scale;
    int xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > a.in) xmax = a.in;
    if (xmin > a.in - 1) xmin = a.in - 1;          // (never for a valid box; keeps every tap inside the crop)
    int n = xmax - xmin;
    n = n < 1 ? 1 : (n > ks ? ks : n);
    double ww = 0.0;
    for (int t = 0; t < n; ++t) ww += rs_filter((xmin + t - center + 0.5) * a.ss, bicubic);
    for (int t = 0; t < n; ++t) {
        double w = rs_filter((xmin + t - center + 0.5) * a.ss, bicubic);
        if (ww != 0.0) w = w / ww;
        k[t * stride] = w < 0 ? (int)(-0.5 + w * (double)(1 << RS_PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << RS_PRECISION_BITS));
    }
    cnt = n;
    return xmin;
}

__device__ __forceinline__ int rs_clip8(int acc) {
    const int v = acc >> RS_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(RS_THREADS) void resample_u8_kernel(const uint8_t* __restrict__ src,
                                                                 const vr_resample_box* __restrict__ boxes,
                                                                 uint8_t* __restrict__ out, int C, int Hs, int Ws, int So_h, int So_w,
                                                                 int bicubic, ResamplePlan plan) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    __shared__ int s_ylo, s_yhi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, r0 = blockIdx.x * plan.band;
    const int bh = min(plan.band, So_h - r0);

    // LDS: hcoef [ksh][So_w] | hmin [So_w] | hcnt [So_w] | vcoef [band][ksv] | vmin [band] | vcnt [band] | tmp [C][nrows][So_w] u8 |
    //      stage [RS_WAVES][plan.stage] u8
    int* hcoef = (int*)rs_lds;
    int* hmin = hcoef + plan.ksh * So_w;
    int* hcnt = hmin + So_w;
    int* vcoef = hcnt + So_w;
    int* vmin = vcoef + plan.band * plan.ksv;
    int* vcnt = vmin + plan.band;
    uint8_t* tmp = (uint8_t*)(vcnt + plan.band);
    uint8_t* stage = tmp + (((size_t)C * plan.nrows * So_w + 15) & ~(size_t)15) + (size_t)wave * plan.stage;

    // the box, clamped into the envelope the plan was sized for
    const vr_resample_box bx = boxes[b];
    const int w = rs_clamp(bx.w, 1, Ws), h = rs_clamp(bx.h, 1, Hs);
    const int x0 = rs_clamp(bx.x0, 0, Ws - w), y0 = rs_clamp(bx.y0, 0, Hs - h);
    const int ow = max(bx.ow, So_w), oh = max(bx.oh, So_h);
    const int wx = rs_clamp(bx.wx, 0, ow - So_w), wy = rs_clamp(bx.wy, 0, oh - So_h);
    const int flip = bx.flip != 0;

    if (tid == 0) {
        s_ylo = Hs;
        s_yhi = 0;
    }
    __syncthreads();
    {
        const RsAxis ax = rs_axis(w, ow, bicubic);
        for (int c = tid; c < So_w; c += RS_THREADS) {
            int cnt;
            hmin[c] = rs_taps(ax, wx + c, bicubic, plan.ksh, hcoef + c, So_w, cnt);
            hcnt[c] = cnt;
        }
        const RsAxis ay = rs_axis(h, oh, bicubic);
        for (int r = tid; r < bh; r += RS_THREADS) {
            int cnt;
            const int ymin = rs_taps(ay, wy + r0 + r, bicubic, plan.ksv, vcoef + r * plan.ksv, 1, cnt);
            vmin[r] = ymin;
            vcnt[r] = cnt;
            atomicMin(&s_ylo, ymin);
            atomicMax(&s_yhi, ymin + cnt);
        }
    }
    __syncthreads();
    const int ylo = s_ylo;
    const int nrows = min(s_yhi - ylo, plan.nrows);

    // horizontal pass: source rows ylo .. ylo + nrows - 1 of the crop, every channel
    const int a0 = x0 & ~3, nd = (((x0 + w + 3) & ~3) - a0) >> 2, off = x0 - a0;     // the aligned dwords that cover the crop's columns
    const int items = nrows * C, trips = (items + RS_WAVES - 1) / RS_WAVES;
    for (int trip = 0; trip < trips; ++trip) {
        const int it = trip * RS_WAVES + wave;
        const bool live = it < items;
        const int c = live ? it / nrows : 0, row = live ? it - c * nrows : 0;
        if (live) {
            const uint32_t* g = (const uint32_t*)(src + (((size_t)b * C + c) * Hs + (y0 + ylo + row)) * Ws + a0);
            for (int i = lane; i < nd; i += 64) ((uint32_t*)stage)[i] = g[i];
        }
        __syncthreads();
        if (live) {
            uint8_t* trow = tmp + ((size_t)c * plan.nrows + row) * So_w;
            for (int col = lane; col < So_w; col += 64) {
                const uint8_t* s = stage + off + hmin[col];
                const int cnt = hcnt[col];
                int acc = 1 << (RS_PRECISION_BITS - 1);
                for (int t = 0; t < cnt; ++t) acc += hcoef[t * So_w + col] * (int)s[t];
                trow[col] = (uint8_t)rs_clip8(acc);
            }
        }
        __syncthreads();
    }

    // vertical pass: 4 output pixels per lane and tap
    const int quads = So_w >> 2, vitems = C * bh * quads;
    const uint32_t* tmp32 = (const uint32_t*)tmp;
    for (int i = tid; i < vitems; i += RS_THREADS) {
        const int q = i % quads, rc = i / quads, r = rc % bh, c = rc / bh;
        const int yrel = vmin[r] - ylo;
        const int cnt = min(vcnt[r], nrows - yrel);
        int a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = 1 << (RS_PRECISION_BITS - 1);
        const uint32_t* col = tmp32 + (((size_t)c * plan.nrows + yrel) * So_w >> 2) + q;
        const int* k = vcoef + r * plan.ksv;
        for (int t = 0; t < cnt; ++t) {
            const uint32_t px = col[(size_t)t * quads];
            const int kk = k[t];
            a[0] += kk * (int)(px & 255u);
            a[1] += kk * (int)((px >> 8) & 255u);
            a[2] += kk * (int)((px >> 16) & 255u);
            a[3] += kk * (int)(px >> 24);
        }
        uint32_t v;
        int oc;
        if (flip) {
            v = (uint32_t)rs_clip8(a[3]) | ((uint32_t)rs_clip8(a[2]) << 8) | ((uint32_t)rs_clip8(a[1]) << 16) | ((uint32_t)rs_clip8(a[0]) << 24);
            oc = So_w - 4 - 4 * q;
        } else {
            v = (uint32_t)rs_clip8(a[0]) | ((uint32_t)rs_clip8(a[1]) << 8) | ((uint32_t)rs_clip8(a[2]) << 16) | ((uint32_t)rs_clip8(a[3]) << 24);
            oc = 4 * q;
        }
        *(uint32_t*)(out + (((size_t)b * C + c) * So_h + (r0 + r)) * So_w + oc) = v;
    }
}

// taps of an axis whose scale is at most in / out (support grows with the scale, so this bounds every box of the launch)
int rs_ksize(int in, int out, int filter) {
    double fs = (double)in / (double)out;
    if (fs < 1.0) fs = 1.0;
    const double support = (filter == 3 ? 2.0 : 1.0) * fs;
    const double c = __builtin_ceil(support);
    return c > 1e6 ? -1 : (int)c * 2 + 1;
}

// the tallest band (<= RS_MAX_BAND rows) whose LDS layout fits the budget; band == 0: not even one row does
ResamplePlan rs_plan(int C, int Hs, int Ws, int So_h, int So_w, int filter) {
    ResamplePlan p = {0, rs_ksize(Ws, So_w, filter), rs_ksize(Hs, So_h, filter), 0, (Ws + 15) & ~15, 0};
    if (p.ksh < 0 || p.ksv < 0) return p;
    const double sy = (double)Hs / (double)So_h, support = (filter == 3 ? 2.0 : 1.0) * (sy < 1.0 ? 1.0 : sy);
    for (int band = So_h < RS_MAX_BAND ? So_h : RS_MAX_BAND; band >= 1; --band) {
        // rows between the first tap of the band's first row and the last tap of its last: the centres are (band - 1) * scale apart,
        // each end adds the support, the two truncations at most one row each
        double rows = __builtin_ceil((band - 1) * sy + 2.0 * support) + 2.0;
        if (rows > Hs) rows = Hs;
        const size_t lds = ((size_t)p.ksh * So_w + 2 * (size_t)So_w + (size_t)band * p.ksv + 2 * (size_t)band) * 4
                           + (((size_t)C * (size_t)rows * So_w + 15) & ~(size_t)15) + (size_t)RS_WAVES * p.stage;
        if (lds <= RS_LDS_BUDGET) {
            p.band = band;
            p.nrows = (int)rows;
            p.lds = lds;
            return p;
        }
    }
    return p;
}

int rs_check_dims(int32_t B, int32_t C, int32_t Hs, int32_t Ws, int32_t So_h, int32_t So_w, int32_t filter) {
    if (B <= 0 || Hs <= 0 || Ws <= 0 || So_h <= 0 || So_w <= 0) return VR_EINVAL;
    if (C < 1 || C > 4 || (filter != 2 && filter != 3)) return VR_EINVAL;
    if (So_w % 4 || Ws % 4 || B > 65535) return VR_EUNSUPPORTED;
    return VR_OK;
}

}  // namespace

static_assert(sizeof(vr_resample_box) == 48, "vr_resample_box is 48 bytes: the host marshals the [B] table as 12 int32 per sample");

extern "C" size_t vr_resample_ws_bytes(int32_t, int32_t, int32_t) { return 0; }   // the coefficients are computed in the kernel

extern "C" int vr_resample_band_rows(int32_t C, int32_t Hs, int32_t Ws, int32_t So_h, int32_t So_w, int32_t filter) {
    const int rc = rs_check_dims(1, C, Hs, Ws, So_h, So_w, filter);
    if (rc != VR_OK) return rc;
    const ResamplePlan p = rs_plan(C, Hs, Ws, So_h, So_w, filter);
    return p.band > 0 ? p.band : VR_EUNSUPPORTED;
}

extern "C" int vr_resample_u8(const uint8_t* src, const vr_resample_box* boxes, uint8_t* out, int32_t B, int32_t C, int32_t Hs,
                              int32_t Ws, int32_t So_h, int32_t So_w, int32_t filter, void* workspace, size_t ws_bytes,
                              vr_stream_t stream) {
    (void)workspace;
    (void)ws_bytes;
    if (!src || !boxes || !out || src == out) return VR_EINVAL;
    const int rc = rs_check_dims(B, C, Hs, Ws, So_h, So_w, filter);
    if (rc != VR_OK) return rc;
    if (((uintptr_t)src & 3) || ((uintptr_t)out & 3) || ((uintptr_t)boxes & 3)) return VR_EALIGN;
    const ResamplePlan p = rs_plan(C, Hs, Ws, So_h, So_w, filter);
    if (p.band <= 0) return VR_EUNSUPPORTED;
    hipLaunchKernelGGL(resample_u8_kernel, dim3((So_h + p.band - 1) / p.band, B), dim3(RS_THREADS), p.lds, (hipStream_t)stream, src,
                       boxes, out, C, Hs, Ws, So_h, So_w, filter == 3 ? 1 : 0, p);
    VR_CHECK_LAUNCH();
    return VR_OK;
}
