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
#include "ragged.h"

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

// ---- the ragged route: vr_resample_ragged_u8 (include/vitres_hip.h) -----------------------------------------------------------------
// The same arithmetic from planes of every sample's own size in a flat buffer, with no limit on the scale: two launches through a
// global workspace instead of one through LDS, so no source row is resampled twice and no table has to hold a whole axis.
//   rs_ragged_h_kernel   one workgroup per (sample, block of RG_HROWS source rows of the crop), all channels.  Per chunk of output
//                        columns: the columns' tap spans and weight sums (one thread per column), their fixed-point coefficients
//                        (one thread per tap), then each wave stages (row, channel) segments as aligned dwords in its LDS slice and
//                        writes the resampled bytes into the sample's intermediate [C][h][So_w] in the workspace.
//   rs_ragged_v_kernel   one workgroup per (sample, band of RG_VROWS output rows): the rows' spans and sums, then their coefficients
//                        a slice of RG_VCOEF / RG_VROWS taps at a time; a lane reads the intermediate a dword per tap and stores 4
//                        output bytes.  With more than one slice the accumulators stay in registers across the slices of a round.
// rs_span / rs_coef are rs_taps taken apart -- the same operators in the same order -- so that the taps of one output index can be
// produced by many threads and in slices.
namespace {

constexpr int RG_HROWS = 32;                  // source rows per workgroup of the horizontal pass
constexpr int RG_VROWS = 8;                   // output rows per workgroup of the vertical pass
constexpr int RG_MAX_SIDE = 8192;             // a box's sides
constexpr int RG_HCOEF = 8200;                // ints: one column of the widest box (w = 8192 to ow = 4, bicubic: 8193 taps) fits
constexpr int RG_HCOLS = 256;                 // columns per chunk at most
constexpr int RG_HFIXED = RG_HCOLS * 16;      // bytes of the per-column tables (sum, first tap, taps)
constexpr int RG_STAGE = 28576;               // bytes at most, shared by the waves: a whole row of 8192 + 8 bytes fits three times
constexpr int RG_VCOEF = 12288;               // ints: 1536 taps of each of the band's rows per slice
constexpr int RG_VF_DWORDS = 24;              // a vertical-first crop has w < 8192 / 100: its aligned dwords per row
static_assert(RG_HCOEF * 4 + RG_HFIXED + RG_STAGE <= (int)RS_LDS_BUDGET && RG_STAGE >= 3 * (RG_MAX_SIDE + 16), "horizontal pass: LDS");
constexpr int RG_VFIXED = RG_VROWS * 16 + 4 * RG_VROWS * RG_VF_DWORDS * 4;
static_assert(RG_VCOEF * 4 + RG_VFIXED <= (int)RS_LDS_BUDGET && (RG_MAX_SIDE / 100 + 7) / 4 <= RG_VF_DWORDS && RG_VCOEF % RG_VROWS == 0, "vertical pass: LDS");

struct RaggedArgs {
    const uint8_t* src;
    long long src_bytes;
    const vr_ragged_plane* planes;
    const vr_resample_box* boxes;
    uint8_t* ws;
    long long ws_bytes;
    uint8_t* out;
    int C, Hs, Ws, So_h, So_w, bicubic;
    // the LDS of the two kernels, sized on the host for the launch's bounds (no box inside them needs more; the kernels clamp to them)
    int hcoef_ints, stage_bytes, vslice;
};

// a sample's box clamped into its own plane, and where its intermediate lives; ok == false: the sample's output is zeros
struct RgSample {
    bool ok, vfirst;                        // vfirst: PIL runs this crop's vertical pass first (below)
    int x0, y0, w, h, ow, oh, wx, wy, flip, pitch, rows;
    long long off, ws_off;
};
__device__ inline RgSample rg_sample(const RaggedArgs& a, int b) {
    RgSample s;
    const vr_ragged_plane p = a.planes[b];
    const vr_resample_box bx = a.boxes[b];
    s.ok = rg_plane_ok(p, a.C, a.src_bytes, a.Hs, a.Ws);
    s.pitch = p.pitch;
    s.rows = p.rows;
    s.off = p.off;
    s.ws_off = p.ws_off;
    if (!s.ok) return s;
    s.w = rs_clamp(bx.w, 1, min(p.pitch, RG_MAX_SIDE));
    s.h = rs_clamp(bx.h, 1, min(p.rows, RG_MAX_SIDE));
    s.x0 = rs_clamp(bx.x0, 0, p.pitch - s.w);
    s.y0 = rs_clamp(bx.y0, 0, p.rows - s.h);
    s.ow = max(bx.ow, a.So_w);
    s.oh = max(bx.oh, a.So_h);
    s.wx = rs_clamp(bx.wx, 0, s.ow - a.So_w);
    s.wy = rs_clamp(bx.wy, 0, s.oh - a.So_h);
    s.flip = bx.flip != 0;
    // PIL's Image.resize: an image more than 100 times as tall as wide that shrinks vertically is resized vertically FIRST
    // (`if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`), the 8-bit intermediate then being w x oh
    s.vfirst = s.h > 100 * s.w && s.oh < s.h;
    const long long need = (long long)a.C * s.h * a.So_w;                       // the intermediate [C][h][So_w]
    if (p.ws_off < 0 || (p.ws_off & 3) || p.ws_off > a.ws_bytes || need > a.ws_bytes - p.ws_off) s.ok = false;
    return s;
}

// taps of output index xx: PIL's bounds and the sum of its weights, accumulated in tap order
struct RsSpan {
    int xmin, n;
    double ww;
};
__device__ inline RsSpan rs_span(const RsAxis& a, int xx, int bicubic) {
    const double center = (xx + 0.5) * a.scale;
    int xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > a.in) xmax = a.in;
    if (xmin > a.in - 1) xmin = a.in - 1;
    int n = xmax - xmin;
    n = n < 1 ? 1 : n;
    double ww = 0.0;
    for (int t = 0; t < n; ++t) ww += rs_filter((xmin + t - center + 0.5) * a.ss, bicubic);
    return RsSpan{xmin, n, ww};
}
// coefficient of tap t of that index
__device__ inline int rs_coef(const RsAxis& a, int xx, int xmin, double ww, int t, int bicubic) {
    const double center = (xx + 0.5) * a.scale;
    double w = rs_filter((xmin + t - center + 0.5) * a.ss, bicubic);
    if (ww != 0.0) w = w / ww;
    return w < 0 ? (int)(-0.5 + w * (double)(1 << RS_PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << RS_PRECISION_BITS));
}
__device__ inline int rs_ktaps(const RsAxis& a, int bicubic) {                  // PIL's ksize: no index has more taps
    return (int)ceil(a.support) * 2 + 1;
}

__global__ __launch_bounds__(RS_THREADS) void rs_ragged_h_kernel(RaggedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
    // LDS: hww [RG_HCOLS] f64 | hmin [RG_HCOLS] | hcnt [RG_HCOLS] | hcoef [tap][column of the chunk], hcoef_ints | stage, stage_bytes
    double* hww = (double*)rg_lds;
    int* hmin = (int*)(hww + RG_HCOLS);
    int* hcnt = hmin + RG_HCOLS;
    int* hcoef = hcnt + RG_HCOLS;
    unsigned char* stage_all = (unsigned char*)(hcoef + a.hcoef_ints);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const RgSample s = rg_sample(a, b);
    if (!s.ok || s.vfirst) return;                                              // (uniform over the workgroup)
    // the crop's rows the window's vertical taps touch: first tap of its first row .. last tap of its last row
    const RsAxis ay = rs_axis(s.h, s.oh, a.bicubic);
    const RsSpan first = rs_span(ay, s.wy, a.bicubic), last = rs_span(ay, s.wy + a.So_h - 1, a.bicubic);
    const int ylo = first.xmin, yhi = last.xmin + last.n;                       // (both bounds grow with the index)
    const int r0 = ylo + blockIdx.x * RG_HROWS;
    if (r0 >= yhi) return;
    const int nrows = min(RG_HROWS, yhi - r0);
    const RsAxis ax = rs_axis(s.w, s.ow, a.bicubic);
    const int ks = min(min(rs_ktaps(ax, a.bicubic), s.w), a.hcoef_ints);        // (a span is clipped to the crop)
    const int chunk = max(1, min(min(RG_HCOLS, a.hcoef_ints / ks), a.So_w));
    uint8_t* inter = a.ws + s.ws_off;
    for (int c0 = 0; c0 < a.So_w; c0 += chunk) {
        const int nc = min(chunk, a.So_w - c0);
        __syncthreads();                                                        // the previous chunk's tables are no longer read
        for (int c = tid; c < nc; c += RS_THREADS) {
            const RsSpan sp = rs_span(ax, s.wx + c0 + c, a.bicubic);
            hmin[c] = sp.xmin;
            hcnt[c] = min(sp.n, ks);
            hww[c] = sp.ww;
        }
        __syncthreads();
        for (int i = tid; i < nc * ks; i += RS_THREADS) {
            const int t = i / nc, c = i - t * nc;
            if (t < hcnt[c]) hcoef[i] = rs_coef(ax, s.wx + c0 + c, hmin[c], hww[c], t, a.bicubic);
        }
        // the aligned dwords that cover the chunk's taps: columns smin .. smax - 1 of the crop
        const int smin = hmin[0], smax = hmin[nc - 1] + hcnt[nc - 1];
        const int a0 = (s.x0 + smin) & ~3, off = s.x0 + smin - a0;
        const int nd = min((((s.x0 + smax + 3) & ~3) - a0) >> 2, a.stage_bytes >> 2);   // (never cut: a crop's row fits the stage)
        const int slice = (nd * 4 + 15) & ~15;
        const int nw = max(1, min(RS_WAVES, a.stage_bytes / slice));
        unsigned char* stage = stage_all + (size_t)(wave < nw ? wave : 0) * slice;
        const int items = nrows * a.C, trips = (items + nw - 1) / nw;
        for (int trip = 0; trip < trips; ++trip) {
            const int it = trip * nw + wave;
            const bool live = wave < nw && it < items;
            const int c = live ? it / nrows : 0, row = live ? it - c * nrows : 0;
            __syncthreads();                                                    // coefficients written; the slices are free again
            if (live) {
                const uint32_t* g = (const uint32_t*)(a.src + s.off + ((size_t)c * s.rows + (s.y0 + r0 + row)) * s.pitch + a0);
                for (int i = lane; i < nd; i += 64) ((uint32_t*)stage)[i] = g[i];
            }
            __syncthreads();
            if (live) {
                uint8_t* trow = inter + ((size_t)c * s.h + (r0 + row)) * a.So_w + c0;
                for (int col = lane; col < nc; col += 64) {
                    const unsigned char* p = stage + off + (hmin[col] - smin);
                    const int cnt = hcnt[col];
                    int acc = 1 << (RS_PRECISION_BITS - 1);
                    for (int t = 0; t < cnt; ++t) acc += hcoef[t * nc + col] * (int)p[t];
                    trow[col] = (uint8_t)rs_clip8(acc);
                }
            }
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void rs_ragged_v_kernel(RaggedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
    // LDS: vww [RG_VROWS] f64 | vmin | vcnt | vtmp (vertical-first: the band's rows of the w x oh image) | vcoef [row][tap of the slice]
    double* vww = (double*)rg_lds;
    int* vmin = (int*)(vww + RG_VROWS);
    int* vcnt = vmin + RG_VROWS;
    uint32_t* vtmp = (uint32_t*)(vcnt + RG_VROWS);
    int* vcoef = (int*)(vtmp + 4 * RG_VROWS * RG_VF_DWORDS);
    const int SLICE = a.vslice;
    const int tid = threadIdx.x;
    const int b = blockIdx.y, r0 = blockIdx.x * RG_VROWS;
    const int bh = min(RG_VROWS, a.So_h - r0);
    const int oquads = a.So_w >> 2;
    const RgSample s = rg_sample(a, b);
    if (!s.ok) {                                                                // (uniform over the workgroup)
        for (int i = tid; i < a.C * bh * oquads; i += RS_THREADS) {
            const int quads = oquads;
            const int q = i % quads, rc = i / quads, r = rc % bh, c = rc / bh;
            *(uint32_t*)(a.out + (((size_t)b * a.C + c) * a.So_h + (r0 + r)) * a.So_w + 4 * q) = 0u;
        }
        return;
    }
    const RsAxis ay = rs_axis(s.h, s.oh, a.bicubic);
    if (tid < bh) {
        const RsSpan sp = rs_span(ay, s.wy + r0 + tid, a.bicubic);
        vmin[tid] = sp.xmin;
        vcnt[tid] = min(sp.n, s.h - sp.xmin);                                   // (never cuts a span: keeps every tap inside the crop)
        vww[tid] = sp.ww;
    }
    __syncthreads();
    int most = 0;
    for (int r = 0; r < bh; ++r) most = max(most, vcnt[r]);
    const int slices = (most + SLICE - 1) / SLICE;
    // what the vertical pass reads: the horizontal pass's intermediate [C][h][So_w] -- or, vertical-first, the crop itself as the
    // aligned dwords that cover its columns
    const uint8_t* vsrc = a.ws + s.ws_off;
    size_t vstride = (size_t)a.So_w, vplane = (size_t)s.h * a.So_w;
    int quads = oquads, xoff = 0;
    if (s.vfirst) {
        const int a0 = s.x0 & ~3;
        quads = (((s.x0 + s.w + 3) & ~3) - a0) >> 2;                            // (<= RG_VF_DWORDS: w <= 81)
        xoff = s.x0 - a0;
        vsrc = a.src + s.off + (size_t)s.y0 * s.pitch + a0;
        vstride = (size_t)s.pitch;
        vplane = (size_t)s.rows * s.pitch;
    }
    const int vitems = a.C * bh * quads;
    const int rounds = (vitems + RS_THREADS - 1) / RS_THREADS;
    for (int round = 0; round < rounds; ++round) {
        const int i = round * RS_THREADS + tid;
        const bool live = i < vitems;
        const int q = live ? i % quads : 0, rc = live ? i / quads : 0, r = rc % bh, c = rc / bh;
        int acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = 1 << (RS_PRECISION_BITS - 1);
        for (int sl = 0; sl < slices; ++sl) {
            const int t0 = sl * SLICE;
            if (slices > 1 || round == 0) {                                     // one slice: the table is filled once for every round
                __syncthreads();
                for (int k = tid; k < bh * SLICE; k += RS_THREADS) {
                    const int rr = k / SLICE, t = t0 + (k - rr * SLICE);
                    if (t < vcnt[rr]) vcoef[k] = rs_coef(ay, s.wy + r0 + rr, vmin[rr], vww[rr], t, a.bicubic);
                }
                __syncthreads();
            }
            if (live) {
                const int cnt = min(vcnt[r] - t0, SLICE);
                const uint32_t* col = (const uint32_t*)(vsrc + (size_t)c * vplane + (size_t)(vmin[r] + t0) * vstride) + q;
                const int* k = vcoef + r * SLICE;
                const size_t step = vstride >> 2;
                for (int t = 0; t < cnt; ++t) {
                    const uint32_t px = col[(size_t)t * step];
                    const int kk = k[t];
                    acc[0] += kk * (int)(px & 255u);
                    acc[1] += kk * (int)((px >> 8) & 255u);
                    acc[2] += kk * (int)((px >> 16) & 255u);
                    acc[3] += kk * (int)(px >> 24);
                }
            }
        }
        if (live && s.vfirst) {
            vtmp[(c * bh + r) * RG_VF_DWORDS + q] = (uint32_t)rs_clip8(acc[0]) | ((uint32_t)rs_clip8(acc[1]) << 8)
                                                    | ((uint32_t)rs_clip8(acc[2]) << 16) | ((uint32_t)rs_clip8(acc[3]) << 24);
        } else if (live) {
            uint32_t v;
            int oc;
            if (s.flip) {
                v = (uint32_t)rs_clip8(acc[3]) | ((uint32_t)rs_clip8(acc[2]) << 8) | ((uint32_t)rs_clip8(acc[1]) << 16)
                    | ((uint32_t)rs_clip8(acc[0]) << 24);
                oc = a.So_w - 4 - 4 * q;
            } else {
                v = (uint32_t)rs_clip8(acc[0]) | ((uint32_t)rs_clip8(acc[1]) << 8) | ((uint32_t)rs_clip8(acc[2]) << 16)
                    | ((uint32_t)rs_clip8(acc[3]) << 24);
                oc = 4 * q;
            }
            *(uint32_t*)(a.out + (((size_t)b * a.C + c) * a.So_h + (r0 + r)) * a.So_w + oc) = v;
        }
    }
    if (!s.vfirst) return;
    // vertical-first: the horizontal pass over the band's rows in LDS; a thread per output byte makes its own coefficients (such
    // crops are at most 81 pixels wide and rare: no table)
    __syncthreads();
    const RsAxis ax = rs_axis(s.w, s.ow, a.bicubic);
    const unsigned char* tb = (const unsigned char*)vtmp;
    for (int i = tid; i < a.C * bh * a.So_w; i += RS_THREADS) {
        const int col = i % a.So_w, rc = i / a.So_w, r = rc % bh, c = rc / bh;
        const RsSpan sp = rs_span(ax, s.wx + col, a.bicubic);
        const int n = min(sp.n, s.w - sp.xmin);
        const unsigned char* p = tb + (size_t)(c * bh + r) * RG_VF_DWORDS * 4 + xoff + sp.xmin;
        int acc = 1 << (RS_PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) acc += rs_coef(ax, s.wx + col, sp.xmin, sp.ww, t, a.bicubic) * (int)p[t];
        a.out[(((size_t)b * a.C + c) * a.So_h + (r0 + r)) * a.So_w + (s.flip ? a.So_w - 1 - col : col)] = (uint8_t)rs_clip8(acc);
    }
}

}  // namespace

extern "C" size_t vr_resample_ragged_ws_bytes(int32_t C, int64_t total_rows, int32_t So_w) {
    if (C <= 0 || total_rows <= 0 || So_w <= 0) return 0;
    return ((size_t)C * (size_t)total_rows * (size_t)So_w + 15) & ~(size_t)15;
}

extern "C" int vr_resample_ragged_u8(const uint8_t* src, int64_t src_bytes, const vr_ragged_plane* planes, const vr_resample_box* boxes,
                                     uint8_t* out, int32_t B, int32_t C, int32_t Hs, int32_t Ws, int32_t So_h, int32_t So_w,
                                     int32_t filter, void* workspace, size_t ws_bytes, vr_stream_t stream) {
    if (!src || !planes || !boxes || !out || src == out || src_bytes <= 0) return VR_EINVAL;
    const int rc = rs_check_dims(B, C, Hs, Ws, So_h, So_w, filter);
    if (rc != VR_OK) return rc;
    if (!workspace || ws_bytes < vr_resample_ragged_ws_bytes(C, 1, So_w) || workspace == (const void*)src || workspace == (void*)out)
        return VR_EINVAL;
    if (((uintptr_t)src & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)planes & 7) || ((uintptr_t)out & 3)
        || ((uintptr_t)boxes & 3))
        return VR_EALIGN;
    RaggedArgs a = {src, (long long)src_bytes, planes, boxes, (uint8_t*)workspace, (long long)ws_bytes, out,
                    C, Hs, Ws, So_h, So_w, filter == 3 ? 1 : 0, 0, 0, 0};
    // a box inside the bounds has at most `most` rows and `wide` columns, so at most these taps per output index: the tables are
    // sized for them (a small launch keeps its LDS small and its workgroups per CU many), never beyond the fixed maxima
    const int most = Hs < RG_MAX_SIDE ? Hs : RG_MAX_SIDE, wide = Ws < RG_MAX_SIDE ? Ws : RG_MAX_SIDE;
    int ksh = rs_ksize(wide, So_w, filter), ksv = rs_ksize(most, So_h, filter);
    ksh = ksh < 0 || ksh > wide ? wide : ksh;
    ksv = ksv < 0 || ksv > most ? most : ksv;
    const long long cols = So_w < RG_HCOLS ? So_w : RG_HCOLS;
    const long long hints = cols * ksh < RG_HCOEF ? cols * ksh : RG_HCOEF;      // (one column always fits: ksh <= 8192)
    a.hcoef_ints = ((int)hints + 3) & ~3;
    const int slice = (wide + 8 + 15) & ~15;
    a.stage_bytes = RS_WAVES * slice < RG_STAGE ? RS_WAVES * slice : RG_STAGE;
    const int vs = ksv < RG_VCOEF / RG_VROWS ? ksv : RG_VCOEF / RG_VROWS;
    a.vslice = (vs + 3) & ~3;
    const size_t hlds = RG_HFIXED + (size_t)a.hcoef_ints * 4 + a.stage_bytes, vlds = RG_VFIXED + (size_t)RG_VROWS * a.vslice * 4;
    hipLaunchKernelGGL(rs_ragged_h_kernel, dim3((most + RG_HROWS - 1) / RG_HROWS, B), dim3(RS_THREADS), hlds, (hipStream_t)stream, a);
    VR_CHECK_LAUNCH();
    hipLaunchKernelGGL(rs_ragged_v_kernel, dim3((So_h + RG_VROWS - 1) / RG_VROWS, B), dim3(RS_THREADS), vlds, (hipStream_t)stream, a);
    VR_CHECK_LAUNCH();
    return VR_OK;
}
