// vr_rand_augment_u8: timm's RandAugment ops on uint8 [B,3,H,W] batches, bit for bit what PIL 12 makes of the HWC RGB image
// (include/vitres_hip.h states every op's arithmetic).
//
// One workgroup per sample walks the sample's layers in order.  A layer reads the whole image and writes the whole image: the last
// applied layer writes `out`, the ones before it alternate between the sample's workspace plane and `out`, so one plane per sample
// is all the workspace there is; a workgroup barrier and a device fence hand the image from layer to layer.  Records that apply
// nothing (VR_RA_IDENTITY, an unknown op / filter, an argument out of range, or one that maps every value to itself) are skipped
// before the first layer runs; with none left the sample is copied.  The whole-image statistics (the histograms of autocontrast /
// equalize, the grey sum of contrast) are gathered in LDS by the one workgroup that owns the sample, so nothing synchronises
// across workgroups.
//   LUT ops       table [3][256] in LDS; a lane maps a dword (4 pixels of one channel)
//   blend ops     a lane takes 4 pixels of all three channels; float32, one rounding per operator (contraction is off)
//   affine        a lane takes 4 output pixels: the source coordinate in double, one rounding per operator, then PIL's bilinear
//                 / bicubic taps per channel, a row's taps in one load
#include "common.h"
#include "../../include/vitres_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int RA_THREADS = 1024;
constexpr int RA_MAX_LAYERS = 4;

struct RaShared {
    int hist[3][256];
    uint8_t lut[3][256];
    unsigned long long lsum;
};

__device__ __forceinline__ int ra_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// does the record change the image?  (uniform over the workgroup)
__device__ inline bool ra_live(const vr_ra_op& r) {
    switch (r.op) {
        case VR_RA_INVERT:
        case VR_RA_AUTOCONTRAST:
        case VR_RA_EQUALIZE:
        case VR_RA_BRIGHTNESS:
        case VR_RA_COLOR:
        case VR_RA_CONTRAST:
        case VR_RA_SHARPNESS: return true;
        case VR_RA_POSTERIZE: return r.iarg >= 0 && r.iarg <= 7;            // 8 bits keep every value
        case VR_RA_SOLARIZE: return r.iarg >= 0 && r.iarg <= 255;           // threshold 256 inverts nothing
        case VR_RA_SOLARIZE_ADD: return r.iarg >= 1 && r.iarg <= 255;       // adding 0 changes nothing
        case VR_RA_AFFINE: return r.filter == 2 || r.filter == 3;
        default: return false;
    }
}

__device__ __forceinline__ uint32_t ra_map4(const uint8_t* lut, uint32_t v) {
    return (uint32_t)lut[v & 255u] | ((uint32_t)lut[(v >> 8) & 255u] << 8) | ((uint32_t)lut[(v >> 16) & 255u] << 16)
           | ((uint32_t)lut[v >> 24] << 24);
}

__device__ void ra_copy(const uint8_t* in, uint8_t* dst, int n4) {
    const int tid = threadIdx.x;
    if ((((uintptr_t)in | (uintptr_t)dst) & 15) == 0) {
        const int n16 = n4 >> 2;
        for (int i = tid; i < n16; i += RA_THREADS) ((uint4*)dst)[i] = ((const uint4*)in)[i];
        for (int i = (n16 << 2) + tid; i < n4; i += RA_THREADS) ((uint32_t*)dst)[i] = ((const uint32_t*)in)[i];
    } else {
        for (int i = tid; i < n4; i += RA_THREADS) ((uint32_t*)dst)[i] = ((const uint32_t*)in)[i];
    }
}

// ---- per-channel LUT ops ------------------------------------------------------------------------------------------------------
// autocontrast / equalize: wave c (c < 3) turns channel c's histogram into its table, a lane holding bins 4l .. 4l + 3
__device__ void ra_stat_lut(RaShared& sh, int op, int npix) {
    const int tid = threadIdx.x, lane = tid & 63, c = tid >> 6;
    if (c >= 3) return;
    int h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = sh.hist[c][4 * lane + j];
    const bool any = (h[0] | h[1] | h[2] | h[3]) != 0;
    const unsigned long long mask = __ballot(any);                        // never 0: the image has pixels
    const int lo_lane = __ffsll((long long)mask) - 1, hi_lane = 63 - __clzll((long long)mask);
    const int first = 4 * lane + (h[0] ? 0 : (h[1] ? 1 : (h[2] ? 2 : 3)));
    const int last = 4 * lane + (h[3] ? 3 : (h[2] ? 2 : (h[1] ? 1 : 0)));
    const int lo = __shfl(first, lo_lane, 64), hi = __shfl(last, hi_lane, 64);
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 4 * lane + j;
    if (op == VR_RA_AUTOCONTRAST) {
        if (hi > lo) {
            const double scale = 255.0 / (double)(hi - lo);
            const double offset = (double)(-lo) * scale;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ra_clampi((int)((double)(4 * lane + j) * scale + offset), 0, 255);
        }
    } else {
        int bins = (h[0] != 0) + (h[1] != 0) + (h[2] != 0) + (h[3] != 0);
        int incl = h[0] + h[1] + h[2] + h[3];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64), upb = __shfl_xor(bins, o, 64);
            if (lane >= o) incl += up;
            bins += upb;
        }
        const int hlast = __shfl(h[last & 3], hi_lane, 64);
        const int step = (npix - hlast) / 255;
        if (bins > 1 && step > 0) {
            int n = step / 2 + incl - (h[0] + h[1] + h[2] + h[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = n / step;
                v[j] = q > 255 ? 255 : q;
                n += h[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sh.lut[c][4 * lane + j] = (uint8_t)v[j];
}

__device__ void ra_lut_layer(RaShared& sh, const vr_ra_op& r, const uint8_t* in, uint8_t* dst, int npix) {
    const int tid = threadIdx.x, q = npix >> 2, n4 = 3 * q;
    const uint32_t* in4 = (const uint32_t*)in;
    if (r.op == VR_RA_AUTOCONTRAST || r.op == VR_RA_EQUALIZE) {
        for (int i = tid; i < 768; i += RA_THREADS) (&sh.hist[0][0])[i] = 0;
        __syncthreads();
        for (int i = tid; i < n4; i += RA_THREADS) {
            const uint32_t v = in4[i];
            int* h = sh.hist[i / q];
            atomicAdd(&h[v & 255u], 1);
            atomicAdd(&h[(v >> 8) & 255u], 1);
            atomicAdd(&h[(v >> 16) & 255u], 1);
            atomicAdd(&h[v >> 24], 1);
        }
        __syncthreads();
        ra_stat_lut(sh, r.op, npix);
    } else if (tid < 256) {
        const int i = tid, a = r.iarg;
        int v;
        if (r.op == VR_RA_INVERT) v = 255 - i;
        else if (r.op == VR_RA_POSTERIZE) v = i & ~((1 << (8 - a)) - 1);
        else if (r.op == VR_RA_SOLARIZE) v = i < a ? i : 255 - i;
        else v = i < 128 ? (i + a > 255 ? 255 : i + a) : i;               // VR_RA_SOLARIZE_ADD
        sh.lut[0][i] = sh.lut[1][i] = sh.lut[2][i] = (uint8_t)v;
    }
    __syncthreads();
    for (int i = tid; i < n4; i += RA_THREADS) ((uint32_t*)dst)[i] = ra_map4(sh.lut[i / q], in4[i]);
}

// ---- blend ops: Image.blend(degenerate, image, factor) ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ra_blend(int d, int x, float alpha, bool interp) {
    const float t = (float)d + alpha * (float)(x - d);
    if (interp) return (uint32_t)(int)t;                                  // between d and x: inside [0, 255]
    if (!(t > 0.0f)) return 0u;
    return t >= 255.0f ? 255u : (uint32_t)(int)t;
}

__device__ __forceinline__ int ra_grey(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ void ra_blend_layer(RaShared& sh, const vr_ra_op& r, const uint8_t* in, uint8_t* dst, int H, int W) {
    const int tid = threadIdx.x, npix = H * W, q = npix >> 2, wq = W >> 2;
    const uint32_t* in4 = (const uint32_t*)in;
    uint32_t* dst4 = (uint32_t*)dst;
    const float alpha = r.factor;
    const bool interp = alpha >= 0.0f && alpha <= 1.0f;
    int mean = 0;
    if (r.op == VR_RA_CONTRAST) {
        if (tid == 0) sh.lsum = 0ull;
        __syncthreads();
        unsigned int part = 0;
        for (int i = tid; i < q; i += RA_THREADS) {
            const uint32_t R = in4[i], G = in4[q + i], B = in4[2 * q + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) part += (unsigned)ra_grey((R >> (8 * j)) & 255, (G >> (8 * j)) & 255, (B >> (8 * j)) & 255);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if ((tid & 63) == 0) atomicAdd(&sh.lsum, (unsigned long long)part);
        __syncthreads();
        mean = (int)((double)sh.lsum / (double)npix + 0.5);
    }
    for (int i = tid; i < q; i += RA_THREADS) {
        uint32_t px[3] = {in4[i], in4[q + i], in4[2 * q + i]};
        uint32_t res[3] = {0u, 0u, 0u};
        if (r.op == VR_RA_SHARPNESS) {
            const int y = i / wq, xq = i - y * wq;
            const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
            const int xl = xq > 0 ? xq - 1 : 0, xr = xq < wq - 1 ? xq + 1 : wq - 1;
            const bool yedge = y == 0 || y == H - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t* pc = in4 + c * q;
                int col[6] = {0, 0, 0, 0, 0, 0};                         // column sums over the three rows, x = 4 xq - 1 .. 4 xq + 4
                const int rows[3] = {ym, y, yp};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t* pr = pc + rows[k] * wq;
                    const uint32_t a = pr[xl], m = pr[xq], b = pr[xr];
                    col[0] += (int)(a >> 24);
                    col[1] += (int)(m & 255u);
                    col[2] += (int)((m >> 8) & 255u);
                    col[3] += (int)((m >> 16) & 255u);
                    col[4] += (int)(m >> 24);
                    col[5] += (int)(b & 255u);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = (int)((px[c] >> (8 * j)) & 255u), xx = 4 * xq + j;
                    // (s / 13 + 0.5 truncated: PIL sums in float32, but an integer s leaves s / 13 + 0.5 at least 1 / 26 from every
                    // integer, so the exact quotient is the same byte); the one-pixel border is the source's
                    const int s = col[j] + col[j + 1] + col[j + 2] + 4 * x;
                    const int d = (yedge || xx == 0 || xx == W - 1) ? x : (2 * s + 13) / 26;
                    res[c] |= ra_blend(d, x, alpha, interp) << (8 * j);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x0 = (int)((px[0] >> (8 * j)) & 255u), x1 = (int)((px[1] >> (8 * j)) & 255u), x2 = (int)((px[2] >> (8 * j)) & 255u);
                const int d = r.op == VR_RA_BRIGHTNESS ? 0 : (r.op == VR_RA_COLOR ? ra_grey(x0, x1, x2) : mean);
                res[0] |= ra_blend(d, x0, alpha, interp) << (8 * j);
                res[1] |= ra_blend(d, x1, alpha, interp) << (8 * j);
                res[2] |= ra_blend(d, x2, alpha, interp) << (8 * j);
            }
        }
        dst4[i] = res[0];
        dst4[q + i] = res[1];
        dst4[2 * q + i] = res[2];
    }
}

// ---- affine: PIL's ImagingGenericTransform with affine_transform and bilinear_filter / bicubic_filter --------------------------------
// A row's taps are neighbouring bytes, so one (unaligned) load fetches them all: the load starts at the first tap clamped so that the
// whole load lies inside the row, and each tap's clamped index picks its byte.  Along x the taps are bytes, so PIL's p2 .. p4 are
// integer expressions: evaluated as integers here (exact either way), which leaves the double unit the Horner form alone.
__device__ __forceinline__ double ra_cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}
__device__ __forceinline__ double ra_cubic_row(const uint8_t* pr, const int* sh, double d) {
    uint32_t w;
    __builtin_memcpy(&w, pr, 4);
    const int v1 = (int)((w >> sh[0]) & 255u), v2 = (int)((w >> sh[1]) & 255u), v3 = (int)((w >> sh[2]) & 255u),
              v4 = (int)((w >> sh[3]) & 255u);
    const double p1 = (double)v2, p2 = (double)(-v1 + v3), p3 = (double)(2 * (v1 - v2) + v3 - v4), p4 = (double)(-v1 + v2 - v3 + v4);
    return p1 + d * (p2 + d * (p3 + d * p4));
}
__device__ __forceinline__ double ra_linear_row(const uint8_t* pr, int sa, int sb, double d) {
    uint16_t w;
    __builtin_memcpy(&w, pr, 2);
    const int a = (int)((w >> sa) & 255u), b = (int)((w >> sb) & 255u);
    return (double)a + (double)(b - a) * d;
}

__device__ void ra_affine_layer(const vr_ra_op& r, const uint8_t* in, uint8_t* dst, int H, int W, uint32_t fill) {
    const int tid = threadIdx.x, npix = H * W, q = npix >> 2, wq = W >> 2;
    const bool bicubic = r.filter == 3;
    const double m0 = r.m[0], m1 = r.m[1], m2 = r.m[2], m3 = r.m[3], m4 = r.m[4], m5 = r.m[5];
    uint32_t* dst4 = (uint32_t*)dst;
    for (int i = tid; i < q; i += RA_THREADS) {
        const int y = i / wq, xq = i - y * wq;
        uint32_t res[3] = {0u, 0u, 0u};
        const double yc = (double)y + 0.5;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const double xc = (double)(4 * xq + j) + 0.5;
            double xin = m0 * xc + m1 * yc + m2;
            double yin = m3 * xc + m4 * yc + m5;
            if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
                res[0] |= (fill & 255u) << (8 * j);
                res[1] |= ((fill >> 8) & 255u) << (8 * j);
                res[2] |= ((fill >> 16) & 255u) << (8 * j);
                continue;
            }
            xin -= 0.5;
            yin -= 0.5;
            const double fx = floor(xin), fy = floor(yin);
            const int x0 = (int)fx, y0 = (int)fy;                         // x0 in [-1, W - 1], y0 in [-1, H - 1]
            const double dx = xin - fx, dy = yin - fy;
            if (bicubic) {
                const int xb = ra_clampi(x0 - 1, 0, W - 4);                 // W >= 4: bytes xb .. xb + 3 lie inside the row
                int sh[4], ys[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    sh[t] = 8 * (ra_clampi(x0 - 1 + t, 0, W - 1) - xb);    // in {0, 8, 16, 24}
                    ys[t] = ra_clampi(y0 - 1 + t, 0, H - 1) * W + xb;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* p = in + (size_t)c * npix;
                    double row[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) row[t] = ra_cubic_row(p + ys[t], sh, dx);
                    const double v = ra_cubic(row[0], row[1], row[2], row[3], dy);
                    const uint32_t b = !(v > 0.0) ? 0u : (v >= 255.0 ? 255u : (uint32_t)(int)v);
                    res[c] |= b << (8 * j);
                }
            } else {
                const int xb = ra_clampi(x0, 0, W - 2);
                const int sa = 8 * (ra_clampi(x0, 0, W - 1) - xb), sb = 8 * (ra_clampi(x0 + 1, 0, W - 1) - xb);   // in {0, 8}
                const int ya = ra_clampi(y0, 0, H - 1) * W + xb, yb = ra_clampi(y0 + 1, 0, H - 1) * W + xb;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* p = in + (size_t)c * npix;
                    const double v1 = ra_linear_row(p + ya, sa, sb, dx);
                    const double v2 = ra_linear_row(p + yb, sa, sb, dx);
                    const double v = v1 + (v2 - v1) * dy;
                    res[c] |= ((uint32_t)ra_clampi((int)v, 0, 255)) << (8 * j);
                }
            }
        }
        dst4[i] = res[0];
        dst4[q + i] = res[1];
        dst4[2 * q + i] = res[2];
    }
}

__global__ __launch_bounds__(RA_THREADS) void rand_augment_u8_kernel(const uint8_t* src, const vr_ra_op* ops, uint8_t* out,
                                                                     uint8_t* ws, int H, int W, int layers, uint32_t fill) {
    __shared__ RaShared sh;
    const int b = blockIdx.x, npix = H * W;
    const size_t plane = (size_t)3 * npix;
    const uint8_t* cur = src + (size_t)b * plane;
    uint8_t* o = out + (size_t)b * plane;
    uint8_t* w = ws ? ws + (size_t)b * plane : nullptr;
    const vr_ra_op* recs = ops + (size_t)b * layers;

    int n = 0;
    for (int k = 0; k < layers; ++k) n += ra_live(recs[k]) ? 1 : 0;
    if (n == 0) {
        ra_copy(cur, o, (int)(plane >> 2));
        return;
    }
    int done = 0;
    for (int k = 0; k < layers; ++k) {
        const vr_ra_op r = recs[k];
        if (!ra_live(r)) continue;
        uint8_t* dst = ((n - 1 - done) & 1) ? w : o;                       // the last applied layer lands in `out`
        if (r.op == VR_RA_AFFINE) ra_affine_layer(r, cur, dst, H, W, fill);
        else if (r.op >= VR_RA_BRIGHTNESS) ra_blend_layer(sh, r, cur, dst, H, W);
        else ra_lut_layer(sh, r, cur, dst, npix);
        cur = dst;
        if (++done < n) {                                                  // the next layer reads what every wave of this one wrote
            __threadfence();
            __syncthreads();
        }
    }
}

}  // namespace

static_assert(sizeof(vr_ra_op) == 64, "vr_ra_op is 64 bytes: the host marshals the [B, layers] table as 16 int32 per record");

extern "C" size_t vr_rand_augment_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t layers) {
    if (B <= 0 || H <= 0 || W <= 0 || layers <= 1) return 0;
    return (size_t)B * 3 * (size_t)H * (size_t)W;
}

extern "C" int vr_rand_augment_u8(const uint8_t* src, const vr_ra_op* ops, uint8_t* out, int32_t B, int32_t H, int32_t W,
                                  int32_t layers, uint32_t fill_rgb, void* workspace, size_t ws_bytes, vr_stream_t stream) {
    if (!src || !ops || !out || src == out) return VR_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || layers < 1 || layers > RA_MAX_LAYERS) return VR_EINVAL;
    const size_t need = vr_rand_augment_ws_bytes(B, H, W, layers);
    if (need && (!workspace || ws_bytes < need || workspace == (const void*)src || workspace == (void*)out)) return VR_EINVAL;
    if (W % 4 || B > 65535 || (long long)H * W * 3 > 0x7fffffffLL) return VR_EUNSUPPORTED;
    if (((uintptr_t)src & 3) || ((uintptr_t)out & 3) || ((uintptr_t)ops & 7) || (need && ((uintptr_t)workspace & 3))) return VR_EALIGN;
    hipLaunchKernelGGL(rand_augment_u8_kernel, dim3(B), dim3(RA_THREADS), 0, (hipStream_t)stream, src, ops, out,
                       need ? (uint8_t*)workspace : nullptr, H, W, layers, fill_rgb);
    VR_CHECK_LAUNCH();
    return VR_OK;
}
