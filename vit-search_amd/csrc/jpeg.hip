// vr_jpeg_reconstruct_u8: the device half of JPEG decoding.  The host (libvitres_jpeg.so) has Huffman-decoded every stream of the
// batch into quantised coefficients; this entry turns them into the zero-padded uint8 canvas batch that pad_collate_u8 would have
// made of PIL's decoded images, bit for bit (include/vitres_hip.h states the arithmetic: libjpeg's ISLOW inverse DCT, its "fancy"
// chroma upsampling and its YCbCr -> RGB tables, all in 32-bit integers).
//
// Two launches inside the one entry, the component sample planes in the caller's workspace between them:
//   1. jpeg_idct_kernel   one 8 x 8 block per thread: eight 16-byte loads of the block's coefficients, dequantisation with the
//                         image's tables (staged in LDS), both IDCT passes in registers, eight 8-byte stores into the block-padded
//                         sample plane of its component.
//   2. jpeg_place_kernel  four canvas pixels of all three channels per thread: a dword of luma, the chroma neighbourhood as two
//                         dwords per row, upsample, convert, three dword stores.  Raw records (kind 1) read their planes straight
//                         from the blob.  Threads outside the image -- and every thread of an image whose record fails the
//                         device's own check -- store zeros, so the launch writes every byte of the canvas.
// Every record is validated against blob_bytes, Hs, Ws and the limits before anything is read through it, by both kernels.
// vr_jpeg_reconstruct_ragged_u8 is the same entry with another destination: launch 1 unchanged, then jpeg_place_ragged_kernel, which
// writes every image's planes of its OWN size (vr_ragged_plane, ragged.h) in a flat buffer -- the pixels come from the same jp_quad.
#include "common.h"
#include "../../include/vitres_hip.h"
#include "ragged.h"

namespace {

constexpr int JP_THREADS = 256;
constexpr int JP_MAX_SIDE = 8192;

// the device's own test of a record: everything the kernels index with is bounded by what is checked here
__device__ bool jp_valid(const vr_jpeg_desc& d, long long blob_bytes, int Hs, int Ws) {
    if ((unsigned)d.kind > 1u) return false;
    if (d.width < 1 || d.width > Ws || d.width > JP_MAX_SIDE || d.height < 1 || d.height > Hs || d.height > JP_MAX_SIDE) return false;
    const int nc = d.ncomp, hs = d.hs, vs = d.vs;
    if (d.kind == VR_JPEG_RAW) {
        if (nc != 3 || hs != 1 || vs != 1) return false;
    } else if (nc == 1) {
        if (hs != 1 || vs != 1) return false;
    } else if (nc == 3) {
        if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    } else {
        return false;
    }
    const int mx = (d.width + 8 * hs - 1) / (8 * hs), my = (d.height + 8 * vs - 1) / (8 * vs);
    const long long unit = d.kind == VR_JPEG_RAW ? 64 : 128;         // bytes of one 8 x 8 block in the blob
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= nc) break;
        const int bw = mx * (c == 0 ? hs : 1), bh = my * (c == 0 ? vs : 1);
        if (d.bw[c] != bw || d.bh[c] != bh || d.off[c] < 0) return false;
        if ((long long)d.off[c] * 16 + (long long)bw * bh * unit > blob_bytes) return false;
    }
    return true;
}

__device__ __forceinline__ uint32_t jp_sra(uint32_t x, int n) { return (uint32_t)((int32_t)x >> n); }

// libjpeg jidctint.c (ISLOW, CONST_BITS 13) on eight values, descaled by SHIFT with rounding; unsigned arithmetic: it wraps
template <int SHIFT>
__device__ __forceinline__ void jp_idct8(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t& c4, uint32_t& c5,
                                         uint32_t& c6, uint32_t& c7) {
    constexpr uint32_t R = 1u << (SHIFT - 1);
    uint32_t z1 = (c2 + c6) * 4433u;
    const uint32_t t2 = z1 - c6 * 15137u, t3 = z1 + c2 * 6270u;
    const uint32_t t0 = (c0 + c4) << 13, t1 = (c0 - c4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t o0 = c7, o1 = c5, o2 = c3, o3 = c1;
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    o0 *= 2446u;
    o1 *= 16819u;
    o2 *= 25172u;
    o3 *= 12299u;
    z1 *= (uint32_t)-7373;
    z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5;
    z4 = z4 * (uint32_t)-3196 + z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    c0 = jp_sra(t10 + o3 + R, SHIFT);
    c7 = jp_sra(t10 - o3 + R, SHIFT);
    c1 = jp_sra(t11 + o2 + R, SHIFT);
    c6 = jp_sra(t11 - o2 + R, SHIFT);
    c2 = jp_sra(t12 + o1 + R, SHIFT);
    c5 = jp_sra(t12 - o1 + R, SHIFT);
    c3 = jp_sra(t13 + o0 + R, SHIFT);
    c4 = jp_sra(t13 - o0 + R, SHIFT);
}

__device__ __forceinline__ uint32_t jp_sample(uint32_t v) {              // + 128, clamped to a byte
    const int32_t s = (int32_t)v + 128;
    return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_idct_kernel(const uint8_t* __restrict__ blob, long long blob_bytes,
                                                               const vr_jpeg_desc* __restrict__ descs,
                                                               const uint16_t* __restrict__ qtabs, uint8_t* __restrict__ ws, int Hs,
                                                               int Ws) {
    __shared__ uint16_t sq[3 * 64];
    const int b = blockIdx.y;
    const vr_jpeg_desc d = descs[b];
    if (!jp_valid(d, blob_bytes, Hs, Ws) || d.kind != VR_JPEG_COEF) return;      // (uniform over the workgroup)
    const int n0 = d.bw[0] * d.bh[0], n1 = d.ncomp == 3 ? d.bw[1] * d.bh[1] : 0, n2 = d.ncomp == 3 ? d.bw[2] * d.bh[2] : 0;
    const int total = n0 + n1 + n2;
    if ((int)(blockIdx.x * JP_THREADS) >= total) return;
    if (threadIdx.x < 3 * 64) sq[threadIdx.x] = qtabs[(size_t)b * 192 + threadIdx.x];
    __syncthreads();
    for (int t = blockIdx.x * JP_THREADS + threadIdx.x; t < total; t += gridDim.x * JP_THREADS) {
        const int c = t < n0 ? 0 : (t < n0 + n1 ? 1 : 2);
        const int i = t - (c == 0 ? 0 : (c == 1 ? n0 : n0 + n1));
        const int bw = c == 0 ? d.bw[0] : (c == 1 ? d.bw[1] : d.bw[2]);
        const int off = c == 0 ? d.off[0] : (c == 1 ? d.off[1] : d.off[2]);
        const int by = i / bw, bx = i - by * bw;
        const uint4* src = (const uint4*)(blob + (size_t)off * 16 + (size_t)i * 128);
        const uint16_t* q = sq + 64 * c;
        uint32_t x[64];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint4 w = src[r];
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[8 * r + 2 * j] = (uint32_t)((int32_t)(int16_t)(ww[j] & 0xffffu) * (int32_t)q[8 * r + 2 * j]);
                x[8 * r + 2 * j + 1] = (uint32_t)((int32_t)(int16_t)(ww[j] >> 16) * (int32_t)q[8 * r + 2 * j + 1]);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)                                                    // columns: descale by CONST_BITS - PASS1_BITS
            jp_idct8<11>(x[k], x[8 + k], x[16 + k], x[24 + k], x[32 + k], x[40 + k], x[48 + k], x[56 + k]);
        uint8_t* dst = ws + (size_t)off * 8 + ((size_t)by * 8 * bw + bx) * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {                                                  // rows: by CONST_BITS + PASS1_BITS + 3
            jp_idct8<18>(x[8 * r], x[8 * r + 1], x[8 * r + 2], x[8 * r + 3], x[8 * r + 4], x[8 * r + 5], x[8 * r + 6], x[8 * r + 7]);
            uint2 o;
            o.x = jp_sample(x[8 * r]) | jp_sample(x[8 * r + 1]) << 8 | jp_sample(x[8 * r + 2]) << 16 | jp_sample(x[8 * r + 3]) << 24;
            o.y = jp_sample(x[8 * r + 4]) | jp_sample(x[8 * r + 5]) << 8 | jp_sample(x[8 * r + 6]) << 16 | jp_sample(x[8 * r + 7]) << 24;
            *(uint2*)(dst + (size_t)r * bw * 8) = o;
        }
    }
}

// The four chroma samples p[i - 1 .. i + 2] of a row (i even, indices clamped to 0 .. dw - 1) from two dword loads.  row32: the row
// as dwords, nd of them.
__device__ __forceinline__ void jp_chroma4(const uint32_t* row32, int nd, int i, int dw, int* p) {
    const int bi = i >> 2;
    int lo, hi, cover;
    if ((i & 2) == 0) {
        lo = bi > 0 ? bi - 1 : 0;
        hi = bi;
        cover = 4 * (bi - 1);
    } else {
        lo = bi;
        hi = bi + 1 < nd ? bi + 1 : nd - 1;
        cover = 4 * bi;
    }
    const unsigned long long v = (unsigned long long)row32[lo] | (unsigned long long)row32[hi] << 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int idx = i - 1 + k;
        idx = idx < 0 ? 0 : (idx > dw - 1 ? dw - 1 : idx);
        p[k] = (int)((v >> (8 * (idx - cover))) & 255ull);                 // idx - cover in 0 .. 7 (see the header of this function)
    }
}

__device__ __forceinline__ uint32_t jp_byte(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// The four pixels (y, x0 .. x0 + 3) of the image of a record that passed jp_valid, a byte each in R, G, B; zero where outside the
// image.  Both place kernels -- the padded canvas and the ragged planes -- get their bytes here.
__device__ __forceinline__ void jp_quad(const uint8_t* __restrict__ blob, const uint8_t* __restrict__ ws, const vr_jpeg_desc& d,
                                        int y, int x0, uint32_t& R, uint32_t& G, uint32_t& B) {
    R = G = B = 0u;
    if (y < d.height && x0 < d.width) {
        const bool raw = d.kind == VR_JPEG_RAW;
        const uint8_t* base = raw ? blob : ws;
        const size_t unit = raw ? 16 : 8;                                    // bytes per offset unit: coefficients are two bytes a sample
        const uint8_t* p0 = base + (size_t)d.off[0] * unit;
        const uint32_t Y4 = *(const uint32_t*)(p0 + (size_t)y * d.bw[0] * 8 + x0);
        if (d.ncomp == 1) {
            R = G = B = Y4;
        } else {
            const uint8_t* p1 = base + (size_t)d.off[1] * unit;
            const uint8_t* p2 = base + (size_t)d.off[2] * unit;
            const int s1 = d.bw[1] * 8, s2 = d.bw[2] * 8;
            if (raw) {
                R = Y4;
                G = *(const uint32_t*)(p1 + (size_t)y * s1 + x0);
                B = *(const uint32_t*)(p2 + (size_t)y * s2 + x0);
            } else {
                int cb[4], cr[4];
                if (d.hs == 1) {
                    const uint32_t b4 = *(const uint32_t*)(p1 + (size_t)y * s1 + x0), r4 = *(const uint32_t*)(p2 + (size_t)y * s2 + x0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        cb[j] = (int)((b4 >> (8 * j)) & 255u);
                        cr[j] = (int)((r4 >> (8 * j)) & 255u);
                    }
                } else {
                    const int dw = (d.width + 1) >> 1, i = x0 >> 1;
                    const bool v2 = d.vs == 2, fancy = dw > 2;
                    const int dh = v2 ? (d.height + 1) >> 1 : d.height;
                    const int r = v2 ? y >> 1 : y;
                    int rn = (y & 1) ? r + 1 : r - 1;                         // the row the vertical filter blends in
                    rn = rn < 0 ? 0 : (rn > dh - 1 ? dh - 1 : rn);
#pragma unroll
                    for (int c = 1; c < 3; ++c) {
                        const uint8_t* pc = c == 1 ? p1 : p2;
                        const int sc = c == 1 ? s1 : s2;
                        int* o = c == 1 ? cb : cr;
                        int a[4];
                        jp_chroma4((const uint32_t*)(pc + (size_t)r * sc), sc >> 2, i, dw, a);
                        if (!fancy) {                                         // plain doubling, both ways
                            o[0] = o[1] = a[1];
                            o[2] = o[3] = a[2];
                        } else if (!v2) {
                            o[0] = (3 * a[1] + a[0] + 1) >> 2;
                            o[1] = (3 * a[1] + a[2] + 2) >> 2;
                            o[2] = (3 * a[2] + a[1] + 1) >> 2;
                            o[3] = (3 * a[2] + a[3] + 2) >> 2;
                        } else {
                            int n[4];
                            jp_chroma4((const uint32_t*)(pc + (size_t)rn * sc), sc >> 2, i, dw, n);
                            const int t0 = 3 * a[0] + n[0], t1 = 3 * a[1] + n[1], t2 = 3 * a[2] + n[2], t3 = 3 * a[3] + n[3];
                            o[0] = (3 * t1 + t0 + 8) >> 4;
                            o[1] = (3 * t1 + t2 + 7) >> 4;
                            o[2] = (3 * t2 + t1 + 8) >> 4;
                            o[3] = (3 * t2 + t3 + 7) >> 4;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int yy = (int)((Y4 >> (8 * j)) & 255u), u = cb[j] - 128, v = cr[j] - 128;
                    R |= jp_byte(yy + ((91881 * v + 32768) >> 16)) << (8 * j);
                    G |= jp_byte(yy + ((-22554 * u - 46802 * v + 32768) >> 16)) << (8 * j);
                    B |= jp_byte(yy + ((116130 * u + 32768) >> 16)) << (8 * j);
                }
            }
        }
        const int left = d.width - x0;                                        // bytes of this quad inside the image
        if (left < 4) {
            const uint32_t m = (1u << (8 * left)) - 1u;
            R &= m;
            G &= m;
            B &= m;
        }
    }
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_place_kernel(const uint8_t* __restrict__ blob, long long blob_bytes,
                                                                const vr_jpeg_desc* __restrict__ descs,
                                                                const uint8_t* __restrict__ ws, uint8_t* __restrict__ canvas, int Hs,
                                                                int Ws) {
    const int b = blockIdx.y, wq = Ws >> 2;
    const long long quad = (long long)blockIdx.x * JP_THREADS + threadIdx.x;
    if (quad >= (long long)Hs * wq) return;
    const int y = (int)(quad / wq), x0 = 4 * (int)(quad - (long long)y * wq);
    const size_t plane = (size_t)Hs * Ws;
    uint32_t* out = (uint32_t*)(canvas + (size_t)b * 3 * plane + (size_t)y * Ws + x0);
    const vr_jpeg_desc d = descs[b];
    uint32_t R = 0u, G = 0u, B = 0u;
    if (jp_valid(d, blob_bytes, Hs, Ws)) jp_quad(blob, ws, d, y, x0, R, G, B);
    out[0] = R;
    *(uint32_t*)((uint8_t*)out + plane) = G;
    *(uint32_t*)((uint8_t*)out + 2 * plane) = B;
}

// The ragged form: the sample's three planes of rows x pitch bytes at its record's offset in the flat buffer, every byte of them.
// A sample whose plane record fails rg_plane_ok, or does not hold the image, has nothing written; an invalid JPEG record zeros.
constexpr int JP_RAGGED_QUADS = 4;                    // quads per thread at the launch's bounds (the grid strides over a sample's)
__global__ __launch_bounds__(JP_THREADS) void jpeg_place_ragged_kernel(const uint8_t* __restrict__ blob, long long blob_bytes,
                                                                       const vr_jpeg_desc* __restrict__ descs,
                                                                       const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst,
                                                                       long long dst_bytes,
                                                                       const vr_ragged_plane* __restrict__ planes, int Hs, int Ws) {
    const int b = blockIdx.y;
    const vr_ragged_plane p = planes[b];
    if (!rg_plane_ok(p, 3, dst_bytes, Hs, Ws)) return;                               // (uniform over the workgroup)
    const int pq = p.pitch >> 2;
    const long long quads = (long long)p.rows * pq;
    if ((long long)blockIdx.x * JP_THREADS >= quads) return;
    const vr_jpeg_desc d = descs[b];
    const bool valid = jp_valid(d, blob_bytes, Hs, Ws);
    if (valid && (d.width > p.pitch || d.height > p.rows)) return;                   // the plane does not hold the image
    const size_t plane = (size_t)p.rows * p.pitch;
    uint8_t* base = dst + p.off;
    for (long long quad = (long long)blockIdx.x * JP_THREADS + threadIdx.x; quad < quads; quad += (long long)gridDim.x * JP_THREADS) {
        const int y = (int)(quad / pq), x0 = 4 * (int)(quad - (long long)y * pq);
        uint32_t R = 0u, G = 0u, B = 0u;
        if (valid) jp_quad(blob, ws, d, y, x0, R, G, B);
        uint8_t* out = base + (size_t)y * p.pitch + x0;
        *(uint32_t*)out = R;
        *(uint32_t*)(out + plane) = G;
        *(uint32_t*)(out + 2 * plane) = B;
    }
}

// What both entries check, in the order EINVAL, EUNSUPPORTED, EALIGN.  dst: the canvas (dst_mask 3) or the flat buffer (15); `more`:
// whether the entry's own further arguments are given (the ragged one's planes and dst_bytes), refused with the first EINVALs.
int jp_check(const void* blob, int64_t blob_bytes, const vr_jpeg_desc* descs, const uint16_t* qtabs, const uint8_t* dst,
             uintptr_t dst_mask, bool more, int32_t B, int32_t Hs, int32_t Ws, const void* workspace, size_t ws_bytes) {
    if (!blob || !descs || !qtabs || !dst || !more || blob_bytes <= 0 || B <= 0 || Hs <= 0 || Ws <= 0) return VR_EINVAL;
    if (!workspace || ws_bytes < vr_jpeg_ws_bytes(blob_bytes) || workspace == blob || workspace == (const void*)dst
        || (const void*)dst == blob)
        return VR_EINVAL;
    if (Ws % 4 || B > 65535 || Hs > JP_MAX_SIDE || Ws > JP_MAX_SIDE) return VR_EUNSUPPORTED;
    if (((uintptr_t)blob & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)dst & dst_mask) || ((uintptr_t)descs & 3)
        || ((uintptr_t)qtabs & 1))
        return VR_EALIGN;
    return VR_OK;
}

// launch 1 of both entries: the component sample planes into the workspace
int jp_launch_idct(const void* blob, int64_t blob_bytes, const vr_jpeg_desc* descs, const uint16_t* qtabs, int32_t B, int32_t Hs,
                   int32_t Ws, void* workspace, vr_stream_t stream) {
    // an image inside the bounds has at most this many blocks (4:4:4: three planes of whole MCUs); the kernel strides over more
    const long long most = 3LL * (Ws / 8 + 2) * (Hs / 8 + 2);
    const unsigned gx = (unsigned)((most + JP_THREADS - 1) / JP_THREADS);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(gx, B), dim3(JP_THREADS), 0, (hipStream_t)stream, (const uint8_t*)blob,
                       (long long)blob_bytes, descs, qtabs, (uint8_t*)workspace, Hs, Ws);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

}  // namespace

static_assert(sizeof(vr_jpeg_desc) == 64, "vr_jpeg_desc is 64 bytes: the host marshals the table as 16 int32 per record");

extern "C" size_t vr_jpeg_ws_bytes(int64_t blob_bytes) {
    if (blob_bytes <= 0) return 0;
    return (((size_t)blob_bytes + 1) / 2 + 15) & ~(size_t)15;
}

extern "C" int vr_jpeg_reconstruct_u8(const void* blob, int64_t blob_bytes, const vr_jpeg_desc* descs, const uint16_t* qtabs,
                                      uint8_t* canvas, int32_t B, int32_t Hs, int32_t Ws, void* workspace, size_t ws_bytes,
                                      vr_stream_t stream) {
    int rc = jp_check(blob, blob_bytes, descs, qtabs, canvas, 3, true, B, Hs, Ws, workspace, ws_bytes);
    if (rc == VR_OK) rc = jp_launch_idct(blob, blob_bytes, descs, qtabs, B, Hs, Ws, workspace, stream);
    if (rc != VR_OK) return rc;
    const long long quads = (long long)Hs * (Ws / 4);
    hipLaunchKernelGGL(jpeg_place_kernel, dim3((unsigned)((quads + JP_THREADS - 1) / JP_THREADS), B), dim3(JP_THREADS), 0,
                       (hipStream_t)stream, (const uint8_t*)blob, (long long)blob_bytes, descs, (const uint8_t*)workspace, canvas, Hs,
                       Ws);
    VR_CHECK_LAUNCH();
    return VR_OK;
}

extern "C" int vr_jpeg_reconstruct_ragged_u8(const void* blob, int64_t blob_bytes, const vr_jpeg_desc* descs, const uint16_t* qtabs,
                                             uint8_t* dst, int64_t dst_bytes, const vr_ragged_plane* planes, int32_t B, int32_t Hs,
                                             int32_t Ws, void* workspace, size_t ws_bytes, vr_stream_t stream) {
    int rc = jp_check(blob, blob_bytes, descs, qtabs, dst, 15, planes && dst_bytes > 0, B, Hs, Ws, workspace, ws_bytes);
    if (rc == VR_OK && ((uintptr_t)planes & 7)) rc = VR_EALIGN;
    if (rc == VR_OK) rc = jp_launch_idct(blob, blob_bytes, descs, qtabs, B, Hs, Ws, workspace, stream);
    if (rc != VR_OK) return rc;
    const long long per = (long long)JP_THREADS * JP_RAGGED_QUADS, quads = (long long)Hs * (Ws / 4);
    hipLaunchKernelGGL(jpeg_place_ragged_kernel, dim3((unsigned)((quads + per - 1) / per), B), dim3(JP_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)blob, (long long)blob_bytes, descs, (const uint8_t*)workspace, dst, (long long)dst_bytes, planes,
                       Hs, Ws);
    VR_CHECK_LAUNCH();
    return VR_OK;
}
