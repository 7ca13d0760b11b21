/*
 * libvitres_jpeg.so: the host half of JPEG decoding -- markers, Huffman decoding, DC prediction, restart markers -- up to the
 * quantised coefficients.  Plain C++ behind a C ABI: no HIP, nothing of libvitres_hip.so; this is what DataLoader workers load.
 * The device half (dequantise, inverse DCT, chroma upsampling, colour conversion, placement) is vr_jpeg_reconstruct_u8 of
 * include/vitres_hip.h.
 *
 * Conventions of vitres_hip.h: every entry returns int, 0 on success, negative on error (VR_EINVAL -1: a null pointer, a buffer that
 * is too small, or a damaged stream; VR_EUNSUPPORTED -3: a stream the fast path does not take).  Nothing is allocated beyond the
 * call, there is no global state, and every entry may be called from any number of threads at once.  The input is untrusted: every
 * read is checked against `len`, every write against the capacity given.
 *
 * What the fast path takes ("supported"): SOF0 (baseline), 8-bit samples, ONE interleaved Huffman scan of all components
 * (Ss = 0, Se = 63, Ah = Al = 0, components in frame order), sides 1..8192, and either
 *   three components, luma sampled 1x1, 2x1 or 2x2 and both chroma 1x1, in the colour space libjpeg would call YCbCr: a JFIF APP0
 *   marker was seen; else an Adobe APP14 marker says transform 1; else (neither marker) the component ids are not 'R','G','B';
 *   or one component sampled 1x1 (grayscale).
 * Everything else -- progressive, SOF1 and up, arithmetic coding, four components, several scans, other sampling factors, DNL, files
 * that are not JPEG, streams that end or break before the scan -- is "not supported".
 */
#ifndef VITRES_JPEG_H
#define VITRES_JPEG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vr_jpeg_info {
    int32_t supported;          /* 1: vr_jpeg_entropy_decode takes the stream; 0: every other field is 0 */
    int32_t width, height;
    int32_t ncomp;              /* 1 or 3 */
    int32_t hs, vs;             /* luma sampling factors (chroma is 1x1) */
    int32_t restart_interval;   /* MCUs between restart markers, 0: none */
    int32_t blocks[3];          /* 8 x 8 blocks of component c: bw[c] * bh[c] */
    int32_t bw[3], bh[3];       /* the component's plane in blocks, padded to whole MCUs */
} vr_jpeg_info;                 /* 16 int32 */

/* Parses the markers up to the first scan and nothing else.  Returns 0 and fills *info for every input, supported or not;
 * VR_EINVAL only for a null pointer or a negative length. */
int vr_jpeg_probe(const uint8_t* data, int64_t len, vr_jpeg_info* info);

/*
 * Decodes the scan of a supported stream.  coef (int16, `coef_capacity` elements, ZERO-FILLED BY THE CALLER) receives the quantised
 * coefficients de-interleaved: component 0's blocks, then component 1's, then component 2's; a component's blocks in raster order
 * of its block-padded plane (bh[c] rows of bw[c] blocks), 64 int16 per block in NATURAL (row-major) order.  Only non-zero
 * coefficients are written.  qtab (uint16 [3][64]) receives each component's quantisation table in natural order (rows of absent
 * components are zeroed).  *info is filled as by vr_jpeg_probe.
 * Returns 0, or with nothing promised about coef / qtab:
 *   VR_EUNSUPPORTED  the stream is not supported (info->supported = 0)
 *   VR_EINVAL        a null pointer; coef_capacity below 64 * (blocks[0] + blocks[1] + blocks[2]); a truncated stream; a bad marker
 *                    length; a missing table; a Huffman code that is not in its table; a run past coefficient 63; an AC size above
 *                    10 or a DC size above 11; a DC value outside int16; |coefficient * quantiser| above 32767; a restart marker
 *                    that is missing or out of order; anything but fill bytes and the end-of-image marker behind the last MCU.
 * Fill bytes (FF) before markers and stuffed FF 00 are handled.
 */
int vr_jpeg_entropy_decode(const uint8_t* data, int64_t len, vr_jpeg_info* info, int16_t* coef, int64_t coef_capacity,
                           uint16_t* qtab);

#ifdef __cplusplus
}
#endif
#endif /* VITRES_JPEG_H */
