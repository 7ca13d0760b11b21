/*
 * vitres_hip.h -- C ABI of libvitres_hip.so, the MI355X (gfx950) kernel library behind the
 * ViT-Res (super)network hot path of yilunliao/vit-search.
 *
 * The reference has NO native code and no FFI: the seam the hot path sits behind is the timm model
 * registry + nn.Module protocol (reference main.py:329-348).  This header is
 * therefore the boundary a maintainer of the reference would bind (with ctypes)
 * to replace the ATen op sequences listed next to each entry point.
 *
 * Conventions (all entry points):
 *   - extern "C", plain device pointers and sizes; no torch types.
 *   - The caller owns every buffer (inputs, outputs, workspaces); the library never allocates,
 *     frees or retains pointers; re-entrant.  Its only mutable state is a few function-local
 *     caches of device facts, filled on first use: the CU count (gemm.hip) and the dynamic-LDS
 *     limit already granted to each attention kernel (attn.hip, attn_mfma.hip).
 *   - All work is enqueued asynchronously on `stream`; no hidden synchronisation.
 *   - Return value: 0 = ok; > 0 = hipError_t of the launch; < 0 = argument validation
 *     (VR_EINVAL -1, VR_EALIGN -2, VR_EUNSUPPORTED -3).  No exceptions cross the ABI.
 *   - dtype codes: VR_F32 = 0 (exact-fp32 parity mode), VR_BF16 = 1 (raw bf16 bits, fast mode), VR_F16 = 2 (raw IEEE
 *     binary16 bits: the forward / evaluation forms only -- every backward / training entry returns VR_EUNSUPPORTED for it,
 *     and so do the opt-in bf16 forms: K-split shares, the panel-resident GEMM, vr_gemm_ln_fold).  bf16 and fp16 never mix
 *     in one call; the 3x3 convolution entries (which name only their output type) take fp16 operands when out_dtype is VR_F16.
 *   - `keep` arrays: int32[B], active channel-prefix length of each sample for that tensor
 *     (the reference's ChannelDrop prefix masks, nets/channel_drop.py:153-154); NULL = dense.
 *   - "rows_per_sample": number of consecutive rows (tokens) that belong to one sample.
 */
#ifndef VITRES_HIP_H
#define VITRES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* vr_stream_t; /* == hipStream_t */

#define VR_F32 0
#define VR_BF16 1
#define VR_F16 2

/* library / ABI version (major*1000 + minor) */
int vr_version(void);

/* row remap of a token-indexed operand: row(m) = (m / rpi) * rps + off + (m % rpi); rpi==0: identity */
typedef struct vr_rowmap {
    int32_t rpi, rps, off;
} vr_rowmap;

/*
 * Generic fused GEMM:  C[M,N] (+)= epilogue( A[M,K] * B[N,K]^T )
 * Replaces: nn.Linear forward/backward in nets/supernet_blocks.py:37-52,102-119 (qkv, proj, fc1, fc2),
 * cls_head/patch_head (nets/vit_sr_supernet.py:440-446), token_transform (:151), the patchify
 * convolutions expressed as GEMMs (timm PatchEmbed, nets/patch_conv.py:56-58, vit_sr_supernet.py:140),
 * and the `x * mask` / drop_path / residual adds that follow them (supernet_blocks.py:214-253).
 *
 *   a_trans/b_trans = 0: operand stored [rows, K] (K contiguous); 1: stored [K, rows] (rows contiguous).
 *   forward   y = x W^T      : a_trans 0, b_trans 0
 *   dgrad     dx = dy W      : a_trans 0, b_trans 1      (B = W viewed as [K_out rows][N_in contraction])
 *   wgrad     dW = dy^T x    : a_trans 1, b_trans 1, contraction over tokens, split_k > 1, atomic = 1
 * Epilogue, in this order:  v = acc (+ bias[n]) (+ pos[m % rows_in][n]);
 *   act==1: C gets the pre-activation u=v, C2 gets gelu(u), both 0 where masked by keep_n;   (Mlp.forward)
 *   dact_u != NULL: v *= gelu'(u[m][n]);                                          (fc2 dgrad -> du)
 *   keep_n: v = 0 where n >= keep_n[sample(m)];  scale: v *= scale[sample(m)];   (ChannelDrop, DropPath)
 *   resid != NULL: v += resid[out_row][n] (fp32, ldc layout);  atomic: atomicAdd into fp32 C.
 * Masked-work skipping (the supernet's sampled sub-networks): keep_k[s] promises that A[m, k] == 0 for
 * rows m of sample s and (k % k_period) >= keep_k[s]; K slices with no kept k for any sample of the tile are not
 * loaded, and output tiles with no kept column (keep_n) skip their whole K loop (they still store the masked value).
 * In wgrad form the samples are those of the token range of the split: keep_k bounds the kept output ROWS, keep_n the
 * kept output COLUMNS (rows/columns beyond are exactly zero gradients); fully masked tiles are not computed -- except the tile that
 * owns bias_grad, which runs whenever a row is kept: the bias gradient sums A over all tokens, whatever columns B keeps.
 */
typedef struct vr_gemm_args {
    const void* A;
    const void* B;
    void* C;
    void* C2;            /* act==1: second output gelu(u) (same dtype/ld as C) while C gets u; NULL with act==1: C gets
                            gelu(u) alone (forward-only evaluation: the pre-activation is not kept) */
    const float* bias;   /* [N] or NULL */
    const float* pos;    /* [rows_in, N] or NULL */
    const float* scale;  /* [batch] or NULL */
    const int32_t* keep_n; /* [batch] or NULL */
    const float* resid;  /* fp32 [*, ldc] or NULL (may alias C for in-place accumulate) */
    const void* dact_u;  /* pre-activation for gelu' (dtype = in_dtype, leading dim ldu) or NULL */
    const int32_t* keep_k; /* [batch] or NULL: work-skipping hint, see below */
    float* bias_grad;    /* wgrad only (a_trans && atomic): bias_grad[m] += sum_k A[k][m]  (the Linear's bias gradient,
                            fused so that dY is read once), or NULL.  The sum runs over ALL tokens: keep_n (the kept columns of X)
                            does not bound it -- a sample whose input width is 0 still has a bias gradient */
    int32_t M, N, K;
    int32_t lda, ldb, ldc, ldu;
    int32_t a_trans, b_trans;
    int32_t in_dtype;    /* dtype of A and B (and dact_u) */
    int32_t out_dtype;   /* dtype of C/C2 */
    int32_t act;         /* 0 none; 1 gelu (dual store with C2: C = u, C2 = gelu(u); single store without: C = gelu(u)); 2 the
                            saved-derivative form of the same pair: forward (no dact_u) C = gelu'(u), C2 = gelu(u); data gradient
                            (dact_u given) multiplies by dact_u as it is -- no transcendental in the backward epilogue;
                            3 relu, single store: C = max(u, 0) (no C2 / dact_u) */
    int32_t atomic;      /* 1: atomicAdd into fp32 C; 2 (weight-gradient form, bf16 operands, 8-element aligned leading dimensions):
                            C and bias_grad are OVERWRITTEN by plain stores -- every output tile is computed by one workgroup over
                            the whole token range (split_k <= 1), fully masked tiles write zeros, the destination need not be
                            zero-filled; VR_EUNSUPPORTED where only the atomic kernels cover the form */
    int32_t split_k;     /* >= 1 */
    int32_t rows_in;     /* rows per sample of the M index (0: single sample); wgrad: tokens per sample of the K index */
    int32_t n_period;    /* > 0: column n is kept iff (n % n_period) < keep_n[s] (per-head prefixes of the qkv layout) */
    int32_t k_period;    /* same for keep_k */
    int32_t sched;       /* scheduling hints (bit mask, 0 = default).  None changes results beyond fp32 summation order.
                            1 = launched beside another kernel on a second stream (general kernel: 128x128 tile, one workgroup per
                                tile instead of persistent workgroups);
                            2 = keep the hardware's round-robin workgroup -> XCD order (default: tiles remapped so that an XCD owns
                                a contiguous run);
                            4 = always use the general kernel (gemm.hip) -- measurement aid;
                            8, 16, 32 = measurement aids of gemm_nt.hip (force its kernels, record stamps in ws);
                            64 (vr_gemm_group, first problem) = tn_body's instruction stream for the weight-gradient group instead of
                                the lean LDS-DMA one (tests); 0x10000 (same place) = the 8-wave, double-buffered group kernel -- one
                                workgroup per CU, one token split for the whole group (faster alone, +0.05 ms inside the step: opt-in);
                            128 (vr_gemm_group, first problem) = the group may fill the chip (default: at most two resident
                                workgroups per CU);
                            0x2000 / 0x4000 (vr_gemm_group weight-gradient problems) = measurement aids that produce WRONG results:
                                the problem skips its epilogue / its K loop; a group whose first problem carries either bit runs on
                                tn_body's group kernel (as with 64);
                            0x100 = gemm_nt.hip's kernels instead of the lean-loop ones (gemm_ntk.hip);
                            0x600 / 0x1800 = slice buffers (1 - 3; see `ring`) / tile (1: 128 x 128, 2: 64 x 128, 3: 64 x 64) of the
                                lean-loop kernels instead of their grid-size rule (tests);
                            0x40000 = the caller vouches that every reader of C / C2 is a kernel that tiles group by group (m_groups
                                below) and skips the masked channels of a row's group: bf16 outputs without a residual then leave
                                tiles that are masked (keep_n) for every row UNWRITTEN instead of storing zeros;
                            0x80000 = an operand of this launch was produced that way -- the launch runs on the group-by-group
                                kernels or fails with VR_EUNSUPPORTED, it is never handed to a kernel that tiles across groups;
                            0x200000 = the panel-resident kernel (gemm_panel.hip: K <= 320, bf16 result, K-contiguous weight; the A
                                panel in LDS, weight strips in registers) wherever it covers the form, 0x800000 with it: its 80-row /
                                4-wave form; 0x400000 / 0x1000000 / 0x2000000 with it: its measurement forms (no MFMA / no weight
                                loads: results are NOT the GEMM's).  Opt-in: measured slower than the tiled kernels */
    vr_rowmap a_map;     /* remap of A's token rows (M index if a_trans==0, K index if a_trans==1) */
    vr_rowmap b_map;     /* remap of B's token rows (only meaningful when b_trans==1 && a_trans==1) */
    vr_rowmap c_map;     /* remap of output rows */
    int32_t m_groups;    /* > 1: the token index (M rows; wgrad: K tokens) consists of this many equal, contiguous groups of samples
                            with different keep_k / keep_n each -- the architecture groups of the supernet's multi-arch step
                            (engine.py:119-165, channel_drop.py:101-105).  The kernels interleave the groups' row tiles (wgrad:
                            token splits) in their XCD-contiguous workgroup order, so that no XCD is dealt only the sparsest (or
                            only the densest) architecture; when m_groups divides the rows, the bf16 kernels (gemm_ntk / gemm_nt_ln
                            / gemm_tn) also cut the grid per group -- no tile or token split holds rows of two groups (the last
                            tile of a group is short).  Results do not depend on it.  A keep value -(k + 2) marks a sample that is
                            masked on its own inside a group of width k (DropPath): every kernel reads it as 0.  0 / 1: one group */
    void* ws;            /* optional workspace of the K-split kernels (k_shares below): the workgroups that share a tile exchange fp32
                            partial accumulators through it.  >= vr_gemm_ws_bytes() bytes, 16-byte aligned, ZERO before its first
                            use (the kernels leave its tickets at zero), never shared by launches that may run concurrently (one per
                            stream).  NULL: every tile is computed by one workgroup. */
    int64_t ws_bytes;
    int32_t ring;        /* lean-loop bf16 kernels (gemm_ntk.hip): slice buffers of the K loop's ring (1 - 6; one slice is multiplied while
                            ring - 1 are in flight).  0 = the library's rule: as deep as LDS allows without lowering the number of
                            workgroups the grid gives a CU */
    int32_t k_shares;    /* lean-loop bf16 kernels: workgroups that share a tile's K slices (needs ws; the partial fp32 tiles meet in ws by
                            plain write-through stores, the last arriver sums them in share order and runs the epilogue -- results do
                            not depend on arrival order, no fp32 atomics touch the output).  0 / 1 = one workgroup per tile (no rule
                            turns the split on: every real split measured slower than the unsplit kernel on the step's shapes,
                            DESIGN.md), 2 - 4 = that many shares wherever the form has a split kernel and ws holds tiles x shares
                            slabs of the tile's fp32 size */
    /* Glue of the spatial-reduction block and of the patch embedding folded into the GEMM that touches the same rows
       (nets/vit_sr_supernet.py:114-172,398-407).  Forward bf16 / fp16 forms with an fp32 result only (gemm_nt.hip; N % 8 == 0,
       ldc % 8 == 0, no act / dact_u / a_trans / b_trans / atomic), VR_EUNSUPPORTED anywhere else.  All zero / NULL: none of it. */
    const float* sr_x;   /* pooled shortcut: fp32 [batch, sr_tokens + sr_g^2, sr_cin], the block's input stream.  Output row
                            (sample s, m = oh * (sr_g/2) + ow) gets, where resid would be added and for columns n < sr_cin,
                            0.25f * (((p00 + p01) + p10) + p11), p_ij = sr_x[s][sr_tokens + (2 oh + i) sr_g + 2 ow + j][n] -- what
                            vr_sr_resid writes and a resid read of it adds.  rows_in == (sr_g/2)^2, sr_cin % 8 == 0; no resid / scale */
    const int32_t* keep_out; /* [batch] or NULL: columns n >= keep_out[s] are stored as exact 0, after every other term (vr_mask_rows
                            on the result).  Not together with keep_n */
    const float* tok_src; /* tok_rows > 0: the launch also stores the tok_rows leading token rows of every sample's output block -- row
                            s * c_map.rps + t, t < tok_rows == c_map.off, c_map.rpi == rows_in -- written by the workgroups that hold the
                            sample's first GEMM row:  C[.][n] = (n < tok_cols ? tok_src[(s * tok_rps + t) * tok_ld + n] : 0)
                            (+ tok_pos[t * N + n]), 0 for n >= keep_out[s] (or keep_n[s]).  tok_rps == 0: the same rows for every sample */
    const float* tok_pos; /* fp32 [tok_rows, N] or NULL */
    int32_t sr_g, sr_cin, sr_tokens;
    int32_t tok_rows, tok_ld, tok_rps, tok_cols;
    int32_t reserved0;
} vr_gemm_args;

/* bytes of vr_gemm_args.ws that enable tile sharing on the current device */
int vr_gemm_ws_bytes(void);

int vr_gemm(const vr_gemm_args* args, vr_stream_t stream);

/*
 * vr_gemm_group: exactly `for (i < count) vr_gemm(&args[i], stream)`, but 2..4 bf16 weight-gradient problems of the split-token
 * form (a_trans && b_trans && atomic, split_k == 0, un-mapped rows) -- the four Linears of one transformer block, autograd of
 * F.linear at nets/supernet_blocks.py:36,48,102,118 -- run as ONE launch whose workgroups share the CUs.  Any other mix is
 * issued problem by problem.  Outputs must not alias between problems.
 */
int vr_gemm_group(const vr_gemm_args* args, int32_t count, vr_stream_t stream);

/*
 * vr_gemm with the adjacent LayerNorm fused into its epilogue (workgroups own whole output rows; bf16 operands, fp32 output,
 * N % 8 == 0, N <= 512, no n_period / pos / act / row maps on the output; ldc is also the row stride of x, resid, gt_out).
 *   mode 0 -- forward of attention `proj` / Mlp `fc2` (nets/supernet_blocks.py:214-253) and the LayerNorm that consumes the
 *     updated residual stream (norm2 of the block, norm1 of the next block):
 *       C = resid + scale[s] * mask_{keep_n}(A B^T + bias)                     exactly vr_gemm
 *       (y, mean, rstd) = MaskedLayerNorm(C; w, b, keep, eps)                  exactly vr_ln_fwd with bf16 output, y is [M, N]
 *   mode 1 -- data gradient of `qkv` / `fc1` and the backward of the LayerNorm that fed them (nets/masked_layer_norm.py:55-88):
 *       dy = A B^T  (A = dU, B = W^T K-contiguous; never written),
 *       C = (resid ? resid : 0) + dLN/dx(dy);  dw += sum dy*xhat;  db += sum dy;
 *       gt_out[m,c] = c < gt_keep[s] ? C[m,c] * gt_scale[s] : 0 (bf16, optional)  exactly vr_ln_bwd on a fp32 dy
 *     (args.bias / scale / keep_n must be NULL; keep_k / k_period / rows_in keep their vr_gemm meaning).
 * Kernel: 64 x 256 / 64 x 320 / 32 x 512 tiles, two or three workgroups per CU (gemm_nt_ln.hip).
 */
typedef struct vr_ln_epilogue {
    int32_t mode;
    float eps;               /* mode 0 */
    const float* w;          /* LayerNorm weight [N] */
    const float* b;          /* LayerNorm bias [N] (mode 0) */
    const int32_t* keep;     /* [batch] kept prefix of the LayerNorm, NULL = all N channels */
    void* y;                 /* mode 0 out: bf16 [M, N] */
    float* mean;             /* mode 0 out / mode 1 in: [M] */
    float* rstd;
    const float* x;          /* mode 1: the LayerNorm's input saved by the forward, fp32 [M, ldc] */
    float* dw;               /* mode 1: fp32 [max(grad_copies,1)][N], accumulated with atomics (see vr_ln_bwd) */
    float* db;
    void* gt_out;            /* mode 1, optional: bf16 [M, ldc] */
    const float* gt_scale;   /* [batch] or NULL */
    const int32_t* gt_keep;  /* [batch] or NULL */
    int32_t grad_copies;     /* mode 1: rows of partial sums behind dw / db, 0 or 1 = accumulate into dw / db themselves */
} vr_ln_epilogue;
int vr_gemm_ln(const vr_gemm_args* args, const vr_ln_epilogue* ln, vr_stream_t stream);
int vr_gemm_ln_supported(int32_t N);

/*
 * vr_gemm_ln_fold: mode 0 of vr_gemm_ln for widths where a row spans several tiles (N up to 2048; the Linear + LayerNorm pairs of
 * stages 2 and 3: nets/supernet_blocks.py:214-253 followed by nets/masked_layer_norm.py:113-125) --
 *   C = resid + scale[s] * mask_{keep_n}(A B^T + bias)   (fp32, exactly vr_gemm),   (y, mean, rstd) = MaskedLayerNorm(C; w, b, keep, eps)
 * in ONE launch of the tiled lean-loop kernel: every 64 x 128 tile stores its part of C write-through and takes the ticket of its row
 * block; the workgroup that holds a block's last ticket runs vr_ln_fwd's row routine on the block's rows (same arithmetic: results
 * equal vr_gemm followed by vr_ln_fwd up to nothing -- the same fp32 operations in the same order per row).
 * bf16 operands, fp32 C with bias and residual, ldc == N, N % 4 == 0, un-mapped output rows, args->ws >= 16 KB with zeroed tickets (the
 * kernels leave them at zero; never shared by launches that may run concurrently).  VR_EUNSUPPORTED (nothing launched) otherwise.
 */
int vr_gemm_ln_fold(const vr_gemm_args* args, const vr_ln_epilogue* ln, vr_stream_t stream);

/* fp32 -> bf16 (round to nearest even), n elements.  Replaces autocast's per-op weight casts (engine.py:112). */
int vr_cast_f32_bf16(const float* src, void* dst, int64_t n, vr_stream_t stream);
/* fp32 -> fp16 (round to nearest even, overflow to +-inf, NaN kept: torch's .half()), n elements -- the weight shadow of the fp16
 * evaluation mode. */
int vr_cast_f32_f16(const float* src, void* dst, int64_t n, vr_stream_t stream);

/*
 * Transposed bf16 shadows of a batch of fp32 matrices in one launch: for every descriptor d,
 *   dst[d.dst_off + c * d.ld_dst + r] = bf16(src[d.src_off + r * d.cols + c])   r < rows, c < cols
 * (offsets in elements; ld_dst >= rows; columns rows..ld_dst of dst are not written -- keep them zero).
 * The data-gradient GEMM of a Linear (autograd of F.linear, nets/supernet_blocks.py:41,110) then reads W^T K-contiguous
 * like the forward reads W.  descs is a DEVICE array of n descriptors; max_tiles = max over d of
 * ceil(rows/64) * ceil(cols/64).
 */
typedef struct vr_tr_desc {
    int64_t src_off;
    int64_t dst_off;
    int32_t rows;
    int32_t cols;
    int32_t ld_dst;
    int32_t reserved;
} vr_tr_desc;
int vr_cast_transpose_batch(const float* src, void* dst, const vr_tr_desc* descs, int32_t n, int32_t max_tiles,
                            vr_stream_t stream);

/*
 * AdamW over the flat fp32 parameter arena (timm create_optimizer -> torch.optim.AdamW, main.py:385; decoupled weight decay,
 * bias-corrected moments), one pass, fused with: the bf16 shadow of the updated parameters (NULL to skip), gradient scaling
 * (grad_scale, e.g. 1/world after a sum all-reduce) and the ModelEmaV2 update ema = d*ema + (1-d)*p (main.py:357-363;
 * NULL to skip).  Hyper-parameters come per GROUP: group_of_8[i] (device, one byte per 8 consecutive elements; arena
 * parameters start at multiples of 8) selects groups[...]; 255 = elements that are not updated (padding, frozen).
 *   p *= 1 - lr*wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/bias_c1 * m / (sqrt(v)/sqrt_bias_c2 + eps)
 * with bias_c1 = 1 - b1^t, sqrt_bias_c2 = sqrt(1 - b2^t) computed by the caller for step t.  n % 8 == 0.
 * The EMA's 1-d is taken on the fp32 d (weights sum to exactly 1); ModelEmaV2 rounds the double 1-d: 1.3e-4 apart at d = 0.99996.
 */
#define VR_ADAMW_MAX_GROUPS 16
typedef struct vr_adamw_group {
    float lr, beta1, beta2, eps, weight_decay, bias_c1, sqrt_bias_c2, grad_scale;
} vr_adamw_group;
int vr_adamw_flat(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                  const uint8_t* group_of_8, const vr_adamw_group* groups, int32_t n_groups, int64_t n,
                  vr_stream_t stream);
/* Same pass with `groups_dev` in DEVICE memory (read by the kernel at run time): a launch captured into a hipGraph then follows the
 * schedule -- the caller rewrites the n_groups structs before every replay.  All array arguments may point into the middle of
 * the arena (a range of it, offsets multiples of 8 elements; group_of_8 advanced by offset / 8).  A group whose bias_c1 is 0
 * (never the case for a real step) is skipped: an all-zero block turns a captured launch into a no-op for that replay. */
int vr_adamw_flat_dev(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                      const uint8_t* group_of_8, const vr_adamw_group* groups_dev, int32_t n_groups, int64_t n,
                      vr_stream_t stream);
/* ... launched with at most max_blocks workgroups (0: the default grid): the update of a finished arena range that runs beside the
 * rest of the backward on the weight gradients' stream (round 4). */
int vr_adamw_flat_dev_capped(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                             const uint8_t* group_of_8, const vr_adamw_group* groups_dev, int32_t n_groups, int64_t n,
                             int32_t max_blocks, vr_stream_t stream);

/*
 * Gradient-norm clipping on the device (torch.nn.utils.clip_grad_norm_, the reference's `--clip-grad`: loss_scaler(...,
 * clip_grad=max_norm), engine.py:178-180), in front of the AdamW pass and capturable into the same hipGraph:
 *   vr_grad_sumsq (one launch per finished arena range)  ->  vr_clip_finish  ->  vr_adamw_flat_clip
 * Stream order is the only synchronisation between the three.  vr_clip_state lives in DEVICE memory: the caller writes max_norm
 * (+inf: measure only) and grad_scale (the factor AdamW applies to every gradient) before a step; vr_clip_finish writes the rest:
 *   norm = grad_scale * sqrt(sum of squares)          the norm of the gradient the optimizer uses, before clipping
 *   coef = min(1, max_norm / (norm + 1e-6))           torch's formula
 *   skip = 1 if norm is inf or NaN (coef is 0 then), skipped += 1 in that case (a running count the caller zeroes once).
 */
typedef struct vr_clip_state {
    float max_norm, grad_scale;   /* in  */
    float norm, coef;             /* out */
    int32_t skip, skipped;        /* out */
    int32_t reserved[2];
} vr_clip_state;
/* Sum of g[i]^2 over the elements of [0, n) whose group byte is not 255 (g, group_of_8 as for vr_adamw_flat_dev: a range of the
 * arena, group_of_8 advanced by offset / 8; n % 8 == 0).  Launches exactly n_partials workgroups of 256 threads; workgroup b writes
 * partials[b] (plain store, 0 if it had no work), so nothing needs zeroing and equal inputs give equal bits.  At most
 * min(n_partials, max_blocks if > 0, ceil(n / 2048)) workgroups share the range (grid-stride, 8 elements per thread and trip, eight
 * independent fp32 accumulators per thread): choose n_partials so that n / (2048 * n_partials) stays <= 256 trips.  Several
 * launches may fill disjoint slices of one partials buffer. */
int vr_grad_sumsq(const float* g, const uint8_t* group_of_8, int64_t n, float* partials, int32_t n_partials,
                  int32_t max_blocks, vr_stream_t stream);
/* One workgroup: sums partials[0 .. n_partials) in double precision and fills the output half of *state (see above). */
int vr_clip_finish(const float* partials, int32_t n_partials, vr_clip_state* state, vr_stream_t stream);
/* Gated forms for gradient accumulation inside ONE captured graph: `gate` points at an int32 in device memory that the host rewrites
 * before each replay.  Gate 0: the launch returns at once, uniformly over the grid -- vr_grad_sumsq_gated leaves its slice of the
 * partial sums untouched, vr_clip_finish_gated every field of *state (skipped included).  Gate != 0: the ungated entry point's result,
 * bit for bit. */
int vr_grad_sumsq_gated(const float* g, const uint8_t* group_of_8, int64_t n, float* partials, int32_t n_partials,
                        int32_t max_blocks, const int32_t* gate, vr_stream_t stream);
int vr_clip_finish_gated(const float* partials, int32_t n_partials, vr_clip_state* state, const int32_t* gate, vr_stream_t stream);
/* vr_adamw_flat (groups_on_device == 0: `groups` in host memory) or vr_adamw_flat_dev_capped (!= 0: in device memory) with the
 * gradient g * grad_scale * clip->coef; if clip->skip is set the launch writes nothing: parameters, both moments, EMA and shadow
 * stay as they were.  max_blocks as for vr_adamw_flat_dev_capped (0: the default grid). */
int vr_adamw_flat_clip(float* p, const float* g, float* m, float* v, void* shadow, float* ema, float ema_decay,
                       const uint8_t* group_of_8, const vr_adamw_group* groups, int32_t groups_on_device, int32_t n_groups,
                       int64_t n, const vr_clip_state* clip, int32_t max_blocks, vr_stream_t stream);


/*
 * Masked LayerNorm forward (nets/masked_layer_norm.py:23-50,113-125).  x fp32 [M,C] -> y (dtype) [M,C];
 * mean/rstd fp32 [M] saved for backward.  keep NULL -> plain LayerNorm (F.layer_norm path :118-122).
 */
int vr_ln_fwd(const float* x, const float* w, const float* b, void* y, float* mean, float* rstd,
              const int32_t* keep, int32_t M, int32_t C, int32_t rows_per_sample, float eps,
              int32_t out_dtype, vr_stream_t stream);

/*
 * Masked LayerNorm backward (nets/masked_layer_norm.py:55-88).  dx_out = (dx_in ? dx_in : 0) + dLN/dx;
 * dw/db (fp32 [C]) are accumulated with atomics (caller zeroes them).  dy has dtype `dy_dtype`.
 * grad_copies > 1: dw and db are [grad_copies][C] rows of partial sums, workgroup i adds into row i % grad_copies (hundreds
 *   of workgroups hitting the same 2C addresses cost a third of the kernel); vr_ln_grad_reduce folds the rows into the
 *   parameter gradients afterwards.
 * gt_out (optional, dtype `dy_dtype`, [M,C]): the gradient entering the NEXT backward branch, written in the same pass --
 *   gt_out[m,c] = c < gt_keep[s] ? dx_out[m,c] * gt_scale[s] : 0   (s = m / rows_per_sample; NULL scale = 1, NULL keep = C)
 * i.e. what vr_scale_mask_cast would produce from dx_out (DropPath nets/drop.py:11-26 + ChannelDrop mask backward).
 */
int vr_ln_bwd(const void* dy, const float* x, const float* w, const float* mean, const float* rstd,
              const int32_t* keep, const float* dx_in, float* dx_out, float* dw, float* db,
              void* gt_out, const float* gt_scale, const int32_t* gt_keep,
              int32_t M, int32_t C, int32_t rows_per_sample, int32_t dy_dtype, int32_t grad_copies, vr_stream_t stream);

/*
 * vr_ln_bwd of the LayerNorm of a spatial-reduction block (nets/vit_sr_supernet.py:114-172), bf16, reading dy and dx_in where the
 * block's backward already holds them instead of from tensors written by vr_sr_col2im / vr_sr_resid_bwd.  The M = B * (T + g*g)
 * rows are those of the block's input (T = num_tokens leading token rows per sample, then the g x g patch rows):
 *   patch row (ih, iw): dy = bf16(sum of the taps (kh, kw) of dcol [B * (g/2)^2, 9 C] that vr_sr_col2im sums, in its order, in fp32)
 *   token row t:        dy = dy_tok[b * T + t]                     (bf16 [B * T, C], the token Linear's data gradient)
 *   dx_in = f * gout[parent row][c]; gout fp32 [B, T + (g/2)^2, Cout], Cout >= C; the parent of a patch row is the pooled row
 *           T + (ih/2) * (g/2) + iw/2 with f = 1/4, that of token row t is row t with f = 1  (what vr_sr_resid_bwd writes)
 * Every output (dx_out, dw / db with grad_copies, gt_out) is bit for bit vr_ln_bwd's on those tensors.  C % 8 == 0, Cout % 4 == 0.
 */
int vr_ln_bwd_sr(const void* dcol, const void* dy_tok, const float* gout, const float* x, const float* w, const float* mean,
                 const float* rstd, const int32_t* keep, float* dx_out, float* dw, float* db,
                 void* gt_out, const float* gt_scale, const int32_t* gt_keep,
                 int32_t B, int32_t g, int32_t C, int32_t Cout, int32_t num_tokens, int32_t grad_copies, vr_stream_t stream);

/*
 * Fold the partial rows written by vr_ln_bwd / vr_gemm_ln (mode 1) with grad_copies = `copies` into the LayerNorm parameter
 * gradients: dw[c] += sum_k part_w[k][c], db[c] += sum_k part_b[k][c]; the partial rows are zero again afterwards (the
 * caller allocates them zero-filled once).  One launch per 32 slots.
 */
typedef struct vr_ln_grad_slot {
    float* part_w;           /* [copies][C] */
    float* part_b;           /* [copies][C] */
    float* dw;               /* [C] */
    float* db;               /* [C] */
    int32_t C;
    int32_t reserved;
} vr_ln_grad_slot;
int vr_ln_grad_reduce(const vr_ln_grad_slot* slots, int32_t count, int32_t copies, vr_stream_t stream);

/*
 * Multi-head self-attention core (nets/supernet_blocks.py:105-109): qkv [B,N,3,H,D] -> o [B,N,H*D],
 * lse fp32 [B,H,N].  Heads h >= keep_hd[b]/D are written as zeros (Attention's ChannelDrop, :111-112).
 */
int vr_attn_fwd(const void* qkv, void* o, float* lse, const int32_t* keep_hd, int32_t B, int32_t N,
                int32_t H, int32_t D, float scale, int32_t dtype, vr_stream_t stream);
int vr_attn_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta /* [B,H,N] scratch */,
                void* dqkv, const int32_t* keep_hd, int32_t B, int32_t N, int32_t H, int32_t D, float scale,
                int32_t dtype, vr_stream_t stream);

/*
 * Soft-target cross entropy, forward + gradient in one pass (timm SoftTargetCrossEntropy as used by
 * engine.py:153-157): loss_rows[r] = sum_k -t[r,k] * log_softmax(x[r])[k];
 * dlogits[r,k] = gscale * (softmax(x[r])[k] * sum_k t[r,k] - t[r,k]).
 */
int vr_softce(const float* logits, const float* target, float* loss_rows, float* dlogits, int32_t R,
              int32_t K, float gscale, vr_stream_t stream);

/*
 * The loss step of the training loop in one pass (engine.py:153-157 with timm's SoftTargetCrossEntropy): row r of `logits`
 * [R, K] belongs to internal sample s = r / rows_per_sample and is scored against target row
 * (sample_map ? sample_map[s] : s) * rows_per_sample + r % rows_per_sample  (the model runs a batch grouped by architecture,
 * targets stay in the caller's order);  *loss_acc += loss_scale * loss_row (atomics; caller zeroes it);
 * dlogits[r, k] = gscale * (softmax(x[r])[k] * sum_k t[.,k] - t[.,k]) in `grad_dtype` with row pitch ld_grad >= K, columns
 * K..ld_grad-1 zeroed -- exactly what the head's backward GEMMs read.
 */
int vr_softce_train(const float* logits, const float* target, const int64_t* sample_map, int32_t rows_per_sample,
                    float* loss_acc, void* dlogits, int32_t ld_grad, int32_t grad_dtype, int32_t R, int32_t K,
                    float gscale, float loss_scale, vr_stream_t stream);

/*
 * Evaluation metrics of one batch, accumulated on the device (engine.py:213-238: CrossEntropyLoss + timm accuracy(topk=(1, 5)) of the
 * class logits and, for two-token models, of the distillation logits and of softmax(logits) + softmax(logits2)).  logits / logits2:
 * fp32 [R, K] with row pitch ld >= K; labels: int64 [R].  Per row CE = logsumexp(x) - x[y] in fp32, summed in double;
 * rank = #{k : v[k] > v[y]} + #{k < y : v[k] == v[y]}, top1 = rank < 1, top5 = rank < min(5, K): exact comparisons on the raw
 * logits (top1 is argmax(...) == y, ties to the lowest index); the joint head ranks v = exp(x - lse) + exp(x2 - lse2) in fp32.
 * A row whose label lies outside [0, K) or that holds a NaN logit is a miss everywhere and makes loss_sum NaN; it reads nothing out
 * of range.  One workgroup per call, no floating-point atomics: equal inputs and equal state give equal bits.  Calls on one state
 * are ordered by the stream.  16-byte loads when ld % 4 == 0 and both logit pointers are 16-byte aligned.
 * VR_EINVAL: R <= 0, K <= 0, ld < K or a NULL logits / labels / state; VR_EALIGN: state or labels not 8-byte, logits not 4-byte aligned.
 */
typedef struct vr_eval_state {   /* device memory; the caller zeroes it once per evaluation */
    double  loss_sum;            /* += mean over this call's R rows of CE(logits[r], labels[r]) */
    int64_t calls, rows;         /* += 1, += R */
    int64_t top1, top5;          /* hits of `logits` */
    int64_t dst_top1, dst_top5;  /* hits of `logits2`            (untouched when logits2 == NULL) */
    int64_t jnt_top1, jnt_top5;  /* hits of softmax(logits) + softmax(logits2) (likewise)         */
    int64_t reserved;
} vr_eval_state;
int vr_eval_metrics(const float* logits, const float* logits2 /* nullable */, const int64_t* labels,
                    int32_t R, int32_t K, int32_t ld, vr_eval_state* state, vr_stream_t stream);

/* out[n] += sum_m in[map(m), n]  (bias gradients; atomics, caller zeroes out).  in: dtype [*, ld]. */
int vr_colsum(const void* in, float* out, int32_t M, int32_t N, int32_t ld, int32_t dtype, vr_rowmap map, vr_stream_t stream);

/*
 * Gradient entering a masked / drop-path'd residual branch (autograd of supernet_blocks.py:243-253 and
 * drop.py:24-25): out[m,c] = dtype(in[m,c] * scale[sample]) for c < keep[sample], else 0.  in fp32 [M,C].
 */
int vr_scale_mask_cast(const float* in, void* out, const float* scale, const int32_t* keep, int32_t M, int32_t C,
                       int32_t rows_per_sample, int32_t out_dtype, vr_stream_t stream);

/*
 * SwitchTokenMix (token_mixup.py:39-162), device half: the caller has drawn, with the reference's generators and order,
 * partner[b] (global sample index each sample is mixed with: the two torch.randperm of :104 and :126 offset into their half),
 * the patch box [y0,y1) x [x0,x1) in units of the patch_len x patch_len grid, lam_patch = 1 - box/grid, lam_img ~ Beta(.8,.8)
 * (each lam and 1 - lam rounded to fp32 from the double, as torch does for `tensor * python_float`), and the smoothed
 * one-hot values on/off (:22-23).  Rows [0, half): out = partner's pixels inside the box; targets = y*lam_p + y[partner]*(1-lam_p);
 * patch_targets[b, (i,j)] = y[partner] inside the box, y outside.  Rows [half, B): out = x*lam_i + x[partner]*(1-lam_i);
 * targets likewise; every patch target = the mixed target.  samples/out fp32 [B,C,H,W] (out != samples: the reference's
 * in-place update reads a gathered COPY), labels int64 [B], targets fp32 [B,K], patch_targets fp32 [B, patch_len^2, K].
 * Bit-exact with the reference (separately rounded products, then one add).
 */
int vr_token_mix(const float* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                 float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes, int32_t patch_len,
                 int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch, float oml_patch,
                 float lam_img, float oml_img, float on_value, float off_value, vr_stream_t stream);

/*
 * The uint8 input side (the reference's datasets.build_dataloader: timm fast_collate + PrefetchLoader -- uint8 NCHW batches,
 * normalised on the GPU by `input.float().sub_(mean).div_(std)` with mean / std = the 0..1 constants * 255).
 *   n(u, c) = (float(u) - mean[c]) / std[c], a correctly rounded IEEE division (no reciprocal): bit-identical with that
 *   statement on the CPU.  mean / std: HOST pointers to C floats, copied into the kernel arguments (no device buffer); C <= 4.
 * vr_normalize_u8:  out[b,c,y,x] = n(in[b,c,y,x], c); in uint8, out fp32, both contiguous [B,C,H,W].
 * vr_token_mix_u8:  vr_token_mix on uint8 samples -- bit-identical with vr_normalize_u8 followed by vr_token_mix (the box takes
 *   n(partner pixel), the image-level half mixes n(own) and n(partner) with separately rounded products), same targets and patch
 *   targets, every other argument as vr_token_mix.  One pass: each uint8 element is read once, the partner only where it is used.
 * Both: W % 4 == 0 (else VR_EUNSUPPORTED); in 4-byte and out 16-byte aligned (else VR_EALIGN); a lane takes 16 pixels when
 * W % 16 == 0 and in is 16-byte aligned, 4 otherwise.  Arguments are validated before anything is launched.
 */
int vr_normalize_u8(const uint8_t* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mean,
                    const float* std, vr_stream_t stream);
int vr_token_mix_u8(const uint8_t* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                    float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes, int32_t patch_len,
                    int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch, float oml_patch,
                    float lam_img, float oml_img, float on_value, float off_value, const float* mean, const float* std,
                    vr_stream_t stream);

/*
 * timm's Mixup / CutMix (timm/data/mixup.py; the reference's `mixup_fn`, main.py:308-314), device half.  Sample i is mixed with
 * sample j = B-1-i (timm's x.flip(0)) by params[i], a DEVICE array of B entries the host has drawn (vitres/mixup.py: timm's batch,
 * elem and pair modes all come down to one table):
 *   cutmix != 0             out[i] = x[j] inside the PIXEL box [y0,y1) x [x0,x1) (aligned to nothing, may be empty), x[i] outside;
 *                           copies, no arithmetic; the partner is read only by lanes that intersect the box
 *   cutmix == 0, lam != 1   out[i] = fl(fl(x[i] * lam) + fl(x[j] * oml))      (no FMA; lam and oml rounded by the host)
 *   cutmix == 0, lam == 1   out[i] = x[i], copied (timm skips these samples; x * 1 + xj * 0 would turn -0.0 into +0.0 and let a
 *                           non-finite partner through); the partner is not read.  (lam == 1 as timm compares it, on its own
 *                           double: a lam just below 1 that the host rounded to 1.f comes with oml != 0 and is blended)
 *   always                  targets[i,c] = fl(fl(y_i(c) * lam) + fl(y_j(c) * oml)), y_s(c) = on_value if c == labels[s] else off_value
 * samples / out contiguous [B,C,H,W], out != samples; labels int64 [B]; targets fp32 [B,num_classes].
 * vr_mixup_u8: uint8 samples, bit-identical with vr_normalize_u8 followed by vr_mixup (own / partner chosen on the bytes, the blend
 *   normalises both); each byte is read once; mean / std and the lane width as vr_normalize_u8.
 * VR_EINVAL: a null pointer or a non-positive size.  VR_EUNSUPPORTED: W % 4, odd B, samples == out, C > 4 (u8).  VR_EALIGN: samples
 * (fp32) or out not 16-byte, uint8 samples or params not 4-byte aligned.  Checked before anything is launched.  The boxes live in
 * device memory: the caller guarantees 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W (vitres.kernels.mixup checks its host copy); a
 * box outside the image addresses nothing outside the buffers, it only selects pixels.
 */
typedef struct vr_mixup_param {
    float lam, oml;
    int32_t y0, y1, x0, x1;
    int32_t cutmix;
    int32_t pad;
} vr_mixup_param;   /* 32 bytes */

int vr_mixup(const float* samples, float* out, const int64_t* labels, float* targets, const vr_mixup_param* params, int32_t B,
             int32_t C, int32_t H, int32_t W, int32_t num_classes, float on_value, float off_value, vr_stream_t stream);
int vr_mixup_u8(const uint8_t* samples, float* out, const int64_t* labels, float* targets, const vr_mixup_param* params, int32_t B,
                int32_t C, int32_t H, int32_t W, int32_t num_classes, float on_value, float off_value, const float* mean,
                const float* std, vr_stream_t stream);

/*
 * timm's RandomErasing (timm/data/random_erasing.py; the reference's --reprob 0.25 --remode pixel --recount 1, applied per sample
 * to the NORMALISED image before collation and therefore before any mix), device half.  The host draws the rectangles
 * (vitres/random_erasing.py: timm's order on Python's `random`); the device fills them.
 *   rects   a DEVICE table [B][R] of vr_erase_rect, 1 <= R <= 4: sample b erases the pixels [y0,y1) x [x0,x1) of every channel for
 *           each of its R rectangles.  y0 == y1 is the empty rectangle.  Where rectangles overlap the LATER one wins (this shows
 *           only in 'rand').  The caller guarantees 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W (vitres.kernels checks its host
 *           copy); the kernels only ever COMPARE pixel coordinates with a rectangle, so one outside the image selects pixels
 *           and addresses nothing outside the buffers.
 *   mode    VR_ERASE_CONST: +0.0.  VR_ERASE_RAND: one N(0,1) value per channel per rectangle.  VR_ERASE_PIXEL: N(0,1) per element.
 * The noise contract -- the value at a pixel is a pure function of (seed, call, b, c, y, x, mode, and the rectangle index for
 * 'rand'); it does not depend on the lane width, the grid, pointer alignment or the entry point that produced it:
 *   (r0, r1, r2, r3) = Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85),
 *       key     = (seed & 0xffffffff, seed >> 32)
 *       counter = (w, b + (domain << 24), call & 0xffffffff, call >> 32)          b < 2^24
 *       domain 0 ('pixel'): w = q = ((c * H + y) * W + x) / 4, the index of the aligned 4-pixel quad within the sample
 *       domain 1 ('rand'):  w = the rectangle's index in the sample's row of the table
 *   two Box-Muller pairs, (r0, r1) -> (z0, z1) and (r2, r3) -> (z2, z3), in fp32:
 *       u1 = ((r >> 8) + 1) * 2^-24   in (0, 1]        u2 = (r' >> 8) * 2^-24   in [0, 1)          (both exact)
 *       rad = sqrtf(-2 * logf(u1))    ang = fl(0x1.921fb6p+2f * u2)    z = fl(rad * cosf(ang)),  z' = fl(rad * sinf(ang))
 *     with the accurate device functions (no fast-math forms), every product rounded on its own.  |z| <= sqrt(48 ln 2) < 5.77.
 *   domain 0: z0..z3 are pixels x .. x+3 of the quad.  domain 1: z0..z3 are the colours of channels 0..3.
 *   `call` is a 64-bit counter the host advances once per batch; `seed` names the stream.
 * vr_random_erase: in place on a normalised fp32 batch [B,C,H,W]; only quads that meet a rectangle are read or written.
 * vr_normalize_u8_erase, vr_token_mix_u8_erase, vr_mixup_u8_erase: the uint8 entries above with the erase folded into the same
 *   pass, bit-identical with vr_normalize_u8 -> vr_random_erase (-> vr_token_mix / vr_mixup): own pixels are erased under the own
 *   sample's rectangles, a pixel taken from the partner carries the PARTNER's erase (its rectangles, its b), blends mix the two
 *   erased values as before, vr_mixup's lam == 1 copy still carries the sample's own erase; targets are unaffected.  Every byte is
 *   still read once and the partner only where it is used; only lanes whose pixels meet a rectangle of a sample they read run
 *   Philox.  `erase` is a HOST struct, copied into the kernel arguments.
 * As the entries they extend, and: VR_EINVAL a null erase / rects, R outside 1..4, an unknown mode; VR_EUNSUPPORTED B > 2^24,
 * C > 4, W % 4; VR_EALIGN x not 16-byte or rects not 4-byte aligned.  Checked before anything is launched.
 */
enum { VR_ERASE_CONST = 0, VR_ERASE_RAND = 1, VR_ERASE_PIXEL = 2 };

typedef struct vr_erase_rect {
    int32_t y0, y1, x0, x1;
} vr_erase_rect;    /* 16 bytes */

typedef struct vr_erase_args {
    const vr_erase_rect* rects;
    int32_t R, mode;
    uint64_t seed, call;
} vr_erase_args;    /* 32 bytes */

int vr_random_erase(float* x, int32_t B, int32_t C, int32_t H, int32_t W, const vr_erase_rect* rects, int32_t R, int32_t mode,
                    uint64_t seed, uint64_t call, vr_stream_t stream);
int vr_normalize_u8_erase(const uint8_t* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, const float* mean,
                          const float* std, const vr_erase_args* erase, vr_stream_t stream);
int vr_token_mix_u8_erase(const uint8_t* samples, float* out, const int64_t* labels, const int64_t* partner, float* targets,
                          float* patch_targets, int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes, int32_t patch_len,
                          int32_t half, int32_t y0, int32_t y1, int32_t x0, int32_t x1, float lam_patch, float oml_patch,
                          float lam_img, float oml_img, float on_value, float off_value, const float* mean, const float* std,
                          const vr_erase_args* erase, vr_stream_t stream);
int vr_mixup_u8_erase(const uint8_t* samples, float* out, const int64_t* labels, float* targets, const vr_mixup_param* params,
                      int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_classes, float on_value, float off_value,
                      const float* mean, const float* std, const vr_erase_args* erase, vr_stream_t stream);

/*
 * The geometric head of the input chain on the device: crop, resize, window and mirror of a uint8 batch in one pass (timm's
 * RandomResizedCropAndInterpolation + RandomHorizontalFlip in training, Resize + CenterCrop in evaluation; datasets.py:117-119 hands
 * both to timm's create_transform).  The loader only decodes and pads its images into a uint8 canvas [B,C,Hs,Ws]; the output is the
 * uint8 [B,C,So_h,So_w] batch vr_normalize_u8 / vr_token_mix_u8 / vr_mixup_u8 take.  Per sample and channel, bit for bit (PIL 12):
 *     PIL.Image.crop((x0, y0, x0+w, y0+h)).resize((ow, oh), filter).crop((wx, wy, wx+So_w, wy+So_h)) [.transpose(FLIP_LEFT_RIGHT) if flip]
 * i.e. PIL's 8-bit resample: a horizontal pass over the source rows the vertical pass touches, rounded and clipped to uint8, then
 * the vertical pass.  Per axis, in double precision and one rounding per operator (no fused multiply-add), in = the crop's size,
 * out = ow / oh:  scale = in / out, fs = max(scale, 1), support = S_f * fs (S_f = 1 bilinear, 2 bicubic), ss = 1 / fs; output index
 * xx has center = (xx + 0.5) * scale, taps x in [max(0, (int)(center - support + 0.5)), min(in, (int)(center + support + 0.5))) with
 * weight f((x - center + 0.5) * ss) divided by the taps' sum; f = 1 - |t| (|t| < 1), or the a = -0.5 cubic ((a+2)|t| - (a+3)) t^2 + 1
 * (|t| < 1), (((|t| - 5)|t| + 8)|t| - 4) a (|t| < 2); fixed point k = (int)(w * 2^22 +- 0.5), the sign following w; int32 sums that
 * start at 2^21; result clamp(sum >> 22, 0, 255).  The supports are clipped to the CROP, not to the canvas (torchvision's
 * resized_crop).  Only the window's pixels and the source rows they need are computed.
 *   random-resized crop: ow = oh = S, wx = wy = 0;   evaluation: box = the image, (ow, oh) = the resized size, window = the centre crop.
 * `boxes` is a DEVICE array read at run time: a captured launch follows boxes rewritten in place, and the entry point does no
 * per-batch host work.  The coefficients are computed inside the kernel (fp64), so vr_resample_ws_bytes is 0 and workspace may be NULL.
 * One workgroup per (sample, band of output rows); the band height (vr_resample_band_rows) is the tallest, up to 32 rows, whose LDS
 * image -- coefficient tables, the uint8 intermediate of the band's source rows, one staged source row per wave -- stays within 64 KiB
 * for the launch's worst possible scale, Hs / So_h and Ws / So_w (a box inside the canvas and a window inside (ow, oh) cannot
 * exceed them).  VR_EUNSUPPORTED when not even a one-row band fits, when So_w % 4 or Ws % 4, or B > 65535; VR_EINVAL: a null pointer,
 * src == out, a non-positive size, C outside 1..4, filter not 2 / 3; VR_EALIGN: src, out or boxes not 4-byte aligned.  The caller
 * guarantees w, h >= 1, the box inside Hs x Ws and the window inside (ow, oh) (vitres.kernels.resample_u8 checks its host copy); the
 * kernel clamps a box that breaks this into range, so it selects other pixels and addresses nothing outside the buffers.
 */
typedef struct vr_resample_box {
    int32_t x0, y0, w, h;      /* source box inside this sample's canvas (the crop); w, h >= 1                       */
    int32_t ow, oh;            /* size of the VIRTUAL resized image the box is resampled to                          */
    int32_t wx, wy;            /* origin of the output window inside that virtual image (0,0 for a plain crop-resize) */
    int32_t flip;              /* != 0: the written window is mirrored left-right                                     */
    int32_t reserved[3];
} vr_resample_box;             /* 48 bytes */
int vr_resample_u8(const uint8_t* src /* [B,C,Hs,Ws] */, const vr_resample_box* boxes /* device, [B] */,
                   uint8_t* out /* [B,C,So_h,So_w] */, int32_t B, int32_t C, int32_t Hs, int32_t Ws,
                   int32_t So_h, int32_t So_w, int32_t filter /* 2 bilinear, 3 bicubic: PIL's numbers */,
                   void* workspace, size_t ws_bytes, vr_stream_t stream);
size_t vr_resample_ws_bytes(int32_t B, int32_t So_h, int32_t So_w);   /* 0: the kernel needs none */
/* output rows per workgroup of that launch (> 0), or the negative code vr_resample_u8 would return for these dimensions */
int vr_resample_band_rows(int32_t C, int32_t Hs, int32_t Ws, int32_t So_h, int32_t So_w, int32_t filter);

/*
 * RandAugment on the device: the stage between vr_resample_u8 and the normalising / mixing passes (timm's create_transform runs
 * crop -> flip -> RandAugment -> ToTensor -> Normalize -> RandomErasing; the recipes train with --aa rand-m9-mstd0.5-inc1).  src and
 * out are uint8 [B,3,H,W]; `ops` holds `layers` records per sample, applied in order, layer k + 1 on layer k's output (its
 * whole-image statistics included).  Eleven op kinds cover timm's fifteen ops; every result is, bit for bit, what PIL 12 makes of
 * the HWC RGB image:
 *   VR_RA_IDENTITY      drawn but not applied; costs nothing beyond getting src into out.
 *   per-channel tables  out = lut[in]:
 *     INVERT            255 - i                                                        (ImageOps.invert)
 *     POSTERIZE         i & ~(2^(8 - iarg) - 1), iarg = bits kept, 0..7                (ImageOps.posterize; 8 is identity)
 *     SOLARIZE          i < iarg ? i : 255 - i, iarg = threshold 0..256                (ImageOps.solarize)
 *     SOLARIZE_ADD      i < 128 ? min(255, i + iarg) : i, iarg = 0..255                (timm's solarize_add)
 *     AUTOCONTRAST      per channel, lo / hi = the histogram's lowest / highest non-empty bin: identity if hi <= lo, else in double
 *                       scale = 255.0 / (hi - lo), offset = -lo * scale, lut[i] = clip((int)(i * scale + offset), 0, 255)
 *                                                                                      (ImageOps.autocontrast, cutoff 0)
 *     EQUALIZE          per channel, step = (pixels - count of the last non-empty bin) / 255 (integers): identity if at most one
 *                       bin is non-empty or step == 0, else n = step / 2; lut[i] = min(255, n / step); n += h[i]
 *                                                                                      (ImageOps.equalize)
 *   blends              Image.blend(degenerate, image, factor) (ImageEnhance.*.enhance) in float32, one rounding per operator:
 *                       t = (float)d + alpha * (float)(x - d), alpha = factor; the byte is (uint8)t when 0 <= alpha <= 1, else 0 if
 *                       t <= 0, 255 if t >= 255, else (uint8)t (truncation).  The degenerate d:
 *     BRIGHTNESS        0
 *     COLOR             L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 in all three channels
 *     CONTRAST          the constant (int)(mean(L) + 0.5), the mean = the integer sum of L over the image / pixels, in double
 *     SHARPNESS         ImageFilter.SMOOTH per channel: (sum of the 3x3 neighbourhood + 4 * centre) / 13 + 0.5 truncated; the
 *                       image's one-pixel border is the source's (there d = x).  PIL sums in float32; an integer sum s leaves
 *                       s / 13 + 0.5 at least 1 / 26 from every integer, so the kernel's exact (2 s + 13) / 26 is the same byte.
 *   AFFINE              Image.transform(size, AFFINE, m, resample = filter, fillcolor = fill), filter 2 (bilinear) or 3 (bicubic)
 *                       PER RECORD, in double, one rounding per operator, left to right: for output pixel (x, y)
 *                       xin = m0 (x + 0.5) + m1 (y + 0.5) + m2, yin likewise from m3..m5; fill where xin < 0, xin >= W, yin < 0 or
 *                       yin >= H; else xin -= 0.5, yin -= 0.5, x0 = floor(xin), dx = xin - x0 (same in y), tap indices clamped
 *                       to the image.  Bilinear: v = a + (b - a) d along x on rows y0, y0 + 1, then along y; (uint8)v.  Bicubic
 *                       over taps x0 - 1 .. x0 + 2: p1 = v2, p2 = -v1 + v3, p3 = 2 (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4,
 *                       v = p1 + d (p2 + d (p3 + d p4)) along x on four rows, then along y; 0 if v <= 0, 255 if v >= 255, else
 *                       (uint8)v.  Rotations, shears and translations differ only in m (vitres/rand_augment.py builds them as
 *                       PIL does).
 * `ops` is a DEVICE array read at run time: a captured launch follows a table rewritten in place, and the entry point does no
 * per-batch host work and no sync.  A record with an unknown op or filter, or iarg out of the ranges above, applies nothing;
 * nothing outside the buffers is addressed whatever the table holds (vitres.kernels.rand_augment_u8 rejects such records on its
 * host copy).  One launch, one workgroup per sample: it walks the sample's applied layers, the last one writing `out` and the ones
 * before alternating between the sample's workspace plane and `out`, a workgroup barrier and a device fence between layers; the
 * histograms and sums live in LDS.  workspace: vr_rand_augment_ws_bytes = B * 3 * H * W when layers > 1, else 0 (NULL allowed);
 * never shared by launches that may run concurrently.  fill_rgb = r | g << 8 | b << 16.
 * VR_EINVAL: a null pointer, src == out, a non-positive size, layers outside 1..4, a workspace that is missing, too small or one of
 * src / out; VR_EUNSUPPORTED: W % 4, B > 65535, 3 * H * W >= 2^31; VR_EALIGN: src, out or workspace not 4-byte, ops not 8-byte
 * aligned.  Checked before anything is launched.
 */
enum {
    VR_RA_IDENTITY = 0, VR_RA_INVERT = 1, VR_RA_POSTERIZE = 2, VR_RA_SOLARIZE = 3, VR_RA_SOLARIZE_ADD = 4, VR_RA_AUTOCONTRAST = 5,
    VR_RA_EQUALIZE = 6, VR_RA_BRIGHTNESS = 7, VR_RA_COLOR = 8, VR_RA_CONTRAST = 9, VR_RA_SHARPNESS = 10, VR_RA_AFFINE = 11
};
typedef struct vr_ra_op {
    int32_t op;                /* VR_RA_*                                                                              */
    int32_t filter;            /* AFFINE: 2 bilinear, 3 bicubic (PIL's numbers)                                        */
    int32_t iarg;              /* POSTERIZE bits, SOLARIZE threshold, SOLARIZE_ADD addend                              */
    float factor;              /* the blend ops' enhancement factor                                                    */
    double m[6];               /* AFFINE: output -> source, as PIL's transform takes it                                */
} vr_ra_op;                    /* 64 bytes */
int vr_rand_augment_u8(const uint8_t* src /* [B,3,H,W] */, const vr_ra_op* ops /* device, [B, layers] */,
                       uint8_t* out /* [B,3,H,W] */, int32_t B, int32_t H, int32_t W, int32_t layers,
                       uint32_t fill_rgb, void* workspace, size_t ws_bytes, vr_stream_t stream);
size_t vr_rand_augment_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t layers);

/*
 * The device half of JPEG decoding.  The host half (libvitres_jpeg.so, include/vitres_jpeg.h) Huffman-decodes every baseline stream
 * of a batch into quantised coefficients; this entry makes of them exactly the canvas batch pad_collate_u8 would have made of
 * PIL's Image.open(f).convert('RGB') of the same files (PIL 12 with libjpeg-turbo): every image top-left in its [3,Hs,Ws] planes,
 * every other byte zero, grayscale streams in all three planes.  The launch writes EVERY byte of the canvas; the caller does not
 * clear it.
 *   blob    the batch's data, `blob_bytes` of it.  kind VR_JPEG_COEF: per component, the blocks of its block-padded plane (bh rows of
 *           bw blocks) in raster order, 64 int16 per block in natural (row-major) order, as vr_jpeg_entropy_decode writes them.
 *           kind VR_JPEG_RAW (files the host decoded some other way): three planes R, G, B of uint8, each bh * 8 rows of bw * 8 bytes.
 *   descs   one record per image (below); off[c] is the component's offset into the blob in units of 16 bytes.
 *   qtabs   uint16 [B,3,64]: the quantisation table of each component in natural order (unused by raw records).
 *   workspace  vr_jpeg_ws_bytes(blob_bytes) = blob_bytes / 2 rounded up to 16: the component sample planes between the two launches
 *           (a sample is one byte where a coefficient was two, so component c of a record lives at off[c] * 8); never shared by
 *           launches that may run concurrently.
 * Arithmetic, all in 32-bit integers that wrap (unsigned operations, arithmetic right shifts), clamped to 0..255 at the end:
 *   dequantise   coefficient * table entry
 *   inverse DCT  libjpeg's jidctint (ISLOW), CONST_BITS 13, PASS1_BITS 2: columns first, descaled by 11 bits, then rows, descaled by
 *                18 bits, each descale adding half and shifting arithmetically; constants 2446 3196 4433 6270 7373 9633 12299
 *                15137 16069 16819 20995 25172; then + 128 and the clamp
 *   chroma       plane size dw = ceil(W / hs), dh = ceil(H / vs); edges replicate within that size, not the block padding.
 *                2x1, dw > 2: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2.
 *                2x2, dw > 2: t = 3 p[r] + p[r-1] for the upper output row of input row r, 3 p[r] + p[r+1] for the lower; then
 *                out[2i] = (3 t[i] + t[i-1] + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4.  dw <= 2: every sample repeated.
 *   colour       with cb, cr minus 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *                B = Y + ((116130 cb + 32768) >> 16)
 * For coefficients no encoder emits (products beyond 16 bits) the pixels are unspecified, the accesses are not.
 * `descs` and `qtabs` are DEVICE arrays read at run time; the entry does no per-batch host work and no sync.  The device checks
 * every record before it reads anything through it: kind 0 / 1; 1 <= width <= min(Ws, 8192), 1 <= height <= min(Hs, 8192); ncomp 1
 * with hs = vs = 1, or ncomp 3 with (hs, vs) one of (1,1) (2,1) (2,2) -- raw: ncomp 3, hs = vs = 1; bw[0] = hs * ceil(width / (8 hs)),
 * bh[0] = vs * ceil(height / (8 vs)), bw[c] = bw[0] / hs and bh[c] = bh[0] / vs for the chroma; off[c] >= 0 and the component's bytes
 * (128 per block, 64 for raw) inside blob_bytes.  A record that fails leaves its image's planes zero and nothing is read for it;
 * no record, valid or not, makes the launches address anything outside the buffers (vitres.kernels.check_jpeg_table rejects such
 * records on the host copy).
 * VR_EINVAL: a null pointer, a non-positive size, a workspace that is missing, too small, or one of blob / canvas; VR_EUNSUPPORTED:
 * Ws % 4, B > 65535, Hs or Ws above 8192 (the sides a record may have: a baseline frame allows 65535, 8192 keeps every index of a
 * plane inside 32 bits with room to spare); VR_EALIGN: blob or workspace not 16-byte, canvas or descs not 4-byte, qtabs not 2-byte
 * aligned.  Checked before anything is launched.
 */
enum { VR_JPEG_COEF = 0, VR_JPEG_RAW = 1 };
typedef struct vr_jpeg_desc {
    int32_t kind;              /* VR_JPEG_COEF / VR_JPEG_RAW                                                           */
    int32_t width, height;
    int32_t ncomp;             /* 1 (grayscale) or 3                                                                   */
    int32_t hs, vs;            /* luma sampling factors (chroma is 1 x 1)                                              */
    int32_t off[3];            /* offset of component c in the blob, units of 16 bytes                                 */
    int32_t bw[3], bh[3];      /* the component's plane in 8 x 8 blocks, padded to whole MCUs                          */
    int32_t reserved;
} vr_jpeg_desc;                /* 64 bytes */
int vr_jpeg_reconstruct_u8(const void* blob, int64_t blob_bytes, const vr_jpeg_desc* descs /* device, [B] */,
                           const uint16_t* qtabs /* device, [B,3,64] */, uint8_t* canvas /* [B,3,Hs,Ws] */, int32_t B, int32_t Hs,
                           int32_t Ws, void* workspace, size_t ws_bytes, vr_stream_t stream);
size_t vr_jpeg_ws_bytes(int64_t blob_bytes);

/*
 * The ragged route through the same two stages: image batches of any size.  The padded entries above take one canvas [B,C,Hs,Ws]
 * whose sides are the batch maxima, so one large photograph costs every sample its memory, its traffic and -- in vr_resample_u8 --
 * the launch itself.  Here every sample has planes of its OWN size in one flat uint8 buffer, placed by a device table:
 *   vr_ragged_plane  off: byte offset of channel 0 in the flat buffer, a multiple of 16; pitch: bytes per row, a multiple of 4 and
 *                    >= the image's width; rows >= the image's height; channel c starts at off + c * rows * pitch.  Columns between
 *                    the width and the pitch are zero.  Nothing requires two samples to share a pitch, and the buffer may have gaps.
 *                    ws_off: vr_resample_ragged_u8 only (below).
 * The device checks a plane record before anything is addressed through it: off >= 0 and off % 16 == 0, 4 <= pitch <= the launch's
 * Ws bound and pitch % 4 == 0, 1 <= rows <= the launch's Hs bound, off + C * rows * pitch <= the declared size of the buffer.
 * vitres.kernels.check_ragged_planes rejects such records -- and planes that overlap -- on the host copy.
 *
 * vr_jpeg_reconstruct_ragged_u8: vr_jpeg_reconstruct_u8 with another destination -- the same blob, records, record checks, raw
 * records, qtabs, arithmetic (the same device code) and workspace rule; Hs and Ws (both <= 8192, Ws % 4 == 0) bound every plane's rows
 * and pitch as they bound every image's sides.  For every image whose plane record passes and holds it (pitch >= width, rows >=
 * height) EVERY byte of its three planes is written, rows * pitch each: the pixels, zero outside the image, zero everywhere if the
 * JPEG record fails its check; grayscale in all three.  Nothing else is written: bytes of dst between planes keep their values, and a
 * sample whose plane record fails, or is too small for its image, has nothing written at all.  No record of either table, valid or
 * not, makes the launches address anything outside blob, dst (dst_bytes) or the workspace.
 * VR_EINVAL: a null pointer, a non-positive size, a workspace that is missing, too small, or one of blob / dst, dst == blob;
 * VR_EUNSUPPORTED: Ws % 4, B > 65535, Hs or Ws above 8192; VR_EALIGN: blob, workspace or dst not 16-byte, planes not 8-byte, descs not
 * 4-byte, qtabs not 2-byte aligned.  Checked before anything is launched.
 *
 * vr_resample_ragged_u8: vr_resample_u8's arithmetic, boxes (the same vr_resample_box table, read on the device), window and mirror
 * semantics and output [B,C,So_h,So_w], bit for bit, from ragged planes of C channels -- with NO limit on the scale: any box with
 * 1 <= w, h <= 8192 inside its own sample's pitch x rows, to any So_h, So_w (So_w % 4 == 0).  Two launches through a global
 * workspace, so that no source row is resampled twice:
 *   horizontal  one workgroup per (sample, block of 32 of the crop's source rows the window's vertical taps touch), all channels:
 *               the horizontal coefficients in LDS a chunk of output columns at a time (a column of the widest box has 8193 taps: one
 *               column then fills the table), row segments staged as aligned dwords, the uint8 intermediate [C][h][So_w] of the sample
 *               written at workspace + ws_off;
 *   vertical    one workgroup per (sample, band of 8 output rows): the band's vertical coefficients in LDS, swept in slices when a
 *               row has more taps than the table holds (h = 8192 to one row: 32769), the intermediate read as dwords, 4 pixels per
 *               lane and tap, the (mirrored) output written.
 * PIL's pass order is followed: Image.resize runs the VERTICAL pass first on an image (here: a crop) with h > 100 w and oh < h, the
 * 8-bit intermediate then being w x oh; such a crop (at most 81 wide) skips the first launch and is done whole by the second
 * (vr_resample_u8 does not do this and differs from PIL for such crops).
 * Hs bounds every plane's rows, Ws every pitch: they size the grids, the check above and -- through the most taps a box inside them
 * can have -- the kernels' LDS, which stays within the 64 KiB a launch gets without raising its limit whatever they are.  workspace: every sample's intermediate is C * h * So_w bytes (h = its box's height) at its record's ws_off, a
 * multiple of 4 the HOST fills so that the intermediates do not overlap; vr_resample_ragged_ws_bytes(C, total_rows, So_w) =
 * C * total_rows * So_w rounded up to 16 is what offsets packed over heights that sum to total_rows need -- the sum of the boxes'
 * heights, or (for tables rewritten under a captured launch) of the planes' rows, which bounds it; never B times the tallest.
 * The kernels clamp every box into its sample's plane, as vr_resample_u8 clamps into the canvas.  A sample whose plane record
 * fails the check above, or whose intermediate does not lie inside ws_bytes, gets zeros in its output and nothing is read for it.
 * `boxes` and `planes` are DEVICE arrays read at run time: a captured launch follows tables rewritten in place.
 * VR_EINVAL: a null pointer, a non-positive size, C outside 1..4, filter not 2 / 3, a workspace that is missing, smaller than
 * vr_resample_ragged_ws_bytes(C, 1, So_w), or one of src / out, src == out; VR_EUNSUPPORTED: So_w % 4, Ws % 4, B > 65535;
 * VR_EALIGN: src or workspace not 16-byte, planes not 8-byte, out or boxes not 4-byte aligned.  Checked before anything is launched.
 */
typedef struct vr_ragged_plane {
    int64_t off;               /* byte offset of channel 0 in the flat buffer, a multiple of 16                        */
    int32_t pitch;             /* bytes per row: a multiple of 4, >= the image's width                                 */
    int32_t rows;              /* rows per channel, >= the image's height                                              */
    int64_t ws_off;            /* vr_resample_ragged_u8: byte offset of the sample's intermediate in the workspace     */
    int32_t reserved[2];
} vr_ragged_plane;             /* 32 bytes */
int vr_jpeg_reconstruct_ragged_u8(const void* blob, int64_t blob_bytes, const vr_jpeg_desc* descs /* device, [B] */,
                                  const uint16_t* qtabs /* device, [B,3,64] */, uint8_t* dst, int64_t dst_bytes,
                                  const vr_ragged_plane* planes /* device, [B] */, int32_t B, int32_t Hs, int32_t Ws,
                                  void* workspace, size_t ws_bytes, vr_stream_t stream);
int vr_resample_ragged_u8(const uint8_t* src, int64_t src_bytes, const vr_ragged_plane* planes /* device, [B] */,
                          const vr_resample_box* boxes /* device, [B] */, uint8_t* out /* [B,C,So_h,So_w] */, int32_t B, int32_t C,
                          int32_t Hs, int32_t Ws, int32_t So_h, int32_t So_w, int32_t filter, void* workspace, size_t ws_bytes,
                          vr_stream_t stream);
size_t vr_resample_ragged_ws_bytes(int32_t C, int64_t total_rows, int32_t So_w);

/*
 * patch_output_type == 'avg' (nets/vit_sr_supernet.py:447-449: patch_features.mean(dim=1) before patch_head):
 * out[b, c] = mean over tokens n in [first, N) of y[b, n, c]; backward writes dy[b, n, c] = dmean[b, c] / (N - first) for those
 * tokens.  All tensors in `dtype`, fp32 accumulation.
 */
int vr_token_mean(const void* y, void* out, int32_t B, int32_t N, int32_t C, int32_t first, int32_t dtype, vr_stream_t stream);
int vr_token_mean_bwd(const void* dmean, void* dy, int32_t B, int32_t N, int32_t C, int32_t first, int32_t dtype,
                      vr_stream_t stream);

/* out[r, c] += sum_b in[b, r, c]   (pos_embed / tokens gradients: sum over the batch; fp32 atomics -- the caller
 * zero-initialises out, as the gradient arena is). */
int vr_batchsum(const float* in, float* out, int32_t B, int64_t inner, vr_stream_t stream);

/*
 * timm PatchEmbed as a GEMM operand (vit_sr_supernet.py:227,234): image fp32 NCHW [B,Cin,H,W] ->
 * col (dtype) [B*gh*gw, ldk] with k = (c, i, j), zero padded up to ldk.
 */
int vr_im2col_patch(const float* img, void* col, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t P,
                    int32_t ldk, int32_t dtype, vr_stream_t stream);
/* The same with output sample b read from image sample_map[b] (NULL: identity): the batch re-ordering of the arch-grouped
 * execution order folded into the gather (one pass over the images instead of index_select + im2col). */
int vr_im2col_patch_map(const float* img, void* col, const int64_t* sample_map, int32_t B, int32_t Cin, int32_t H, int32_t W,
                        int32_t P, int32_t ldk, int32_t dtype, vr_stream_t stream);

/* token rows of the embedding: x[b,t,c] = (tokens[t,c] + pos[t,c]) masked by keep, t < num_tokens (1: class token; 2: class +
 * distillation token of the *_distill_* factories) (vit_sr_supernet.py:399-407) */
int vr_embed_cls(const float* tokens, const float* pos, float* x, const int32_t* keep, int32_t B, int32_t N,
                 int32_t C, int32_t num_tokens, vr_stream_t stream);

/*
 * SpatialReductionPatchEmbedding pieces (nets/vit_sr_supernet.py:114-172), grid g x g -> g/2 x g/2:
 * T = num_tokens leading token rows per sample (1 or 2), then the g*g patch rows:
 *  vr_sr_im2col : y (dtype) [B,T+g*g,C] -> col (dtype) [B*(g/2)^2, 9*C], k = (kh,kw,c), 3x3 stride 2 pad 1
 *  vr_sr_col2im : dcol -> dy rows T.. (gather form, no atomics); token rows left untouched
 *  vr_sr_resid  : out fp32 [B,T+(g/2)^2,Cout] = zero-padded residual (token rows copied; 2x2 avg-pool of patches)
 *  vr_sr_resid_bwd : dx[b,t,:C] (+)= dout[b,t,:C] for t < T; dx[b,T+p,:C] (+)= 0.25*dout[b,T+p/2..]
 */
int vr_sr_im2col(const void* y, void* col, int32_t B, int32_t g, int32_t C, int32_t num_tokens, int32_t dtype, vr_stream_t stream);
int vr_sr_col2im(const void* dcol, void* dy, int32_t B, int32_t g, int32_t C, int32_t num_tokens, int32_t dtype, vr_stream_t stream);
int vr_sr_resid(const float* x, float* out, int32_t B, int32_t g, int32_t Cin, int32_t Cout, int32_t num_tokens, vr_stream_t stream);
int vr_sr_resid_bwd(const float* dout, float* dx, int32_t B, int32_t g, int32_t Cin, int32_t Cout,
                    int32_t accumulate, int32_t num_tokens, vr_stream_t stream);

/*
 * Zero-fill ranges [lo[i], lo[i] + count[i]) (elements) of one fp32 buffer in one launch: optimizer.zero_grad() of the flat
 * gradient arena (reference engine.py:175) minus the spans whose weight gradients are written in store form (vr_gemm atomic == 2).
 */
#define VR_MAX_ZERO_RANGES 24
typedef struct vr_range_list {
    int64_t lo[VR_MAX_ZERO_RANGES];
    int64_t count[VR_MAX_ZERO_RANGES];
    int32_t n;
    int32_t reserved;
} vr_range_list;
int vr_zero_ranges(float* base, const vr_range_list* ranges, vr_stream_t stream);
/* The same behind a gate word (int32, device memory): *gate == 0 leaves the buffer untouched (the first micro-step of an update
 * window clears the gradient arena, the others add to it; one captured graph serves all of them). */
int vr_zero_ranges_gated(float* base, const vr_range_list* ranges, const int32_t* gate, vr_stream_t stream);

/*
 * dst[a * dst_ld + c * B + b] = src[a * src_ld + b * C + c]  (dtype codes as everywhere; pad columns of dst untouched).
 * Replaces the `.permute(0, 2, 3, 1).reshape(...)` / `.permute(0, 3, 1, 2)` copies between the reference's convolution weights
 * [out, in, kh, kw] (nets/patch_conv.py:26-27, vit_sr_supernet.py:96-97) and the [out, (kh, kw, in)] form their GEMMs read, and the
 * row copy of the timm PatchEmbed weight into 16-byte-aligned rows (B = 1).
 */
int vr_relayout(const void* src, void* dst, int32_t A, int32_t B, int32_t C, int64_t src_ld, int64_t dst_ld, int32_t src_dtype,
                int32_t dst_dtype, vr_stream_t stream);
/* dst[a * dst_ld + c * B + b] += src[a * src_ld + b * C + c], fp32 both sides: the same index map, adding -- the gradient writers that
 * go through a temporary (convolution-shaped weight gradients, padded rows) under gradient accumulation.  A = B = 1: dst += src. */
int vr_relayout_add(const float* src, float* dst, int32_t A, int32_t B, int32_t C, int64_t src_ld, int64_t dst_ld, vr_stream_t stream);

/* x[m, c] = 0 for c >= keep[sample(m)]  (ChannelDrop.forward `x * mask`, nets/channel_drop.py:82) */
int vr_mask_rows(float* x, const int32_t* keep, int32_t M, int32_t C, int32_t rows_per_sample, vr_stream_t stream);

/*
 * Convolutional patch embedding (reference nets/patch_conv.py:23-73) as NHWC gathers around vr_gemm.
 *  vr_im2col3x3   : 3x3 / pad 1 window gather -> col [B*Ho*Wo, ld], k = (kh, kw, c).  src_nchw_f32 = 1: src is the fp32
 *                   NCHW image (conv1, any stride, ld >= 9*C zero padded); 0: src is NHWC in `dtype` (stride 1, C % 8 == 0,
 *                   ld == 9*C).
 *  vr_col2im3x3   : its adjoint for the NHWC / stride-1 case (gather form, no atomics).
 *  vr_bn_stats    : sum[c] += sum_r z[r,c], sumsq[c] += sum_r z[r,c]^2  (train-mode BatchNorm2d statistics; caller zeroes).
 *  vr_bn_relu     : out = relu(z * scale[c] + shift[c]) (+ res)          (ConvBnAct.forward :34-38 with folded BN affine).
 *  vr_bn_bwd      : g = da * [bn(z) > 0]; sg[c] += sum g; sgz[c] += sum g*zhat (caller zeroes); then
 *                   dz = scale * (g - sg/R - zhat*sgz/R) (training) or scale * g (eval).  d gamma = sgz, d beta = sg.
 *  z (the pre-BatchNorm convolution output) is fp32 or, with bf16 activations, bf16 (`z_dtype`; what autocast gives the reference's
 *  convolutions): statistics and gradients are accumulated in fp32 either way.
 *  vr_patch_unfold: non-overlapping P x P patches, a NHWC [B, gh*P, gw*P, C] <-> col [B*gh*gw, (i, j, c)] (fold != 0: col -> a).
 */
int vr_im2col3x3(const void* src, void* col, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                 int32_t src_nchw_f32, int32_t ld, int32_t dtype, vr_stream_t stream);
int vr_col2im3x3(const void* dcol, void* dsrc, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, vr_stream_t stream);

/*
 * Direct 3x3 / stride 1 / pad 1 convolution on MFMA (bf16 fast path of patch_conv.py's conv2 / conv3 and, with the weights
 * flipped and transposed by the caller, of their data gradients): a bf16 NHWC [B,H,W,Cin], w bf16 [Cout, (kh,kw,ci)],
 * out [B*H*W, Cout] in out_dtype.  No im2col matrix is materialised.  Cin in {16, 24, 32}, Cout <= 32, Cout % 4 == 0;
 * VR_EUNSUPPORTED otherwise (callers fall back to vr_im2col3x3 + vr_gemm).
 */
int vr_conv3x3(const void* a, const void* w, void* out, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
               int32_t out_dtype, vr_stream_t stream);
/*
 * The same convolution with BatchNorm folded in for evaluation (nets/patch_conv.py:23-73 in eval mode: the caller scales the
 * weights by gamma / sqrt(var + eps) per output channel): out = relu(conv(a, w) + bias[co]) (+ res[pixel, co], bf16).
 */
int vr_conv3x3_bias_relu(const void* a, const void* w, const float* bias, const void* res, void* out, int32_t B, int32_t H,
                         int32_t W, int32_t Cin, int32_t Cout, int32_t out_dtype, vr_stream_t stream);
/* The same with the result written as the patchify operand of the projection behind it ([B*(H/patch)*(W/patch), (i, j, co)], the layout of
 * vr_patch_unfold; H, W multiples of patch): the last ReLU of the stem and the unfold in one pass (evaluation). */
int vr_conv3x3_bias_relu_patch(const void* a, const void* w, const float* bias, const void* res, void* out, int32_t B, int32_t H,
                               int32_t W, int32_t Cin, int32_t Cout, int32_t patch, int32_t out_dtype, vr_stream_t stream);
/* out = conv(a, w) + res[pixel, co] (bf16): the data gradient of conv2 plus the gradient arriving over the stem's skip connection
 * (autograd of `x = conv3(conv2(a1)) + a1`, nets/patch_conv.py:69) without a separate add pass. */
int vr_conv3x3_res(const void* a, const void* w, const void* res, void* out, int32_t B, int32_t H, int32_t W, int32_t Cin,
                   int32_t Cout, int32_t out_dtype, vr_stream_t stream);
/* the same with `res` stored in PATCH order (vr_patch_unfold's layout, windows of res_patch x res_patch pixels): the projection's data
 * gradient as its GEMM writes it -- no fold pass between the 7 x 7 / stride-7 projection and the stem's backward (round 4). */
int vr_conv3x3_res_patch(const void* a, const void* w, const void* res, void* out, int32_t B, int32_t H, int32_t W, int32_t Cin,
                         int32_t Cout, int32_t out_dtype, int32_t res_patch, vr_stream_t stream);
/* Weights of that data-gradient convolution: dst[ci, (kh, kw, co)] = src[co, ci, 2 - kh, 2 - kw] (src fp32 [Co, Ci, 3, 3]). */
int vr_conv_w_flip(const float* src, void* dst, int32_t Co, int32_t Ci, int32_t dst_dtype, vr_stream_t stream);

/*
 * conv1 of the conv patch embedding (nets/patch_conv.py:63: 3x3 / stride 2 / pad 1, 3 -> Cout <= 32 channels) straight from
 * the fp32 NCHW image: out [B*Ho*Wo, Cout] (NHWC, fp32 or bf16) = conv(img, w) (+ bias, relu: the evaluation form with
 * BatchNorm folded in).  w bf16 [Cout, 32]: k = (kh, kw, c) in the first 27 columns, zeros behind.  No im2col matrix.
 */
int vr_conv1_direct(const float* img, const void* w, const float* bias, void* out, int32_t B, int32_t H, int32_t W, int32_t Cout,
                    int32_t relu, int32_t out_dtype, vr_stream_t stream);
/* Its weight gradient: dw[co, (kh,kw,ci)] (fp32, [Cout, 9*Cin]) += sum over pixels of dz[p, co] * a[p + (kh-1, kw-1), ci]; a, dz
 * bf16 NHWC.  Covered: Cin == Cout in {16, 24, 32} (the stem's conv2 / conv3); VR_EUNSUPPORTED otherwise. */
int vr_conv3x3_wgrad(const void* a, const void* dz, float* dw, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                     vr_stream_t stream);
int vr_bn_stats(const void* z, float* sum, float* sumsq, int64_t R, int32_t C, int32_t z_dtype, vr_stream_t stream);
/* Between vr_bn_stats and vr_bn_relu in training (torch.nn.BatchNorm2d, nets/patch_conv.py:23-38): mean = sum / n, var = sumsq / n -
 * mean^2 (>= 0); running_mean / running_var (optional, both or none) <- (1 - momentum) * running + momentum * (mean | var * n / (n - 1));
 * *num_batches_tracked += 1 (optional); rstd = 1 / sqrt(var + eps), scale = weight * rstd, shift = bias - mean * scale. */
int vr_bn_finalize(const float* sum, const float* sumsq, int64_t n, const float* weight, const float* bias, float eps, float momentum,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, float* scale, float* shift, float* mean,
                   float* rstd, int32_t C, vr_stream_t stream);
int vr_bn_relu(const void* z, const float* scale, const float* shift, const void* res, void* out, int64_t R, int32_t C,
               int32_t dtype, int32_t z_dtype, vr_stream_t stream);
int vr_bn_bwd(const void* da, const void* z, const float* scale, const float* shift, const float* mean, const float* rstd,
              float* sg, float* sgz, void* dz, int64_t R, int32_t C, int32_t training, int32_t dtype, int32_t z_dtype,
              vr_stream_t stream);
int vr_patch_unfold(void* a, void* col, int32_t B, int32_t gh, int32_t gw, int32_t P, int32_t C, int32_t fold, int32_t dtype,
                    vr_stream_t stream);
/* Training-mode patchify without the unfold / fold passes (nets/patch_conv.py:56-58,70-72; round 4): vr_bn_relu_patch writes
 * relu(bn(z)) (+ res, NHWC) straight into the patchify operand col [B*(H/patch)*(W/patch), (i, j, c)] of the projection GEMM;
 * vr_bn_bwd_patch reads `da` in that layout (the projection's data gradient as its GEMM leaves it), z and dz stay NHWC. */
int vr_bn_relu_patch(const void* z, const float* scale, const float* shift, const void* res, void* out, int32_t B, int32_t H,
                     int32_t W, int32_t patch, int32_t C, int32_t dtype, int32_t z_dtype, vr_stream_t stream);
int vr_bn_bwd_patch(const void* da, const void* z, const float* scale, const float* shift, const float* mean, const float* rstd,
                    float* sg, float* sgz, void* dz, int32_t B, int32_t H, int32_t W, int32_t patch, int32_t C, int32_t training,
                    int32_t dtype, int32_t z_dtype, vr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VITRES_HIP_H */
