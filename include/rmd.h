/*
 * rmd.h — C ABI of the MI355X (gfx950) cost-volume backend for qzed/raft-meets-dicl.
 *
 * Plain pointers, sizes and a HIP stream handle; no torch types.  Every entry point enqueues
 * work on `stream` (a hipStream_t passed as void*; NULL = the default stream) and returns
 * immediately: launchers never allocate, free or synchronise, so a caller may capture them into
 * a hipGraph.  Outputs and workspaces are caller-allocated device memory.
 *
 * Return codes: RMD_OK (0) or a negative RMD_ERR_* code; rmd_last_error() returns a
 * human-readable message for the last failing call on the calling thread.
 *
 * Each entry point names the reference function it replaces (qzed/raft-meets-dicl v2,
 * file:line).  The reference has no native code: these are the boundary its Python modules bind
 * through (ctypes stub in INTEGRATION.md; host mirror in raft-meets-dicl_amd/rmd/).
 *
 * Tensor conventions (all device pointers, contiguous, row-major):
 *   fmap   (B, C, H, W)  float32      feature maps at 1/8 resolution (raft.py:381 `.float()`)
 *   coords (B, 2, H, W)  float32      ch0 = x, ch1 = y, level-0 pixel units (grid.py:4-12)
 *   out    (B, L*(2r+1)^2, H, W) float32, channel = level*(2r+1)^2 + a*(2r+1) + b with x-offset
 *          a-r and y-offset b-r (meshgrid(dx, dy, indexing='ij'), raft.py:57-59).
 */
#ifndef RMD_H
#define RMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMD_OK 0
#define RMD_ERR_ARG (-1)          /* null pointer / bad enum */
#define RMD_ERR_SHAPE (-2)        /* unsupported or inconsistent sizes */
#define RMD_ERR_LAUNCH (-3)       /* kernel launch failed (hipGetLastError) */

/* element / compute types */
#define RMD_F32 0
#define RMD_F16 1
#define RMD_BF16 2
#define RMD_BF16X3 3   /* compute only: fp32-accurate split bf16, hi.hi + hi.lo + lo.hi per k-step */
#define RMD_S24 4      /* storage only: an fp32 value rounded to its top 24 bits (sign, exponent, 15 mantissa
                          bits; round half away from zero, NaN stays NaN), stored as 3 little-endian bytes
                          (bytes 1..3 of the float); row layout only, written by the x3 GEMM */

#define RMD_MAX_LEVELS 4

/*
 * Layout of a correlation pyramid in HBM (one allocation, `total_elements` elements of
 * `storage` type).  Level l has floor-halved sizes level_h[l] x level_w[l] (raft.py:38-47).  The
 * target map of each level is cut into chunks of tile_h[l] x tile_w[l] elements and chunks are
 * QUERY-MINOR: every chunk position holds the chunk of all `query_slots` queries back to back,
 *
 *   element(b, p, y, x) at level l =
 *     level_offset[l] + ((((b*tiles_y[l] + y/tile_h[l])*tiles_x[l] + x/tile_w[l]) * query_slots
 *                         + slot(p)) * tile_h[l]*tile_w[l]) + (y%tile_h[l])*tile_w[l] + x%tile_w[l]
 *
 * with tiles_y[l] = ceil(level_h[l] / tile_h[l]), tiles_x[l] = ceil(level_w[l] / tile_w[l]) and
 * p = y1*W + x1 the query pixel.  Two layouts (`layout`):
 *
 *  RMD_LAYOUT_ROWS  (every GEMM except w8): chunks 1 x (8, 8, 4, 2) (RMD_S24 storage: 1 x (8, 8, 4, 4),
 *    so every S24 chunk is a multiple of 4 bytes), slot(p) = p, query_slots = H*W.
 *  RMD_LAYOUT_TILES (the w8 GEMM: bf16 compute, fp16 storage): chunks 2x4, 2x4, 1x4, 1x2 and query
 *    slots in 2 x 16 query tiles whose 8-slot groups are 2 x 4 query patches:
 *      y1 < 2*floor(H/2): slot = ((y1/2)*QX + x1/16)*32 + ((x1%16)/4)*8 + (y1%2)*4 + x1%4, QX = ceil(W/16)
 *      y1 = H-1, H odd  : slot = floor(H/2)*QX*32 + x1            (the last row in raster order)
 *    query_slots = floor(H/2)*QX*32 (+ ceil(W/32)*32 for odd H); slots of no pixel (x1 >= W) hold
 *    unspecified values.  A 128-B line of a level-0/1 chunk position then holds a 2 x 4 target patch
 *    of a 2 x 4 query patch, so the windows of neighbouring queries share lines in both directions
 *    (cfg2 lookup reads 55 MB modelled vs 66 MB in the row layout, tools/lookup_line_model.py).
 *
 * In both layouts consecutive slots' chunks are adjacent, so a wave of 64 consecutive slots reads
 * (lookup) and writes (GEMM epilogue) 64 x 16 B of contiguous memory per chunk position (DESIGN.md
 * §3).  Padding rows/columns of a level's last chunks hold unspecified values and are never read.
 */
#define RMD_LAYOUT_ROWS 0
#define RMD_LAYOUT_TILES 1

typedef struct rmd_pyramid_desc {
    int batch, height, width;          /* query grid == level-0 target grid                  */
    int levels;                        /* 1 .. RMD_MAX_LEVELS                                */
    int storage;                       /* RMD_F32, RMD_F16 or RMD_S24 (3 bytes per element)   */
    int level_h[RMD_MAX_LEVELS], level_w[RMD_MAX_LEVELS];
    int tile_h[RMD_MAX_LEVELS], tile_w[RMD_MAX_LEVELS];
    int tiles_y[RMD_MAX_LEVELS], tiles_x[RMD_MAX_LEVELS];
    long long level_offset[RMD_MAX_LEVELS];    /* in elements */
    long long total_elements;
    int layout;                        /* RMD_LAYOUT_ROWS or RMD_LAYOUT_TILES                */
    int query_slots;                   /* query positions per chunk position (>= H*W)        */
} rmd_pyramid_desc;

/* Fill `desc` for a (batch, height, width) query grid in the row layout.  Host-only, no device work. */
int rmd_pyramid_describe(int batch, int height, int width, int levels, int storage,
                         rmd_pyramid_desc* desc);

/* Same for an explicit layout (RMD_LAYOUT_TILES needs storage RMD_F16). */
int rmd_pyramid_describe_layout(int batch, int height, int width, int levels, int storage, int layout,
                                rmd_pyramid_desc* desc);

/* Describe the pyramid rmd_corr_pyramid writes for (channels, compute): the tiles layout when the
 * call runs the w8 GEMM (see rmd_corr_gemm_kernel), the row layout otherwise.  rmd_corr_pyramid
 * rejects a desc whose layout its GEMM does not write. */
int rmd_pyramid_describe_for(int batch, int height, int width, int levels, int storage, int channels,
                             int compute, rmd_pyramid_desc* desc);

/* Bytes of device workspace rmd_corr_pyramid needs for `compute` (operand staging). */
size_t rmd_corr_pyramid_workspace_bytes(const rmd_pyramid_desc* desc, int channels, int compute);

/*
 * All-pairs correlation + pooled pyramid.  Replaces raft.CorrBlock.__init__
 * (src/models/impls/raft.py:18-47): corr0 = scale * fmap1^T fmap2 over each batch, then
 * levels-1 successive 2x2 average pools over the target dims, floor sizes.  scale = 1/sqrt(C) is
 * raft.CorrBlock (raft.py:33); scale = 1 gives raft_fs.CorrBlock's unnormalised products
 * (src/models/impls/raft_fs.py:13-87, whose pooled-feature dot equals the pooled volume).
 *   compute = RMD_F32    : exact f32 MFMA (v_mfma_f32_32x32x2_f32)
 *   compute = RMD_BF16X3 : fp32-accurate split bf16 MFMA, x = hi + lo, three bf16 products per
 *                          k-step (~2^-16 relative per product; f32 storage, C <= 256; other cases
 *                          run the exact f32 kernel) — the default parity mode
 *   compute = RMD_BF16   : bf16 MFMA operands, f32 accumulation (performance mode)
 * All levels are produced by the GEMM epilogue from the f32 accumulators and stored as
 * desc->storage.
 */
int rmd_corr_pyramid(const float* fmap1, const float* fmap2, int channels, float scale,
                     const rmd_pyramid_desc* desc, int compute, void* pyramid, void* workspace,
                     void* stream);

/* Name of the GEMM kernel rmd_corr_pyramid runs for these arguments: "w8" (bf16 operands, fp16
 * pyramid, C <= 256: the performance path), "stationary" (the same with 64-bit store addressing, for
 * maps whose level-0 row span passes 1 GiB, e.g. 4K frames), "x3" (RMD_BF16X3 with an f32 pyramid),
 * "tiled" (exact f32 MFMA or any other combination), or "invalid".  Host-only; for tests and introspection. */
const char* rmd_corr_gemm_kernel(const rmd_pyramid_desc* desc, int channels, int compute);

/* The two halves of rmd_corr_pyramid, for callers that time or overlap them separately:
 * rmd_corr_prepare transposes/converts both feature maps into the workspace (pixel-major,
 * channel-contiguous operands); rmd_corr_pyramid_prepared runs the GEMM + pyramid epilogue on them. */
int rmd_corr_prepare(const float* fmap1, const float* fmap2, int channels, float scale,
                     const rmd_pyramid_desc* desc, int compute, void* workspace, void* stream);
int rmd_corr_pyramid_prepared(int channels, float scale, const rmd_pyramid_desc* desc, int compute,
                              void* pyramid, void* workspace, void* stream);

/* rmd_corr_pyramid without the target operand's round trip through the workspace.  Where the call runs the w8
 * GEMM (rmd_corr_gemm_kernel) only fmap1 is converted into the workspace and the GEMM builds its target tiles
 * from fmap2 (fp32) itself; the pyramid is bit-identical to rmd_corr_pyramid's.  Every other GEMM runs
 * rmd_corr_pyramid's two halves.  Same arguments, descriptor, workspace size and error codes as rmd_corr_pyramid. */
int rmd_corr_pyramid_fused(const float* fmap1, const float* fmap2, int channels, float scale,
                           const rmd_pyramid_desc* desc, int compute, void* pyramid, void* workspace,
                           void* stream);

/* The two halves of rmd_corr_pyramid_fused's w8 route, for callers that time them separately.  Both return
 * RMD_ERR_ARG for a null pointer and for arguments another GEMM than w8 serves (after rmd_corr_pyramid's own
 * checks of desc, channels and compute).  rmd_corr_pyramid_staged reads what rmd_corr_prepare_queries (or
 * rmd_corr_prepare) left in the workspace for the same arguments. */
int rmd_corr_prepare_queries(const float* fmap1, int channels, const rmd_pyramid_desc* desc, int compute,
                             void* workspace, void* stream);
int rmd_corr_pyramid_staged(const float* fmap2, int channels, float scale, const rmd_pyramid_desc* desc,
                            int compute, void* pyramid, void* workspace, void* stream);

/*
 * Windowed bilinear pyramid lookup.  Replaces raft.CorrBlock.__call__ (raft.py:49-95):
 * level i is sampled at (x/2^i + a - r, y/2^i + b - r), bilinear, align_corners=True, zero
 * padding per tap.  Bit i of `zero_level_mask` zeroes level i (mask_costs entry i+3,
 * raft.py:86-87).  A level with height or width 1 yields NaN (the reference divides by zero at
 * raft.py:73-74).  radius 1..8.
 */
int rmd_corr_lookup(const void* pyramid, const rmd_pyramid_desc* desc, const float* coords,
                    int radius, unsigned zero_level_mask, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * On-the-fly windowed correlation (no all-pairs volume).  Replaces raft_fs.CorrBlock
 * (src/models/impls/raft_fs.py:13-87; scale = 1) and, with levels = 1 and scale = 1/sqrt(C), the
 * window dot of corr/dot.py:25-57.  rmd_corr_otf_prepare writes the pixel-major query rows
 * (fmap1 * scale) and the avg-pooled target rows of every level into `workspace`
 * (rmd_corr_otf_workspace_bytes; compute RMD_BF16X3 = fp32-accurate split-bf16 MFMA, lo.hi + hi.lo +
 * hi.hi over operands stored as (hi, lo) bf16 pairs; RMD_F32 = exact f32 MFMA; RMD_BF16 = bf16 MFMA);
 * rmd_corr_otf_lookup then produces rmd_corr_lookup's output for `coords` from them each iteration.
 */
size_t rmd_corr_otf_workspace_bytes(int batch, int channels, int height, int width, int levels, int compute);
int rmd_corr_otf_prepare(const float* fmap1, const float* fmap2, int batch, int channels, int height, int width,
                         int levels, float scale, int compute, void* workspace, void* stream);
int rmd_corr_otf_lookup(const void* workspace, int batch, int channels, int height, int width, int levels,
                        int compute, const float* coords, int radius, unsigned zero_level_mask, float* out,
                        void* stream);

/*
 * Backward of the on-the-fly lookup (training at resolutions where the volume does not fit; autograd of
 * raft_fs.py:25-87 — grid_sample backward, the matmul with fmap1 and the avg-pool chain — without any
 * O(N^2) buffer).  After each lookup's forward, its backward records the lookup's per-query patch
 * weights: rmd_corr_otf_record turns grad_out (B, L*(2r+1)^2, H, W) and the lookup's coords into a
 * record of rmd_corr_otf_record_bytes() (per level and query: the window origin and the (2r+2)^2
 * bilinear patch weights of grad_out).  rmd_corr_otf_backward then computes, from all records of one
 * rmd_corr_otf_prepare (fmap1, fmap2, scale as given there, its workspace unchanged):
 *   grad_fmap1 = scale * sum_l G_l P_l,   grad_fmap2 = sum_l avgpool_l^T(G_l^T (scale * fmap1))
 * with G_l the sum of the records' level-l patch weights and P_l the level-l pooled fmap2; both
 * outputs are overwritten (B, C, H, W) float32.  C <= 256.  compute as in rmd_corr_otf_prepare
 * (RMD_F32 and RMD_BF16X3: split-bf16 products, fp32 accumulation; RMD_BF16: bf16 products).
 * Masked and 1-pixel levels and non-finite coordinates record no contribution.  `records` is a host
 * array of `nrecords` device pointers.  Deterministic: records are summed in a fixed order, and the
 * pooled gradient adds per-workgroup fp32 tile sums as 64-bit fixed point (integer atomics, associative,
 * so bitwise order-independent for any dynamic range) at a power-of-two scale chosen per call from the
 * largest recorded |weight| and |scale * fmap1| so that no sum can overflow; non-finite contributions
 * propagate through a float side buffer.  A record carries a 256-B header after its weights.
 */
size_t rmd_corr_otf_record_bytes(int batch, int height, int width, int levels, int radius);
int rmd_corr_otf_record(const float* grad_out, const float* coords, int batch, int height, int width, int levels,
                        int radius, unsigned zero_level_mask, void* record, void* stream);
size_t rmd_corr_otf_backward_workspace_bytes(int batch, int channels, int height, int width, int levels, int compute);
int rmd_corr_otf_backward(const float* fmap1, const float* fmap2, const void* otf_workspace, int batch, int channels,
                          int height, int width, int levels, float scale, int compute, int radius, int nrecords,
                          const void* const* records, float* grad_fmap1, float* grad_fmap2, void* workspace,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the RAFT correlation (training; autograd of raft.py:18-95).  Coordinates are
 * detached in the reference (raft.py:402), so only the feature maps receive gradients.
 *
 * Gradient of the pyramid, dense float32 "G", in the forward pyramid's chunked query-minor order
 * with 8-target chunks: target row (l, y) is cut into nch(l) = ceil(W_l/8) chunks, chunk
 * ch(l, y, x) = coff(l) + y*nch(l) + x/8 with coff(l) = sum_{l'<l} H_l'*nch(l'), TC chunks per image,
 * and element (b, target (l, y, x), query p) at ((b*TC + ch)*N + p)*8 + x%8.  Seen as a matrix over
 * the padded targets t' = 8*ch + x%8 (T' = 8*TC = rmd_corr_grad_targets(); pad targets x >= W_l stay
 * zero) G is (T' x N) stored in 8-row blocks.  With P = rmd_corr_pool_targets(fmap2, scale =
 * 1/sqrt(C)) as (B, C, T') in the same target order:
 *   grad_fmap1 (B, C, N) = P G     (rmd_corr_grad_gemm layout 3, lda = T', ldb = N)
 *   dP (B, C, T') = fmap1 G^T      (rmd_corr_grad_gemm layout 2, lda = N, ldb = N)
 *   grad_fmap2 = rmd_corr_unpool_targets(dP, scale = 1/sqrt(C)).
 * A wave of 64 consecutive queries whose (smooth) flow moves their windows one column per query
 * touches 3 128-B lines per 8 lanes at every tap (8 lines in a plain (B, T, N) order).
 */

/* Padded targets per image of G (T' = 8 * chunks over all levels), or -1 on bad sizes.  Host-only. */
long long rmd_corr_grad_targets(int height, int width, int levels);

/* grad_levels (G, caller-zeroed once per forward) += d(lookup)/d(pyramid)^T grad_out, where
 * grad_out is (B, L*(2r+1)^2, H, W) like rmd_corr_lookup's output.  Replaces the
 * grid_sampler_2d_backward of raft.py:80.  Zeroed levels (mask) and 1-pixel (NaN) levels add
 * nothing.  Deterministic (no atomics). */
int rmd_corr_lookup_backward(const float* grad_out, const rmd_pyramid_desc* desc, const float* coords,
                             int radius, unsigned zero_level_mask, float* grad_levels, void* stream);

/* G of ALL nlookups lookups of one forward in one pass: grad_levels = (accumulate ? G : 0)
 * + sum over i in order of lookup i's contribution (grad_outs[i], coords[i], zero_level_masks[i] —
 * each as in rmd_corr_lookup_backward; masks may be NULL), writing every element of G (no zero fill
 * needed).  Same arithmetic and summation order as the sequence of rmd_corr_lookup_backward calls
 * i = 0, 1, ... into a zeroed G.  grad_outs / coords / zero_level_masks are HOST arrays of device
 * pointers / values.  Replaces the per-lookup grid_sampler_2d_backward of raft.py:80 plus the
 * accumulation of those gradients into the correlation volume that autograd performs. */
int rmd_corr_grad_build(const float* const* grad_outs, const float* const* coords,
                        const unsigned* zero_level_masks, int nlookups, const rmd_pyramid_desc* desc, int radius,
                        int accumulate, float* grad_levels, void* stream);

/* rmd_corr_grad_build with bf16_out != 0: G stored as bfloat16 (round to nearest even of the fp32 sums,
 * the same element order, 2 bytes each) — what rmd_corr_grad_gemm_bf16g reads in the bf16 precision
 * mode, whose fp32-G GEMM rounds G to bfloat16 on load anyway (bit-identical results, half the G
 * traffic).  bf16_out requires accumulate == 0 and nlookups <= 16. */
int rmd_corr_grad_build_ex(const float* const* grad_outs, const float* const* coords,
                           const unsigned* zero_level_masks, int nlookups, const rmd_pyramid_desc* desc, int radius,
                           int accumulate, int bf16_out, void* grad_levels, void* stream);

/* pooled (B, C, T') = avg_pool_{2^l}(fmap2) * scale for every level, in G's padded target order (pad
 * targets 0) (raft.py:35-47 applied to the feature map, which commutes with the product). */
int rmd_corr_pool_targets(const float* fmap2, int batch, int channels, int height, int width, int levels,
                          float scale, float* pooled, void* stream);

/* grad_fmap2 (B, C, H, W) = scale * sum_l avg_pool_{2^l}^T(grad_pooled level l)  (avg_pool2d_backward);
 * grad_pooled is (B, C, T') in G's padded target order. */
int rmd_corr_unpool_targets(const float* grad_pooled, int batch, int channels, int height, int width, int levels,
                            float scale, float* grad_fmap2, void* stream);

/* The two GEMMs of the backward (autograd of the matmul at raft.py:31-33), batched over `batch`;
 * compute RMD_BF16X3: fp32-accurate from three split-bf16 MFMA products (hi.hi + hi.lo + lo.hi, the fp32
 * precision modes); RMD_BF16: one bf16 product per k-step, fp32 accumulation (the bf16 mode):
 *   out[b] (m x nc, row-major) = a[b] (m x k, row stride lda) . B[b]
 *   layout 0: B element (k, n) at bm[k*ldb + n]                 (k x nc, ldb >= nc)
 *   layout 1: B element (k, n) at bm[n*ldb + k]                 (nc x k, ldb >= k)
 *   layout 2: B element (k, n) at bm[((n/8)*ldb + k)*8 + n%8]   (ldb >= k)  -> dP = fmap1 G^T
 *   layout 3: B element (k, n) at bm[((k/8)*ldb + n)*8 + k%8]   (ldb >= nc) -> grad_fmap1 = P G
 * Batch strides are m*lda for a and k*ldb, nc*ldb, ceil(nc/8)*8*ldb, ceil(k/8)*8*ldb for bm
 * (layouts 0-3); out is contiguous.  K may be
 * split over workgroups: then `workspace` must hold rmd_corr_grad_gemm_workspace_bytes() bytes
 * (0 = none needed) and a second pass sums the partial tiles in a fixed order (deterministic). */
size_t rmd_corr_grad_gemm_workspace_bytes(int batch, int m, int k, int nc);
int rmd_corr_grad_gemm(const float* a, long long lda, const float* bm, long long ldb, int batch, int m, int k, int nc,
                       int layout, int compute, float* out, void* workspace, void* stream);

/* rmd_corr_grad_gemm with compute RMD_BF16 and a bfloat16 B (layouts 2 / 3: G from
 * rmd_corr_grad_build_ex with bf16_out): the fp32-B GEMM rounds B to bfloat16 on load, so the result
 * is bit-identical to rmd_corr_grad_gemm(..., RMD_BF16, ...) on the fp32 G; B's base 8-byte aligned
 * for vector loads.  Same workspace as rmd_corr_grad_gemm_workspace_bytes. */
int rmd_corr_grad_gemm_bf16g(const float* a, long long lda, const void* bm, long long ldb, int batch, int m, int k,
                             int nc, int layout, float* out, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DICL cost volumes.  Shapes: fmap1 (B, C, h, w); fmap2 (B, C, hl, wl); coords (B, 2, h, w);
 * stack (B, d, d, 2C [+2], h, w) float32 contiguous with d = 2r+1, dim 1 the x-offset a-r and
 * dim 2 the y-offset b-r — exactly the MatchingNet input (blocks/dicl.py:111-118).  h*w must be a
 * multiple of 4 (MatchingNet already needs even h and w).
 */

/*
 * Displacement stack with bilinear sampling.  Replaces the grid_sample/expand/cat of
 * corr.dicl.CorrelationModule.forward (src/models/common/corr/dicl.py:26-54; dicl_1x1.py:51-79),
 * of dicl_emb.py:51-89 (extra_delta = 1 appends the (a-r, b-r) channels) and the per-level gather
 * of raft_dicl_ml.CorrelationModule.forward (src/models/impls/raft_dicl_ml.py:294-315):
 *   stack[b,a,bb,0:C]  = fmap1
 *   stack[b,a,bb,C:2C] = bilinear(fmap2, ((x/2^level + a-r) * (wl-1)/(norm_w-1),
 *                                        (y/2^level + bb-r) * (hl-1)/(norm_h-1)))
 * zero padding per tap.  corr/dicl.py: level 0, norm = (h, w) = (hl, wl); raft_dicl_ml level i:
 * norm = fmap1's (h, w) (the reference normalises with the full-resolution size, :300-305).
 */
int rmd_dicl_stack(const float* fmap1, const float* fmap2, const float* coords, int batch, int channels,
                   int height, int width, int level_height, int level_width, int radius, int level,
                   int norm_height, int norm_width, int extra_delta, float* out, void* stream);

/* Gradients of rmd_dicl_stack: grad_fmap1 = sum over displacements of the first C channels
 * (deterministic); grad_fmap2 = bilinear scatter of channels C..2C-1 (float atomics, as ATen's
 * grid_sampler_2d_backward).  Coordinates carry no gradient (they are detached, raft.py:402). */
int rmd_dicl_stack_backward(const float* grad_stack, const float* coords, int batch, int channels,
                            int height, int width, int level_height, int level_width, int radius,
                            int level, int norm_height, int norm_width, int extra_delta,
                            float* grad_fmap1, float* grad_fmap2, void* stream);

/*
 * Name of the kernel rmd_dicl_stack (backward = 0) or rmd_dicl_stack_backward (backward = 1) runs for
 * these arguments: the launchers dispatch on the same decision.  Host only, no GPU call; the string
 * is static.  Forward: "patch/R" (unit steps, R = 1..4), "separable/R/K" (scaled grid, R = 3, 4,
 * K x K patch, K = 4, 6, 8), "general".  Backward: "patch2/R/small|large" and "patch1/R/small|large"
 * (unit steps, two pixels or one per lane; one only for stacks of >= 4 GiB per image),
 * "separable2/K/small|large" (K = 4, 6, 8), "separable1/10/small|large", "general/small|large" and
 * "fallback"; small / large is the LDS window, 16 or 48 KiB.  "invalid" for arguments the calls reject.
 * rmd_dicl_stack_kernel_list: every kernel name the query can return for that direction,
 * comma-separated ("invalid" names no kernel and is not listed).
 */
const char* rmd_dicl_stack_kernel(int batch, int channels, int height, int width, int level_height,
                                  int level_width, int radius, int level, int norm_height, int norm_width,
                                  int extra_delta, int backward);
const char* rmd_dicl_stack_kernel_list(int backward);

/* Bytes of device workspace rmd_dicl_stack_int(_backward) needs (occlusion mask, 1 B/pixel). */
size_t rmd_dicl_stack_int_workspace_bytes(int batch, int height, int width);

/*
 * DICL baseline integer matching volume with occlusion mask.  Replaces
 * FlowLevel.compute_cost's volume build (src/models/impls/dicl.py:212-238): for di = i-ru (x),
 * dj = j-rv (y), both halves are copied where (x+di, y+dj) is inside and zero elsewhere, then the
 * whole 2C vector is zeroed where sum_c of its f2 half == 0.  out (B, 2ru+1, 2rv+1, 2C, h, w).
 */
int rmd_dicl_stack_int(const float* fmap1, const float* fmap2, int batch, int channels, int height, int width,
                       int ru, int rv, float* out, void* workspace, void* stream);

/* Gradients of rmd_dicl_stack_int (the mask is detached, dicl.py:236): deterministic gathers. */
int rmd_dicl_stack_int_backward(const float* grad_mvol, const float* fmap2, int batch, int channels,
                                int height, int width, int ru, int rv, float* grad_fmap1,
                                float* grad_fmap2, void* workspace, void* stream);

/*
 * Backward warping.  Replaces common.warp.warp_backwards (src/models/common/warp.py:5-33):
 *   out[b,c,y,x] = mask * bilinear(img2[b,c], x + flow[b,0,y,x], y + flow[b,1,y,x])   (zero padding,
 *   align_corners=True), mask = (in-bounds bilinear weight > 1 - eps) (grid_sample of ones, :28-30).
 * img2, out (B, C, h, w); flow (B, 2, h, w); mask (B, h, w) uint8 or NULL (the reference's bool mask is
 * this plane broadcast over C).  The flow carries no gradient (dicl.py:178 detaches it).
 */
int rmd_warp_backwards(const float* img2, const float* flow, int batch, int channels, int height, int width,
                       float eps, float* out, unsigned char* mask, void* stream);

/* d img2 (B, C, h, w) = bilinear^T(mask * grad_out); zeroes grad_img2 first (float atomics, like ATen). */
int rmd_warp_backwards_backward(const float* grad_out, const float* flow, int batch, int channels, int height,
                                int width, float eps, float* grad_img2, void* stream);

/* Bytes of device workspace rmd_dicl_stack_int_warped(_backward) needs (warped map + flags). */
size_t rmd_dicl_stack_int_warped_workspace_bytes(int batch, int channels, int height, int width);

/*
 * FlowLevel with a coarse flow (src/models/impls/dicl.py:171-238): feat2 is warped back by `flow`
 * (warp_backwards, eps 1e-5) and the masked integer volume of rmd_dicl_stack_int is built on it.  The
 * warp runs inside the occlusion-flag pass, so the volume costs the same launches as without warping.
 */
int rmd_dicl_stack_int_warped(const float* fmap1, const float* fmap2, const float* flow, int batch, int channels,
                              int height, int width, int ru, int rv, float* out, void* workspace, void* stream);

/* Gradients of rmd_dicl_stack_int_warped w.r.t. fmap1 and fmap2 (flow and masks detached). */
int rmd_dicl_stack_int_warped_backward(const float* grad_mvol, const float* fmap2, const float* flow, int batch,
                                       int channels, int height, int width, int ru, int rv, float* grad_fmap1,
                                       float* grad_fmap2, void* workspace, void* stream);

/*
 * Displacement-aware projection: out[b,o,p] = sum_i W[o,i] x[b,i,p] (1x1 conv, no bias) with
 * W = conv1.weight[:,:,0,0] (D x D).  Replaces DisplacementAwareProjection.forward
 * (src/models/common/blocks/dicl.py:143-150), the per-level DAPs of raft.py:146-168 and the
 * 324x324 'full' DAP of raft_dicl_ml.py:268-273,339-341.  transpose = 1 applies W^T (the input
 * gradient).  x, out: (B, D, pixels) float32.  Computed as a split-bf16 MFMA GEMM (W and x split
 * into hi + lo bf16, W_lo.x_hi + W_hi.x_lo + W_hi.x_hi accumulated in fp32: ~1.5e-5 of float64)
 * for D <= 1024; larger D falls back to an exact-fp32 VALU kernel.
 */
int rmd_dap(const float* x, const float* weight, int batch, int disp, int pixels, int transpose, float* out,
            void* stream);

/* Weight gradient of rmd_dap (autograd of the 1x1 conv weight, blocks/dicl.py:137,147):
 *   grad_weight[o][i] = sum_b sum_p grad_out[b, o, p] x[b, i, p]      (D x D, overwritten)
 * split-bf16 MFMA (lo.hi + hi.lo + hi.hi, fp32 accumulation), the batch x pixel sum split over
 * workgroups into `workspace` (rmd_dap_weight_grad_workspace_bytes) and summed in a fixed order
 * (deterministic). */
size_t rmd_dap_weight_grad_workspace_bytes(int batch, int disp, int pixels);
int rmd_dap_weight_grad(const float* grad_out, const float* x, int batch, int disp, int pixels, float* grad_weight,
                        void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-iteration flow heads on either side of the lookup.
 */

/*
 * Convex 8x upsampling.  Replaces the tail of Up8Network.forward (src/models/impls/raft.py:319-331)
 * after its two convolutions: mask (B, 576, h, w) logits with channel = k*64 + i*8 + j (neighbour
 * k = 3*ky + kx, sub-pixel (i, j)), flow (B, 2, h, w) ->
 *   out[b, c, 8y+i, 8x+j] = sum_k softmax_k(mask[b, k*64+i*8+j, y, x] / temperature) * 8*flow[b, c, y+ky-1, x+kx-1]
 * (zero outside the map; F.unfold(8*flow, 3, padding=1)).  out (B, 2, 8h, 8w) float32.
 */
int rmd_up8(const float* mask, const float* flow, int batch, int height, int width, float temperature,
            float* out, void* stream);

/* Bytes of device workspace rmd_up8_backward needs (per-pixel neighbour sums, 72 B/pixel). */
size_t rmd_up8_workspace_bytes(int batch, int height, int width);

/* Gradients of rmd_up8 w.r.t. mask (B, 576, h, w) and flow (B, 2, h, w); deterministic (no atomics). */
int rmd_up8_backward(const float* mask, const float* flow, const float* grad_out, int batch, int height, int width,
                     float temperature, float* grad_mask, float* grad_flow, void* workspace, void* stream);

/*
 * Soft-argmax flow regression.  Replaces raft.SoftArgMaxFlowRegression.forward (raft.py:112-135;
 * levels = L, level l scaled by 2^l) and the single-level SoftArgMaxFlowRegression of
 * corr/dicl.py:64-85, corr/dot.py:69-90, dicl_1x1.py:89-110, dicl_emb.py:107-134 (levels = 1):
 *   p_k = softmax_k(cost[b, l*(2r+1)^2 + k, :] / temperature),  k = a*(2r+1) + bb,
 *   flows[l, b, 0] = 2^l * sum_k p_k (a - r),  flows[l, b, 1] = 2^l * sum_k p_k (bb - r).
 * cost (B, cost_channels, pixels) float32 with cost_channels >= L*(2r+1)^2 (extra trailing channels
 * are ignored: dicl_emb regresses on the first (2r+1)^2 of its embedding); flows (L, B, 2, pixels).
 * radius 1..4.  The *WithDap variants run rmd_dap on each level first (raft.py:139-181).
 */
int rmd_softargmax(const float* cost, int batch, int cost_channels, int pixels, int levels, int radius,
                   float temperature, float* flows, void* stream);

/* d cost for channels [0, L*(2r+1)^2) of each batch row (others untouched) from grad_flows (L, B, 2, pixels). */
int rmd_softargmax_backward(const float* cost, const float* grad_flows, int batch, int cost_channels, int pixels,
                            int levels, int radius, float temperature, float* grad_cost, void* stream);

/*
 * DICL flow head: the two modules between the DAP and the context network of a DICL level, from one
 * read of the cost.  Replaces FlowRegression.forward (src/models/impls/dicl.py:53-85),
 * FlowEntropy.forward (dicl.py:31-50) and the coarse-flow addition of FlowLevel.compute_flow
 * (dicl.py:195).  cost (B, du, dv, pixels) float32, du = 2 ru + 1 (dim 1: the u / x offset), dv = 2 rv + 1
 * (dim 2: the v / y offset), ru and rv independent in 0..8; with D = du * dv:
 *   p_ij      = softmax over all (i, j) of cost[b, i, j, :], max-subtracted
 *   out[b, 0] = sum p_ij (i - ru)  (+ flow_coarse[b, 0]),   out[b, 1] = sum p_ij (j - rv)  (+ flow_coarse[b, 1])
 *   out[b, 2] = -sum p_ij log(clamp(p_ij, eps, 1 - eps)) / log(D)
 * all in float32 (1 - eps and log(D) included: 1 - 1e-9 is 1).  out (B, 3, pixels); flow_coarse
 * (B, 2, pixels) or NULL; eps in [0, 0.5).  D = 1 gives flow 0 and entropy 0/0 = NaN, as the reference.
 * A NaN or +inf cost at a pixel, or all costs -inf, makes its three outputs NaN (torch's softmax); a
 * single -inf cost has p = 0 and adds 0 to the entropy.  Square windows of radius 1..4 keep the costs
 * in registers; every other (ru, rv) reads them again per pass.
 */
int rmd_dicl_flow_head(const float* cost, const float* flow_coarse, int batch, int du, int dv, int pixels, float eps,
                       float* out, void* stream);

/*
 * d cost (B, du, dv, pixels) of rmd_dicl_flow_head from grad_out (B, 3, pixels): autograd of dicl.py:43-50
 * and :78-83 in one pass that recomputes p (nothing is saved by the forward):
 *   grad_cost_k = p_k (g_k - sum_j p_j g_j),
 *   g_k = gu u_k + gv v_k - gH (log(clamp(p_k, eps, 1 - eps)) + [eps <= p_k <= 1 - eps]) / log(D)
 * (the bracket is torch's clamp subgradient), with g taken relative to the arg-max displacement so a
 * peaked softmax keeps its relative accuracy.  No atomics, no workspace: bitwise reproducible.  A pixel
 * whose outputs are NaN gets a NaN gradient, a -inf cost gradient 0.  The gradient with respect to
 * flow_coarse is grad_out[:, :2] and needs no kernel.
 */
int rmd_dicl_flow_head_backward(const float* cost, const float* grad_out, int batch, int du, int dv, int pixels,
                                float eps, float* grad_cost, void* stream);

/*
 * Local cross-attention of the hidden-state upsampler HUpCrossAttn (src/models/common/hsup.py:71-92):
 * q (B, ck, h, w) float32 from the fine level, k (B, ck, h2, w2) and v (B, cv, h2, w2) from the coarse
 * one, out (B, cv, h, w).  h = fy h2 and w = fx w2 with integer factors 1..64; wy, wx in {1, 3, 5}.  For
 * the fine pixel (y, x) with parent cell (Y, X) = (y / fy, x / fx) and window entry j = (jy, jx):
 *   cell_j = (Y + jy - wy/2, X + jx - wx/2)
 *   s_j    = sum_c q[c, y, x] k[c, cell_j]      a cell outside the map is a zero key: logit 0, not masked
 *   a      = softmax(s)                         the maximum subtracted, no 1/sqrt(ck) scaling
 *   out[c, y, x] = sum_j a_j v[c, cell_j]       a cell outside the map is a zero value
 * (F.unfold's zero padding, hsup.py:71, :76).  One launch; K and V are never expanded to the fine
 * resolution.  A weight is always multiplied with its value, so non-finite inputs spread as in the
 * reference (0 * inf = NaN; a NaN logit makes the pixel's softmax NaN).
 * rmd_local_cross_attn_kernel names the route a call takes: "w3x3_f2x2" (the models' 3 x 3 window at
 * factor 2 x 2), "generic", or "invalid" for arguments the calls refuse (host only).
 */
const char* rmd_local_cross_attn_kernel(int batch, int ck, int cv, int h, int w, int h2, int w2, int wy, int wx);
int rmd_local_cross_attn(const float* q, const float* k, const float* v, int batch, int ck, int cv, int h, int w,
                         int h2, int w2, int wy, int wx, float* out, void* stream);

/*
 * Gradients of rmd_local_cross_attn from grad_out (B, cv, h, w); only q, k and v are read again, the
 * softmax is recomputed.  With g = grad_out at a pixel:
 *   da_j = sum_c g[c] v[c, cell_j],  ds_j = a_j (da_j - sum_i a_i da_i)
 *   grad_q[c] = sum_j ds_j k[c, cell_j]
 *   grad_k[c, cell] = sum of ds_{p,j} q_p[c], grad_v[c, cell] = sum of a_{p,j} g_p[c]
 * over every fine pixel p and entry j with cell_j(p) = cell.  A pass per fine pixel writes grad_q and
 * a, ds to `workspace` (rmd_local_cross_attn_workspace_bytes() bytes: (B, 2 wy wx, h, w) float32); a
 * pass per coarse cell then adds its wy wx neighbour cells x fy fx fine pixels in a fixed order.  No
 * atomics: bitwise reproducible.  All three gradients are written.
 */
size_t rmd_local_cross_attn_workspace_bytes(int batch, int h, int w, int wy, int wx);
int rmd_local_cross_attn_backward(const float* grad_out, const float* q, const float* k, const float* v, int batch,
                                  int ck, int cv, int h, int w, int h2, int w2, int wy, int wx, float* grad_q,
                                  float* grad_k, float* grad_v, void* workspace, void* stream);

/*
 * Input format (src/models/input.py).  rmd_input_images replaces Input.__getitem__'s clip and range
 * map (input.py:215-221), ModuloPadding.apply (input.py:79-138) and TorchAdapter's permute to NCHW
 * (input.py:280-281) for one image tensor of a pair:
 *   out[b, k, y, x] = (range_max - range_min) * clip(img[b, sy, sx, k], clip_min, clip_max) + range_min
 * with (sy, sx) = (y - pad_top, x - pad_left) mapped into the image by the pad mode, or the constant
 * 0 / 1 for RMD_PAD_ZEROS / RMD_PAD_ONES outside it.  img (B, H, W, C) float32 NHWC, out (B, C, H', W').
 * Modes: numpy 'edge' == torch 'replicate' (EDGE), numpy/torch 'reflect' (REFLECT), numpy 'symmetric',
 * numpy 'wrap' == torch 'circular' (WRAP).  The statistic modes (maximum, mean, median, minimum) are
 * not provided (no config uses them; every cfg pads with zeros).
 * rmd_input_flow replaces the flow / valid side (input.py:120-122, 301-313): flow (B, H, W, 2) float32,
 * valid (B, H, W) bytes -> flow_out (B, 2, H', W') with NaN -> 0 and values clipped to +-flow_inf,
 * valid_out (B, H', W') bytes; padding is zero flow / invalid.
 */
#define RMD_PAD_ZEROS 0
#define RMD_PAD_ONES 1
#define RMD_PAD_EDGE 2
#define RMD_PAD_REFLECT 3
#define RMD_PAD_SYMMETRIC 4
#define RMD_PAD_WRAP 5

int rmd_input_images(const float* img, int batch, int height, int width, int channels, float clip_min,
                     float clip_max, float range_min, float range_max, int padded_height, int padded_width,
                     int pad_top, int pad_left, int mode, float* out, void* stream);

int rmd_input_flow(const float* flow, const unsigned char* valid, int batch, int height, int width,
                   int padded_height, int padded_width, int pad_top, int pad_left, float flow_inf, float* flow_out,
                   unsigned char* valid_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sequence losses (the part of a training step the reference keeps in its model package).  One
 * operation covers the four loss types:
 *   raft/sequence               SequenceLoss.compute, src/models/impls/raft.py:616-644
 *   raft+dicl/mlseq             MultiLevelSequenceLoss.compute + upsample, src/models/common/loss/mlseq.py:34-67
 *   raft+dicl/mlseq-restricted  RestrictedMultiLevelSequenceLoss.compute, src/models/impls/raft_dicl_ctf_l3.py:430-473
 *   dicl/multiscale             MultiscaleLoss.compute + upsample, src/models/impls/dicl.py:436-472
 * For npred predictions flow_k (B, 2, h_k, w_k) float32 against target (B, 2, H, W) and a validity
 * mask (B, H, W) of bytes (non-zero = set; a prediction's own `mask` replaces the shared `valid`):
 *   f    = flow_k where (h_k, w_k) == (H, W), else its bilinear align_corners=True upsample with
 *          component 0 times W/w_k and component 1 times H/h_k (mlseq.py:59-67; ATen's index rule:
 *          source = dst * ((in-1)/(out-1)) in fp32, 0 for out == 1, i0 = floor, i1 = i0 + (i0 < in-1))
 *   dist = |d0|+|d1| (RMD_LOSS_L1), sqrt(d0^2+d1^2) (RMD_LOSS_L2), (|d0|+|d1|)/2 (RMD_LOSS_ABSMEAN,
 *          raft.py:627-628), (|d0|+|d1|+1e-8)^0.4 (RMD_LOSS_ROBUST, dicl.py:450-451), d = f - target
 *   S_k  = sum of dist over set pixels (a selection: raft.py:639), N_k = their number; with
 *          include_invalid S_k = sum of dist * mask (a product: raft.py:633) and N_k = B*H*W
 *   loss = scale * sum_k weight_k * S_k / N_k
 * N_k == 0 gives NaN as mean() of an empty tensor does; with skip_empty such a prediction adds exactly
 * 0 (`if torch.any(valid_lvl)`, raft_dicl_ctf_l3.py:453, decided on the device).  `loss` is 1 float,
 * `counts` npred 64-bit integers (N_k, read again by the backward), `workspace`
 * rmd_sequence_loss_workspace_bytes() bytes.  Per-block partial sums are added in a fixed order in
 * double: no atomics, bitwise reproducible.  At most RMD_LOSS_MAX_PREDICTIONS per call (the table is a
 * kernel argument); a caller chunks longer lists and adds the chunk losses.
 */
#define RMD_LOSS_MAX_PREDICTIONS 32
#define RMD_LOSS_L1 1
#define RMD_LOSS_L2 2
#define RMD_LOSS_ABSMEAN 3
#define RMD_LOSS_ROBUST 4

typedef struct rmd_loss_prediction {
    const float* flow;             /* (B, 2, height, width)                                           */
    const unsigned char* mask;     /* own (B, H, W) mask, or NULL: the call's shared `valid`           */
    float* grad;                   /* backward: (B, 2, height, width) output, NULL = none required     */
    int height, width;
    float weight;
} rmd_loss_prediction;

size_t rmd_sequence_loss_workspace_bytes(int batch, int height, int width, int npred);
int rmd_sequence_loss(const rmd_loss_prediction* preds, int npred, const float* target, const unsigned char* valid,
                      int batch, int height, int width, int norm, int include_invalid, int skip_empty, float scale,
                      float* loss, long long* counts, void* workspace, void* stream);

/* Gradients of rmd_sequence_loss (autograd of the lines above), recomputed from the inputs: nothing
 * is saved by the forward but `counts`.  grad_loss (1 float, the upstream gradient) and counts are
 * read from DEVICE memory.  Every preds[k].grad that is not NULL is overwritten:
 *   full resolution: grad = grad_loss * scale * weight_k / N_k * m(p) * d dist / d d_c, with
 *     sign(d_c) (sign(0) = 0) for L1, half that for ABSMEAN, d_c/|d| (0 where |d| = 0, as torch's norm
 *     backward) for L2, 0.4 (|d0|+|d1|+1e-8)^-0.6 sign(d_c) for ROBUST;
 *   upsampled: the transpose of the bilinear map in gather form (each coarse pixel sums the fine
 *     pixels whose i0 / i1 select it, in a fixed order) — no atomics, bitwise reproducible.
 * N_k == 0 gives an all-zero gradient. */
int rmd_sequence_loss_backward(const rmd_loss_prediction* preds, int npred, const float* target,
                               const unsigned char* valid, int batch, int height, int width, int norm,
                               int include_invalid, float scale, const float* grad_loss, const long long* counts,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Flow metrics (what an evaluation or training loop computes next from the same three tensors).
 * One operation covers the reference's flow metrics, for every estimate of a call and every sample
 * of the batch on its own (the evaluator's per-sample loop, src/evaluation/evaluator.py:29-37):
 *   epe             EndPointError.compute, src/metrics/epe.py:35-53
 *   fl-all          FlAll.compute, src/metrics/fl_all.py:29-44
 *   aae             AverageAngularError.compute, src/metrics/aae.py:30-44
 *   flow-magnitude  FlowMagnitude.compute, src/metrics/flow.py:32-36
 * `estimates` is a HOST array of nest device pointers, each (B, 2, H, W) float32; target (B, 2, H, W)
 * float32; valid (B, H, W) bytes (non-zero = set); `distances` a HOST array of nd floats.  The result
 * is RAW statistics, stats (nest, B, RMD_METRICS_SLOTS) float64 — the caller divides:
 *   slot 0       H*W
 *   slot 1       number of set mask bytes of the sample
 *   slot 2       sum over the set pixels of epe = sqrtf(d0*d0 + d1*d1), d = estimate - target, each
 *                operation rounded in fp32 (epe.py:39), the sum in double
 *   slot 3       number of set pixels with epe > fl_abs && epe > fl_rel * |target|_2, both norms and the
 *                product in fp32 (fl_all.py:33-41; the reference's constants are 3 and 0.05f)
 *   slot 4, 5    sum of the angle in radians over all pixels / over the set pixels:
 *                acos(clamp((u u' + v v' + 1) / (|est| |tgt| + 1), -1, 1)) (aae.py:35-44) with u, v the
 *                components 0, 1 of the CHANNEL axis, evaluated in double from the fp32 inputs; the clamp
 *                keeps NaN as torch.clamp does
 *   slot 6       sum over all pixels of |estimate|_ord in fp32 (flow.py:34), mag_ord = 1, 2, +inf or any
 *                other p > 0 (anything else: RMD_ERR_ARG)
 *   slot 7       number of pixels with a non-finite estimate component
 *   slot 8 + i   number of set pixels with epe <= distances[i], i < nd <= RMD_METRICS_MAX_DISTANCES
 *                (epe.py:51); slots past 8 + nd are 0
 * Sums are double and carry NaN / Inf; counts are integers, exact; a comparison with NaN is false.  A
 * pixel outside the mask reaches slots 0, 4, 6 and 7 of its own sample only, and no sample reaches
 * another sample's row.  No set pixel is not special: the caller's division gives NaN as mean() of an
 * empty tensor does.  Blocks write partial rows to `workspace` (rmd_flow_metrics_workspace_bytes()
 * bytes) with plain stores and a second kernel adds them in block order: no atomics, bitwise
 * reproducible, and an estimate's rows do not depend on the other estimates of the call.  At most
 * RMD_METRICS_MAX_ESTIMATES per call (the table is a kernel argument); a caller chunks longer lists.
 * All argument checks run on the host before any launch.
 */
#define RMD_METRICS_MAX_ESTIMATES 32
#define RMD_METRICS_MAX_DISTANCES 8
#define RMD_METRICS_SLOTS 16

size_t rmd_flow_metrics_workspace_bytes(int batch, int height, int width, int nest);
int rmd_flow_metrics(const float* const* estimates, int nest, const float* target, const unsigned char* valid,
                     int batch, int height, int width, const float* distances, int nd, float fl_abs, float fl_rel,
                     float mag_ord, double* stats, void* workspace, void* stream);

/*
 * Fused dicl-1x1 cost: the displacement gather of corr.dicl_1x1.CorrelationModule.forward
 * (src/models/common/corr/dicl_1x1.py:51-79) and MatchingNet1x1 (dicl_1x1.py:8-30) with its norm layers
 * folded into the weights, in one kernel; neither the (B, d, d, 2C, h, w) stack nor a hidden activation
 * is written.  fmap1, fmap2 (B, C, h, w), coords (B, 2, h, w), out (B, 2r+1, 2r+1, h, w) (dim 1 = x offset,
 * dim 2 = y offset), all float32.  For pixel p and displacement (a, bb) the column is
 *   x = [fmap1[:, p] ; bilinear(fmap2, coords[p] + (a - r, bb - r))]
 * sampled as rmd_dicl_stack does at level 0 with fmap1's own (h, w) (zero padding per tap; a non-finite
 * sample position gives NaN samples), and
 *   out = w4 . relu(W3 relu(W2 relu(W1 x + t1) + t2) + t3) + b4
 * with W1 (c1, 2C), W2 (c2, c1), W3 (c3, c2) row-major, t1..t3 and w4 (c3) vectors, b4 one float, all
 * float32 device memory; relu keeps NaN as torch's does.  C a multiple of 16 up to 64; c1, c2, c3
 * multiples of 32 up to 128 (a caller pads narrower layers with zero rows / columns: relu(0) = 0 adds
 * nothing); radius 1..4 — rmd_dicl_match_1x1_supported answers 1 for exactly these (host only), and
 * every other call fails with RMD_ERR_SHAPE.
 *   compute = RMD_BF16X3 : three split-bf16 MFMA products per layer (hi.hi + hi.lo + lo.hi), fp32
 *                          accumulation — the parity mode
 *   compute = RMD_BF16   : one bf16 product per layer
 * The last layer and the biases are fp32 in both.  Hidden activations pass through bfloat16 (hi + lo in
 * the parity mode), so an activation beyond bfloat16's range turns non-finite.  `workspace` holds
 * rmd_dicl_match_1x1_workspace_bytes() bytes (0 = unsupported arguments): the call first repacks the
 * weights into it as MFMA A fragments, so it may be reused by the next call on the same stream.
 * Every output is computed from its own column only, in a fixed order: bitwise reproducible.
 */
int rmd_dicl_match_1x1_supported(int channels, int c1, int c2, int c3, int radius);
size_t rmd_dicl_match_1x1_workspace_bytes(int channels, int c1, int c2, int c3, int compute);
int rmd_dicl_match_1x1(const float* fmap1, const float* fmap2, const float* coords, int batch, int channels,
                       int height, int width, int radius, const float* w1, const float* t1, const float* w2,
                       const float* t2, const float* w3, const float* t3, const float* w4, const float* b4,
                       int c1, int c2, int c3, int compute, float* out, void* workspace, void* stream);

/*
 * Backward of rmd_dicl_match_1x1 (same tensors, shapes and folded parameters; b4 is not needed).  For
 * every column x with upstream scalar g = grad_cost[b, a, bb, p] the forward is recomputed exactly as the
 * forward kernel does it, and with a0 = x, z_l = W_l a_{l-1} + t_l, a_l = relu(z_l):
 *   dz3 = (z3 > 0) ? w4 g : 0         gw4 += a3 g        gb4 += g
 *   da_{l-1} = W_l^T dz_l             dz_{l-1} = (z_{l-1} > 0) ? da_{l-1} : 0
 *   gW_l += dz_l a_{l-1}^T            gt_l += dz_l
 *   grad_fmap1[:, p] += dx[0:C]       grad_fmap2 += bilinear adjoint of dx[C:2C] at the column's taps
 * (zero padding per tap; a non-finite sample position scatters nothing; coordinates carry no gradient).
 * The mask is z > 0 on the recomputed pre-activation, so a NaN pre-activation blocks the gradient as
 * torch's ReLU backward does, while NaN activations still reach the weight gradients through 0 * NaN.
 * Every matrix product is three split-bf16 MFMA products (hi.hi + hi.lo + lo.hi) with fp32 accumulation;
 * dz3, the mask selects, gw4, gb4 and gt_l are fp32 VALU.  Only compute = RMD_BF16X3 has a backward: with
 * one product per layer the recomputed masks differ from the exact ones on 2-4 % of the hidden units, so
 * RMD_BF16 fails with RMD_ERR_ARG.  Supported shapes are the forward's
 * (rmd_dicl_match_1x1_backward_supported, host only).  grad_fmap1 (B, C, h, w) or grad_fmap2 may be NULL
 * to skip a feature gradient; the eight parameter-gradient pointers (shaped like their parameters,
 * grad_b4 one float) are all given or all NULL.  Neither the stack nor a hidden activation or its
 * gradient is written to memory: `workspace` (rmd_dicl_match_1x1_backward_workspace_bytes() bytes, 0 =
 * unsupported arguments) holds the repacked weight fragments, plain and transposed, and one partial of
 * the parameter gradients per workgroup.  grad_fmap1 and all parameter gradients are bitwise
 * reproducible (partials written with plain stores, then added in a fixed order by a second kernel; no
 * float atomics).  grad_fmap2 is zeroed and then accumulated with float atomics, as
 * rmd_dicl_stack_backward's: its last bits depend on the order of the additions.  The launcher never
 * allocates, frees or synchronises, and all argument checks run before any launch.
 */
int rmd_dicl_match_1x1_backward_supported(int channels, int c1, int c2, int c3, int radius);
size_t rmd_dicl_match_1x1_backward_workspace_bytes(int batch, int channels, int height, int width, int radius,
                                                   int c1, int c2, int c3);
int rmd_dicl_match_1x1_backward(const float* grad_cost, const float* fmap1, const float* fmap2, const float* coords,
                                int batch, int channels, int height, int width, int radius, const float* w1,
                                const float* t1, const float* w2, const float* t2, const float* w3, const float* t3,
                                const float* w4, int c1, int c2, int c3, int compute, float* grad_fmap1,
                                float* grad_fmap2, float* grad_w1, float* grad_t1, float* grad_w2, float* grad_t2,
                                float* grad_w3, float* grad_t3, float* grad_w4, float* grad_b4, void* workspace,
                                void* stream);

/*
 * Fused SepConvGRU, inference only: SepConvGru.forward (src/models/impls/raft.py:228-259).  h (B, Hd, H, W),
 * x (B, Xd, H, W), out (B, Hd, H, W), all float32.  One half-step along one axis (axis 0: 1x5 along W with
 * padding (0, 2); axis 1: 5x1 along H with padding (2, 0)) is
 *   hx = [h ; x]    z = sigmoid(Wz * hx + bz)    r = sigmoid(Wr * hx + br)
 *   q = tanh(Wq * [r.h ; x] + bq)                h' = (1 - z) h + z q
 * where * is F.conv2d's cross-correlation (tap t reads position p + t - 2, zero outside the map).
 * rmd_sepconv_gru (raft.py:228-259) runs both halves: weights / biases are host arrays of six device
 * pointers in the order z1, r1, q1 (each (Hd, Hd + Xd, 1, 5)), z2, r2, q2 (each (Hd, Hd + Xd, 5, 1)), biases
 * Hd floats each.  rmd_sepconv_gru_half (raft.py:240-247 for axis 0, 249-256 for axis 1) runs one half with
 * three weights and biases (z, r, q).  Every convolution is an MFMA implicit GEMM whose operands pass
 * through bfloat16:
 *   compute = RMD_BF16X3 : three split-bf16 products (hi.hi + hi.lo + lo.hi), fp32 accumulation — the
 *                          parity mode
 *   compute = RMD_BF16   : one bf16 product
 * Biases, sigmoid, tanh and the gating are fp32 in both.  A NaN input gives NaN in exactly the outputs
 * whose receptive field holds it; a +-inf input gives NaN there in the parity mode (inf - inf in the
 * residual), the one deviation from the reference.  Supported (rmd_sepconv_gru_supported, host only;
 * RMD_ERR_SHAPE otherwise): Hd a multiple of 32 in 32..128, Xd a multiple of 16, Hd + Xd <= 512,
 * (Hd + Xd) H W < 2^30, any B, H, W >= 1.  `out` must not overlap `h` or `x` (RMD_ERR_ARG).  `workspace`
 * holds rmd_sepconv_gru_workspace_bytes() bytes (0 = unsupported arguments) = the packed weights
 * (6 Hd 5 (Hd + Xd) elements x 2 parts x 2 bytes) + three (B, Hd, H, W) fp32 maps (z, r.h, and the h
 * between the halves) + 1024: the call first repacks the weights into it as MFMA A fragments, so it may be
 * reused by the next call on the same stream.  Nothing else is written to memory: no cat, no unfolded
 * tensor, no pre-activation.  The summation order is fixed and a sample's result does not depend on the
 * rest of the batch: bitwise reproducible.  The launcher never allocates, frees or synchronises, reads no
 * environment variable, and all argument checks run before any launch.
 */
int rmd_sepconv_gru_supported(int hidden, int input);
size_t rmd_sepconv_gru_workspace_bytes(int batch, int hidden, int input, int height, int width);
int rmd_sepconv_gru(const float* h, const float* x, const float* const* weights, const float* const* biases,
                    float* out, void* workspace, int batch, int hidden, int input, int height, int width,
                    int compute, void* stream);
int rmd_sepconv_gru_half(const float* h, const float* x, const float* const* weights, const float* const* biases,
                         float* out, void* workspace, int batch, int hidden, int input, int height, int width,
                         int axis, int compute, void* stream);

/*
 * Fused k x k convolution, inference only: the convolutions next to the recurrent unit in RAFT's update block
 * (BasicMotionEncoder raft.py:193-225, FlowHead raft.py:262-273, Up8Network's mask head raft.py:299-331).
 * A stride-1, "same"-padded dense convolution with bias and activation over the channel concatenation of up to
 * two float32 NCHW maps, written into a channel slice of a float32 NCHW destination:
 *   out[b, off + o, y, x] = act(bias[o] + sum_{c,i,j} W[o, c, i, j] in[b, c, y + i - kh/2, x + j - kw/2])
 *   in = cat(in0 (B, C0, H, W), in1 (B, C1, H, W); NULL exactly when C1 = 0), zero outside the map
 * weight (Cout, C0 + C1, kh, kw), bias Cout floats, out (B, out_channels_total, H, W) of which only channels
 * out_offset .. out_offset + Cout - 1 are written (the others are not touched), act 0 = none, 1 = ReLU
 * (v < 0 ? 0 : v: NaN stays NaN, as torch.relu).  An MFMA implicit GEMM whose operands pass through bfloat16:
 * compute = RMD_BF16X3 (three split-bf16 products, the parity mode) or RMD_BF16 (one), bias and activation
 * fp32, as rmd_sepconv_gru.  A NaN input gives NaN in exactly the outputs whose receptive field holds it; a
 * +-inf input gives NaN there in the parity mode (inf - inf in the residual), the one deviation from the
 * reference.  Supported (rmd_conv2d_supported, host only; RMD_ERR_SHAPE otherwise): kh, kw odd in 1..7
 * independently, C0 >= 1, C1 >= 0, C0 + C1 <= 512, Cout in 1..1024 — no channel count needs to be a multiple of
 * anything —, (C0 + C1) H W < 2^30 and out_channels_total H W < 2^30, any B, H, W >= 1.  `out` must not overlap
 * an input, and `workspace` no tensor (RMD_ERR_ARG).  `workspace` holds rmd_conv2d_workspace_bytes() bytes
 * (0 = unsupported arguments) = the packed weights (ceil(Cout / 32) 32 x kh kw x ceil((C0 + C1) / 16) 16
 * elements x 2 parts x 2 bytes) + 256: the call first repacks the weights into it as MFMA A fragments, so it
 * may be reused by the next call on the same stream.  The summation order of an output is fixed and does not
 * depend on the batch, the other tiles or out_offset: bitwise reproducible, per-sample independent.
 *
 * rmd_motion_encoder runs BasicMotionEncoder.forward: flow (B, 2, H, W), corr (B, corr_planes, H, W) ->
 * out (B, 128, H, W); weights / biases are host arrays of five device pointers in the order convc1
 * (256, corr_planes, 1, 1), convc2 (192, 256, 3, 3), convf1 (128, 2, 7, 7), convf2 (64, 128, 3, 3), conv
 * (126, 256, 3, 3).  Five launches of the same kernel over one workspace (the five packed weights + the maps
 * (B, 256, H, W), (B, 128, H, W) and (B, 256, H, W); convc2 and convf2 write channels 0-191 and 192-255 of
 * the last, conv channels 0-125 of out) and a copy of flow into channels 126-127: no cat, no ReLU pass.
 * The launchers never allocate, free or synchronise, read no environment variable, and all argument checks
 * run before any launch.
 */
int rmd_conv2d_supported(int kh, int kw, int c0, int c1, int cout);
size_t rmd_conv2d_workspace_bytes(int c0, int c1, int cout, int kh, int kw);
int rmd_conv2d(const float* in0, const float* in1, const float* weight, const float* bias, float* out,
               void* workspace, int batch, int c0, int c1, int cout, int kh, int kw, int height, int width,
               int out_channels_total, int out_offset, int act, int compute, void* stream);
size_t rmd_motion_encoder_workspace_bytes(int batch, int corr_planes, int height, int width);
int rmd_motion_encoder(const float* flow, const float* corr, const float* const* weights, const float* const* biases,
                       float* out, void* workspace, int batch, int corr_planes, int height, int width, int compute,
                       void* stream);

/*
 * The backward of rmd_conv2d in the parity mode (RMD_BF16X3), for training the same convolutions
 * (BasicMotionEncoder raft.py:193-225, FlowHead raft.py:262-273, Up8Network's mask head raft.py:299-331) under
 * autograd.  With x = cat(in0, in1), y = act(conv(x, W) + b), grad = dL/dy (B, Cout, H, W) and gm = grad where
 * !(y <= 0) and exactly 0 elsewhere (act = 1; a NaN in y keeps the gradient, as torch.relu's backward) or
 * gm = grad (act = 0, y = NULL):
 *   grad_bias[o]           = sum_{b,y,x} gm[b, o, y, x]                          (float64 sums, fixed order)
 *   grad_in[b, c, y, x]    = sum_{o,i,j} W[o, c, i, j] gm[b, o, y - i + kh/2, x - j + kw/2]
 *   grad_weight[o,c,i,j]   = sum_{b,y,x} gm[b, o, y, x] x[b, c, y + i - kh/2, x + j - kw/2]   (zero outside the map)
 * grad_in0 (B, C0, H, W) and grad_in1 (B, C1, H, W) are the two channel ranges of grad_in, written to two tensors.
 * Any of the four outputs may be NULL: that gradient is not computed and its kernels are not launched.  y is
 * NULL exactly when act = 0, in1 exactly when C1 = 0 (grad_in1 must then be NULL).  The data gradient is
 * rmd_conv2d's own kernel over gm behind the flipped, transposed weights (its contraction runs over Cout, up to
 * 1024); the weight gradient is an MFMA GEMM with the pixels on K whose per-slice partials are summed in a fixed
 * order.  Three split-bf16 products, fp32 accumulators, no atomics: bitwise reproducible, and grad_in of one sample
 * does not depend on the others.  A NaN in gm reaches exactly the grad_in positions whose transposed receptive
 * field holds it, and every element of grad_weight[o] and grad_bias[o] of its channel o.
 * Supported (rmd_conv2d_backward_supported, host only): the shapes of rmd_conv2d, with (C0 + C1) H W < 2^30 and
 * Cout H W < 2^30.  No output may overlap an input, another output or the workspace (RMD_ERR_ARG).  `workspace`
 * holds rmd_conv2d_backward_workspace_bytes() bytes (0 = unsupported arguments), whichever outputs are asked for
 *   = gm        align256(4 B Cout H W)
 *   + packed W' for each source of n = C0, C1 > 0 channels: ceil(n / 32) 32 x kh kw x ceil(Cout / 16) 16 elements
 *               x 2 parts x 2 bytes, + align256(4 x 32 ceil(n / 32)) bytes of the zero bias the forward kernel adds
 *   + partials  align256(4 S Cout (C0 + C1) kh kw), S = max(1, min(B H, 32, ceil(1024 / (ceil(Cout / 128)
 *               ceil((C0 + C1) / 32) kh)))) slices of the (image, row) list
 *   + 256
 * and may be reused by the next call on the same stream.  The launcher never allocates, frees or synchronises,
 * reads no environment variable, and all argument checks run before any launch.
 */
int rmd_conv2d_backward_supported(int kh, int kw, int c0, int c1, int cout);
/* The kernels a call with these outputs (non-zero: wanted) launches, in order, separated by spaces: "mask_bias"
 * ("mask_bias+gm" where it writes gm), "pack0 conv0", "pack1 conv1", "wgrad reduce"; "" for no output.  Host only. */
const char* rmd_conv2d_backward_kernels(int want_in0, int want_in1, int want_weight, int want_bias, int act);
size_t rmd_conv2d_backward_workspace_bytes(int batch, int c0, int c1, int cout, int kh, int kw, int height, int width);
int rmd_conv2d_backward(const float* grad, const float* y /* NULL iff act == 0 */, const float* in0, const float* in1,
                        const float* weight, float* grad_in0, float* grad_in1, float* grad_weight, float* grad_bias,
                        void* workspace, int batch, int c0, int c1, int cout, int kh, int kw, int height, int width,
                        int act, void* stream);

/*
 * RAFT's feature / context encoder, inference only: FeatureEncoder (common/encoders/raft/s3.py:8-72) and its
 * ResidualBlock (common/blocks/raft.py:13-46) for the norm types 'none' and 'instance' (eval-mode batch norm
 * arrives folded into the weights and biases: norm none).  All maps float32 NCHW.
 *
 * rmd_conv2d_strided is rmd_conv2d's MFMA implicit GEMM (same compute modes, same NaN / inf behaviour) over one
 * map with a stride, an optional transform on load and an optional residual:
 *   in'[b, c, p]    = scale ? relu(in[b, c, p] scale[b, c] + shift[b, c]) : in[b, c, p]     (fp32, NaN kept)
 *   v               = act(bias[o] + sum_{c,i,j} W[o, c, i, j] in'[b, c, s y + i - kh/2, s x + j - kw/2])
 *   out[b, o, y, x] = residual ? relu(v + residual[b, o, y, x]) : v
 * in (B, C, H, W), weight (Cout, C, kh, kw), out and residual (B, Cout, (H - 1) / s + 1, (W - 1) / s + 1),
 * scale and shift (B, C), both or neither.  Positions outside the map read zero — the padding of the transformed
 * map, not relu(shift).  Supported (rmd_conv2d_strided_supported, host only; RMD_ERR_SHAPE otherwise): kh, kw
 * odd in 1..7, stride 1 or 2, C in 1..512, Cout in 1..1024, C H W < 2^30 and Cout Ho Wo < 2^30.  `workspace`
 * holds rmd_conv2d_strided_workspace_bytes() bytes (the packed weights + 256), as rmd_conv2d's.
 *
 * rmd_instance_stats gives nn.InstanceNorm2d (no affine, no running statistics) in scale / shift form: for every
 * plane (b, c) of x (B, C, H, W), scale = 1 / sqrt(var + eps) with the biased variance and shift = -mean scale,
 * so that norm(x) = x scale + shift.  Mean, then centred squares, accumulated in float64 in a fixed order by one
 * workgroup per plane: no atomics, bitwise reproducible, per-sample independent.  H W = 1 is RMD_ERR_SHAPE
 * (the reference raises there as well).
 *
 * rmd_residual_join: out = relu(xs + relu(ys)), ys = y or y y_scale + y_shift, xs = x or x x_scale + x_shift
 * (the projection's norm, no ReLU); y, x, out (B, C, H, W), the statistics (B, C), a scale with its shift.
 *
 * rmd_feature_encoder runs FeatureEncoder.forward: x (B, 3, H, W) -> out (B, output_dim, H8, W8) with
 * H2 = (H - 1) / 2 + 1, H4 and H8 likewise.  weights / biases are host arrays of 16 device pointers in module
 * order: conv1 (64, 3, 7, 7); per ResidualBlock conv1, conv2 and, in the first block of layer2 and layer3,
 * downsample.0; conv2 (output_dim, 128, 1, 1).  norm = RMD_NORM_NONE: per block the projection if present, conv1
 * with ReLU, conv2 with the ReLU-and-residual epilogue.  norm = RMD_NORM_INSTANCE (eps as nn.InstanceNorm2d's):
 * conv1 raw, its statistics, conv2 normalising on load, its statistics, the same two steps for the projection,
 * the join.  One workspace of rmd_feature_encoder_workspace_bytes() bytes (0 = unsupported arguments): the 16
 * packed weights, six (B, 128) statistics vectors, three maps that every block's input and two results rotate
 * through — B max(64 H2 W2, 96 H4 W4, 128 H8 W8) floats each: the first term wherever the sides still halve, but a
 * side of 1 stays 1 — and one of B max(96 H4 W4, 128 H8 W8) floats for both projections;
 * rmd_feature_encoder_workspace_regions() writes the four sizes (all packed weights, one statistics vector, one
 * map, the projection map; bytes, host only) to regions[0..3].  Supported
 * (rmd_feature_encoder_supported, host only): output_dim in 1..1024, the two norms; with the instance norm
 * H8 W8 > 1.  The launchers never allocate, free or synchronise, read no environment variable, and all argument
 * checks (null pointers, overlaps, the 32-bit offset limits) run before any launch.
 */
#define RMD_NORM_NONE 0
#define RMD_NORM_INSTANCE 1
int rmd_conv2d_strided_supported(int kh, int kw, int stride, int c, int cout);
size_t rmd_conv2d_strided_workspace_bytes(int c, int cout, int kh, int kw);
int rmd_conv2d_strided(const float* in, const float* scale, const float* shift, const float* weight,
                       const float* bias, const float* residual, float* out, void* workspace, int batch, int c,
                       int cout, int kh, int kw, int height, int width, int stride, int act, int compute,
                       void* stream);
int rmd_instance_stats(const float* x, float* scale, float* shift, int batch, int channels, int height, int width,
                       float eps, void* stream);
int rmd_residual_join(const float* y, const float* y_scale, const float* y_shift, const float* x,
                      const float* x_scale, const float* x_shift, float* out, int batch, int channels, int height,
                      int width, void* stream);
int rmd_feature_encoder_supported(int output_dim, int norm);
size_t rmd_feature_encoder_workspace_bytes(int batch, int height, int width, int output_dim);
int rmd_feature_encoder_workspace_regions(int batch, int height, int width, int output_dim, size_t* regions);
int rmd_feature_encoder(const float* x, const float* const* weights, const float* const* biases, float* out,
                        void* workspace, int batch, int height, int width, int output_dim, int norm, float eps,
                        int compute, void* stream);

/*
 * The k x k DICL MatchingNet, inference only: MatchingNet (common/blocks/dicl.py:93-118) — four ConvBlocks
 * (:15-23; 3 x 3 at stride 1, 2, 1, 1), one ConvBlockTransposed (:26-34; 4 x 4, stride 2, padding 1) and a 3 x 3
 * convolution with bias to one channel (:108) — for the norm types 'none' and eval-mode 'batch', which arrives
 * folded into the weights and biases: every block is relu(W' x + t).  All maps float32 NCHW.
 *
 * rmd_mnet_tail computes the last two layers in one kernel; the c4-channel map between them never reaches memory:
 *   u[n, o, Y, X]  = relu(bias5[o] + sum_{c,ky,kx} weight5[c, o, ky, kx] x[n, c, iy, ix])
 *                    over Y = 2 iy - 1 + ky, X = 2 ix - 1 + kx with (iy, ix) inside the map
 *   cost[n, Y, X]  = bias6[0] + sum_{o,i,j} weight6[o, i, j] u[n, o, Y + i - 1, X + j - 1], u zero outside the map
 * x (images, c3, h2, w2), weight5 (c3, c4, 4, 4) in nn.ConvTranspose2d's layout, bias5 c4 floats, weight6 (c4, 3, 3),
 * bias6 one float on the device, cost (images, 2 h2, 2 w2).  Layer 5 runs as four MFMA implicit GEMMs, one per
 * output parity class, whose operands pass through bfloat16: compute = RMD_BF16X3 (three split-bf16 products, the
 * parity mode) or RMD_BF16 (one); bias5 and the ReLU (v < 0 ? 0 : v: NaN stays NaN) are fp32, and layer 6 is fp32
 * in both modes.  A NaN input gives NaN in exactly the outputs whose receptive field holds it; a +-inf input gives
 * NaN there in the parity mode (inf - inf in the residual), the one deviation from the reference.  Supported
 * (rmd_mnet_tail_supported, host only; RMD_ERR_SHAPE otherwise): c3 in 1..64, c4 in 1..32 — neither needs to be a
 * multiple of anything —, h2, w2 >= 1 with c3 h2 w2 < 2^30, any number of images.  `workspace` holds
 * rmd_mnet_tail_workspace_bytes() bytes (0 = unsupported arguments) = the packed weights (4 classes x 4 taps x
 * ceil(c3 / 16) fragments of 1 KiB x 2 parts) + 256: the call first repacks weight5 into it.
 *
 * rmd_matching_net runs the whole network: mvol (images, c_in, h, w) — the displacement stack viewed as in
 * MatchingNet.forward (:111-118) — -> cost (images, h, w).  weights / biases are host arrays of six device
 * pointers: four (Cout, Cin, 3, 3) weights with their Cout-float biases (c_in -> c1 -> c2 -> c2 -> c3), weight5
 * and bias5, weight6 and bias6 as above.  Layers 1-4 are rmd_conv2d_strided's kernel with the ReLU epilogue.  All
 * five weights are packed once per call; then the images are walked in groups of `group` (the last one smaller),
 * five launches per group, over one workspace of rmd_matching_net_workspace_bytes() bytes (0 = unsupported
 * arguments): the five packed weights, then one group's four intermediate maps — group c1 h w, group c2 h/2 w/2
 * twice and group c3 h/2 w/2 floats, each rounded up to 256 bytes — + 256.  A group larger than `images` counts as
 * `images`.  Supported (rmd_matching_net_supported, host only): h and w even (on odd sides the reference's view
 * fails), c_in, c1, c2 in 1..512, c3 and c4 as the tail's, channels x H x W < 2^30 for every map.  Every image's
 * result is independent of the other images and of `group`, bit for bit.  The launchers never allocate, free or
 * synchronise, read no environment variable, and all argument checks (null pointers, overlaps, group < 1, the
 * 32-bit offset limits) run before any launch.
 */
int rmd_mnet_tail_supported(int c3, int c4, int h2, int w2);
size_t rmd_mnet_tail_workspace_bytes(int c3, int c4);
int rmd_mnet_tail(const float* x, const float* weight5, const float* bias5, const float* weight6, const float* bias6,
                  float* cost, void* workspace, int images, int c3, int c4, int h2, int w2, int compute,
                  void* stream);
int rmd_matching_net_supported(int c_in, int c1, int c2, int c3, int c4, int h, int w);
size_t rmd_matching_net_workspace_bytes(int group, int c_in, int c1, int c2, int c3, int c4, int h, int w);
int rmd_matching_net(const float* mvol, const float* const* weights, const float* const* biases, float* cost,
                     void* workspace, int images, int group, int c_in, int c1, int c2, int c3, int c4, int h, int w,
                     int compute, void* stream);

/* Message for the last failing call on this thread ("" if none). */
const char* rmd_last_error(void);

/* Library version string, e.g. "rmd 0.2 gfx950 abi 2". */
const char* rmd_version(void);

/* ABI revision of the exported signatures.  A binding checks it against the RMD_ABI_VERSION of the
 * header it was written for and refuses a mismatch (rmd/_lib.py does).  History:
 *   1  rounds 1-4
 *   2  rmd_corr_grad_gemm gained `compute` (RMD_BF16X3 / RMD_BF16) before `out` (round 5) */
#define RMD_ABI_VERSION 2
int rmd_abi_version(void);

/* Fingerprint of the sources this library was built from (16 hex digits of the sha256 of
 * raft-meets-dicl_amd/csrc/{*.cpp,*.h,*.hip} in name order followed by this header; the Makefile
 * computes it).  Not part of the reference interface: it lets a binding or a test tell a library
 * rebuilt from the tree it sits in from a stale one.  Additive, so the ABI revision stays 2. */
const char* rmd_source_hash(void);

#ifdef __cplusplus
}
#endif

#endif /* RMD_H */
