// corr_pyramid.h — internal interface of the four correlation GEMMs (corr_pyramid_{w8,stationary,tiled,x3}.hip)
// to their router (corr_pyramid.hip), and the few pieces more than one of them uses.
#pragma once

#include "mfma_bf16.h"

namespace rmd {

// ---- shared pieces -----------------------------------------------------------------------------

constexpr int kKC = 64;      // channel granule: operands are zero-padded to a multiple (the tiled kernel's K chunk)
inline int padded_channels(int C) { return (C + kKC - 1) / kKC * kKC; }

__device__ __forceinline__ unsigned pack_half2(float a, float b) {
    const __half2 h = __floats2half2_rn(a, b);
    return *reinterpret_cast<const unsigned*>(&h);
}

// x of lanes 32-63 <-> y of lanes 0-31
__device__ __forceinline__ void swap32(unsigned& x, unsigned& y) {
    auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    x = r[0];
    y = r[1];
}

// A 16 x 16 target block as 8 MFMA 32x32 tiles (tile 2i + cg = target rows 4i..4i+3 x cols 8cg..8cg+7) in
// accumulators acc[8]: lane (j, h)'s level-0 value for query j at block row `row`, col 8 cg + 4 h + k
#define RMD_ACC(acc, row, cg, k) (acc[2 * ((row) >> 2) + (cg)][((row) & 3) * 4 + (k)])

// ---- the GEMMs ---------------------------------------------------------------------------------
// eligible(): this GEMM handles the call (the router asks in the order x3 | w8, stationary; tiled takes the
// rest).  prepare(): feature maps -> operands in the workspace.  pyramid(): operands -> pyramid.

namespace x3 {   // fp32-accurate split bf16: fp32 / S24 storage, C <= 256, 32-bit store offsets

bool eligible(const rmd_pyramid_desc& d, int channels);
size_t workspace_bytes(const rmd_pyramid_desc& d);
int prepare(const float* fmap1, const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d,
            void* workspace, hipStream_t st);
int pyramid(const rmd_pyramid_desc& d, void* pyramid, void* workspace, hipStream_t st);

}  // namespace x3

namespace w8 {   // bf16, fp16 storage in the tiles layout, C <= 256, 32-bit store offsets

bool eligible(const rmd_pyramid_desc& d, int channels);
int prepare(const float* fmap1, const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d,
            void* workspace, hipStream_t st);
int pyramid(const rmd_pyramid_desc& d, void* pyramid, void* workspace, hipStream_t st);
// the same pyramid without the A operand's round trip through the workspace: prepare_queries() writes the B operand
// only and pyramid_staged() builds its A tiles from fmap2 (fp32) itself
int prepare_queries(const float* fmap1, int channels, const rmd_pyramid_desc& d, void* workspace, hipStream_t st);
int pyramid_staged(const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d, void* pyramid,
                   void* workspace, hipStream_t st);

}  // namespace w8

namespace stationary {   // bf16, fp16 storage in rows, C <= 256, 64-bit addressing; operands by tiled::prepare

bool eligible(const rmd_pyramid_desc& d, int channels);
int pyramid(const rmd_pyramid_desc& d, void* pyramid, void* workspace, hipStream_t st);

}  // namespace stationary

namespace tiled {   // any C; compute RMD_BF16 or RMD_F32 (exact f32 MFMA), storage RMD_F16 or RMD_F32 in rows

int prepare(const float* fmap1, const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d, int compute,
            void* workspace, hipStream_t st);
int pyramid(int channels, float scale, const rmd_pyramid_desc& d, int compute, void* pyramid, void* workspace,
            hipStream_t st);

}  // namespace tiled

}  // namespace rmd
