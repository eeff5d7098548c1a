// conv_internal.h — what conv_backward.hip borrows from conv.hip: the forward GEMM kernel behind weights that
// the caller packed itself.  conv.hip's kernels stay in its translation unit; this is a host-side door to them.
#pragma once

#include "rmd_common.h"

namespace rmd {

// contraction channels the internal launch accepts.  rmd_conv2d's public limit (C0 + C1 <= 512) is an acceptance
// limit of conv_supported(): conv_kernel loops over P.C in chunks, indexes the fragments with size_t and holds no
// table sized by it, so the kernel itself only needs channels x H x W < 2^30 (its 32-bit offsets inside an image).
constexpr int kConvInternalMaxC = 1024;

// bytes of the A fragments of a (cout, c, kh, kw) weight in conv_pack_kernel's layout, both parts
size_t conv_fragment_bytes(int c, int cout, int kh, int kw);

// out (B, cout, H, W) = the "same" convolution of in (B, c, H, W) with the A fragments at `frags` (conv.hip's
// layout: fragment (m taps + t) ks + k, hi parts then lo parts) + bias, no activation, three split-bf16 products:
// conv_kernel<3, MT, KC> as rmd_conv2d launches it.  No checks: the caller made them (c <= kConvInternalMaxC,
// cout <= 1024, c H W and cout H W < 2^30).
void conv_run_prepacked(const float* in, const void* frags, const float* bias, float* out, int batch, int c, int cout,
                        int kh, int kw, int height, int width, hipStream_t st);

}  // namespace rmd
