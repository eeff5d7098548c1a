// encoder.h — the two steps of encoder.hip's strided convolution, for launchers in other files that run several
// convolutions over weights packed once (mnet.hip): pack a weight into MFMA A fragments, and launch sconv_kernel
// on packed fragments.  rmd_conv2d_strided performs the same two steps in sequence.  Internal: not part of the
// C ABI.
#pragma once

#include "rmd_common.h"

namespace rmd {

// bytes of the packed weights of one convolution (both parts, whatever the compute mode): a multiple of 256
size_t sconv_frag_bytes(int c, int cout, int kh, int kw);

// the shape checks of one convolution of entry point `name` (supported kernel, 32-bit offsets inside an image, the
// grid's size): RMD_OK or an error code with the message set.  No pointer is looked at
int sconv_check_shape(const char* name, int batch, int c, int cout, int kh, int kw, int height, int width, int stride);

// weight (Cout, C, kh, kw) -> A fragments at `frags` (256-byte aligned, sconv_frag_bytes() bytes); one launch
void sconv_pack(const float* weight, void* frags, int c, int cout, int kh, int kw, int compute, hipStream_t st);

// out (B, Cout, Ho, Wo) = act(bias + conv(in (B, C, H, W))) on fragments packed for the same `compute`; no load
// transform, no residual; one launch.  The arguments have passed sconv_check_shape
void sconv_packed(const float* in, const void* frags, const float* bias, float* out, int batch, int c, int cout, int kh,
                  int kw, int height, int width, int stride, int act, int compute, hipStream_t st);

}  // namespace rmd
