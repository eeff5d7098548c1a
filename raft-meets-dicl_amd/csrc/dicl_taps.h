// dicl_taps.h — the bilinear taps of one DICL sample position, shared by the stack kernels (dicl_stack.hip,
// dicl_stack_backward.hip) and the fused dicl-1x1 cost (dicl_match.hip, dicl_match_grad.hip): every kernel
// that gathers from fmap2 or scatters into its gradient means the same sample by it.
#pragma once

#include "rmd_common.h"

namespace rmd {

// bilinear, align_corners=True, zero padding per tap: the 4 taps of one sample position
struct Taps {
    int idx[4];
    float wgt[4];
};

__device__ __forceinline__ Taps make_taps(float px, float py, int hl, int wl) {
    Taps t;
    px = fminf(fmaxf(px, -1.0e6f), 1.0e6f);
    py = fminf(fmaxf(py, -1.0e6f), 1.0e6f);
    const float fx0 = floorf(px), fy0 = floorf(py);
    const float fx = px - fx0, fy = py - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
        const bool ok = xx >= 0 && xx < wl && yy >= 0 && yy < hl;
        const float wx = (k & 1) ? fx : 1.f - fx;
        const float wy = (k >> 1) ? fy : 1.f - fy;
        t.idx[k] = ok ? yy * wl + xx : 0;
        t.wgt[k] = ok ? wx * wy : 0.f;
    }
    return t;
}

// Forward only: a sample position that is not finite (a NaN or +-inf coordinate, a non-finite grid
// scale) samples NaN, as the reference's grid_sample does; make_taps alone clamps it far outside the
// map (fmaxf drops a NaN) and would sample zeros.  The backward keeps make_taps: such a position has
// no tap inside the map and contributes nothing to grad_fmap2.
__device__ __forceinline__ Taps make_taps_fwd(float px, float py, int hl, int wl) {
    Taps t = make_taps(px, py, hl, wl);
    if (!(__builtin_isfinite(px) && __builtin_isfinite(py))) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t.idx[k] = 0;
            t.wgt[k] = __builtin_nanf("");
        }
    }
    return t;
}

}  // namespace rmd
