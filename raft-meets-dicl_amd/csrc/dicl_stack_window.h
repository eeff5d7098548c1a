// dicl_stack_window.h — the LDS window of the stack backward kernels (dicl_stack_backward.hip), written once.
//
// A workgroup's pixels scatter their grad_f2 taps into a few neighbouring rows of the level.  Each window
// kernel declares `__shared__ float win[WIN]` and `__shared__ int wmin` and runs this protocol on them:
//   window_zero     clear the window
//   window_rows     the window starts at the workgroup's lowest row: wy0, and holds wrows = WIN / wl rows
//   Window::add*    a tap inside the window is summed in LDS (ds_add_f32), one outside goes to a global atomic
//   Window::flush   the window is added to grad_f2, one global atomic per non-zero element
// Rows outside the window stay correct, so WIN (kWinSmall or kWinFloats, dicl_stack.h) only affects speed.
// tests/test_dicl_stack_window_single_definition.py keeps the protocol from being copied into a kernel again.
// The statements of a kernel keep their order around these calls: the compiled kernels are those of the
// separate copies (tools/device_asm_diff.py).
#pragma once

#include "dicl_stack.h"

namespace rmd {
namespace {

// one coordinate of a pixel (element i of coords) at the level's scale; CLAMP as make_taps clamps a sample
template <bool CLAMP>
__device__ __forceinline__ float stack_coord(const float* __restrict__ coords, size_t i, float inv_scale) {
    const float c = coords[i] * inv_scale;
    return CLAMP ? fminf(fmaxf(c, -1.0e6f), 1.0e6f) : c;
}

template <int WIN>
__device__ __forceinline__ void window_zero(float (&win)[WIN], int& wmin) {
    if (threadIdx.x == 0) wmin = 1 << 30;
    for (int k = threadIdx.x; k < WIN; k += kThreads) win[k] = 0.f;
    __syncthreads();
}

// ylow: the lowest row a valid lane (pv) adds to, clamped to >= 0
template <int WIN>
__device__ __forceinline__ void window_rows(int& wmin, bool pv, int ylow, const StackParams& P, int& wy0, int& wrows) {
    if (pv) atomicMin(&wmin, ylow);
    __syncthreads();
    wy0 = min(wmin, P.hl);
    wrows = min(P.hl - wy0, WIN / P.wl);
}

// The two targets of an add are two pointer types.  Once the window has passed through a function its pointer
// is generic like the global one, the compiler merges the two branches' adds into one on a selected pointer,
// and every add becomes a flat atomic: 4x the whole kernel (0.96 vs 0.23 ms).  A pointer typed as LDS cannot
// be merged with a global one (tests/test_asm_audit.py::test_dicl_backward_has_no_flat_atomics).
typedef __attribute__((address_space(3))) float lds_float;

template <int WIN>
__device__ __forceinline__ lds_float* lds(float (&win)[WIN]) { return (lds_float*)win; }

__device__ __forceinline__ void add_to(lds_float* p, float v) {      // atomicAdd's own body: ds_add_f32
    __HIP_ATOMIC_BACKWARD_COMPAT_MEMORY { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}

// The window of one (batch, channel) plane g2c of grad_f2, LDS and global targets in separate branches.
// LOW: the row may lie above the window (a lane's lowest row is only an estimate of its taps'); without it
// every row is >= wy0 by construction and the test is left out.  The row test stands in the `if` itself:
// through a helper that returns it the compiler lays the branches out differently.
struct Window {
    float* g2c;
    int wl, wy0, wrows;

    template <bool LOW, int WIN>
    __device__ __forceinline__ void add(float (&win)[WIN], int yy, int xx, float v) const {
        if ((!LOW || yy >= wy0) && yy - wy0 < wrows) add_to(lds(win) + (yy - wy0) * wl + xx, v);
        else atomicAdd(g2c + (size_t)yy * wl + xx, v);
    }

    // the 4 bilinear taps of one sample, gradient gv
    template <int WIN>
    __device__ __forceinline__ void add_taps(float (&win)[WIN], const Taps& t, float gv) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (t.wgt[k] == 0.f) continue;
            const int yy = t.idx[k] / wl;
            if (yy >= wy0 && yy - wy0 < wrows) add_to(lds(win) + (t.idx[k] - wy0 * wl), gv * t.wgt[k]);
            else atomicAdd(g2c + t.idx[k], gv * t.wgt[k]);
        }
    }

    template <int WIN>
    __device__ __forceinline__ void flush(float (&win)[WIN]) const {
        __syncthreads();
        float* gw = g2c + (size_t)wy0 * wl;
        for (int k = threadIdx.x; k < wrows * wl; k += kThreads) {
            const float v = win[k];
            if (v != 0.f) atomicAdd(gw + k, v);
        }
    }
};

// ---- the cross-lane chain of the two-pixel kernels --------------------------------------------------
// link: lane l's joint box (origin oy, ox; merged: gm) continues lane l-1's STEP columns further on the same
// rows (smooth flow).  The wave then sums the overlapping runs with DPP lane shifts and each lane adds only its
// own STEP new columns; a chain's last lane (no link_next) adds its whole tail.
template <int STEP>
__device__ __forceinline__ void chain_links(bool gm, int oy, int ox, bool& link, bool& link_next) {
    const int poy = __builtin_amdgcn_update_dpp((int)0x80000000, oy, 0x138, 0xf, 0xf, false);   // wave_shr:1
    const int pox = __builtin_amdgcn_update_dpp((int)0x80000000, ox, 0x138, 0xf, 0xf, false);
    const int pgm = __builtin_amdgcn_update_dpp(0, (int)gm, 0x138, 0xf, 0xf, false);
    link = gm && pgm != 0 && poy == oy && pox + STEP == ox;
    link_next = __builtin_amdgcn_update_dpp(0, (int)link, 0x130, 0xf, 0xf, false) != 0;      // wave_shl:1
}

}  // namespace
}  // namespace rmd
