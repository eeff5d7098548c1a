// dicl_stack_backward.hip — backward of the DICL bilinear displacement stack (dicl_stack.hip).
//
// Replaces (qzed/raft-meets-dicl v2): autograd through the gather/expand/cat of
// corr.dicl.CorrelationModule.forward (src/models/common/corr/dicl.py:26-54, dicl_1x1.py:51-79,
// dicl_emb.py:51-89) and of raft_dicl_ml.CorrelationModule.forward (src/models/impls/raft_dicl_ml.py:294-315),
// i.e. ATen's grid_sampler_2d_backward plus the sum over the expanded f1 copies
//    -> rmd_dicl_stack_backward
//
// grad_f1 is a plain sum over displacements; grad_f2 is a bilinear scatter.  Five kernels sum a workgroup's
// scatter in an LDS window first (dicl_stack_window.h); two fallback kernels scatter straight to global memory.

#include "dicl_stack.h"
#include "dicl_stack_window.h"

namespace rmd {
namespace {

// backward: grad_f1 = sum over displacements of the f1 half (deterministic, no atomics)
__global__ void __launch_bounds__(kThreads)
dicl_stack_grad_f1_kernel(const float* __restrict__ g, StackParams P, float* __restrict__ gf1) {
    const int n = P.h * P.w;
    const int quad = blockIdx.x * kThreads + threadIdx.x;
    const int p0 = quad * 4;
    if (p0 >= n) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const int d = 2 * P.radius + 1, C2 = 2 * P.C + P.extra;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* gp = g + ((size_t)b * d * d * C2 + c) * n + p0;
    for (int disp = 0; disp < d * d; ++disp) {
        const float4 v = *reinterpret_cast<const float4*>(gp + (size_t)disp * C2 * n);
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
    }
    *reinterpret_cast<float4*>(gf1 + ((size_t)b * P.C + c) * n + p0) = s;
}

// backward: grad_f2 = bilinear scatter of the f2 half (float atomics, like grid_sampler backward)
__global__ void __launch_bounds__(kThreads)
dicl_stack_grad_f2_kernel(const float* __restrict__ g, const float* __restrict__ coords, StackParams P,
                          float* __restrict__ gf2) {
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const int d = 2 * P.radius + 1;
    const int disp = blockIdx.y;
    const int a = disp / d, bb = disp - a * d;
    const int b = blockIdx.z;
    const int C = P.C, C2 = 2 * C + P.extra;
    const float px = (coords[(size_t)b * 2 * n + p] * P.inv_scale + (float)(a - P.radius)) * P.sx;
    const float py = (coords[(size_t)b * 2 * n + n + p] * P.inv_scale + (float)(bb - P.radius)) * P.sy;
    const Taps t = make_taps(px, py, P.hl, P.wl);
    const float* gp = g + ((size_t)(b * d * d + disp) * C2 + C) * n + p;
    float* gb = gf2 + (size_t)b * C * nl;
    for (int c = 0; c < C; ++c) {
        const float gv = gp[(size_t)c * n];
        float* gc = gb + (size_t)c * nl;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.wgt[k] != 0.f) atomicAdd(gc + t.idx[k], gv * t.wgt[k]);
    }
}

// backward of the unit-step stack: grad_f1[c,p] = sum of the (2r+1)^2 f1-half gradients (plain
// store); grad_f2 = the f2-half tap gradients spread over p's patch with the forward's separable
// weights (as rmd_corr_lookup_backward).  The patches of a workgroup's 256 consecutive pixels are
// summed in LDS (ds_add_f32) over the row window [wy0, wy0 + wrows) starting at the group's lowest
// patch row; rows past the window go straight to global float atomics; the window is then added
// to grad_f2 once per element.  grid (pixels/256, C, B).
template <int R, int WIN>
__global__ void __launch_bounds__(kThreads)
dicl_stack_patch_backward_kernel(const float* __restrict__ g, const float* __restrict__ coords, StackParams P,
                                 float* __restrict__ gf1, float* __restrict__ gf2) {
    constexpr int D = 2 * R + 1, K = 2 * R + 2;
    __shared__ float win[WIN];
    __shared__ int wmin;
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    const bool pv = p < n;
    float fx = 0.f, fy = 0.f;
    int xs = 0, ys = 1 << 30;
    if (pv) {
        const float cx = stack_coord<true>(coords, (size_t)b * 2 * n + p, P.inv_scale);
        const float cy = stack_coord<true>(coords, (size_t)b * 2 * n + n + p, P.inv_scale);
        const float fx0 = floorf(cx), fy0 = floorf(cy);
        fx = cx - fx0;
        fy = cy - fy0;
        xs = (int)fx0 - R;
        ys = (int)fy0 - R;
    }
    window_zero(win, wmin);
    int wy0, wrows;
    window_rows<WIN>(wmin, pv, max(ys, 0), P, wy0, wrows);
    const int C = P.C, C2 = 2 * C + P.extra;
    const size_t dstride = (size_t)C2 * n;
    float* g2c = gf2 + ((size_t)b * C + c) * nl;
    const Window W{g2c, P.wl, wy0, wrows};
    if (pv) {
        const float* gp = g + (size_t)b * D * D * dstride + p;
        float s1 = 0.f;
        float qprev[K];
#pragma unroll
        for (int i = 0; i < K; ++i) qprev[i] = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            float qcur[K];
            if (j < D) {
                float gr[D];
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    const float* gd = gp + (size_t)(a * D + j) * dstride;
                    s1 += gd[(size_t)c * n];
                    gr[a] = gd[(size_t)(C + c) * n];
                }
#pragma unroll
                for (int i = 0; i < K; ++i)
                    qcur[i] = (i < D ? gr[i] * (1.0f - fx) : 0.f) + (i >= 1 ? gr[i - 1] * fx : 0.f);
            } else {
#pragma unroll
                for (int i = 0; i < K; ++i) qcur[i] = 0.f;
            }
            const int yy = ys + j;
            if (yy >= 0 && yy < P.hl) {
                // this kernel's own row add, LDS and global in separate branches as Window::add: through a shared
                // row form the compiler tests the columns once for both branches (other instruction counts)
                if (yy - wy0 < wrows) {
                    float* r = win + (yy - wy0) * P.wl;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const int xx = xs + i;
                        if (xx >= 0 && xx < P.wl) atomicAdd(r + xx, qcur[i] * (1.0f - fy) + qprev[i] * fy);
                    }
                } else {
                    float* r = g2c + (size_t)yy * P.wl;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const int xx = xs + i;
                        if (xx >= 0 && xx < P.wl) atomicAdd(r + xx, qcur[i] * (1.0f - fy) + qprev[i] * fy);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < K; ++i) qprev[i] = qcur[i];
        }
        gf1[((size_t)b * C + c) * n + p] = s1;
    }
    W.flush(win);
}


// Same backward, 2 pixels per lane, with a GENERAL merge of the lane's two patches: whenever the
// pixels' integer window origins differ by at most 1 row and 2 columns (any smooth flow), the two
// (2r+2)^2 patches are summed in registers over their joint box of (2r+3) rows x (2r+4) columns and
// every lane adds one run of 2r+4 values per joint row.  The round-1 kernel merged only origins exactly one
// column apart and sends every other lane through a per-pixel path of 2 (2r+2) adds per row; because
// a wave executes every path one of its lanes takes, a wave with both kinds paid for both (the
// cost of the LDS atomics, ~100 cycles per ds_add_f32 wave-instruction, is per instruction).  Here
// all lanes of a smooth-flow wave take one path: (2r+3) (2r+4) add instructions per wave instead of
// up to (2r+2) (2r+3) + 2 (2r+2)^2.  Lanes outside the merge condition still add per pixel.  With CH,
// lanes whose joint box continues the previous lane's two columns further on the same rows (smooth
// flow) sum the overlapping runs through DPP lane shifts, so only a chain's last lane adds more than
// its own two new columns (far fewer active lanes per add instruction).
// grid (pixels/512, C, B).
template <int R, int WIN, bool CH>
__global__ void __launch_bounds__(kThreads)
dicl_stack_patch_backward_gm_kernel(const float* __restrict__ g, const float* __restrict__ coords, StackParams P,
                                    float* __restrict__ gf1, float* __restrict__ gf2) {
    constexpr int D = 2 * R + 1, K = 2 * R + 2, PX = 2, MW = K + 2;
    __shared__ float win[WIN];
    __shared__ int wmin;
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int p0 = (blockIdx.x * kThreads + threadIdx.x) * PX;
    const int c = blockIdx.y, b = blockIdx.z;
    const bool pv = p0 < n;               // n % 4 == 0: a lane's PX pixels are all valid or all not
    float fx[PX], fy[PX];
    int xs[PX], ys[PX];
    int ymin = 1 << 30;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        fx[k] = fy[k] = 0.f;
        xs[k] = 0;
        ys[k] = 1 << 30;
        if (pv) {
            const float cx = stack_coord<true>(coords, (size_t)b * 2 * n + p0 + k, P.inv_scale);
            const float cy = stack_coord<true>(coords, (size_t)b * 2 * n + n + p0 + k, P.inv_scale);
            const float fx0 = floorf(cx), fy0 = floorf(cy);
            fx[k] = cx - fx0;
            fy[k] = cy - fy0;
            xs[k] = (int)fx0 - R;
            ys[k] = (int)fy0 - R;
            ymin = min(ymin, max(ys[k], 0));
        }
    }
    // joint box origin and per-pixel offsets inside it
    const int oy = min(ys[0], ys[1]), ox = min(xs[0], xs[1]);
    const int dy0 = ys[0] - oy, dy1 = ys[1] - oy, dx0 = xs[0] - ox, dx1 = xs[1] - ox;
    const bool gm = pv && dy0 + dy1 <= 1 && dx0 + dx1 <= 2;      // |dy| <= 1, |dx| <= 2
    bool link = false, link_next = false;       // CH: the chain of dicl_stack_window.h, two columns per lane
    if constexpr (CH) chain_links<PX>(gm, oy, ox, link, link_next);
    window_zero(win, wmin);
    int wy0, wrows;
    window_rows<WIN>(wmin, pv, ymin, P, wy0, wrows);
    const int C = P.C, C2 = 2 * C + P.extra;
    const size_t dstride = (size_t)C2 * n;
    float* g2c = gf2 + ((size_t)b * C + c) * nl;
    const Window W{g2c, P.wl, wy0, wrows};
    typedef typename FVec<PX>::T v2;
    auto add = [&](int yy, int xx, float v) { W.add<false>(win, yy, xx, v); };
    if (pv) {
        const char* gb = reinterpret_cast<const char*>(g + (size_t)b * D * D * dstride);
        const unsigned lo1 = (unsigned)(((size_t)c * n + p0) * sizeof(float));
        const unsigned lo2 = lo1 + (unsigned)((size_t)C * n * sizeof(float));
        v2 s1 = v2(0.f);
        float qprev[PX][K], vprev[PX][K];
#pragma unroll
        for (int k = 0; k < PX; ++k)
#pragma unroll
            for (int i = 0; i < K; ++i) qprev[k][i] = vprev[k][i] = 0.f;
#pragma unroll 1
        for (int j = 0; j <= K; ++j) {     // patch rows 0..K-1, plus the joint box's extra row K
            float qcur[PX][K];
            if (j < D) {
                v2 gr[D];
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    const char* gd = gb + (size_t)(a * D + j) * dstride * sizeof(float);
                    s1 += *reinterpret_cast<const v2*>(gd + lo1);
                    gr[a] = *reinterpret_cast<const v2*>(gd + lo2);
                }
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int i = 0; i < K; ++i)
                        qcur[k][i] = (i < D ? gr[i][k] * (1.0f - fx[k]) : 0.f) + (i >= 1 ? gr[i - 1][k] * fx[k] : 0.f);
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int i = 0; i < K; ++i) qcur[k][i] = 0.f;
            }
            float val[PX][K];              // patch row j of each pixel (0 for j == K)
#pragma unroll
            for (int k = 0; k < PX; ++k)
#pragma unroll
                for (int i = 0; i < K; ++i) val[k][i] = qcur[k][i] * (1.0f - fy[k]) + qprev[k][i] * fy[k];
            if (gm) {
                // joint row j: pixel k contributes its patch row j - dy_k (this row or the previous one)
                const int yy = oy + j;
                if (yy >= 0 && yy < P.hl) {
                    float mm[MW];
#pragma unroll
                    for (int t = 0; t < MW; ++t) {
                        float m = 0.f;
#pragma unroll
                        for (int k = 0; k < PX; ++k) {
                            const int dyk = k ? dy1 : dy0, dxk = k ? dx1 : dx0;
                            const float* row = dyk ? vprev[k] : val[k];
                            // element t - dx_k of the row, dx_k in {0, 1, 2}
                            const float e0 = t < K ? row[t] : 0.f;
                            const float e1 = (t >= 1 && t - 1 < K) ? row[t - 1] : 0.f;
                            const float e2 = (t >= 2 && t - 2 < K) ? row[t - 2] : 0.f;
                            m += dxk == 0 ? e0 : (dxk == 1 ? e1 : e2);
                        }
                        mm[t] = m;
                    }
                    if constexpr (CH) {
                        // r_t(l) = mm_l[t] + link_l r_{t+2}(l-1): column ox_l + t of the chain
#pragma unroll
                        for (int t = 0; t < MW; ++t) {
                            const int kmax = (MW - 1 - t) / PX;
                            float rr = mm[t + PX * kmax];
#pragma unroll
                            for (int k = kmax - 1; k >= 0; --k) {
                                const float up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(rr), 0x138, 0xf, 0xf, false));
                                rr = mm[t + PX * k] + (link ? up : 0.f);
                            }
                            mm[t] = (t < PX || !link_next) ? rr : 0.f;
                        }
                    }
#pragma unroll
                    for (int t = 0; t < MW; ++t) {
                        const int xx = ox + t;
                        if (xx >= 0 && xx < P.wl && mm[t] != 0.f) add(yy, xx, mm[t]);
                    }
                }
            } else if (j < K) {
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const int yy = ys[k] + j;
                    if (yy < 0 || yy >= P.hl) continue;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const int xx = xs[k] + i;
                        if (xx >= 0 && xx < P.wl) add(yy, xx, val[k][i]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < PX; ++k)
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    qprev[k][i] = qcur[k][i];
                    vprev[k][i] = val[k][i];
                }
        }
        *reinterpret_cast<v2*>(gf1 + ((size_t)b * C + c) * n + p0) = s1;
    }
    W.flush(win);
}

// backward of the general (scaled-grid) stack, raft_dicl_ml levels > 0: every displacement has its
// own bilinear weights, so each lane (pixel p, channel c) walks the (2r+1)^2 displacements, adds its
// f1-half gradients into grad_f1 (plain store) and its 4 f2 taps into the workgroup's LDS window
// (rows [wy0, wy0 + wrows) from the group's lowest tap row; taps past it go to global atomics);
// the window is then added to grad_f2 once per element.  grid (pixels/256, C, B).
template <int WIN>
__global__ void __launch_bounds__(kThreads)
dicl_stack_general_backward_kernel(const float* __restrict__ g, const float* __restrict__ coords, StackParams P,
                                   float* __restrict__ gf1, float* __restrict__ gf2) {
    __shared__ float win[WIN];
    __shared__ int wmin;
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    const bool pv = p < n;
    const int d = 2 * P.radius + 1;
    float cxs = 0.f, cys = 0.f;
    if (pv) {           // not clamped here: make_taps clamps each sample position
        cxs = stack_coord<false>(coords, (size_t)b * 2 * n + p, P.inv_scale);
        cys = stack_coord<false>(coords, (size_t)b * 2 * n + n + p, P.inv_scale);
    }
    window_zero(win, wmin);
    int ylow = 0, wy0, wrows;
    if (pv) {
        // lowest tap row of this pixel: y of displacement bb = 0 (sy >= 0), clamped into the level
        const float py = fminf(fmaxf((cys - (float)P.radius) * P.sy, -1.0e6f), 1.0e6f);
        ylow = min(max((int)floorf(py), 0), P.hl);
    }
    window_rows<WIN>(wmin, pv, ylow, P, wy0, wrows);
    const int C = P.C, C2 = 2 * C + P.extra;
    const size_t dstride = (size_t)C2 * n;
    float* g2c = gf2 + ((size_t)b * C + c) * nl;
    const Window W{g2c, P.wl, wy0, wrows};
    if (pv) {
        const float* gp = g + (size_t)b * d * d * dstride + p;
        float s1 = 0.f;
        for (int a = 0; a < d; ++a) {
            for (int bb = 0; bb < d; ++bb) {
                const float* gd = gp + (size_t)(a * d + bb) * dstride;
                s1 += gd[(size_t)c * n];
                const float gv = gd[(size_t)(C + c) * n];
                const float px = (cxs + (float)(a - P.radius)) * P.sx;
                const float py = (cys + (float)(bb - P.radius)) * P.sy;
                W.add_taps(win, make_taps(px, py, P.hl, P.wl), gv);
            }
        }
        gf1[((size_t)b * C + c) * n + p] = s1;
    }
    W.flush(win);
}

// Separable form of the general backward (scaled grids with 0 <= sx, sy <= 1, raft_dicl_ml levels > 0).
// The x-weights of displacement (a, bb) depend on a only and the y-weights on bb only, so a lane's 81
// f2-half gradients reach a K x K patch as  patch[j][i] = sum_bb wy_bb(j) * sum_a wx_a(i) * g[a][bb]:
// K FMAs per displacement plus K^2 per row bb, all in registers, then K^2 window atomics per lane
// instead of 4 per displacement (324 for r = 4).  A lane whose taps do not fit the patch (fp32
// rounding at an exact span bound) takes the per-tap path, so the result never depends on K.
template <int K, int WIN>
__global__ void __launch_bounds__(kThreads)
dicl_stack_sep_backward_kernel(const float* __restrict__ g, const float* __restrict__ coords, StackParams P,
                               float* __restrict__ gf1, float* __restrict__ gf2) {
    __shared__ float win[WIN];
    __shared__ int wmin;
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    const bool pv = p < n;
    const int d = 2 * P.radius + 1;
    float cxs = 0.f, cys = 0.f;
    if (pv) {
        cxs = stack_coord<true>(coords, (size_t)b * 2 * n + p, P.inv_scale);
        cys = stack_coord<true>(coords, (size_t)b * 2 * n + n + p, P.inv_scale);
    }
    window_zero(win, wmin);
    const float py0 = (cys - (float)P.radius) * P.sy, px0 = (cxs - (float)P.radius) * P.sx;
    const int ybase = (int)floorf(py0), xbase = (int)floorf(px0);
    int wy0, wrows;
    window_rows<WIN>(wmin, pv, min(max(ybase, 0), P.hl), P, wy0, wrows);
    const int C = P.C, C2 = 2 * C + P.extra;
    const size_t dstride = (size_t)C2 * n;
    float* g2c = gf2 + ((size_t)b * C + c) * nl;
    const Window W{g2c, P.wl, wy0, wrows};
    if (pv) {
        const float* gp = g + (size_t)b * d * d * dstride + p;
        // does every tap land inside the K x K patch?
        const float pxl = (cxs + (float)P.radius) * P.sx, pyl = (cys + (float)P.radius) * P.sy;
        const bool fits = (int)floorf(pxl) - xbase <= K - 2 && (int)floorf(pyl) - ybase <= K - 2;
        float s1 = 0.f;
        if (fits) {
            float patch[K][K];
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int i = 0; i < K; ++i) patch[j][i] = 0.f;
            for (int bb = 0; bb < d; ++bb) {
                float row[K];
#pragma unroll
                for (int i = 0; i < K; ++i) row[i] = 0.f;
                for (int a = 0; a < d; ++a) {
                    const float* gd = gp + (size_t)(a * d + bb) * dstride;
                    s1 += gd[(size_t)c * n];
                    const float gv = gd[(size_t)(C + c) * n];
                    const float px = (cxs + (float)(a - P.radius)) * P.sx;
                    const float fx0 = floorf(px);
                    const int rx = (int)fx0 - xbase;
                    const float w1 = (px - fx0) * gv, w0 = gv - w1;
#pragma unroll
                    for (int i = 0; i < K; ++i) row[i] += i == rx ? w0 : (i == rx + 1 ? w1 : 0.f);
                }
                const float py = (cys + (float)(bb - P.radius)) * P.sy;
                const float fy0 = floorf(py);
                const int ry = (int)fy0 - ybase;
                const float fy = py - fy0;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float wy = j == ry ? 1.f - fy : (j == ry + 1 ? fy : 0.f);
#pragma unroll
                    for (int i = 0; i < K; ++i) patch[j][i] = fmaf(wy, row[i], patch[j][i]);
                }
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int yy = ybase + j;
                if (yy < 0 || yy >= P.hl) continue;
                // this kernel's own row add (as the one-pixel patch kernel's: a shared row form compiles differently)
                if (yy >= wy0 && yy - wy0 < wrows) {
                    float* r = win + (yy - wy0) * P.wl;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const int xx = xbase + i;
                        if (xx >= 0 && xx < P.wl && patch[j][i] != 0.f) atomicAdd(r + xx, patch[j][i]);
                    }
                } else {
                    float* r = g2c + (size_t)yy * P.wl;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const int xx = xbase + i;
                        if (xx >= 0 && xx < P.wl && patch[j][i] != 0.f) atomicAdd(r + xx, patch[j][i]);
                    }
                }
            }
        } else {
            for (int a = 0; a < d; ++a) {
                for (int bb = 0; bb < d; ++bb) {
                    const float* gd = gp + (size_t)(a * d + bb) * dstride;
                    s1 += gd[(size_t)c * n];
                    const float gv = gd[(size_t)(C + c) * n];
                    W.add_taps(win, make_taps((cxs + (float)(a - P.radius)) * P.sx, (cys + (float)(bb - P.radius)) * P.sy,
                                              P.hl, P.wl), gv);
                }
            }
        }
        gf1[((size_t)b * C + c) * n + p] = s1;
    }
    W.flush(win);
}

// Separable backward, two pixels per lane with the unit-step kernel's merge: when both pixels' K x K
// patches fit and their origins differ by <= 1 row and <= 2 columns (any smooth flow; at level-1
// scale adjacent pixels' origins move half a column), the patches are summed in registers over their
// joint (K+1) x (K+2) box and, where lane l's box sits one column right of lane l-1's on the same rows
// (the common step: 2 pixels x 0.5), the overlapping runs are summed through DPP lane shifts so each
// lane adds only its one new column (a chain's last lane its whole tail).  Other lanes add per pixel
// (or per tap).  grid (pixels / 512, C, B).
template <int K, int WIN>
__global__ void __launch_bounds__(kThreads)
dicl_stack_sep_backward2_kernel(const float* __restrict__ g, const float* __restrict__ coords, StackParams P,
                                float* __restrict__ gf1, float* __restrict__ gf2) {
    constexpr int PX = 2, MW = K + 2, MH = K + 1;
    __shared__ float win[WIN];
    __shared__ int wmin;
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int p0 = (blockIdx.x * kThreads + threadIdx.x) * PX;
    const int c = blockIdx.y, b = blockIdx.z;
    const bool pv = p0 < n;                       // n % 4 == 0: both pixels valid or neither
    const int d = 2 * P.radius + 1;
    float cxs[PX], cys[PX];
    int xbase[PX], ybase[PX];
    bool fits[PX];
    int ymin = 1 << 30;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        cxs[k] = cys[k] = 0.f;
        if (pv) {
            cxs[k] = stack_coord<true>(coords, (size_t)b * 2 * n + p0 + k, P.inv_scale);
            cys[k] = stack_coord<true>(coords, (size_t)b * 2 * n + n + p0 + k, P.inv_scale);
        }
        ybase[k] = (int)floorf((cys[k] - (float)P.radius) * P.sy);
        xbase[k] = (int)floorf((cxs[k] - (float)P.radius) * P.sx);
        const float pxl = (cxs[k] + (float)P.radius) * P.sx, pyl = (cys[k] + (float)P.radius) * P.sy;
        fits[k] = (int)floorf(pxl) - xbase[k] <= K - 2 && (int)floorf(pyl) - ybase[k] <= K - 2;
        if (pv) ymin = min(ymin, max(ybase[k], 0));
    }
    const int oy = min(ybase[0], ybase[1]), ox = min(xbase[0], xbase[1]);
    const int dy0 = ybase[0] - oy, dy1 = ybase[1] - oy, dx0 = xbase[0] - ox, dx1 = xbase[1] - ox;
    const bool gm = pv && fits[0] && fits[1] && dy0 + dy1 <= 1 && dx0 + dx1 <= 2;
    bool link, link_next;                       // the chain of dicl_stack_window.h, one column per lane
    chain_links<1>(gm, oy, ox, link, link_next);
    window_zero(win, wmin);
    int wy0, wrows;
    window_rows<WIN>(wmin, pv, ymin, P, wy0, wrows);
    const int C = P.C, C2 = 2 * C + P.extra;
    const size_t dstride = (size_t)C2 * n;
    float* g2c = gf2 + ((size_t)b * C + c) * nl;
    const Window W{g2c, P.wl, wy0, wrows};
    auto add = [&](int yy, int xx, float v) { W.add<true>(win, yy, xx, v); };
    typedef typename FVec<PX>::T v2;
    if (pv) {
        const char* gb = reinterpret_cast<const char*>(g + (size_t)b * d * d * dstride);
        const unsigned lo1 = (unsigned)(((size_t)c * n + p0) * sizeof(float));
        const unsigned lo2 = lo1 + (unsigned)((size_t)C * n * sizeof(float));
        v2 s1 = v2(0.f);
        float patch[PX][K][K];
#pragma unroll
        for (int k = 0; k < PX; ++k)
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int i = 0; i < K; ++i) patch[k][j][i] = 0.f;
        const bool any_fit = fits[0] || fits[1];
        for (int bb = 0; bb < d; ++bb) {
            float row[PX][K];
#pragma unroll
            for (int k = 0; k < PX; ++k)
#pragma unroll
                for (int i = 0; i < K; ++i) row[k][i] = 0.f;
            for (int a = 0; a < d; ++a) {
                const char* gd = gb + (size_t)(a * d + bb) * dstride * sizeof(float);
                s1 += *reinterpret_cast<const v2*>(gd + lo1);
                const v2 gv = *reinterpret_cast<const v2*>(gd + lo2);
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    if (fits[k]) {
                        const float px = (cxs[k] + (float)(a - P.radius)) * P.sx;
                        const float fx0 = floorf(px);
                        const int rx = (int)fx0 - xbase[k];
                        const float w1 = (px - fx0) * gv[k], w0 = gv[k] - w1;
#pragma unroll
                        for (int i = 0; i < K; ++i) row[k][i] += i == rx ? w0 : (i == rx + 1 ? w1 : 0.f);
                    } else {                           // per-tap path (fp32 rounding at a span bound)
                        const Taps t = make_taps((cxs[k] + (float)(a - P.radius)) * P.sx,
                                                 (cys[k] + (float)(bb - P.radius)) * P.sy, P.hl, P.wl);
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (t.wgt[q] != 0.f) add(t.idx[q] / P.wl, t.idx[q] % P.wl, gv[k] * t.wgt[q]);
                    }
                }
            }
            if (any_fit) {
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const float py = (cys[k] + (float)(bb - P.radius)) * P.sy;
                    const float fy0 = floorf(py);
                    const int ry = (int)fy0 - ybase[k];
                    const float fy = py - fy0;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const float wy = j == ry ? 1.f - fy : (j == ry + 1 ? fy : 0.f);
#pragma unroll
                        for (int i = 0; i < K; ++i) patch[k][j][i] = fmaf(wy, row[k][i], patch[k][j][i]);
                    }
                }
            }
        }
        if (gm) {
#pragma unroll
            for (int r = 0; r < MH; ++r) {
                const int yy = oy + r;
                if (yy < 0 || yy >= P.hl) continue;
                float mm[MW];
#pragma unroll
                for (int t = 0; t < MW; ++t) {
                    float m = 0.f;
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        // element (r - dy_k, t - dx_k) of pixel k's patch: select among the compile-time
                        // candidates rows {r, r-1} x columns {t, t-1, t-2}
                        const int dyk = k ? dy1 : dy0, dxk = k ? dx1 : dx0;
                        float e[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const int i = t - q;
                            const float a0 = (i >= 0 && i < K && r < K) ? patch[k][r < K ? r : 0][i >= 0 && i < K ? i : 0] : 0.f;
                            const float a1 = (i >= 0 && i < K && r >= 1 && r - 1 < K)
                                                 ? patch[k][r >= 1 && r - 1 < K ? r - 1 : 0][i >= 0 && i < K ? i : 0] : 0.f;
                            e[q] = dyk ? a1 : a0;
                        }
                        m += dxk == 0 ? e[0] : (dxk == 1 ? e[1] : e[2]);
                    }
                    mm[t] = m;
                }
                // r_t(l) = mm_l[t] + link_l r_{t+1}(l-1): column ox_l + t of the chain (its own text: written once
                // with the step as a parameter, the K = 8 kernel compiles to other instruction counts)
#pragma unroll
                for (int t = 0; t < MW; ++t) {
                    const int kmax = MW - 1 - t;
                    float rr = mm[t + kmax];
#pragma unroll
                    for (int q = kmax - 1; q >= 0; --q) {
                        const float up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(rr), 0x138, 0xf, 0xf, false));
                        rr = mm[t + q] + (link ? up : 0.f);
                    }
                    mm[t] = (t < 1 || !link_next) ? rr : 0.f;
                }
#pragma unroll
                for (int t = 0; t < MW; ++t) {
                    const int xx = ox + t;
                    if (xx >= 0 && xx < P.wl && mm[t] != 0.f) add(yy, xx, mm[t]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                if (!fits[k]) continue;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const int yy = ybase[k] + j;
                    if (yy < 0 || yy >= P.hl) continue;
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const int xx = xbase[k] + i;
                        if (xx >= 0 && xx < P.wl && patch[k][j][i] != 0.f) add(yy, xx, patch[k][j][i]);
                    }
                }
            }
        }
        *reinterpret_cast<v2*>(gf1 + ((size_t)b * C + c) * n + p0) = s1;
    }
    W.flush(win);
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" int rmd_dicl_stack_backward(const float* grad_stack, const float* coords, int batch, int channels,
                                       int height, int width, int level_height, int level_width, int radius,
                                       int level, int norm_height, int norm_width, int extra_delta,
                                       float* grad_fmap1, float* grad_fmap2, void* stream) {
    RMD_REQUIRE(grad_stack && coords && grad_fmap1 && grad_fmap2, RMD_ERR_ARG, "rmd_dicl_stack_backward: null pointer");
    StackParams P;
    int rc = stack_params(P, batch, channels, height, width, level_height, level_width, radius, level, norm_height,
                          norm_width, extra_delta);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const int d = 2 * radius + 1;
    const StackBwdRoute route = stack_backward_route(P);
    (void)hipMemsetAsync(grad_fmap2, 0, sizeof(float) * (size_t)batch * channels * level_height * level_width, st);
    const dim3 grid((height * width + kThreads - 1) / kThreads, channels, batch);            // one pixel per lane
    const dim3 grid2((height * width / 2 + kThreads - 1) / kThreads, channels, batch);       // two
// the kernel (its template arguments included, the window size spelled WIN) on GRID with the route's LDS window
#define RMD_WIN(GRID, ...)                                                                                  \
    do {                                                                                                    \
        if (route.small) {                                                                                  \
            constexpr int WIN = kWinSmall;                                                                  \
            __VA_ARGS__<<<GRID, kThreads, 0, st>>>(grad_stack, coords, P, grad_fmap1, grad_fmap2);          \
        } else {                                                                                            \
            constexpr int WIN = kWinFloats;                                                                 \
            __VA_ARGS__<<<GRID, kThreads, 0, st>>>(grad_stack, coords, P, grad_fmap1, grad_fmap2);          \
        }                                                                                                   \
    } while (0)
    switch (route.family) {
        case StackBwdFamily::Patch2:
            switch (route.R) {
#define RMD_CASE(RR) case RR: RMD_WIN(grid2, dicl_stack_patch_backward_gm_kernel<RR, WIN, true>); break;
                RMD_CASE(1) RMD_CASE(2) RMD_CASE(3) RMD_CASE(4)
#undef RMD_CASE
            }
            return check_launch("rmd_dicl_stack_backward/patch2");
        case StackBwdFamily::Patch1:
            switch (route.R) {
#define RMD_CASE(RR) case RR: RMD_WIN(grid, dicl_stack_patch_backward_kernel<RR, WIN>); break;
                RMD_CASE(1) RMD_CASE(2) RMD_CASE(3) RMD_CASE(4)
#undef RMD_CASE
            }
            return check_launch("rmd_dicl_stack_backward/patch");
        case StackBwdFamily::Separable2:
            switch (route.K) {
#define RMD_CASE(KK) case KK: RMD_WIN(grid2, dicl_stack_sep_backward2_kernel<KK, WIN>); break;
                RMD_CASE(4) RMD_CASE(6) RMD_CASE(8)
#undef RMD_CASE
            }
            return check_launch("rmd_dicl_stack_backward/separable2");
        case StackBwdFamily::Separable1:
            RMD_WIN(grid, dicl_stack_sep_backward_kernel<10, WIN>);
            return check_launch("rmd_dicl_stack_backward/separable");
        case StackBwdFamily::General:
            RMD_WIN(grid, dicl_stack_general_backward_kernel<WIN>);
            return check_launch("rmd_dicl_stack_backward/general");
        case StackBwdFamily::Fallback: break;
    }
#undef RMD_WIN
    dim3 g1((height * width / 4 + kThreads - 1) / kThreads, channels, batch);
    dicl_stack_grad_f1_kernel<<<g1, kThreads, 0, st>>>(grad_stack, P, grad_fmap1);
    dim3 g2((height * width + kThreads - 1) / kThreads, d * d, batch);
    dicl_stack_grad_f2_kernel<<<g2, kThreads, 0, st>>>(grad_stack, coords, P, grad_fmap2);
    return check_launch("rmd_dicl_stack_backward");
}
