// dicl_stack.hip — DICL displacement-invariant cost-volume construction: the bilinear displacement stack,
// forward.  The backward is dicl_stack_backward.hip.
//
// Replaces (qzed/raft-meets-dicl v2):
//  * corr.dicl.CorrelationModule.forward gather/expand/cat  src/models/common/corr/dicl.py:26-54
//    (same in dicl_1x1.py:51-79; dicl_emb.py:51-89 adds the 2 displacement channels) and the
//    per-level gather of raft_dicl_ml.CorrelationModule.forward (src/models/impls/raft_dicl_ml.py:294-315)
//    -> rmd_dicl_stack
//
// An HBM-bound byte mover: one lane owns 4 consecutive pixels of one displacement plane, so
// every store is a 16-byte-per-lane, fully coalesced row of the contiguous (B, du, dv, 2C(+2), h, w)
// MatchingNet input; the f1 half is re-read from L2 per displacement.

#include "dicl_stack.h"

namespace rmd {
namespace {

// grid: (pixel quads, d*d, B); one lane = 4 consecutive pixels of one displacement plane.  The
// channel loop is unrolled by U so a lane's f1 row loads and 16 U bilinear taps are in flight
// before its 2 U stores; stores are non-temporal (the volume is written once, read by MatchingNet).
template <bool NT, int U>
__global__ void __launch_bounds__(kThreads)
dicl_stack_kernel(const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ coords,
                  StackParams P, float* __restrict__ out) {
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int quad = blockIdx.x * kThreads + threadIdx.x;
    const int p0 = quad * 4;
    if (p0 >= n) return;
    const int d = 2 * P.radius + 1;
    const int disp = blockIdx.y;                 // a * d + bb
    const int a = disp / d, bb = disp - a * d;
    const int b = blockIdx.z;
    const int C = P.C, C2 = 2 * C + P.extra;
    const float* cx = coords + (size_t)b * 2 * n;
    const float* cy = cx + n;
    Taps t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k;
        const float px = (cx[p] * P.inv_scale + (float)(a - P.radius)) * P.sx;
        const float py = (cy[p] * P.inv_scale + (float)(bb - P.radius)) * P.sy;
        t[k] = make_taps_fwd(px, py, P.hl, P.wl);
    }
    float* o = out + ((size_t)(b * d * d + disp) * C2) * n + p0;
    const float* f1b = f1 + (size_t)b * C * n + p0;
    const float* f2b = f2 + (size_t)b * C * nl;
    for (int c0 = 0; c0 < C; c0 += U) {
        f4_t a1[U], v2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u < C) {
                const float* f2c = f2b + (size_t)(c0 + u) * nl;
                a1[u] = *reinterpret_cast<const f4_t*>(f1b + (size_t)(c0 + u) * n);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    v2[u][k] = t[k].wgt[0] * f2c[t[k].idx[0]] + t[k].wgt[1] * f2c[t[k].idx[1]] +
                               t[k].wgt[2] * f2c[t[k].idx[2]] + t[k].wgt[3] * f2c[t[k].idx[3]];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u < C) {
                st4<NT>(o + (size_t)(c0 + u) * n, a1[u]);
                st4<NT>(o + (size_t)(C + c0 + u) * n, v2[u]);
            }
        }
    }
    if (P.extra) {       // dicl_emb.py:81-85: delta (dx = a-r, dy = bb-r) as two constant channels
        const float dx = (float)(a - P.radius), dy = (float)(bb - P.radius);
        *reinterpret_cast<float4*>(o + (size_t)(2 * C) * n) = make_float4(dx, dx, dx, dx);
        *reinterpret_cast<float4*>(o + (size_t)(2 * C + 1) * n) = make_float4(dy, dy, dy, dy);
    }
}

// Scaled-grid forward (raft_dicl_ml levels > 0, sx, sy < 1): displacement (a, bb) samples
// x = (cx + a - r) sx, y = (cy + bb - r) sy, so all (2r+1)^2 samples of a pixel lie in a K x K
// integer patch (K = floor(2 r s) + 2, rounded up to even) and the x weights depend on a only, the
// y weights on bb only.  One lane per (pixel, channel) loads the patch once (K^2 loads instead of
// 4 (2r+1)^2 gathers), interpolates along x into K row values per a, then along y with per-bb
// weight vectors held in registers; lanes whose samples leave the patch (fp32 rounding at an
// exact span bound) fall back to the per-tap formula.  Stores: wave-uniform plane base + 32-bit
// lane offset, non-temporal.  grid (pixels/256, C, B).
template <int R, int K, bool NT>
__global__ void __launch_bounds__(kThreads)
dicl_stack_sep_kernel(const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ coords,
                      StackParams P, float* __restrict__ out) {
    constexpr int D = 2 * R + 1;
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (p >= n) return;
    const float cxr = coords[(size_t)b * 2 * n + p] * P.inv_scale, cyr = coords[(size_t)b * 2 * n + n + p] * P.inv_scale;
    // a NaN or +-inf coordinate: the pixel's whole window is NaN (grid_sample); the clamp below would
    // turn it into a far-away finite one (fmaxf drops a NaN) and the window into zeros
    const bool finite = __builtin_isfinite(cxr) && __builtin_isfinite(cyr);
    const float cxs = fminf(fmaxf(cxr, -1.0e6f), 1.0e6f);
    const float cys = fminf(fmaxf(cyr, -1.0e6f), 1.0e6f);
    const int xbase = (int)floorf((cxs - (float)R) * P.sx), ybase = (int)floorf((cys - (float)R) * P.sy);
    int rx[D], ry[D];
    float fxa[D], fyb[D];
    bool fits = true;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const float px = fminf(fmaxf((cxs + (float)(a - R)) * P.sx, -1.0e6f), 1.0e6f);
        const float py = fminf(fmaxf((cys + (float)(a - R)) * P.sy, -1.0e6f), 1.0e6f);
        const float x0 = floorf(px), y0 = floorf(py);
        rx[a] = (int)x0 - xbase;
        ry[a] = (int)y0 - ybase;
        fxa[a] = px - x0;
        fyb[a] = py - y0;
        fits = fits && rx[a] >= 0 && rx[a] <= K - 2 && ry[a] >= 0 && ry[a] <= K - 2;
    }
    const int C = P.C, C2 = 2 * C + P.extra;
    const size_t dstride = (size_t)C2 * n;
    float* const ob = out + (size_t)b * D * D * dstride;
    const unsigned lo1 = (unsigned)(((size_t)c * n + p) * sizeof(float));
    const unsigned lo2 = lo1 + (unsigned)((size_t)C * n * sizeof(float));
    const float v1 = f1[((size_t)b * C + c) * n + p];
    const float* f2c = f2 + ((size_t)b * C + c) * nl;
    auto put = [&](int a, int bb, float v) {
        char* od = reinterpret_cast<char*>(ob + (size_t)(a * D + bb) * dstride);
        v = finite ? v : __builtin_nanf("");
        if constexpr (NT) {
            __builtin_nontemporal_store(v1, reinterpret_cast<float*>(od + lo1));
            __builtin_nontemporal_store(v, reinterpret_cast<float*>(od + lo2));
        } else {
            *reinterpret_cast<float*>(od + lo1) = v1;
            *reinterpret_cast<float*>(od + lo2) = v;
        }
    };
    if (fits) {
        float patch[K][K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int yy = ybase + j;
            const bool rok = yy >= 0 && yy < P.hl;
            const int roff = min(max(yy, 0), P.hl - 1) * P.wl;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int xx = xbase + i;
                const float e = f2c[roff + min(max(xx, 0), P.wl - 1)];
                patch[j][i] = (rok && xx >= 0 && xx < P.wl) ? e : 0.f;
            }
        }
        float wy[D][K];                 // y weights of displacement row bb over the patch rows
#pragma unroll
        for (int bb = 0; bb < D; ++bb)
#pragma unroll
            for (int j = 0; j < K; ++j) wy[bb][j] = j == ry[bb] ? 1.f - fyb[bb] : (j == ry[bb] + 1 ? fyb[bb] : 0.f);
#pragma unroll
        for (int a = 0; a < D; ++a) {
            float col[K];               // the patch interpolated along x at displacement a, per row
#pragma unroll
            for (int j = 0; j < K; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const float wx = i == rx[a] ? 1.f - fxa[a] : (i == rx[a] + 1 ? fxa[a] : 0.f);
                    acc = fmaf(wx, patch[j][i], acc);
                }
                col[j] = acc;
            }
#pragma unroll
            for (int bb = 0; bb < D; ++bb) {
                float v = 0.f;
#pragma unroll
                for (int j = 0; j < K; ++j) v = fmaf(wy[bb][j], col[j], v);
                put(a, bb, v);
            }
        }
    } else {
        for (int a = 0; a < D; ++a)
            for (int bb = 0; bb < D; ++bb) {
                const Taps t = make_taps((cxs + (float)(a - R)) * P.sx, (cys + (float)(bb - R)) * P.sy, P.hl, P.wl);
                put(a, bb, t.wgt[0] * f2c[t.idx[0]] + t.wgt[1] * f2c[t.idx[1]] + t.wgt[2] * f2c[t.idx[2]] +
                               t.wgt[3] * f2c[t.idx[3]]);
            }
    }
    if (P.extra && c == 0) {       // dicl_emb.py:81-85: delta (dx = a-r, dy = bb-r) as two constant channels
        for (int a = 0; a < D; ++a)
            for (int bb = 0; bb < D; ++bb) {
                float* od = ob + (size_t)(a * D + bb) * dstride + p;
                od[(size_t)(2 * C) * n] = (float)(a - R);
                od[(size_t)(2 * C + 1) * n] = (float)(bb - R);
            }
    }
}

// ---- unit-step fast path ---------------------------------------------------------------------
// When the sample grid has unit steps (sx = sy = 1: corr/dicl.py and every same-size call), the
// (2r+1)^2 displacements of pixel p sample (x_p + a - r, y_p + b - r) with ONE fractional weight
// set, so together they read exactly the (2r+2)^2 integer patch [x0-r, x0+r+1] x [y0-r, y0+r+1]
// (as the RAFT lookup).  One lane per pixel, all displacements, a loop over channels: per channel
// the patch is read once (instead of 4 taps x (2r+1)^2 gathers), interpolated separably (x, then y)
// and the (2r+1)^2 f2 values plus the f1 copies are stored as coalesced 256-B wave rows.
template <int R, int PX, bool NT>
__global__ void __launch_bounds__(kThreads)
dicl_stack_patch_kernel(const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ coords,
                        StackParams P, int nxb, int remap, float* __restrict__ out) {
    // PX consecutive pixels per lane (each with its own patch) so every store is a PX-float vector
    // (PX * 256 B per wave-instruction); one channel per thread: 1-D grid of (pixels / 256 PX) x C x B
    // blocks, optionally remapped so an XCD works on one batch image.  Product PX = 1: 56 VGPRs at
    // r = 4, 7 waves per SIMD, the most stores in flight (PX = 2 needs ~106 VGPRs, PX = 4 ~200).
    typedef typename FVec<PX>::T V;
    constexpr int D = 2 * R + 1, K = 2 * R + 2;
    const int n = P.h * P.w, nl = P.hl * P.wl;
    const int lid = remap ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int xb = lid % nxb, rest = lid / nxb;
    const int c = rest % P.C, b = rest / P.C;
    const int p0 = (xb * kThreads + threadIdx.x) * PX;
    if (p0 >= n) return;
    float fx[PX], fy[PX];
    int xs[PX], ys[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        float cx = coords[(size_t)b * 2 * n + p0 + k] * P.inv_scale;
        float cy = coords[(size_t)b * 2 * n + n + p0 + k] * P.inv_scale;
        // a NaN or +-inf coordinate: NaN weights make the pixel's whole window NaN (grid_sample), at no
        // cost in the store loop; the clamp alone turns it into a far-away finite coordinate (fmaxf
        // drops a NaN) and the window into zeros
        const bool finite = __builtin_isfinite(cx) && __builtin_isfinite(cy);
        cx = fminf(fmaxf(cx, -1.0e6f), 1.0e6f);
        cy = fminf(fmaxf(cy, -1.0e6f), 1.0e6f);
        const float fx0 = floorf(cx), fy0 = floorf(cy);
        fx[k] = finite ? cx - fx0 : __builtin_nanf("");
        fy[k] = finite ? cy - fy0 : __builtin_nanf("");
        xs[k] = (int)fx0 - R;
        ys[k] = (int)fy0 - R;
    }
    const int C = P.C, C2 = 2 * C + P.extra;
    const size_t dstride = (size_t)C2 * n;                       // next displacement plane
    float* o = out + (size_t)b * D * D * dstride + p0;
    // stores: wave-uniform plane base + one 32-bit lane offset (saddr + voffset addressing; the
    // host checks that a batch image's volume stays below 4 GiB), so the 2 D^2 store addresses
    // cost no VGPRs
    float* const ob = out + (size_t)b * D * D * dstride;
    const unsigned lo1 = (unsigned)(((size_t)c * n + p0) * sizeof(float));
    const unsigned lo2 = lo1 + (unsigned)((size_t)C * n * sizeof(float));
    const V v1 = *reinterpret_cast<const V*>(f1 + ((size_t)b * C + c) * n + p0);
    const float* f2c = f2 + ((size_t)b * C + c) * nl;
    float hprev[PX][D];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        float hcur[PX][D];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const int yy = ys[k] + j;
            const bool rok = yy >= 0 && yy < P.hl;
            const unsigned roff = (unsigned)(min(max(yy, 0), P.hl - 1) * P.wl);
            float v[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int xx = xs[k] + i;
                const float e = f2c[roff + (unsigned)min(max(xx, 0), P.wl - 1)];
                v[i] = (rok && xx >= 0 && xx < P.wl) ? e : 0.f;
            }
#pragma unroll
            for (int a = 0; a < D; ++a) hcur[k][a] = fmaf(fx[k], v[a + 1] - v[a], v[a]);
        }
        if (j > 0) {
            const int bb = j - 1;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                char* od = reinterpret_cast<char*>(ob + (size_t)(a * D + bb) * dstride);
                stv<NT>(reinterpret_cast<float*>(od + lo1), v1);
                V r;
#pragma unroll
                for (int k = 0; k < PX; ++k) r[k] = fmaf(fy[k], hcur[k][a] - hprev[k][a], hprev[k][a]);
                stv<NT>(reinterpret_cast<float*>(od + lo2), r);
            }
        }
#pragma unroll
        for (int k = 0; k < PX; ++k)
#pragma unroll
            for (int a = 0; a < D; ++a) hprev[k][a] = hcur[k][a];
    }
    if (P.extra && c == 0) {       // dicl_emb.py:81-85: delta (dx = a-r, dy = bb-r) as two constant channels
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int bb = 0; bb < D; ++bb) {
                float* od = o + (size_t)(a * D + bb) * dstride;
                const float dx = (float)(a - R), dy = (float)(bb - R);
                *reinterpret_cast<V*>(od + (size_t)(2 * C) * n) = V(dx);
                *reinterpret_cast<V*>(od + (size_t)(2 * C + 1) * n) = V(dy);
            }
    }
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" const char* rmd_dicl_stack_kernel(int batch, int channels, int height, int width, int level_height,
                                             int level_width, int radius, int level, int norm_height,
                                             int norm_width, int extra_delta, int backward) {
    StackParams P;
    if (stack_params(P, batch, channels, height, width, level_height, level_width, radius, level, norm_height,
                     norm_width, extra_delta))
        return "invalid";
    const RouteNames& t = route_names(backward != 0);
    const char* name = t.find(backward ? route_name(stack_backward_route(P)) : route_name(stack_route(P)));
    return name ? name : "invalid";
}

extern "C" const char* rmd_dicl_stack_kernel_list(int backward) { return route_names(backward != 0).joined.c_str(); }

extern "C" int rmd_dicl_stack(const float* fmap1, const float* fmap2, const float* coords, int batch, int channels,
                              int height, int width, int level_height, int level_width, int radius, int level,
                              int norm_height, int norm_width, int extra_delta, float* out, void* stream) {
    RMD_REQUIRE(fmap1 && fmap2 && coords && out, RMD_ERR_ARG, "rmd_dicl_stack: null pointer");
    StackParams P;
    int rc = stack_params(P, batch, channels, height, width, level_height, level_width, radius, level, norm_height,
                          norm_width, extra_delta);
    if (rc) return rc;
    const int d = 2 * radius + 1;
    hipStream_t st = as_stream(stream);
    const StackRoute route = stack_route(P);
    switch (route.family) {
        case StackFamily::Patch: {
            // Measured at cfg4 (profiles/dicl_ab_r01.json, dicl_px_ab_r02.json): non-temporal stores are the
            // win (0.33 -> 0.26 ms); one pixel per lane (56 VGPRs, 7 waves per SIMD instead of 4 with 2 or 4
            // pixels per lane) keeps more stores in flight: 0.238 vs 0.256 ms; an XCD remap changes nothing
            constexpr int px = 1;
            const int nxb = (height * width / px + kThreads - 1) / kThreads;
            const long long nwg = (long long)nxb * channels * batch;
            RMD_REQUIRE(nwg < (1ll << 31), RMD_ERR_SHAPE, "rmd_dicl_stack: grid too large");
            constexpr int remap = 0;
            switch (route.R) {
#define RMD_CASE(RR) case RR: \
                dicl_stack_patch_kernel<RR, px, true><<<(unsigned)nwg, kThreads, 0, st>>>(fmap1, fmap2, coords, P, nxb, remap, out); \
                break;
                RMD_CASE(1) RMD_CASE(2) RMD_CASE(3) RMD_CASE(4)
#undef RMD_CASE
            }
            return check_launch("rmd_dicl_stack/patch");
        }
        case StackFamily::Separable: {
            dim3 g1((height * width + kThreads - 1) / kThreads, channels, batch);
            switch (route.R * 100 + route.K) {
#define RMD_SCASE(RR, KK) case RR * 100 + KK: dicl_stack_sep_kernel<RR, KK, true><<<g1, kThreads, 0, st>>>(fmap1, fmap2, coords, P, out); break;
                RMD_SCASE(3, 4) RMD_SCASE(3, 6) RMD_SCASE(3, 8) RMD_SCASE(4, 4) RMD_SCASE(4, 6) RMD_SCASE(4, 8)
#undef RMD_SCASE
            }
            return check_launch("rmd_dicl_stack/separable");
        }
        case StackFamily::General: break;
    }
    dim3 grid((height * width / 4 + kThreads - 1) / kThreads, d * d, batch);
    dicl_stack_kernel<true, 1><<<grid, kThreads, 0, st>>>(fmap1, fmap2, coords, P, out);
    return check_launch("rmd_dicl_stack");
}
