// dicl_int.hip — the DICL baseline's integer-displacement volume with its occlusion mask, and the backward
// warp that feeds it.
//
// Replaces (qzed/raft-meets-dicl v2):
//  * FlowLevel.compute_cost volume build + occlusion mask   src/models/impls/dicl.py:212-238
//    -> rmd_dicl_stack_int / rmd_dicl_stack_int_backward
//  * warp_backwards (grid_sample of the image and of a ones mask)   src/models/common/warp.py:5-33
//    -> rmd_warp_backwards / rmd_warp_backwards_backward
//  * FlowLevel.forward's warp followed by compute_cost       src/models/impls/dicl.py:178-181 -> 212-238
//    -> rmd_dicl_stack_int_warped / rmd_dicl_stack_int_warped_backward (the warp writes the occlusion
//       flags, so the two kernel groups live in one file)
//
// The volume is an HBM-bound byte mover like the bilinear stack: one lane owns 4 consecutive
// pixels of one displacement plane, every store a 16-byte-per-lane coalesced row.

#include "dicl_stack.h"      // kThreads, f4_t, st4

namespace rmd {
namespace {

// ---- DICL baseline integer volume ------------------------------------------------------------
struct IntParams {
    int B, C, h, w, ru, rv;
};

// occlusion mask of dicl.py:236-237 depends only on the displaced f2 pixel: nz = sum_c f2 != 0
__global__ void __launch_bounds__(kThreads)
dicl_nz_kernel(const float* __restrict__ f2, IntParams P, unsigned char* __restrict__ nz) {
    const int n = P.h * P.w;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const int b = blockIdx.y;
    const float* f = f2 + (size_t)b * P.C * n + p;
    float s = 0.f;
    for (int c = 0; c < P.C; ++c) s += f[(size_t)c * n];
    nz[(size_t)b * n + p] = s != 0.f;
}

// Integer volume (impls/dicl.py:212-238), written for the write stream: a 1-D grid remapped per
// XCD (one batch image's f1/f2 — 2 x 1.5 MB at cfg3 level 2 — stay in that XCD's L2 while its 49
// displacement planes re-read them), the channel loop unrolled by U so a lane's loads of U channels
// are all in flight before its 2U stores, and optionally non-temporal stores (the 1.2 GB volume is
// written once and read by the next kernel, never by this one).
template <int CT, bool NT, int WPE = 1>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WPE)))
dicl_stack_int_v2_kernel(const float* __restrict__ f1, const float* __restrict__ f2,
                         const unsigned char* __restrict__ nz, IntParams P, int nqb, int remap,
                         float* __restrict__ out) {
    constexpr int U = 8;
    const int n = P.h * P.w;
    const int dv = 2 * P.rv + 1, ndisp = (2 * P.ru + 1) * dv;
    const int lid = remap ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int xb = lid % nqb, rest = lid / nqb;
    const int disp = rest % ndisp, b = rest / ndisp;
    const int p0 = (xb * kThreads + threadIdx.x) * 4;
    if (p0 >= n) return;
    const int i = disp / dv, jj = disp - i * dv;
    const int di = i - P.ru, dj = jj - P.rv;
    int src[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k;
        const int y = p / P.w, x = p - y * P.w;
        const int xx = x + di, yy = y + dj;
        const bool inb = xx >= 0 && xx < P.w && yy >= 0 && yy < P.h;
        src[k] = inb ? yy * P.w + xx : 0;
        ok[k] = inb && nz[(size_t)b * n + src[k]];
    }
    const int C = CT ? CT : P.C;
    float* o = out + ((size_t)(b * ndisp + disp) * 2 * C) * n + p0;
    const float* f1b = f1 + (size_t)b * C * n + p0;
    const float* f2b = f2 + (size_t)b * C * n;
#pragma unroll 4
    for (int c0 = 0; c0 < C; c0 += U) {
        f4_t a[U], v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (CT || c0 + u < C) {
                const float* f2c = f2b + (size_t)(c0 + u) * n;
                a[u] = *reinterpret_cast<const f4_t*>(f1b + (size_t)(c0 + u) * n);
                v[u] = f4_t{f2c[src[0]], f2c[src[1]], f2c[src[2]], f2c[src[3]]};
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (CT || c0 + u < C) {
                const f4_t m1{ok[0] ? a[u].x : 0.f, ok[1] ? a[u].y : 0.f, ok[2] ? a[u].z : 0.f, ok[3] ? a[u].w : 0.f};
                const f4_t m2{ok[0] ? v[u].x : 0.f, ok[1] ? v[u].y : 0.f, ok[2] ? v[u].z : 0.f, ok[3] ? v[u].w : 0.f};
                st4<NT>(o + (size_t)(c0 + u) * n, m1);
                st4<NT>(o + (size_t)(C + c0 + u) * n, m2);
            }
        }
    }
}

// launch the integer volume (nz already computed).  Measured at cfg3 (profiles/dicl_ab_r01.json): 0.366 ms
// for the first formulation (3-D grid, rolled channel loop) -> 0.234 ms (unrolled, non-temporal stores,
// no XCD remap); 8 waves per SIMD forced is slower (0.235 ms, profiles/dicl_int_wpe_ab_r02.json)
int launch_stack_int(const float* fmap1, const float* fmap2, const unsigned char* nz, const IntParams& P,
                     float* out, hipStream_t st) {
    const int n = P.h * P.w;
    const int ndisp = (2 * P.ru + 1) * (2 * P.rv + 1);
    const int nqb = (n / 4 + kThreads - 1) / kThreads;
    const long long nwg = (long long)nqb * ndisp * P.B;
    RMD_REQUIRE(nwg < (1ll << 31), RMD_ERR_SHAPE, "rmd_dicl_stack_int: grid too large");
    const bool remap = false;
    if (P.C == 32) {
        dicl_stack_int_v2_kernel<32, true><<<(unsigned)nwg, kThreads, 0, st>>>(fmap1, fmap2, nz, P, nqb, remap, out);
    } else {
        dicl_stack_int_v2_kernel<0, true><<<(unsigned)nwg, kThreads, 0, st>>>(fmap1, fmap2, nz, P, nqb, remap, out);
    }
    return check_launch("rmd_dicl_stack_int");
}

// backward (deterministic gathers, no atomics):
//   grad_f1[c, p] = sum_{i,j} ok_ij(p) g[i,j,c,p];   grad_f2[c, q] = sum_{i,j} ok_ij(q-d_ij) g[i,j,C+c,q-d_ij]
__global__ void __launch_bounds__(kThreads)
dicl_stack_int_backward_kernel(const float* __restrict__ g, const unsigned char* __restrict__ nz, IntParams P,
                               float* __restrict__ gf1, float* __restrict__ gf2) {
    const int n = P.h * P.w;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const int C = P.C;
    const int du = 2 * P.ru + 1, dv = 2 * P.rv + 1;
    const int y = p / P.w, x = p - y * P.w;
    const unsigned char* nzb = nz + (size_t)b * n;
    const bool nzp = nzb[p];
    const float* gb = g + (size_t)b * du * dv * 2 * C * n;
    float s1 = 0.f, s2 = 0.f;
    for (int i = 0; i < du; ++i) {
        for (int jj = 0; jj < dv; ++jj) {
            const int di = i - P.ru, dj = jj - P.rv;
            const size_t plane = (size_t)(i * dv + jj) * 2 * C;
            // this pixel as the query: its f1 half (needs target p + d in bounds and non-zero)
            const int xx = x + di, yy = y + dj;
            if (xx >= 0 && xx < P.w && yy >= 0 && yy < P.h && nzb[yy * P.w + xx]) s1 += gb[(plane + c) * n + p];
            // this pixel as the target of query p - d: its f2 half
            const int qx = x - di, qy = y - dj;
            if (nzp && qx >= 0 && qx < P.w && qy >= 0 && qy < P.h) s2 += gb[(plane + C + c) * n + qy * P.w + qx];
        }
    }
    gf1[((size_t)b * C + c) * n + p] = s1;
    gf2[((size_t)b * C + c) * n + p] = s2;
}

// ---- backward warping (common/warp.py:5-33), alone or fused into the occlusion pass of the integer
// volume (impls/dicl.py:178-181 -> 212-238) ---------------------------------------------------------
// warped[c, p] = mask(p) * bilinear(img2[c], x + fx, y + fy) with zero padding, where mask(p) = the
// in-bounds bilinear weight > 1 - eps (grid_sample of a ones tensor, warp.py:28-30).  One lane per pixel
// loops over the channels; with NZ it also writes the occlusion flag sum_c warped[c, p] != 0 that
// integer-volume kernel consumes, so the warp costs no extra pass over the warped map.
struct WarpTaps {
    int idx[4];
    float wgt[4];
    bool valid;
};

__device__ __forceinline__ WarpTaps warp_taps(const float* __restrict__ flow, int b, int p, int h, int w, float eps) {
    const int n = h * w;
    const int y = p / w, x = p - y * w;
    const float ix = (float)x + flow[((size_t)b * 2 + 0) * n + p];
    const float iy = (float)y + flow[((size_t)b * 2 + 1) * n + p];
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float ax = ix - fx0, ay = iy - fy0;
    WarpTaps t;
    float wsum = 0.f;
    // far-away positions: clamp before the int conversion (their taps are all out of bounds anyway)
    const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f), y0 = (int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dx = k & 1, dy = k >> 1;
        const int xx = x0 + dx, yy = y0 + dy;
        const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
        const float wk = (dx ? ax : 1.f - ax) * (dy ? ay : 1.f - ay);
        t.idx[k] = in ? yy * w + xx : 0;
        t.wgt[k] = in ? wk : 0.f;
        wsum += t.wgt[k];
    }
    t.valid = wsum > 1.0f - eps;
    return t;
}

template <bool NZ>
__global__ void __launch_bounds__(kThreads)
warp_kernel(const float* __restrict__ img2, const float* __restrict__ flow, int C, int h, int w, float eps,
            float* __restrict__ out, unsigned char* __restrict__ mask, unsigned char* __restrict__ nz) {
    const int n = h * w;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= n) return;
    const WarpTaps t = warp_taps(flow, b, p, h, w, eps);
    const float* src = img2 + (size_t)b * C * n;
    float* o = out + (size_t)b * C * n + p;
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* sc = src + (size_t)c * n;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) v = fmaf(t.wgt[k], sc[t.idx[k]], v);
        v = t.valid ? v : 0.f;
        o[(size_t)c * n] = v;
        s += v;
    }
    if (mask) mask[(size_t)b * n + p] = t.valid;
    if (NZ) nz[(size_t)b * n + p] = s != 0.f;
}

// d img2 += bilinear^T (mask * grad): float atomics onto the 4 taps (as ATen's grid_sampler_2d_backward)
__global__ void __launch_bounds__(kThreads)
warp_backward_kernel(const float* __restrict__ grad, const float* __restrict__ flow, int C, int h, int w, float eps,
                     float* __restrict__ grad_img2) {
    const int n = h * w;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= n) return;
    const WarpTaps t = warp_taps(flow, b, p, h, w, eps);
    if (!t.valid) return;
    const float* g = grad + (size_t)b * C * n + p;
    float* d = grad_img2 + (size_t)b * C * n;
    for (int c = 0; c < C; ++c) {
        const float gv = g[(size_t)c * n];
        if (gv == 0.f) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.wgt[k] != 0.f) atomicAdd(d + (size_t)c * n + t.idx[k], t.wgt[k] * gv);
    }
}

// ---- host side shared by the four integer-volume entry points -------------------------------------
// Their size checks in their order: the warped ones launch the warp on a (pixels, batch) grid, hence the batch
// limit; the forward ones write 4 pixels per lane.
int int_params(IntParams& P, const char* name, int batch, int channels, int height, int width, int ru, int rv,
               bool warped, bool forward) {
    RMD_REQUIRE(batch > 0 && (!warped || batch <= 65535) && channels > 0 && height > 0 && width > 0 && ru >= 0 && rv >= 0,
                RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(!forward || (height * width) % 4 == 0, RMD_ERR_SHAPE, "%s: h*w must be a multiple of 4", name);
    P = IntParams{batch, channels, height, width, ru, rv};
    return RMD_OK;
}

// one lane per pixel of every image, or of every channel of every image
dim3 pixel_grid(const IntParams& P) { return dim3((P.h * P.w + kThreads - 1) / kThreads, P.B); }
dim3 channel_grid(const IntParams& P) { return dim3((P.h * P.w + kThreads - 1) / kThreads, P.C, P.B); }

// workspace of the unwarped entry points: the occlusion flags of fmap2, computed here
unsigned char* launch_nz(const float* fmap2, const IntParams& P, void* workspace, hipStream_t st) {
    unsigned char* nz = reinterpret_cast<unsigned char*>(workspace);
    dicl_nz_kernel<<<pixel_grid(P), kThreads, 0, st>>>(fmap2, P, nz);
    return nz;
}

// workspace of the warped entry points: the warped fmap2 at its start, then the occlusion flags returned
// here; the warp writes both
unsigned char* launch_warp_nz(const float* fmap2, const float* flow, const IntParams& P, void* workspace, hipStream_t st) {
    float* warped = static_cast<float*>(workspace);
    unsigned char* nz = reinterpret_cast<unsigned char*>(warped + (size_t)P.B * P.C * P.h * P.w);
    warp_kernel<true><<<pixel_grid(P), kThreads, 0, st>>>(fmap2, flow, P.C, P.h, P.w, 1e-5f, warped, nullptr, nz);
    return nz;
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" size_t rmd_dicl_stack_int_workspace_bytes(int batch, int height, int width) {
    return (size_t)batch * height * width;
}

extern "C" int rmd_dicl_stack_int(const float* fmap1, const float* fmap2, int batch, int channels, int height,
                                  int width, int ru, int rv, float* out, void* workspace, void* stream) {
    RMD_REQUIRE(fmap1 && fmap2 && out && workspace, RMD_ERR_ARG, "rmd_dicl_stack_int: null pointer");
    IntParams P;
    if (int rc = int_params(P, "rmd_dicl_stack_int", batch, channels, height, width, ru, rv, false, true)) return rc;
    hipStream_t st = as_stream(stream);
    return launch_stack_int(fmap1, fmap2, launch_nz(fmap2, P, workspace, st), P, out, st);
}

extern "C" int rmd_dicl_stack_int_backward(const float* grad_mvol, const float* fmap2, int batch, int channels,
                                           int height, int width, int ru, int rv, float* grad_fmap1,
                                           float* grad_fmap2, void* workspace, void* stream) {
    RMD_REQUIRE(grad_mvol && fmap2 && grad_fmap1 && grad_fmap2 && workspace, RMD_ERR_ARG,
                "rmd_dicl_stack_int_backward: null pointer");
    IntParams P;
    if (int rc = int_params(P, "rmd_dicl_stack_int_backward", batch, channels, height, width, ru, rv, false, false))
        return rc;
    hipStream_t st = as_stream(stream);
    const unsigned char* nz = launch_nz(fmap2, P, workspace, st);
    dicl_stack_int_backward_kernel<<<channel_grid(P), kThreads, 0, st>>>(grad_mvol, nz, P, grad_fmap1, grad_fmap2);
    return check_launch("rmd_dicl_stack_int_backward");
}

extern "C" int rmd_warp_backwards(const float* img2, const float* flow, int batch, int channels, int height,
                                  int width, float eps, float* out, unsigned char* mask, void* stream) {
    RMD_REQUIRE(img2 && flow && out, RMD_ERR_ARG, "rmd_warp_backwards: null pointer");
    RMD_REQUIRE(batch > 0 && batch <= 65535 && channels > 0 && height > 0 && width > 0, RMD_ERR_SHAPE,
                "rmd_warp_backwards: bad sizes");
    const int n = height * width;
    warp_kernel<false><<<dim3((n + kThreads - 1) / kThreads, batch), kThreads, 0, as_stream(stream)>>>(
        img2, flow, channels, height, width, eps, out, mask, nullptr);
    return check_launch("rmd_warp_backwards");
}

extern "C" int rmd_warp_backwards_backward(const float* grad_out, const float* flow, int batch, int channels,
                                           int height, int width, float eps, float* grad_img2, void* stream) {
    RMD_REQUIRE(grad_out && flow && grad_img2, RMD_ERR_ARG, "rmd_warp_backwards_backward: null pointer");
    RMD_REQUIRE(batch > 0 && batch <= 65535 && channels > 0 && height > 0 && width > 0, RMD_ERR_SHAPE,
                "rmd_warp_backwards_backward: bad sizes");
    const int n = height * width;
    hipStream_t st = as_stream(stream);
    (void)hipMemsetAsync(grad_img2, 0, sizeof(float) * (size_t)batch * channels * n, st);
    warp_backward_kernel<<<dim3((n + kThreads - 1) / kThreads, batch), kThreads, 0, st>>>(
        grad_out, flow, channels, height, width, eps, grad_img2);
    return check_launch("rmd_warp_backwards_backward");
}

extern "C" size_t rmd_dicl_stack_int_warped_workspace_bytes(int batch, int channels, int height, int width) {
    if (batch < 1 || channels < 1 || height < 1 || width < 1) return 0;
    const size_t n = (size_t)height * width;
    return align256((size_t)batch * channels * n * sizeof(float) + 2 * (size_t)batch * n);
}

extern "C" int rmd_dicl_stack_int_warped(const float* fmap1, const float* fmap2, const float* flow, int batch,
                                         int channels, int height, int width, int ru, int rv, float* out,
                                         void* workspace, void* stream) {
    RMD_REQUIRE(fmap1 && fmap2 && flow && out && workspace, RMD_ERR_ARG, "rmd_dicl_stack_int_warped: null pointer");
    IntParams P;
    if (int rc = int_params(P, "rmd_dicl_stack_int_warped", batch, channels, height, width, ru, rv, true, true))
        return rc;
    hipStream_t st = as_stream(stream);
    const unsigned char* nz = launch_warp_nz(fmap2, flow, P, workspace, st);
    const int rc = launch_stack_int(fmap1, static_cast<float*>(workspace), nz, P, out, st);
    return rc ? rc : check_launch("rmd_dicl_stack_int_warped");
}

extern "C" int rmd_dicl_stack_int_warped_backward(const float* grad_mvol, const float* fmap2, const float* flow,
                                                  int batch, int channels, int height, int width, int ru, int rv,
                                                  float* grad_fmap1, float* grad_fmap2, void* workspace,
                                                  void* stream) {
    RMD_REQUIRE(grad_mvol && fmap2 && flow && grad_fmap1 && grad_fmap2 && workspace, RMD_ERR_ARG,
                "rmd_dicl_stack_int_warped_backward: null pointer");
    IntParams P;
    if (int rc = int_params(P, "rmd_dicl_stack_int_warped_backward", batch, channels, height, width, ru, rv, true, false))
        return rc;
    hipStream_t st = as_stream(stream);
    // recompute the occlusion flags; the warped map's buffer then receives d warped
    float* warped = static_cast<float*>(workspace);
    const unsigned char* nz = launch_warp_nz(fmap2, flow, P, workspace, st);
    dicl_stack_int_backward_kernel<<<channel_grid(P), kThreads, 0, st>>>(grad_mvol, nz, P, grad_fmap1, warped);
    (void)hipMemsetAsync(grad_fmap2, 0, sizeof(float) * (size_t)batch * channels * height * width, st);
    warp_backward_kernel<<<pixel_grid(P), kThreads, 0, st>>>(warped, flow, channels, height, width, 1e-5f, grad_fmap2);
    return check_launch("rmd_dicl_stack_int_warped_backward");
}
