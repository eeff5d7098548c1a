// dicl_head.hip — the per-level flow head of the DICL baseline: soft-argmin flow regression and the
// normalised entropy of the same softmax, from ONE read of the cost.
//
// * FlowRegression.forward (qzed/raft-meets-dicl src/models/impls/dicl.py:53-85): softmax over the
//   du*dv costs of a pixel, expectation of the displacement (i - ru, j - rv); the coarse flow of
//   FlowLevel.compute_flow (dicl.py:195) is added in the same pass.
// * FlowEntropy.forward (dicl.py:31-50): -sum p log(clamp(p, eps, 1 - eps)) / log(du*dv) of that softmax.
//
// Both are HBM-bound reductions over the displacement planes of a (B, du, dv, h*w) tensor: 4 D bytes
// read and 12 written per pixel.  One lane per pixel, consecutive lanes on consecutive
// pixels, so every plane read of a wave is one coalesced 256 B run.  A block is ONE wave: the largest
// cfg3 level has 98 304 pixels, i.e. 1536 waves or 6 per CU, which 256-thread blocks would hand out
// as 1 or 2 blocks per CU.  For square windows of radius 1..4 the costs stay in registers between
// the max and exp passes (D is a compile-time constant); every other (ru, rv) re-reads them, which
// hits L1/L2.  All arithmetic is float32, all offsets 64-bit; there are no atomics and no workspace,
// so results are bitwise repeatable.

#include <cmath>

#include "rmd_common.h"

namespace rmd {
namespace {

constexpr int kHeadThreads = 64;
constexpr int kHeadMaxRange = 8;

struct HeadParams {
    float eps;          // clamp bounds of the entropy's log (dicl.py:48): [eps, 1 - eps], 1 - eps in float32
    float hi;
    float log_d;        // log(du*dv) rounded to float32 (dicl.py:50: a float32 tensor over a Python scalar)
};

// log(clamp(p, eps, 1 - eps)).  fmaxf / fminf drop a NaN p; every caller multiplies the result by p.
__device__ __forceinline__ float clamped_log(float p, const HeadParams& hp) {
    return logf(fminf(fmaxf(p, hp.eps), hp.hi));
}

// d (p log clamp(p)) / d p = log clamp(p) + [eps <= p <= 1 - eps]: torch's clamp passes the gradient
// on the closed interval
__device__ __forceinline__ float entropy_slope(float p, const HeadParams& hp) {
    return clamped_log(p, hp) + ((p >= hp.eps && p <= hp.hi) ? 1.0f : 0.0f);
}

__device__ __forceinline__ void head_store(float* __restrict__ out, const float* __restrict__ coarse, size_t b,
                                           size_t n, size_t p, float fu, float fv, float ent, const HeadParams& hp) {
    if (coarse) {
        fu += coarse[(b * 2 + 0) * n + p];
        fv += coarse[(b * 2 + 1) * n + p];
    }
    float* o = out + b * 3 * n + p;
    o[0] = fu;
    o[n] = fv;
    o[2 * n] = -ent / hp.log_d;
}

// ---- square windows of radius 1..4: costs in registers ---------------------------------------------

// softmax numerators exp(c_k - max) in v, 1 / their sum in inv; returns the index of the (first) largest
// cost.  A NaN or +inf cost, or all costs -inf, makes every numerator NaN (inf - inf), as torch's softmax.
template <int D>
__device__ __forceinline__ int head_probs(const float* __restrict__ c, size_t n, float (&v)[D], float& inv) {
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        v[k] = c[(size_t)k * n];
        if (v[k] > mx) {
            mx = v[k];
            am = k;
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        v[k] = expf(v[k] - mx);
        s += v[k];
    }
    inv = 1.0f / s;
    return am;
}

template <int R>
__global__ void __launch_bounds__(kHeadThreads) dicl_head_kernel(const float* __restrict__ cost,
                                                                 const float* __restrict__ coarse, long long n,
                                                                 HeadParams hp, float* __restrict__ out) {
    constexpr int D2 = 2 * R + 1, D = D2 * D2;
    const size_t p = (size_t)blockIdx.x * kHeadThreads + threadIdx.x;
    const size_t b = blockIdx.y;
    if (p >= (size_t)n) return;
    float v[D], inv;
    head_probs<D>(cost + b * D * (size_t)n + p, (size_t)n, v, inv);
    float fu = 0.0f, fv = 0.0f, ent = 0.0f;
#pragma unroll
    for (int i = 0; i < D2; ++i) {
#pragma unroll
        for (int j = 0; j < D2; ++j) {
            const float pk = v[i * D2 + j] * inv;
            fu = fmaf(pk, (float)(i - R), fu);
            fv = fmaf(pk, (float)(j - R), fv);
            ent = fmaf(pk, clamped_log(pk, hp), ent);
        }
    }
    head_store(out, coarse, b, (size_t)n, p, fu, fv, ent, hp);
}

// d cost_k = p_k (g_k - sum_j p_j g_j) with g_k = gu u_k + gv v_k - gH (log clamp(p_k) + [..]) / log D.
// g is evaluated relative to the argmax m (g_k - g_m, which leaves the bracket unchanged): the
// displacement part becomes gu (u_k - u_m) + gv (v_k - v_m), exact small integers, and a peaked
// softmax keeps its relative accuracy (softargmax_backward_kernel, heads.hip).
template <int R>
__global__ void __launch_bounds__(kHeadThreads) dicl_head_backward_kernel(const float* __restrict__ cost,
                                                                          const float* __restrict__ grad_out,
                                                                          long long n, HeadParams hp,
                                                                          float* __restrict__ grad_cost) {
    constexpr int D2 = 2 * R + 1, D = D2 * D2;
    const size_t p = (size_t)blockIdx.x * kHeadThreads + threadIdx.x;
    const size_t b = blockIdx.y;
    if (p >= (size_t)n) return;
    const size_t off = b * D * (size_t)n + p;
    float v[D], g[D], inv;
    const int am = head_probs<D>(cost + off, (size_t)n, v, inv);
    const int mi = am / D2, mj = am - mi * D2;
    const float* go = grad_out + b * 3 * (size_t)n + p;
    const float gu = go[0], gv = go[n], ge = -go[2 * n] / hp.log_d;
    float pm = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        v[k] *= inv;
        pm = am == k ? v[k] : pm;
    }
    const float sm = entropy_slope(pm, hp);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < D2; ++i) {
#pragma unroll
        for (int j = 0; j < D2; ++j) {
            const int k = i * D2 + j;
            const float disp = fmaf(gu, (float)(i - mi), gv * (float)(j - mj));
            g[k] = fmaf(ge, entropy_slope(v[k], hp) - sm, disp);
            s = fmaf(v[k], g[k], s);
        }
    }
    float* gc = grad_cost + off;
#pragma unroll
    for (int k = 0; k < D; ++k) gc[(size_t)k * n] = v[k] * (g[k] - s);
}

// ---- every other (ru, rv): the costs are read again per pass -----------------------------------------

__device__ __forceinline__ int head_scan(const float* __restrict__ c, size_t n, int d, float& mx, float& inv) {
    mx = -INFINITY;
    int am = 0;
    for (int k = 0; k < d; ++k) {
        const float x = c[(size_t)k * n];
        if (x > mx) {
            mx = x;
            am = k;
        }
    }
    float s = 0.0f;
    for (int k = 0; k < d; ++k) s += expf(c[(size_t)k * n] - mx);
    inv = 1.0f / s;
    return am;
}

__global__ void __launch_bounds__(kHeadThreads) dicl_head_generic_kernel(const float* __restrict__ cost,
                                                                         const float* __restrict__ coarse, int du,
                                                                         int dv, long long n, HeadParams hp,
                                                                         float* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * kHeadThreads + threadIdx.x;
    const size_t b = blockIdx.y;
    if (p >= (size_t)n) return;
    const int d = du * dv, ru = du >> 1, rv = dv >> 1;
    const float* c = cost + b * d * (size_t)n + p;
    float mx, inv;
    head_scan(c, (size_t)n, d, mx, inv);
    float fu = 0.0f, fv = 0.0f, ent = 0.0f;
    for (int i = 0; i < du; ++i) {
        for (int j = 0; j < dv; ++j) {
            const float pk = expf(c[(size_t)(i * dv + j) * n] - mx) * inv;
            fu = fmaf(pk, (float)(i - ru), fu);
            fv = fmaf(pk, (float)(j - rv), fv);
            ent = fmaf(pk, clamped_log(pk, hp), ent);
        }
    }
    head_store(out, coarse, b, (size_t)n, p, fu, fv, ent, hp);
}

__global__ void __launch_bounds__(kHeadThreads) dicl_head_backward_generic_kernel(
    const float* __restrict__ cost, const float* __restrict__ grad_out, int du, int dv, long long n, HeadParams hp,
    float* __restrict__ grad_cost) {
    const size_t p = (size_t)blockIdx.x * kHeadThreads + threadIdx.x;
    const size_t b = blockIdx.y;
    if (p >= (size_t)n) return;
    const int d = du * dv;
    const size_t off = b * d * (size_t)n + p;
    const float* c = cost + off;
    float mx, inv;
    const int am = head_scan(c, (size_t)n, d, mx, inv);
    const int mi = am / dv, mj = am - mi * dv;
    const float* go = grad_out + b * 3 * (size_t)n + p;
    const float gu = go[0], gv = go[n], ge = -go[2 * n] / hp.log_d;
    const float sm = entropy_slope(expf(c[(size_t)am * n] - mx) * inv, hp);
    float s = 0.0f;
    for (int i = 0; i < du; ++i) {
        for (int j = 0; j < dv; ++j) {
            const float pk = expf(c[(size_t)(i * dv + j) * n] - mx) * inv;
            const float disp = fmaf(gu, (float)(i - mi), gv * (float)(j - mj));
            s = fmaf(pk, fmaf(ge, entropy_slope(pk, hp) - sm, disp), s);
        }
    }
    float* gc = grad_cost + off;
    for (int i = 0; i < du; ++i) {
        for (int j = 0; j < dv; ++j) {
            const size_t k = (size_t)(i * dv + j) * n;
            const float pk = expf(c[k] - mx) * inv;
            const float disp = fmaf(gu, (float)(i - mi), gv * (float)(j - mj));
            gc[k] = pk * (fmaf(ge, entropy_slope(pk, hp) - sm, disp) - s);
        }
    }
}

inline int head_check(const char* what, int batch, int du, int dv, int pixels, float eps) {
    RMD_REQUIRE(batch >= 1 && batch <= 65535 && pixels >= 1, RMD_ERR_SHAPE, "%s: bad sizes (batch=%d pixels=%d)", what,
                batch, pixels);
    RMD_REQUIRE(du >= 1 && dv >= 1 && (du & 1) && (dv & 1), RMD_ERR_SHAPE,
                "%s: du=%d dv=%d must be odd (2 ru + 1, 2 rv + 1)", what, du, dv);
    RMD_REQUIRE(du <= 2 * kHeadMaxRange + 1 && dv <= 2 * kHeadMaxRange + 1, RMD_ERR_SHAPE,
                "%s: du=%d dv=%d: ranges above %d are not supported", what, du, dv, kHeadMaxRange);
    RMD_REQUIRE(eps >= 0.0f && eps < 0.5f, RMD_ERR_ARG, "%s: eps %g not in [0, 0.5)", what, (double)eps);   // NaN fails
    return RMD_OK;
}

inline HeadParams head_params(int du, int dv, float eps) {
    HeadParams hp;
    hp.eps = eps;
    hp.hi = 1.0f - eps;
    hp.log_d = (float)std::log((double)(du * dv));
    return hp;
}

}  // namespace
}  // namespace rmd

using namespace rmd;

#define RMD_HEAD_CASES(X) X(1) X(2) X(3) X(4)

extern "C" int rmd_dicl_flow_head(const float* cost, const float* flow_coarse, int batch, int du, int dv, int pixels,
                                  float eps, float* out, void* stream) {
    RMD_REQUIRE(cost && out, RMD_ERR_ARG, "rmd_dicl_flow_head: null pointer");
    const int rc = head_check("rmd_dicl_flow_head", batch, du, dv, pixels, eps);
    if (rc) return rc;
    const HeadParams hp = head_params(du, dv, eps);
    const dim3 grid((unsigned)(((long long)pixels + kHeadThreads - 1) / kHeadThreads), (unsigned)batch);
    hipStream_t st = as_stream(stream);
    switch (du == dv ? du >> 1 : 0) {
#define RMD_HEAD(RR) \
    case RR: dicl_head_kernel<RR><<<grid, kHeadThreads, 0, st>>>(cost, flow_coarse, pixels, hp, out); break;
        RMD_HEAD_CASES(RMD_HEAD)
#undef RMD_HEAD
        default:
            dicl_head_generic_kernel<<<grid, kHeadThreads, 0, st>>>(cost, flow_coarse, du, dv, pixels, hp, out);
    }
    return check_launch("rmd_dicl_flow_head");
}

extern "C" int rmd_dicl_flow_head_backward(const float* cost, const float* grad_out, int batch, int du, int dv,
                                           int pixels, float eps, float* grad_cost, void* stream) {
    RMD_REQUIRE(cost && grad_out && grad_cost, RMD_ERR_ARG, "rmd_dicl_flow_head_backward: null pointer");
    const int rc = head_check("rmd_dicl_flow_head_backward", batch, du, dv, pixels, eps);
    if (rc) return rc;
    const HeadParams hp = head_params(du, dv, eps);
    const dim3 grid((unsigned)(((long long)pixels + kHeadThreads - 1) / kHeadThreads), (unsigned)batch);
    hipStream_t st = as_stream(stream);
    switch (du == dv ? du >> 1 : 0) {
#define RMD_HEAD(RR) \
    case RR: dicl_head_backward_kernel<RR><<<grid, kHeadThreads, 0, st>>>(cost, grad_out, pixels, hp, grad_cost); break;
        RMD_HEAD_CASES(RMD_HEAD)
#undef RMD_HEAD
        default:
            dicl_head_backward_generic_kernel<<<grid, kHeadThreads, 0, st>>>(cost, grad_out, du, dv, pixels, hp,
                                                                             grad_cost);
    }
    return check_launch("rmd_dicl_flow_head_backward");
}
