// metrics.hip — the flow metrics of an evaluation or training step, fused: every estimate of a call
// against one target in one streaming pass, raw statistics per estimate and per sample.
//
// Replaces (qzed/raft-meets-dicl v2):
//  * EndPointError.compute        src/metrics/epe.py:35-53
//  * FlAll.compute                src/metrics/fl_all.py:29-44
//  * AverageAngularError.compute  src/metrics/aae.py:30-44 (on the channel axis, see rmd.h)
//  * FlowMagnitude.compute        src/metrics/flow.py:32-36
//  * the per-sample loop          src/evaluation/evaluator.py:29-37 (one row of statistics per sample)
// -> rmd_flow_metrics
//
// A work item is 4 adjacent pixels of a sample's plane (16-B loads; 1 pixel when H*W % 4 != 0 or a base
// pointer is not 16-B aligned).  A block owns tiles of kThreads * T items of ONE sample (grid.y = sample,
// grid.x strides over the sample's tiles).  Per tile a thread loads target and validity of its T items
// once, keeps them in registers, and loops over the estimate table (a kernel argument); the accumulators
// of the current estimate live in registers.  The angle's double arithmetic bounds the kernel, not the
// loads.  Per (tile, estimate) the accumulators are reduced with a fixed-order shuffle tree per wave,
// then over the block's waves through LDS, and added to the block's running row of that estimate in
// LDS.  Each block writes its rows to the workspace with plain stores; a second kernel adds the blocks
// of each (estimate, sample) in block-index order.  No atomics anywhere: bitwise run-to-run
// reproducible, and an estimate's row does not depend on which other estimates share the call.  Sums
// are double, counts integers (exact).

#include <cmath>

#include "rmd_common.h"

namespace rmd {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;       // bounded grid: 8 blocks per CU on 256 CUs
constexpr int kSlots = RMD_METRICS_SLOTS;
constexpr int kScalarItems = 4;        // items per thread and tile, 1-pixel items
constexpr int kVectorItems = 2;        // items per thread and tile, 4-pixel items

enum { ORD_P = 0, ORD_1 = 1, ORD_2 = 2, ORD_INF = 3 };

struct MetricTable {
    const float* est[RMD_METRICS_MAX_ESTIMATES];
    int n;
};

struct MetricParams {
    float dist[RMD_METRICS_MAX_DISTANCES];
    int nd;
    float fl_abs, fl_rel;
    float ord;                         // p of the general norm
    int ord_kind;
};

// slots 2, 4, 5, 6 are double sums, every other slot an integer count (rmd.h)
__host__ __device__ constexpr bool is_sum_slot(int s) { return s == 2 || s == 4 || s == 5 || s == 6; }

template <int VEC>
__device__ __forceinline__ unsigned load_m(const unsigned char* p) {
    if constexpr (VEC == 4) {
        const unsigned u = *reinterpret_cast<const unsigned*>(p);
        unsigned bits = 0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) bits |= (((u >> (8 * v)) & 0xffu) != 0 ? 1u : 0u) << v;
        return bits;
    } else {
        return *p != 0 ? 1u : 0u;
    }
}

// a thread's T items of both component planes of one (B, 2, H, W) sample; items past the end read as 0
template <int VEC, int T>
__device__ __forceinline__ void load_items(const float* __restrict__ p, long long plane, long long first,
                                           long long items, float (&c0)[VEC * T], float (&c1)[VEC * T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const long long it = first + (long long)t * kThreads;
        if constexpr (VEC == 4) {
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
            if (it < items) {
                q0 = *reinterpret_cast<const float4*>(p + it * 4);
                q1 = *reinterpret_cast<const float4*>(p + plane + it * 4);
            }
            c0[t * 4 + 0] = q0.x; c0[t * 4 + 1] = q0.y; c0[t * 4 + 2] = q0.z; c0[t * 4 + 3] = q0.w;
            c1[t * 4 + 0] = q1.x; c1[t * 4 + 1] = q1.y; c1[t * 4 + 2] = q1.z; c1[t * 4 + 3] = q1.w;
        } else {
            float q0 = 0.f, q1 = 0.f;
            if (it < items) {
                q0 = p[it];
                q1 = p[plane + it];
            }
            c0[t] = q0;
            c1[t] = q1;
        }
    }
}

// the 2-norm of two fp32 components in fp32, each operation rounded on its own (no contraction):
// what vector_norm(ord=2, dim=-3) evaluates (epe.py:39, fl_all.py:33-34)
__device__ __forceinline__ float norm2f(float a, float b) {
    return sqrtf(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)));
}

// max that carries NaN as torch's does (fmaxf drops it)
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ float magnitude(float e0, float e1, const MetricParams& mp) {
    const float a0 = fabsf(e0), a1 = fabsf(e1);
    switch (mp.ord_kind) {
        case ORD_1: return a0 + a1;
        case ORD_2: return norm2f(e0, e1);
        case ORD_INF: return nan_max(a0, a1);
        default: return powf(powf(a0, mp.ord) + powf(a1, mp.ord), 1.f / mp.ord);
    }
}

// aae.py:35-44 in double from the fp32 inputs; |est| |tgt| is taken as sqrt(|est|^2 |tgt|^2) (one root;
// squares of fp32 values and their product stay far inside double's range); the clamp keeps NaN (both
// comparisons false), as torch.clamp
__device__ __forceinline__ double angle(float u, float v, float ut, float vt) {
    const double du = u, dv = v, dut = ut, dvt = vt;
    const double norms = sqrt((du * du + dv * dv) * (dut * dut + dvt * dvt));
    double c = (du * dut + dv * dvt + 1.0) / (norms + 1.0);
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    return acos(c);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// grid (blocks per sample, B).  part: [B][gridDim.x][n][kSlots] 8-byte words (double or long long by slot)
template <int VEC, int T>
__global__ void __launch_bounds__(kThreads)
metrics_partial_kernel(MetricTable tab, MetricParams mp, const float* __restrict__ target,
                       const unsigned char* __restrict__ valid, long long plane, long long* __restrict__ part) {
    constexpr int PX = VEC * T;
    __shared__ long long swave[kWaves][kSlots];
    __shared__ long long srow[RMD_METRICS_MAX_ESTIMATES][kSlots];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y;
    for (int i = tid; i < tab.n * kSlots; i += kThreads) (&srow[0][0])[i] = 0;      // +0.0 and 0 alike
    __syncthreads();

    const long long items = plane / VEC;
    const long long tile_items = (long long)kThreads * T;
    const long long tiles = (items + tile_items - 1) / tile_items;
    const float* tg = target + (size_t)b * 2 * plane;
    const unsigned char* va = valid + (size_t)b * plane;

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // this thread's T items of the tile: target, validity and what depends on them alone
        float t0[PX], t1[PX], thr[PX];
        const long long first = tile * tile_items + tid;
        load_items<VEC, T>(tg, plane, first, items, t0, t1);
        unsigned mbits = 0, inb = 0;               // bit j: pixel j of this thread is set / exists
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const long long it = first + (long long)t * kThreads;
            if (it < items) {
                mbits |= load_m<VEC>(va + it * VEC) << (t * VEC);
                inb |= ((1u << VEC) - 1u) << (t * VEC);
            }
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) thr[j] = __fmul_rn(mp.fl_rel, norm2f(t0[j], t1[j]));       // fl_all.py:41
        const int nmask = __popc(mbits);

        for (int e = 0; e < tab.n; ++e) {
            float e0[PX], e1[PX];
            load_items<VEC, T>(tab.est[e] + (size_t)b * 2 * plane, plane, first, items, e0, e1);
            double s_epe = 0.0, s_ang = 0.0, s_angv = 0.0, s_mag = 0.0;
            int c_fl = 0, c_bad = 0, c_near[RMD_METRICS_MAX_DISTANCES];
#pragma unroll
            for (int i = 0; i < RMD_METRICS_MAX_DISTANCES; ++i) c_near[i] = 0;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                if (!((inb >> j) & 1u)) continue;
                const bool m = (mbits >> j) & 1u;
                const float epe = norm2f(e0[j] - t0[j], e1[j] - t1[j]);             // epe.py:39
                const double ang = angle(e0[j], e1[j], t0[j], t1[j]);
                s_ang += ang;
                s_mag += (double)magnitude(e0[j], e1[j], mp);                       // flow.py:34
                c_bad += !(fabsf(e0[j]) < INFINITY && fabsf(e1[j]) < INFINITY);
                if (m) {                                                            // a selection: epe[valid]
                    s_epe += (double)epe;
                    s_angv += ang;
                    c_fl += (epe > mp.fl_abs && epe > thr[j]);                      // fl_all.py:41
#pragma unroll
                    for (int i = 0; i < RMD_METRICS_MAX_DISTANCES; ++i)
                        if (i < mp.nd) c_near[i] += (epe <= mp.dist[i]);            // epe.py:51
                }
            }
            // fixed-order shuffle tree per wave; lane 0 holds the wave's value
            s_epe = wave_sum(s_epe);
            s_ang = wave_sum(s_ang);
            s_angv = wave_sum(s_angv);
            s_mag = wave_sum(s_mag);
            c_fl = wave_sum(c_fl);
            c_bad = wave_sum(c_bad);
            const int c_mask = wave_sum(nmask);
#pragma unroll
            for (int i = 0; i < RMD_METRICS_MAX_DISTANCES; ++i)
                if (i < mp.nd) c_near[i] = wave_sum(c_near[i]);
            if (lane == 0) {
                long long* w = swave[wave];
                w[0] = 0;
                w[1] = c_mask;
                w[2] = __double_as_longlong(s_epe);
                w[3] = c_fl;
                w[4] = __double_as_longlong(s_ang);
                w[5] = __double_as_longlong(s_angv);
                w[6] = __double_as_longlong(s_mag);
                w[7] = c_bad;
#pragma unroll
                for (int i = 0; i < RMD_METRICS_MAX_DISTANCES; ++i) w[8 + i] = c_near[i];
            }
            __syncthreads();
            if (tid < kSlots) {                    // the block's waves in order, then onto the running row
                if (is_sum_slot(tid)) {
                    double a = __longlong_as_double(swave[0][tid]);
#pragma unroll
                    for (int k = 1; k < kWaves; ++k) a += __longlong_as_double(swave[k][tid]);
                    srow[e][tid] = __double_as_longlong(__longlong_as_double(srow[e][tid]) + a);
                } else {
                    long long c = swave[0][tid];
#pragma unroll
                    for (int k = 1; k < kWaves; ++k) c += swave[k][tid];
                    srow[e][tid] += c;
                }
            }
            __syncthreads();
        }
    }
    long long* out = part + ((size_t)b * gridDim.x + blockIdx.x) * tab.n * kSlots;
    for (int i = tid; i < tab.n * kSlots; i += kThreads) out[i] = (&srow[0][0])[i];
}

// one thread per (estimate, sample, slot): the blocks of the sample in block-index order
__global__ void __launch_bounds__(kThreads)
metrics_final_kernel(const long long* __restrict__ part, int nblocks, int n, int B, long long plane,
                     double* __restrict__ stats) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n * B * kSlots) return;
    const int slot = idx % kSlots, b = (idx / kSlots) % B, e = idx / (kSlots * B);
    const long long* src = part + ((size_t)b * nblocks * n + e) * kSlots + slot;
    const size_t step = (size_t)n * kSlots;
    double r;
    if (slot == 0) {
        r = (double)plane;
    } else if (is_sum_slot(slot)) {
        double a = 0.0;
        for (int i = 0; i < nblocks; ++i) a += __longlong_as_double(src[i * step]);
        r = a;
    } else {
        long long c = 0;
        for (int i = 0; i < nblocks; ++i) c += src[i * step];
        r = (double)c;
    }
    stats[idx] = r;                                // (N, B, kSlots)
}

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// blocks per sample the workspace is sized for: the scalar path's tile count, bounded
inline int max_blocks_per_sample(int batch, long long plane) {
    const long long tiles = ceil_div(plane, (long long)kThreads * kScalarItems);
    const long long cap = kMaxBlocks / batch > 0 ? kMaxBlocks / batch : 1;
    return (int)(tiles < cap ? tiles : cap);
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" size_t rmd_flow_metrics_workspace_bytes(int batch, int height, int width, int nest) {
    if (batch < 1 || batch > 65535 || height < 1 || width < 1 || nest < 1 || nest > RMD_METRICS_MAX_ESTIMATES) return 0;
    const long long plane = (long long)height * width;
    return (size_t)batch * max_blocks_per_sample(batch, plane) * nest * kSlots * sizeof(long long);
}

extern "C" int rmd_flow_metrics(const float* const* estimates, int nest, const float* target,
                                const unsigned char* valid, int batch, int height, int width, const float* distances,
                                int nd, float fl_abs, float fl_rel, float mag_ord, double* stats, void* workspace,
                                void* stream) {
    RMD_REQUIRE(estimates && target && valid && stats && workspace, RMD_ERR_ARG, "rmd_flow_metrics: null pointer");
    RMD_REQUIRE(nest >= 1 && nest <= RMD_METRICS_MAX_ESTIMATES, RMD_ERR_ARG,
                "rmd_flow_metrics: %d estimates (1..%d per call; chunk longer lists)", nest, RMD_METRICS_MAX_ESTIMATES);
    RMD_REQUIRE(nd >= 0 && nd <= RMD_METRICS_MAX_DISTANCES, RMD_ERR_ARG,
                "rmd_flow_metrics: %d distances (0..%d per call; chunk longer lists)", nd, RMD_METRICS_MAX_DISTANCES);
    RMD_REQUIRE(nd == 0 || distances, RMD_ERR_ARG, "rmd_flow_metrics: null distances with nd = %d", nd);
    RMD_REQUIRE(batch > 0 && batch <= 65535 && height > 0 && width > 0, RMD_ERR_SHAPE,
                "rmd_flow_metrics: bad sizes (batch=%d height=%d width=%d)", batch, height, width);
    RMD_REQUIRE(mag_ord > 0.f, RMD_ERR_ARG, "rmd_flow_metrics: bad mag_ord %g (1, 2, +inf or any other p > 0)",
                (double)mag_ord);                                          // NaN, 0 and negatives fail the comparison
    for (int k = 0; k < nest; ++k) RMD_REQUIRE(estimates[k], RMD_ERR_ARG, "rmd_flow_metrics: estimate %d: null", k);

    MetricTable tab{};
    tab.n = nest;
    for (int k = 0; k < nest; ++k) tab.est[k] = estimates[k];
    MetricParams mp{};
    mp.nd = nd;
    for (int i = 0; i < nd; ++i) mp.dist[i] = distances[i];
    mp.fl_abs = fl_abs;
    mp.fl_rel = fl_rel;
    mp.ord = mag_ord;
    mp.ord_kind = mag_ord == 1.f ? ORD_1 : mag_ord == 2.f ? ORD_2 : std::isinf(mag_ord) ? ORD_INF : ORD_P;

    const long long plane = (long long)height * width;
    bool vec = plane % 4 == 0 && aligned(target, 16) && aligned(valid, 4);
    for (int k = 0; k < nest && vec; ++k) vec = aligned(estimates[k], 16);
    const int cap = max_blocks_per_sample(batch, plane);
    const long long tiles = vec ? ceil_div(plane / 4, (long long)kThreads * kVectorItems)
                                : ceil_div(plane, (long long)kThreads * kScalarItems);
    const int bps = (int)(tiles < cap ? tiles : cap);          // never above what the workspace was sized for
    long long* part = static_cast<long long*>(workspace);
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)bps, (unsigned)batch);
    if (vec) metrics_partial_kernel<4, kVectorItems><<<grid, kThreads, 0, s>>>(tab, mp, target, valid, plane, part);
    else metrics_partial_kernel<1, kScalarItems><<<grid, kThreads, 0, s>>>(tab, mp, target, valid, plane, part);
    const int cells = nest * batch * kSlots;
    metrics_final_kernel<<<(cells + kThreads - 1) / kThreads, kThreads, 0, s>>>(part, bps, nest, batch, plane, stats);
    return check_launch("rmd_flow_metrics");
}
