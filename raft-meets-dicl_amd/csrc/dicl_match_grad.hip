// dicl_match_grad.hip — backward of the fused dicl-1x1 cost (dicl_match.hip): recomputes the MLP per column
// on the MFMA pipe and never writes the (B, d, d, 2C, h, w) stack, a hidden activation or its gradient.
//
// Orientation and fragment order as the forward kernel (dicl_match_common.h): a wave owns a column set — 32
// consecutive pixels at ONE displacement — with the samples on the MFMA column (lane & 31) and channels on
// the row.  The forward is recomputed by the forward kernel's own templates in their three-product mode
// (same taps, same three split-bf16 products, same fragment order), keeping a 16-bit mask (z > 0) per
// accumulator tile.  dz_l is built on the VALU in the accumulator layout of z_l, so after the split to bf16
// hi / lo it is two k-steps of the B operand of W_l^T dz_l, with W_l^T packed as A fragments in the same k
// order; the result lands in the layout of z_{l-1}, where the mask applies in registers.  Every product is
// hi.hi + hi.lo + lo.hi with fp32 accumulation.
//
// Weight gradients gW_l = dz_l a_{l-1}^T need the samples on K.  A workgroup is 4 waves (one per SIMD, the
// whole register file each); per round every wave takes one displacement of the workgroup's strip and
// stages dz_l and a_{l-1} of its column set in LDS as [channel][32 samples] bf16 hi / lo, so both become
// row-major A / B operand reads of 8 consecutive samples.  The 32 x 32 tiles of gW_l are dealt round-robin
// to the 4 waves, which accumulate their tiles over all four staged column sets (K = 128 per round, two
// barriers per layer) in registers for the whole kernel.  gt_l, gw4 and gb4 are fp32 VALU sums (a tile's
// rows are summed over its 32 samples through a wave-private LDS transpose, in a fixed order).  Every
// workgroup writes its partial parameter gradients to the workspace with plain stores and a second kernel
// adds them in workgroup order: no float atomics, bitwise reproducible.  grad_fmap1 is summed over a
// wave's displacements in registers and over the 4 waves through LDS in wave order (one workgroup owns a
// whole strip): bitwise reproducible.  grad_fmap2 is the bilinear adjoint of dx[C:2C] on float atomics, as
// rmd_dicl_stack_backward's.
//
// Resources: every instance runs at 512 registers and spills — 4872 / 728 / 5736 B of scratch per lane for the
// exact, 2/2/2/1 and 4/4/4/4 instances (times in profiles/dicl_match_share_r14.json).
//
// A lane without a column of its own (a strip remainder, a wave past the last displacement) runs with
// g = 0 and stages zeros, so it adds nothing anywhere — not even 0 * NaN.

#include "dicl_match_common.h"

#include <algorithm>

namespace rmd {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kStagePart = kMaxWidth * 32 * 2;         // one [channel][32 samples] bf16 array
constexpr int kStageWave = 4 * kStagePart;             // dz hi | dz lo | a hi | a lo of one wave
constexpr int kRedStride = 33;                         // wave-private [32 rows][32 samples] f32, padded
constexpr int kRedWave = 32 * kRedStride * 4;
constexpr int kLdsBytes = kBiasBytes + kWaves * (kStageWave + kRedWave);
static_assert(kLdsBytes <= 160 * 1024, "LDS budget");

struct GradParams : MatchGeom {
    int nw, nv;          // floats of one partial: the three matrices; gw4 | gt1 | gt2 | gt3 | gb4
    int params;          // parameter gradients wanted
};

// LDS traffic between the lanes of ONE wave: DS operations of a wave execute in order; the fences keep
// the compiler from moving them and wait for the data
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sum of every row of an accumulator-layout tile over its 32 samples, fp32, fixed order: lanes (row, half)
// add 16 samples each, then the two halves.  Returned on both lanes of row (lane & 31).
__device__ __forceinline__ float tile_rowsum(const float* v, float* red, int lane) {
    const int r = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) red[acc_row(i, hh) * kRedStride + r] = v[i];
    wave_lds_sync();
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += red[r * kRedStride + 16 * hh + q];
    wave_lds_sync();
    return s + __shfl_xor(s, 32, 64);
}

// one k-step fragment (channel chbase + frag_k(ks, hh, j) of sample r) into a [channel][32] hi / lo pair
__device__ __forceinline__ void stage_frag(unsigned char* hi_arr, int chbase, int ks, int r, int hh, bool live,
                                           const bf16x8& h, const bf16x8& l) {
    __bf16* ph = reinterpret_cast<__bf16*>(hi_arr);
    __bf16* pl = reinterpret_cast<__bf16*>(hi_arr + kStagePart);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int at = (chbase + frag_k(ks, hh, j)) * 32 + r;
        ph[at] = live ? h[j] : (__bf16)0.f;
        pl[at] = live ? l[j] : (__bf16)0.f;
    }
}

// this wave's tiles (t = s * kWaves + wave < tiles; tile t = (row tile t / ncol, column tile t % ncol)) of
// gW += dz a^T over the staged column sets of all waves: samples on K, 8 consecutive per lane
template <int S>
__device__ __forceinline__ void wgrad(f32x16 (&acc)[S], int tiles, int ncol, int wave, int r, int hh,
                                      const unsigned char* stage) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int t = s * kWaves + wave;
        if (t < tiles) {
            __builtin_amdgcn_sched_barrier(0);
            const int mo = t / ncol, no = t - mo * ncol;
            for (int wv = 0; wv < kWaves; ++wv) {
                const unsigned char* base = stage + wv * kStageWave;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int so = (16 * ks + 8 * hh) * 2;
                    const int ao = (32 * mo + r) * 64 + so, bo = (32 * no + r) * 64 + so;
                    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(base + ao);
                    const bf16x8 al = *reinterpret_cast<const bf16x8*>(base + kStagePart + ao);
                    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(base + 2 * kStagePart + bo);
                    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(base + 3 * kStagePart + bo);
                    mma<3>(acc[s], ah, al, bh, bl);
                }
            }
        }
    }
}

template <int S>
__device__ __forceinline__ void store_tiles(const f32x16 (&acc)[S], int tiles, int ncol, int cols, int wave, int r,
                                            int hh, float* __restrict__ dst) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int t = s * kWaves + wave;
        if (t < tiles) {
            const int mo = t / ncol, no = t - mo * ncol;
#pragma unroll
            for (int i = 0; i < 16; ++i) dst[(size_t)(32 * mo + acc_row(i, hh)) * cols + 32 * no + r] = acc[s][i];
        }
    }
}

// KF, M1..M3: compile-time bounds of the k-step / tile loops (register arrays); EXACT: they are the sizes
// themselves, else P's sizes guard.
template <bool EXACT, int KF, int M1, int M2, int M3>
__global__ void __launch_bounds__(kThreads)
dicl_match_grad_kernel(const float* __restrict__ gcost, const float* __restrict__ f1, const float* __restrict__ f2,
                       const float* __restrict__ coords, const bf16x8* __restrict__ frags,
                       const float* __restrict__ t1, const float* __restrict__ t2, const float* __restrict__ t3,
                       const float* __restrict__ w4, GradParams P, float* __restrict__ gf1, float* __restrict__ gf2,
                       float* __restrict__ partw, float* __restrict__ partv) {
    constexpr int S1 = (M1 * KF + kWaves - 1) / kWaves, S2 = (M2 * M1 + kWaves - 1) / kWaves,
                  S3 = (M3 * M2 + kWaves - 1) / kWaves, G1 = (KF + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    float* const sb = reinterpret_cast<float*>(sm);                 // t1 | t2 | t3 | w4, kMaxWidth each
    unsigned char* const stage = sm + kBiasBytes;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    unsigned char* const mine = stage + wave * kStageWave;
    float* const red = reinterpret_cast<float*>(sm + kBiasBytes + kWaves * kStageWave + wave * kRedWave);
    const int kf = EXACT ? KF : P.kf, m1 = EXACT ? M1 : P.m1, m2 = EXACT ? M2 : P.m2, m3 = EXACT ? M3 : P.m3;
    const bool params = P.params != 0;

    stage_biases(sb, t1, t2, t3, w4, m1, m2, m3, tid, kThreads);
    __syncthreads();

    // plain fragments (parts 0, 1) and transposed ones (parts 2, 3); both orientations of a layer hold the
    // same number of fragments, so one set of layer bases serves both
    auto afrag = [&](int f, int part) -> bf16x8 { return frags[(unsigned)((part * P.nfrag + f) * 64 + lane)]; };
    const int fb2 = m1 * 2 * kf, fb3 = fb2 + m2 * 2 * m1;           // layer 1: 0

    f32x16 gw1[S1], gw2[S2], gw3[S3];
#pragma unroll
    for (int s = 0; s < S1; ++s) gw1[s] = f32x16{};
#pragma unroll
    for (int s = 0; s < S2; ++s) gw2[s] = f32x16{};
#pragma unroll
    for (int s = 0; s < S3; ++s) gw3[s] = f32x16{};
    float gt1[M1] = {}, gt2[M2] = {}, gt3[M3] = {}, gw4[M3] = {}, gb4 = 0.f;

    const int d = 2 * P.radius + 1, dd = d * d;
    const int n = P.n;
    const int rounds = (dd + kWaves - 1) / kWaves;
    const long long items = (long long)P.B * P.nstrips;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int b = (int)(item / P.nstrips);
        const int p0 = (int)(item - (long long)b * P.nstrips) * 32;
        const int p = p0 + r;
        const bool valid = p < n;
        const int pc = valid ? p : n - 1;
        const float cx = coords[(size_t)b * 2 * n + pc], cy = coords[((size_t)b * 2 + 1) * n + pc];
        const float* f1b = f1 + (size_t)b * P.C * n;
        const float* f2b = f2 + (size_t)b * P.C * n;
        const unsigned half_off = (unsigned)(4 * hh * n);
        const unsigned off1 = (half_off + (unsigned)pc) * 4u;

        // layer-1 accumulators of the f1 half, plus t1: once per strip
        f32x16 base[M1];
        bf16x8 x1h[KF], x1l[KF];
        f1_frags<3, EXACT, KF>(f1b, n, off1, kf, x1h, x1l);
        layer1_base<3, EXACT, KF, M1>(base, afrag, sb, kf, m1, hh, x1h, x1l);

        f32x16 g1acc[G1];            // dx rows of the f1 half, summed over this wave's displacements
#pragma unroll
        for (int s = 0; s < G1; ++s) g1acc[s] = f32x16{};

        for (int rd = 0; rd < rounds; ++rd) {
            const int dr = rd * kWaves + wave;
            const bool live = valid && dr < dd;
            const int disp = dr < dd ? dr : dd - 1;
            const int a = disp / d, bb = disp - a * d;
            const float px = (cx + (float)(a - P.radius)) * P.sx;
            const float py = (cy + (float)(bb - P.radius)) * P.sy;
            const Taps t = make_taps_fwd(px, py, P.h, P.w);
            const float g = live ? gcost[((size_t)b * dd + disp) * n + pc] : 0.f;
            gb4 += hh == 0 ? g : 0.f;       // both lane halves hold the sample's g

            // ---- forward, dicl_match_kernel<3>'s, keeping the masks ----
            bf16x8 xh[KF], xl[KF], yh[2 * M1], yl[2 * M1], zh[2 * M2], zl[2 * M2];
            unsigned mask1[M1], mask2[M2];
            f2_frags<3, EXACT, KF>(f2b, n, half_off, t, kf, xh, xl);
            layer1<3, EXACT, true, KF, M1>(base, afrag, kf, m1, hh, xh, xl, yh, yl, mask1);
            layer2<3, EXACT, true, M1, M2>(afrag, sb, fb2, m1, m2, hh, yh, yl, zh, zl, mask2);
            // layer 3: dz3 = (z3 > 0) ? w4 g : 0, gw4 += a3 g, gt3 += dz3
            bf16x8 d3h[2 * M3], d3l[2 * M3];
#pragma unroll
            for (int mo = 0; mo < M3; ++mo) {
                if (EXACT || mo < m3) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = {};
                    mma_tile<3, EXACT, 2 * M2>(acc, afrag, fb3 + mo * 2 * m2, 0, 2 * m2, zh, zl);
                    float dz[16], ag[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = 32 * mo + acc_row(i, hh);
                        const float z = acc[i] + sb[2 * kMaxWidth + row];
                        dz[i] = (live && z > 0.f) ? sb[3 * kMaxWidth + row] * g : 0.f;
                        ag[i] = live ? relu_nan(z) * g : 0.f;
                    }
                    if (params) {
                        gw4[mo] += tile_rowsum(ag, red, lane);
                        gt3[mo] += tile_rowsum(dz, red, lane);
                    }
                    split<3>(dz, d3h[2 * mo], d3l[2 * mo]);
                    split<3>(dz + 8, d3h[2 * mo + 1], d3l[2 * mo + 1]);
                }
            }

            // ---- gW3 += dz3 a2^T ----
            if (params) {
#pragma unroll
                for (int ks = 0; ks < 2 * M3; ++ks)
                    if (EXACT || ks < 2 * m3) stage_frag(mine, 0, ks, r, hh, live, d3h[ks], d3l[ks]);
#pragma unroll
                for (int ks = 0; ks < 2 * M2; ++ks)
                    if (EXACT || ks < 2 * m2) stage_frag(mine + 2 * kStagePart, 0, ks, r, hh, live, zh[ks], zl[ks]);
                __syncthreads();
                wgrad<S3>(gw3, m3 * m2, m2, wave, r, hh, stage);
                __syncthreads();
            }

            // ---- da2 = W3^T dz3, dz2 = mask2 ? da2 : 0 ----
            bf16x8 d2h[2 * M2], d2l[2 * M2];
#pragma unroll
            for (int mo = 0; mo < M2; ++mo) {
                if (EXACT || mo < m2) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = {};
                    mma_tile<3, EXACT, 2 * M3>(acc, afrag, fb3 + mo * 2 * m3, 2, 2 * m3, d3h, d3l);
                    float dz[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) dz[i] = ((mask2[mo] >> i) & 1u) ? acc[i] : 0.f;
                    if (params) gt2[mo] += tile_rowsum(dz, red, lane);
                    split<3>(dz, d2h[2 * mo], d2l[2 * mo]);
                    split<3>(dz + 8, d2h[2 * mo + 1], d2l[2 * mo + 1]);
                }
            }

            // ---- gW2 += dz2 a1^T ----
            if (params) {
#pragma unroll
                for (int ks = 0; ks < 2 * M2; ++ks)
                    if (EXACT || ks < 2 * m2) stage_frag(mine, 0, ks, r, hh, live, d2h[ks], d2l[ks]);
#pragma unroll
                for (int ks = 0; ks < 2 * M1; ++ks)
                    if (EXACT || ks < 2 * m1) stage_frag(mine + 2 * kStagePart, 0, ks, r, hh, live, yh[ks], yl[ks]);
                __syncthreads();
                wgrad<S2>(gw2, m2 * m1, m1, wave, r, hh, stage);
                __syncthreads();
            }

            // ---- da1 = W2^T dz2, dz1 = mask1 ? da1 : 0 ----
            bf16x8 d1h[2 * M1], d1l[2 * M1];
#pragma unroll
            for (int mo = 0; mo < M1; ++mo) {
                if (EXACT || mo < m1) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = {};
                    mma_tile<3, EXACT, 2 * M2>(acc, afrag, fb2 + mo * 2 * m2, 2, 2 * m2, d2h, d2l);
                    float dz[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) dz[i] = ((mask1[mo] >> i) & 1u) ? acc[i] : 0.f;
                    if (params) gt1[mo] += tile_rowsum(dz, red, lane);
                    split<3>(dz, d1h[2 * mo], d1l[2 * mo]);
                    split<3>(dz + 8, d1h[2 * mo + 1], d1l[2 * mo + 1]);
                }
            }

            // ---- gW1 += dz1 x^T, x = [f1 ; f2 sample] ----
            if (params) {
#pragma unroll
                for (int ks = 0; ks < 2 * M1; ++ks)
                    if (EXACT || ks < 2 * m1) stage_frag(mine, 0, ks, r, hh, live, d1h[ks], d1l[ks]);
#pragma unroll
                for (int ks = 0; ks < KF; ++ks) {
                    if (EXACT || ks < kf) {
                        stage_frag(mine + 2 * kStagePart, 0, ks, r, hh, live, x1h[ks], x1l[ks]);
                        stage_frag(mine + 2 * kStagePart, P.C, ks, r, hh, live, xh[ks], xl[ks]);
                    }
                }
                __syncthreads();
                wgrad<S1>(gw1, m1 * kf, kf, wave, r, hh, stage);
                __syncthreads();
            }

            // ---- dx = W1^T dz1: rows < C to grad_fmap1 (registers), the others scattered to grad_fmap2 ----
            if (gf1 != nullptr || gf2 != nullptr) {
                const Taps tb = make_taps(px, py, P.h, P.w);
                float* g2b = gf2 != nullptr ? gf2 + (size_t)b * P.C * n : nullptr;
#pragma unroll
                for (int mo = 0; mo < KF; ++mo) {
                    if (EXACT || mo < kf) {
                        __builtin_amdgcn_sched_barrier(0);
                        f32x16 acc = {};
                        mma_tile<3, EXACT, 2 * M1>(acc, afrag, mo * 2 * m1, 2, 2 * m1, d1h, d1l);
                        if (mo < G1) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) g1acc[mo < G1 ? mo : 0][i] += live ? acc[i] : 0.f;
                        }
                        if (g2b != nullptr && live) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) {
                                const int c = 32 * mo + acc_row(i, hh) - P.C;
                                if (c >= 0) {
                                    float* gc = g2b + (size_t)c * n;
#pragma unroll
                                    for (int k = 0; k < 4; ++k)
                                        if (tb.wgt[k] != 0.f) atomicAdd(gc + tb.idx[k], acc[i] * tb.wgt[k]);
                                }
                            }
                        }
                    }
                }
            }
        }

        // grad_fmap1: the four waves' sums through LDS, added in wave order
        if (gf1 != nullptr) {
            float* part = reinterpret_cast<float*>(mine);
#pragma unroll
            for (int mo = 0; mo < G1; ++mo) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = 32 * mo + acc_row(i, hh);
                    if (row < P.C) part[row * 32 + r] = g1acc[mo][i];
                }
            }
            __syncthreads();
            for (int e = tid; e < P.C * 32; e += kThreads) {
                float s = 0.f;
                for (int wv = 0; wv < kWaves; ++wv) s += reinterpret_cast<const float*>(stage + wv * kStageWave)[e];
                const int pp = p0 + (e & 31);
                if (pp < n) gf1[((size_t)b * P.C + (e >> 5)) * n + pp] = s;
            }
            __syncthreads();
        }
    }

    // this workgroup's partial parameter gradients, plain stores
    if (params) {
        float* pw = partw + (size_t)blockIdx.x * P.nw;
        const int c1 = 32 * m1, c2 = 32 * m2, c3 = 32 * m3;
        store_tiles<S1>(gw1, m1 * kf, kf, 2 * P.C, wave, r, hh, pw);
        store_tiles<S2>(gw2, m2 * m1, m1, c1, wave, r, hh, pw + (size_t)c1 * 2 * P.C);
        store_tiles<S3>(gw3, m3 * m2, m2, c2, wave, r, hh, pw + (size_t)c1 * 2 * P.C + (size_t)c2 * c1);
        float* pv = partv + ((size_t)blockIdx.x * kWaves + wave) * P.nv;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) gb4 += __shfl_xor(gb4, off, 64);
        if (hh == 0) {
#pragma unroll
            for (int mo = 0; mo < M3; ++mo)
                if (EXACT || mo < m3) pv[32 * mo + r] = gw4[mo];
#pragma unroll
            for (int mo = 0; mo < M1; ++mo)
                if (EXACT || mo < m1) pv[c3 + 32 * mo + r] = gt1[mo];
#pragma unroll
            for (int mo = 0; mo < M2; ++mo)
                if (EXACT || mo < m2) pv[c3 + c1 + 32 * mo + r] = gt2[mo];
#pragma unroll
            for (int mo = 0; mo < M3; ++mo)
                if (EXACT || mo < m3) pv[c3 + c1 + c2 + 32 * mo + r] = gt3[mo];
            if (r == 0) pv[2 * c3 + c1 + c2] = gb4;
        }
    }
}

struct ReduceOut {
    float* w[3];
    int wn[3];
    float* v[5];          // gw4, gt1, gt2, gt3, gb4
    int vn[5];
};

// partials added in workgroup (and, for the vectors, wave) order
__global__ void __launch_bounds__(256)
dicl_match_grad_reduce_kernel(const float* __restrict__ partw, const float* __restrict__ partv, int grid, int nw,
                              int nv, ReduceOut O) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nw) {
        float s = 0.f;
        for (int g = 0; g < grid; ++g) s += partw[(size_t)g * nw + e];
        int m = 0;
        while (e >= O.wn[m]) e -= O.wn[m++];
        O.w[m][e] = s;
    } else if (e < nw + nv) {
        e -= nw;
        float s = 0.f;
        for (int g = 0; g < grid * kWaves; ++g) s += partv[(size_t)g * nv + e];
        int m = 0;
        while (e >= O.vn[m]) e -= O.vn[m++];
        O.v[m][e] = s;
    }
}

int grad_grid(int batch, long long n) { return (int)std::min<long long>((long long)batch * ((n + 31) / 32), kCUs); }

struct Layout {
    size_t frag_bytes, partw_off, partv_off, total;
    int nw, nv;
};

Layout grad_layout(int batch, int channels, long long n, int c1, int c2, int c3) {
    Layout L;
    L.frag_bytes = (size_t)4 * match_nfrag(channels, c1, c2, c3) * 64 * sizeof(bf16x8);
    L.nw = c1 * 2 * channels + c2 * c1 + c3 * c2;
    L.nv = 2 * c3 + c1 + c2 + 1;
    const size_t grid = (size_t)grad_grid(batch, n);
    L.partw_off = align256(L.frag_bytes);
    L.partv_off = align256(L.partw_off + grid * L.nw * sizeof(float));
    L.total = align256(L.partv_off + grid * kWaves * L.nv * sizeof(float));
    return L;
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" int rmd_dicl_match_1x1_backward_supported(int channels, int c1, int c2, int c3, int radius) {
    return match_supported(channels, c1, c2, c3, radius) ? 1 : 0;
}

extern "C" size_t rmd_dicl_match_1x1_backward_workspace_bytes(int batch, int channels, int height, int width,
                                                              int radius, int c1, int c2, int c3) {
    if (!match_supported(channels, c1, c2, c3, radius) || batch <= 0 || height <= 0 || width <= 0) return 0;
    return grad_layout(batch, channels, (long long)height * width, c1, c2, c3).total;
}

extern "C" int rmd_dicl_match_1x1_backward(const float* grad_cost, const float* fmap1, const float* fmap2,
                                           const float* coords, int batch, int channels, int height, int width,
                                           int radius, const float* w1, const float* t1, const float* w2,
                                           const float* t2, const float* w3, const float* t3, const float* w4, int c1,
                                           int c2, int c3, int compute, float* grad_fmap1, float* grad_fmap2,
                                           float* grad_w1, float* grad_t1, float* grad_w2, float* grad_t2,
                                           float* grad_w3, float* grad_t3, float* grad_w4, float* grad_b4,
                                           void* workspace, void* stream) {
    RMD_REQUIRE(grad_cost && fmap1 && fmap2 && coords && w1 && t1 && w2 && t2 && w3 && t3 && w4 && workspace,
                RMD_ERR_ARG, "rmd_dicl_match_1x1_backward: null pointer");
    RMD_REQUIRE(compute == RMD_BF16X3, RMD_ERR_ARG,
                "rmd_dicl_match_1x1_backward: only compute = RMD_BF16X3 has a backward (the one-product mode's "
                "ReLU masks differ from float64's on 2-4 %% of the hidden units), got %d", compute);
    const int ngiven = (grad_w1 != nullptr) + (grad_t1 != nullptr) + (grad_w2 != nullptr) + (grad_t2 != nullptr) +
                       (grad_w3 != nullptr) + (grad_t3 != nullptr) + (grad_w4 != nullptr) + (grad_b4 != nullptr);
    RMD_REQUIRE(ngiven == 0 || ngiven == 8, RMD_ERR_ARG,
                "rmd_dicl_match_1x1_backward: the eight parameter-gradient pointers are all given or all NULL (%d given)",
                ngiven);
    if (int rc = match_check_shape("rmd_dicl_match_1x1_backward", batch, channels, height, width, radius, c1, c2, c3))
        return rc;
    const long long n = (long long)height * width;
    if (ngiven == 0 && !grad_fmap1 && !grad_fmap2) return RMD_OK;

    GradParams P;
    static_cast<MatchGeom&>(P) = match_geom(batch, channels, height, width, radius, c1, c2, c3);
    const Layout L = grad_layout(batch, channels, n, c1, c2, c3);
    P.nw = L.nw; P.nv = L.nv;
    P.params = ngiven == 8;
    const int grid = grad_grid(batch, n);
    hipStream_t st = as_stream(stream);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    bf16x8* frags = reinterpret_cast<bf16x8*>(ws);
    float* partw = reinterpret_cast<float*>(ws + L.partw_off);
    float* partv = reinterpret_cast<float*>(ws + L.partv_off);

    // plain fragments for the recomputed forward, transposed ones for the data backward
    match_pack<2>(match_pack_desc(w1, w2, w3, channels, c1, c2, c3, 2), P.nfrag, true, frags, st);
    if (grad_fmap2) (void)hipMemsetAsync(grad_fmap2, 0, sizeof(float) * (size_t)batch * channels * n, st);

#define RMD_MATCH_GRAD(EX, KF, M1, M2, M3)                                                                        \
    launch_lds(dicl_match_grad_kernel<EX, KF, M1, M2, M3>, grid, kThreads, kLdsBytes, st, grad_cost, fmap1, fmap2, \
               coords, frags, t1, t2, t3, w4, P, grad_fmap1, grad_fmap2, partw, partv)
    // the forward's classes: the two kernels cannot disagree on which instance a shape gets
    switch (match_class(P)) {
    case MatchClass::kExact2342: RMD_MATCH_GRAD(true, 2, 3, 4, 2); break;
    case MatchClass::kGuarded2221: RMD_MATCH_GRAD(false, 2, 2, 2, 1); break;
    case MatchClass::kGuarded4444: RMD_MATCH_GRAD(false, 4, 4, 4, 4); break;
    }
#undef RMD_MATCH_GRAD
    if (P.params) {
        ReduceOut O;
        O.w[0] = grad_w1; O.w[1] = grad_w2; O.w[2] = grad_w3;
        O.wn[0] = c1 * 2 * channels; O.wn[1] = c2 * c1; O.wn[2] = c3 * c2;
        O.v[0] = grad_w4; O.v[1] = grad_t1; O.v[2] = grad_t2; O.v[3] = grad_t3; O.v[4] = grad_b4;
        O.vn[0] = c3; O.vn[1] = c1; O.vn[2] = c2; O.vn[3] = c3; O.vn[4] = 1;
        dicl_match_grad_reduce_kernel<<<(L.nw + L.nv + 255) / 256, 256, 0, st>>>(partw, partv, grid, L.nw, L.nv, O);
    }
    return check_launch("rmd_dicl_match_1x1_backward");
}
