// dicl_match.hip — fused dicl-1x1 cost: displacement gather + 1x1 MatchingNet in one MFMA kernel.
//
// Replaces (qzed/raft-meets-dicl v2) the gather/expand/cat of corr.dicl_1x1.CorrelationModule.forward
// (src/models/common/corr/dicl_1x1.py:51-79) together with MatchingNet1x1 (dicl_1x1.py:8-30) in eval
// mode: a per-(pixel, displacement) MLP 2C -> c1 -> c2 -> c3 -> 1 whose norm layers are folded into the
// weights (W', t) by the caller.  Neither the (B, d, d, 2C, h, w) stack nor any hidden activation is
// written to memory.
//
// Orientation, fragment order, the weight pack kernel and the forward up to the layer-2 activations:
// dicl_match_common.h, shared with the backward (dicl_match_grad.hip), which recomputes this forward.
//
// Work split: a work item is a strip of 32 pixels and a share of its (2r+1)^2 displacements; the 8 waves
// of a (persistent) workgroup take displacements round-robin.  W1' x = W1a' f1[p] + W1b' f2sample: each
// wave computes the f1 half (+ t1) once per strip and starts every displacement's layer-1 accumulators
// from it, which halves layer 1.  The f2 samples are bilinear gathers from fmap2 through L2 (sample
// position, zero padding per tap and NaN for non-finite positions as rmd_dicl_stack at level 0).  The
// weight fragments live in LDS when they fit beside the biases (every mnet-scale <= 1 configuration
// does), else they are read from global memory.  The last layer (c3 -> 1) and all biases are f32 VALU.

#include "dicl_match_common.h"

#include <algorithm>

namespace rmd {
namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kLdsMax = 160 * 1024;

struct MatchParams : MatchGeom {
    int dsplit;          // workgroups sharing one strip's displacements
};

// NP: bf16 products per layer.  WLDS: weight fragments staged in LDS.  KF, M1..M3: compile-time bounds of
// the k-step / tile loops (register arrays); EXACT: they are the sizes themselves, else P's sizes guard.
template <int NP, bool WLDS, bool EXACT, int KF, int M1, int M2, int M3>
__global__ void __launch_bounds__(kThreads)
dicl_match_kernel(const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ coords,
                  const bf16x8* __restrict__ frags, const float* __restrict__ t1, const float* __restrict__ t2,
                  const float* __restrict__ t3, const float* __restrict__ w4, const float* __restrict__ b4,
                  MatchParams P, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    float* const sb = reinterpret_cast<float*>(sm);                 // t1 | t2 | t3 | w4, kMaxWidth each
    const bf16x8* const sfr = reinterpret_cast<const bf16x8*>(sm + kBiasBytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int kf = EXACT ? KF : P.kf, m1 = EXACT ? M1 : P.m1, m2 = EXACT ? M2 : P.m2, m3 = EXACT ? M3 : P.m3;

    stage_biases(sb, t1, t2, t3, w4, m1, m2, m3, tid, kThreads);
    if constexpr (WLDS) {
        bf16x8* dst = reinterpret_cast<bf16x8*>(sm + kBiasBytes);
        const int total = P.nfrag * 64 * (NP == 3 ? 2 : 1);
        for (int i = tid; i < total; i += kThreads) dst[i] = frags[i];
    }
    __syncthreads();
    const float bias4 = b4[0];

    auto afrag = [&](int f, int part) -> bf16x8 {
        const unsigned i = (unsigned)((part * P.nfrag + f) * 64 + lane);
        if constexpr (WLDS) return sfr[i];
        else return frags[i];
    };
    const int fb2 = m1 * 2 * kf, fb3 = fb2 + m2 * 2 * m1;   // fragment base of layers 2, 3 (layer 1: 0)

    const int d = 2 * P.radius + 1, dd = d * d;
    const int n = P.n;
    const long long items = (long long)P.B * P.nstrips * P.dsplit;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int part = (int)(item % P.dsplit);
        const long long strip = item / P.dsplit;
        const int b = (int)(strip / P.nstrips);
        const int p = (int)(strip - (long long)b * P.nstrips) * 32 + r;
        const bool valid = p < n;
        const int pc = valid ? p : n - 1;
        const float cx = coords[(size_t)b * 2 * n + pc], cy = coords[((size_t)b * 2 + 1) * n + pc];
        const float* f1b = f1 + (size_t)b * P.C * n;          // wave-uniform bases, 32-bit lane offsets
        const float* f2b = f2 + (size_t)b * P.C * n;
        const unsigned half_off = (unsigned)(4 * hh * n);     // this lane half's channel group (frag_k)
        const unsigned off1 = (half_off + (unsigned)pc) * 4u;

        // layer-1 accumulators of the f1 half, plus t1: once per strip
        f32x16 base[M1];
        {
            bf16x8 xh[KF], xl[KF];
            f1_frags<NP, EXACT, KF>(f1b, n, off1, kf, xh, xl);
            layer1_base<NP, EXACT, KF, M1>(base, afrag, sb, kf, m1, hh, xh, xl);
        }

        for (int disp = part * kWaves + wave; disp < dd; disp += kWaves * P.dsplit) {
            const int a = disp / d, bb = disp - a * d;
            const float px = (cx + (float)(a - P.radius)) * P.sx;
            const float py = (cy + (float)(bb - P.radius)) * P.sy;
            const Taps t = make_taps_fwd(px, py, P.h, P.w);
            bf16x8 xh[KF], xl[KF], yh[2 * M1], yl[2 * M1], zh[2 * M2], zl[2 * M2];
            f2_frags<NP, EXACT, KF>(f2b, n, half_off, t, kf, xh, xl);
            layer1<NP, EXACT, false, KF, M1>(base, afrag, kf, m1, hh, xh, xl, yh, yl, nullptr);
            // layer 2 -> layer-3 B fragments: the loop of dicl_match_common.h's layer2(), kept here.  Called as
            // that function, the EXACT instances take 240 / 164 VGPRs instead of 186 / 140 (the bf16 one 4 below
            // the limit of its 3 waves per SIMD)
#pragma unroll
            for (int mo = 0; mo < M2; ++mo) {
                if (EXACT || mo < m2) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = {};
                    mma_tile<NP, EXACT, 2 * M1>(acc, afrag, fb2 + mo * 2 * m1, 0, 2 * m1, yh, yl);
                    relu_frags<NP, true, false>(acc, sb + kMaxWidth + 32 * mo, hh, zh + 2 * mo, zl + 2 * mo);
                }
            }

            // layer 3, then the c3 -> 1 layer on the VALU: this lane's rows, then the other half's
            float cost = 0.f;
#pragma unroll
            for (int mo = 0; mo < M3; ++mo) {
                if (EXACT || mo < m3) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = {};
                    mma_tile<NP, EXACT, 2 * M2>(acc, afrag, fb3 + mo * 2 * m2, 0, 2 * m2, zh, zl);
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = 32 * mo + acc_row(i, hh);
                        cost += sb[3 * kMaxWidth + row] * relu_nan(acc[i] + sb[2 * kMaxWidth + row]);
                    }
                }
            }
            cost += __shfl_xor(cost, 32, 64);
            if (hh == 0 && valid) out[((size_t)b * dd + disp) * n + p] = cost + bias4;
        }
    }
}

template <int NP>
int launch_match(const float* f1, const float* f2, const float* coords, const bf16x8* frags, const float* t1,
                 const float* t2, const float* t3, const float* w4, const float* b4, const MatchParams& P, int grid,
                 bool wlds, size_t lds, float* out, hipStream_t st) {
#define RMD_MATCH(WLDS, EX, KF, M1, M2, M3)                                                                       \
    launch_lds(dicl_match_kernel<NP, WLDS, EX, KF, M1, M2, M3>, grid, kThreads, lds, st, f1, f2, coords, frags, t1, \
               t2, t3, w4, b4, P, out)
    // the exact and the 2/2/2/1 class always fit LDS; the 4-tile loops read the weights from global memory
    // past LDS (three-product mode only: the widest one-product fragment set is 96 KB)
    switch (match_class(P)) {
    case MatchClass::kExact2342: RMD_MATCH(true, true, 2, 3, 4, 2); break;
    case MatchClass::kGuarded2221: RMD_MATCH(true, false, 2, 2, 2, 1); break;
    case MatchClass::kGuarded4444:
        if (wlds) RMD_MATCH(true, false, 4, 4, 4, 4);
        else if constexpr (NP == 3) RMD_MATCH(false, false, 4, 4, 4, 4);
        else RMD_REQUIRE(false, RMD_ERR_SHAPE, "rmd_dicl_match_1x1: one-product weight fragments always fit LDS");
        break;
    }
#undef RMD_MATCH
    return check_launch("rmd_dicl_match_1x1");
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" int rmd_dicl_match_1x1_supported(int channels, int c1, int c2, int c3, int radius) {
    return match_supported(channels, c1, c2, c3, radius) ? 1 : 0;
}

extern "C" size_t rmd_dicl_match_1x1_workspace_bytes(int channels, int c1, int c2, int c3, int compute) {
    if (!match_supported(channels, c1, c2, c3, 1) || (compute != RMD_BF16X3 && compute != RMD_BF16)) return 0;
    return (size_t)match_nfrag(channels, c1, c2, c3) * 64 * sizeof(bf16x8) * (compute == RMD_BF16X3 ? 2 : 1);
}

extern "C" int rmd_dicl_match_1x1(const float* fmap1, const float* fmap2, const float* coords, int batch, int channels,
                                  int height, int width, int radius, const float* w1, const float* t1,
                                  const float* w2, const float* t2, const float* w3, const float* t3,
                                  const float* w4, const float* b4, int c1, int c2, int c3, int compute, float* out,
                                  void* workspace, void* stream) {
    RMD_REQUIRE(fmap1 && fmap2 && coords && w1 && t1 && w2 && t2 && w3 && t3 && w4 && b4 && out && workspace,
                RMD_ERR_ARG, "rmd_dicl_match_1x1: null pointer");
    RMD_REQUIRE(compute == RMD_BF16X3 || compute == RMD_BF16, RMD_ERR_ARG,
                "rmd_dicl_match_1x1: compute must be RMD_BF16X3 or RMD_BF16, got %d", compute);
    if (int rc = match_check_shape("rmd_dicl_match_1x1", batch, channels, height, width, radius, c1, c2, c3)) return rc;
    MatchParams P;
    static_cast<MatchGeom&>(P) = match_geom(batch, channels, height, width, radius, c1, c2, c3);
    const long long strips = (long long)batch * P.nstrips;
    const int dd = (2 * radius + 1) * (2 * radius + 1);
    // few strips: several workgroups share one strip's displacements, so that every CU has work
    P.dsplit = (int)std::min<long long>(std::max<long long>(kCUs / strips, 1), (dd + kWaves - 1) / kWaves);
    const int grid = (int)std::min<long long>(strips * P.dsplit, kCUs);
    const int parts = compute == RMD_BF16X3 ? 2 : 1;      // hi, and the lo part of the three-product mode
    hipStream_t st = as_stream(stream);
    bf16x8* frags = reinterpret_cast<bf16x8*>(workspace);
    match_pack<1>(match_pack_desc(w1, w2, w3, channels, c1, c2, c3, 1), P.nfrag, parts == 2, frags, st);
    const size_t wbytes = (size_t)P.nfrag * 64 * sizeof(bf16x8) * parts;
    const bool wlds = kBiasBytes + wbytes <= (size_t)kLdsMax;
    const size_t lds = kBiasBytes + (wlds ? wbytes : 0);
    return compute == RMD_BF16X3
               ? launch_match<3>(fmap1, fmap2, coords, frags, t1, t2, t3, w4, b4, P, grid, wlds, lds, out, st)
               : launch_match<1>(fmap1, fmap2, coords, frags, t1, t2, t3, w4, b4, P, grid, wlds, lds, out, st);
}
