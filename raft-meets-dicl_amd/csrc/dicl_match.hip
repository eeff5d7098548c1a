// dicl_match.hip — fused dicl-1x1 cost: displacement gather + 1x1 MatchingNet in one MFMA kernel.
//
// Replaces (qzed/raft-meets-dicl v2) the gather/expand/cat of corr.dicl_1x1.CorrelationModule.forward
// (src/models/common/corr/dicl_1x1.py:51-79) together with MatchingNet1x1 (dicl_1x1.py:8-30) in eval
// mode: a per-(pixel, displacement) MLP 2C -> c1 -> c2 -> c3 -> 1 whose norm layers are folded into the
// weights (W', t) by the caller.  Neither the (B, d, d, 2C, h, w) stack nor any hidden activation is
// written to memory.
//
// Orientation (one wave, v_mfma_f32_32x32x16_bf16): 32 samples — 32 consecutive pixels at ONE
// displacement — sit on the MFMA column (lane & 31), channels on the row; weights are the A operand,
// activations the B operand.  A layer's f32 accumulator tile (32 channels x 32 samples, 16 registers)
// then IS two k-steps of the next layer's B operand after relu + cvt to bf16: registers 8s..8s+7 are
// the fragment of k-step s, element j of lane half hh holding channel 16s + 8(j>>2) + 4hh + (j&3).
// rmd_dicl_match_1x1's pack kernel writes every weight matrix as A fragments in that k order (bf16 hi
// and, for RMD_BF16X3, the bf16 of the residual), and the first layer's B fragments are built in the
// same order, so one fragment format serves all three layers.  No activation crosses lanes or LDS.
//
// Work split: a work item is a strip of 32 pixels and a share of its (2r+1)^2 displacements; the 8 waves
// of a (persistent) workgroup take displacements round-robin.  W1' x = W1a' f1[p] + W1b' f2sample: each
// wave computes the f1 half (+ t1) once per strip and starts every displacement's layer-1 accumulators
// from it, which halves layer 1.  The f2 samples are bilinear gathers from fmap2 through L2 (sample
// position, zero padding per tap and NaN for non-finite positions as rmd_dicl_stack at level 0).  The
// weight fragments live in LDS when they fit beside the biases (every mnet-scale <= 1 configuration
// does), else they are read from global memory.  The last layer (c3 -> 1) and all biases are f32 VALU.

#include "rmd_common.h"

#include <algorithm>

namespace rmd {
namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kMaxWidth = 128;                 // hidden widths and 2C
constexpr int kBiasBytes = 4 * kMaxWidth * 4;  // t1, t2, t3, w4 in LDS
constexpr int kLdsMax = 160 * 1024;
constexpr int kCUs = 256;

struct MatchParams {
    int B, C, n, h, w, radius;
    int kf;              // k-steps of one feature half: C / 16
    int m1, m2, m3;      // 32-row tiles of the three hidden layers
    int nfrag;           // A fragments (of 64 lanes x 8 bf16) of one part (hi or lo)
    int nstrips;         // 32-pixel strips per batch image
    int dsplit;          // workgroups sharing one strip's displacements
    float sx, sy;        // (w-1)/(w-1), (h-1)/(h-1): 1, or NaN for a 1-pixel side, as the reference
};

// channel of element j of lane half hh in k-step ks (the accumulator-as-operand k order)
__host__ __device__ __forceinline__ int frag_k(int ks, int hh, int j) { return 16 * ks + 8 * (j >> 2) + 4 * hh + (j & 3); }

// ---- weights -> A fragments ------------------------------------------------------------------------
// fragment (layer base + mo * ksteps + ks), lane l = (row 32 mo + (l & 31), half l >> 5), element j:
// W[row][frag_k(ks, l >> 5, j)].  hi part first, then (parts == 2) the lo part.
__global__ void __launch_bounds__(256)
dicl_match_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ w3,
                       MatchParams P, int parts, bf16x8* __restrict__ frags) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= P.nfrag * 64) return;
    int f = id >> 6;
    const int lane = id & 63;
    const int n1 = P.m1 * 2 * P.kf, n2 = P.m2 * 2 * P.m1;
    const float* wm;
    int ksteps;
    if (f < n1) { wm = w1; ksteps = 2 * P.kf; }
    else if (f < n1 + n2) { wm = w2; ksteps = 2 * P.m1; f -= n1; }
    else { wm = w3; ksteps = 2 * P.m2; f -= n1 + n2; }
    const int mo = f / ksteps, ks = f - mo * ksteps;
    const float* row = wm + (size_t)(32 * mo + (lane & 31)) * (16 * ksteps);
    bf16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = row[frag_k(ks, lane >> 5, j)];
        hi[j] = (__bf16)v;
        lo[j] = (__bf16)(v - (float)hi[j]);
    }
    frags[id] = hi;
    if (parts == 2) frags[(size_t)P.nfrag * 64 + id] = lo;
}

// ---- device helpers --------------------------------------------------------------------------------

// bilinear, align_corners=True, zero padding per tap; a non-finite position samples NaN (dicl.hip's
// make_taps_fwd, restated: the two kernels must agree on the sample, not share an object file)
struct Taps {
    int idx[4];
    float wgt[4];
};

__device__ __forceinline__ Taps match_taps(float px, float py, int hl, int wl) {
    Taps t;
    const bool finite = __builtin_isfinite(px) && __builtin_isfinite(py);
    px = fminf(fmaxf(px, -1.0e6f), 1.0e6f);
    py = fminf(fmaxf(py, -1.0e6f), 1.0e6f);
    const float fx0 = floorf(px), fy0 = floorf(py);
    const float fx = px - fx0, fy = py - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
        const bool ok = finite && xx >= 0 && xx < wl && yy >= 0 && yy < hl;
        const float wx = (k & 1) ? fx : 1.f - fx;
        const float wy = (k >> 1) ? fy : 1.f - fy;
        t.idx[k] = ok ? yy * wl + xx : 0;
        t.wgt[k] = finite ? (ok ? wx * wy : 0.f) : __builtin_nanf("");
    }
    return t;
}

// torch's relu keeps NaN (fmaxf(x, 0) would drop it): IEEE maximum, one v_maximum3_f32
__device__ __forceinline__ float relu_nan(float x) { return __builtin_elementwise_maximum(x, 0.f); }

// a float at a 32-bit byte offset from a wave-uniform base (scalar base + vector offset addressing)
__device__ __forceinline__ float ld_off(const float* base, unsigned byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

// frag_k without the lane-half term: the wave-uniform part of a fragment element's channel
__device__ __forceinline__ int frag_k_uniform(int ks, int j) { return 16 * ks + 8 * (j >> 2) + (j & 3); }

template <int NP>
__device__ __forceinline__ void split8(const float* v, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        hi[j] = (__bf16)v[j];
        if constexpr (NP == 3) lo[j] = (__bf16)(v[j] - (float)hi[j]);
    }
}

// acc += A . B with NP bf16 products: hi.hi, and for NP == 3 also lo.hi and hi.lo (small terms first)
template <int NP>
__device__ __forceinline__ void mma(f32x16& acc, const bf16x8& ah, const bf16x8& al, const bf16x8& bh,
                                    const bf16x8& bl) {
    if constexpr (NP == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// accumulator row of register i for lane half hh (32x32 C/D map)
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

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

    for (int i = tid; i < 4 * kMaxWidth; i += kThreads) {
        const int which = i / kMaxWidth, c = i - which * kMaxWidth;
        const float* src = which == 0 ? t1 : which == 1 ? t2 : which == 2 ? t3 : w4;
        const int width = 32 * (which == 0 ? m1 : which == 1 ? m2 : m3);
        sb[i] = c < width ? src[c] : 0.f;
    }
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
    const int fb1 = 0, fb2 = m1 * 2 * kf, fb3 = fb2 + m2 * 2 * m1;   // fragment base of each layer

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
#pragma unroll
            for (int ks = 0; ks < KF; ++ks) {
                if (EXACT || ks < kf) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = ld_off(f1b + (size_t)frag_k_uniform(ks, j) * n, off1);
                    split8<NP>(v, xh[ks], xl[ks]);
                }
            }
#pragma unroll
            for (int mo = 0; mo < M1; ++mo) {
                if (EXACT || mo < m1) {
                    f32x16 acc;
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[i] = sb[32 * mo + acc_row(i, hh)];
#pragma unroll
                    for (int ks = 0; ks < KF; ++ks) {
                        if (EXACT || ks < kf) {
                            const int f = fb1 + mo * 2 * kf + ks;
                            mma<NP>(acc, afrag(f, 0), NP == 3 ? afrag(f, 1) : bf16x8{}, xh[ks], xl[ks]);
                        }
                    }
                    base[mo] = acc;
                }
            }
        }

        for (int disp = part * kWaves + wave; disp < dd; disp += kWaves * P.dsplit) {
            const int a = disp / d, bb = disp - a * d;
            const float px = (cx + (float)(a - P.radius)) * P.sx;
            const float py = (cy + (float)(bb - P.radius)) * P.sy;
            const Taps t = match_taps(px, py, P.h, P.w);
            unsigned off2[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) off2[k] = (half_off + (unsigned)t.idx[k]) * 4u;

            // f2 half of the column: bilinear samples, straight into layer-1 B fragments
            bf16x8 xh[KF], xl[KF];
#pragma unroll
            for (int ks = 0; ks < KF; ++ks) {
                if (EXACT || ks < kf) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float* fc = f2b + (size_t)frag_k_uniform(ks, j) * n;      // wave-uniform
                        v[j] = t.wgt[0] * ld_off(fc, off2[0]) + t.wgt[1] * ld_off(fc, off2[1]) +
                               t.wgt[2] * ld_off(fc, off2[2]) + t.wgt[3] * ld_off(fc, off2[3]);
                    }
                    split8<NP>(v, xh[ks], xl[ks]);
                }
            }

            // layer 1 (f2 half on top of base) -> layer-2 B fragments
            bf16x8 yh[2 * M1], yl[2 * M1];
#pragma unroll
            for (int mo = 0; mo < M1; ++mo) {
                if (EXACT || mo < m1) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = base[mo];
#pragma unroll
                    for (int ks = 0; ks < KF; ++ks) {
                        if (EXACT || ks < kf) {
                            const int f = fb1 + mo * 2 * kf + kf + ks;
                            mma<NP>(acc, afrag(f, 0), NP == 3 ? afrag(f, 1) : bf16x8{}, xh[ks], xl[ks]);
                        }
                    }
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        float v[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = relu_nan(acc[8 * s + j]);
                        split8<NP>(v, yh[2 * mo + s], yl[2 * mo + s]);
                    }
                }
            }

            // layer 2 -> layer-3 B fragments
            bf16x8 zh[2 * M2], zl[2 * M2];
#pragma unroll
            for (int mo = 0; mo < M2; ++mo) {
                if (EXACT || mo < m2) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = {};
#pragma unroll
                    for (int ks = 0; ks < 2 * M1; ++ks) {
                        if (EXACT || ks < 2 * m1) {
                            const int f = fb2 + mo * 2 * m1 + ks;
                            mma<NP>(acc, afrag(f, 0), NP == 3 ? afrag(f, 1) : bf16x8{}, yh[ks], yl[ks]);
                        }
                    }
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        float v[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            v[j] = relu_nan(acc[8 * s + j] + sb[kMaxWidth + 32 * mo + acc_row(8 * s + j, hh)]);
                        split8<NP>(v, zh[2 * mo + s], zl[2 * mo + s]);
                    }
                }
            }

            // layer 3, then the c3 -> 1 layer on the VALU: this lane's rows, then the other half's
            float cost = 0.f;
#pragma unroll
            for (int mo = 0; mo < M3; ++mo) {
                if (EXACT || mo < m3) {
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = {};
#pragma unroll
                    for (int ks = 0; ks < 2 * M2; ++ks) {
                        if (EXACT || ks < 2 * m2) {
                            const int f = fb3 + mo * 2 * m2 + ks;
                            mma<NP>(acc, afrag(f, 0), NP == 3 ? afrag(f, 1) : bf16x8{}, zh[ks], zl[ks]);
                        }
                    }
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

bool width_ok(int c) { return c >= 32 && c <= kMaxWidth && c % 32 == 0; }

bool match_supported(int channels, int c1, int c2, int c3, int radius) {
    return channels >= 16 && channels % 16 == 0 && 2 * channels <= kMaxWidth && width_ok(c1) && width_ok(c2) &&
           width_ok(c3) && radius >= 1 && radius <= 4;
}

int match_nfrag(int channels, int c1, int c2, int c3) {
    return (c1 / 32) * (2 * channels / 16) + (c2 / 32) * (c1 / 16) + (c3 / 32) * (c2 / 16);
}

template <int NP>
int launch_match(const float* f1, const float* f2, const float* coords, const bf16x8* frags, const float* t1,
                 const float* t2, const float* t3, const float* w4, const float* b4, const MatchParams& P, int grid,
                 bool wlds, size_t lds, float* out, hipStream_t st) {
#define RMD_MATCH(WLDS, EX, KF, M1, M2, M3)                                                                    \
    do {                                                                                                        \
        auto k = dicl_match_kernel<NP, WLDS, EX, KF, M1, M2, M3>;                                               \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  (int)lds);                                                                   \
        k<<<grid, kThreads, lds, st>>>(f1, f2, coords, frags, t1, t2, t3, w4, b4, P, out);                      \
    } while (0)
    // the two shapes of the reference's configurations have loops of their own size (they always fit LDS);
    // everything else runs the 4-tile loops guarded by the sizes, weights from global memory past LDS
    // (three-product mode only: the widest one-product fragment set is 96 KB)
    if (P.kf == 2 && P.m1 == 3 && P.m2 == 4 && P.m3 == 2) RMD_MATCH(true, true, 2, 3, 4, 2);         // C = 32, mnet scale 1
    else if (P.kf <= 2 && P.m1 <= 2 && P.m2 <= 2 && P.m3 <= 1) RMD_MATCH(true, false, 2, 2, 2, 1);   // mnet scale 0.5
    else if (wlds) RMD_MATCH(true, false, 4, 4, 4, 4);
    else if constexpr (NP == 3) RMD_MATCH(false, false, 4, 4, 4, 4);
    else RMD_REQUIRE(false, RMD_ERR_SHAPE, "rmd_dicl_match_1x1: one-product weight fragments always fit LDS");
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
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "rmd_dicl_match_1x1: bad sizes");
    RMD_REQUIRE(match_supported(channels, c1, c2, c3, radius), RMD_ERR_SHAPE,
                "rmd_dicl_match_1x1: unsupported (channels=%d widths=%d,%d,%d radius=%d): channels a multiple of 16 "
                "up to 64, widths multiples of 32 up to 128, radius 1..4", channels, c1, c2, c3, radius);
    const long long n = (long long)height * width;
    // 32-bit lane offsets into one image's feature map, 64-bit everywhere else (the output included)
    RMD_REQUIRE(n * channels < (1ll << 30), RMD_ERR_SHAPE, "rmd_dicl_match_1x1: %lld pixels x %d channels per image",
                n, channels);
    MatchParams P;
    P.B = batch; P.C = channels; P.n = (int)n; P.h = height; P.w = width; P.radius = radius;
    P.kf = channels / 16; P.m1 = c1 / 32; P.m2 = c2 / 32; P.m3 = c3 / 32;
    P.nfrag = match_nfrag(channels, c1, c2, c3);
    P.nstrips = (int)((n + 31) / 32);
    // 0/0 -> NaN for a 1-pixel side, exactly as the reference's normalisation (rmd_dicl_stack)
    P.sx = (float)(width - 1) / (float)(width - 1);
    P.sy = (float)(height - 1) / (float)(height - 1);
    const long long strips = (long long)batch * P.nstrips;
    const int dd = (2 * radius + 1) * (2 * radius + 1);
    // few strips: several workgroups share one strip's displacements, so that every CU has work
    P.dsplit = (int)std::min<long long>(std::max<long long>(kCUs / strips, 1), (dd + kWaves - 1) / kWaves);
    const int grid = (int)std::min<long long>(strips * P.dsplit, kCUs);
    const int parts = compute == RMD_BF16X3 ? 2 : 1;
    hipStream_t st = as_stream(stream);
    bf16x8* frags = reinterpret_cast<bf16x8*>(workspace);
    dicl_match_pack_kernel<<<(P.nfrag * 64 + 255) / 256, 256, 0, st>>>(w1, w2, w3, P, parts, frags);
    const size_t wbytes = (size_t)P.nfrag * 64 * sizeof(bf16x8) * parts;
    const bool wlds = kBiasBytes + wbytes <= (size_t)kLdsMax;
    const size_t lds = kBiasBytes + (wlds ? wbytes : 0);
    return compute == RMD_BF16X3
               ? launch_match<3>(fmap1, fmap2, coords, frags, t1, t2, t3, w4, b4, P, grid, wlds, lds, out, st)
               : launch_match<1>(fmap1, fmap2, coords, frags, t1, t2, t3, w4, b4, P, grid, wlds, lds, out, st);
}
