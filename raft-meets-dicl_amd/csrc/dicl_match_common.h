// dicl_match_common.h — what the fused dicl-1x1 cost (dicl_match.hip) and its recomputing backward
// (dicl_match_grad.hip) mean the same thing by: the MFMA orientation and fragment order, the supported
// shapes and their instance classes, the weight pack kernel, and the forward of the MLP up to the layer-2
// activations.  The backward recomputes the forward with these very templates (NP = 3), so the two kernels
// cannot disagree on the sample, the products or their order; tests/test_gpu_dicl_match_digest.py pins the
// outputs of both bit for bit.  The split-bf16 arithmetic itself (types, split, mma<NP>, acc_row) is
// mfma_bf16.h's, shared with every other MFMA kernel.
//
// Orientation (one wave, v_mfma_f32_32x32x16_bf16): 32 samples — 32 consecutive pixels at ONE
// displacement — sit on the MFMA column (lane & 31), channels on the row; weights are the A operand,
// activations the B operand.  A layer's f32 accumulator tile (32 channels x 32 samples, 16 registers)
// then IS two k-steps of the next layer's B operand after relu + cvt to bf16: registers 8s..8s+7 are
// the fragment of k-step s, element j of lane half hh holding channel 16s + 8(j>>2) + 4hh + (j&3).
// The pack kernel writes every weight matrix as A fragments in that k order (bf16 hi and the bf16 of the
// residual), and the first layer's B fragments are built in the same order, so one fragment format serves
// all layers — and, with W^T packed the same way, the data backward.  No activation crosses lanes or LDS.
#pragma once

#include "dicl_taps.h"
#include "mfma_bf16.h"

namespace rmd {

constexpr int kMaxWidth = 128;                 // hidden widths and 2C
constexpr int kBiasBytes = 4 * kMaxWidth * 4;  // t1, t2, t3, w4 in LDS
constexpr int kCUs = 256;

// ---- shapes (host) ---------------------------------------------------------------------------------

struct MatchGeom {
    int B, C, n, h, w, radius;
    int kf;              // k-steps of one feature half: C / 16 (= 32-row tiles of the 2C input rows)
    int m1, m2, m3;      // 32-row tiles of the three hidden layers
    int nfrag;           // A fragments (of 64 lanes x 8 bf16) of one part (hi or lo) of one orientation
    int nstrips;         // 32-pixel strips per batch image
    float sx, sy;        // (w-1)/(w-1), (h-1)/(h-1): 1, or NaN for a 1-pixel side, as the reference
};

inline bool width_ok(int c) { return c >= 32 && c <= kMaxWidth && c % 32 == 0; }

inline bool match_supported(int channels, int c1, int c2, int c3, int radius) {
    return channels >= 16 && channels % 16 == 0 && 2 * channels <= kMaxWidth && width_ok(c1) && width_ok(c2) &&
           width_ok(c3) && radius >= 1 && radius <= 4;
}

inline int match_nfrag(int channels, int c1, int c2, int c3) {
    return (c1 / 32) * (2 * channels / 16) + (c2 / 32) * (c1 / 16) + (c3 / 32) * (c2 / 16);
}

// the shape checks of entry point `name`
inline int match_check_shape(const char* name, int batch, int channels, int height, int width, int radius, int c1,
                             int c2, int c3) {
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(match_supported(channels, c1, c2, c3, radius), RMD_ERR_SHAPE,
                "%s: unsupported (channels=%d widths=%d,%d,%d radius=%d): channels a multiple of 16 up to 64, "
                "widths multiples of 32 up to 128, radius 1..4", name, channels, c1, c2, c3, radius);
    const long long n = (long long)height * width;
    // 32-bit lane offsets into one image's feature map, 64-bit everywhere else (the outputs included)
    RMD_REQUIRE(n * channels < (1ll << 30), RMD_ERR_SHAPE, "%s: %lld pixels x %d channels per image", name, n,
                channels);
    return RMD_OK;
}

inline MatchGeom match_geom(int batch, int channels, int height, int width, int radius, int c1, int c2, int c3) {
    MatchGeom G;
    const long long n = (long long)height * width;
    G.B = batch; G.C = channels; G.n = (int)n; G.h = height; G.w = width; G.radius = radius;
    G.kf = channels / 16; G.m1 = c1 / 32; G.m2 = c2 / 32; G.m3 = c3 / 32;
    G.nfrag = match_nfrag(channels, c1, c2, c3);
    G.nstrips = (int)((n + 31) / 32);
    // 0/0 -> NaN for a 1-pixel side, exactly as the reference's normalisation (rmd_dicl_stack)
    G.sx = (float)(width - 1) / (float)(width - 1);
    G.sy = (float)(height - 1) / (float)(height - 1);
    return G;
}

// The kernel instance of a shape: the two shapes of the reference's configurations have loops of their own
// size; everything else runs the 4-tile loops guarded by the sizes.
enum class MatchClass {
    kExact2342,       // C = 32, mnet scale 1: <EXACT, KF 2, M 3, 4, 2>
    kGuarded2221,     // mnet scale 0.5 and below: <guarded, 2, 2, 2, 1>
    kGuarded4444,     // <guarded, 4, 4, 4, 4>
};

inline MatchClass match_class(const MatchGeom& G) {
    if (G.kf == 2 && G.m1 == 3 && G.m2 == 4 && G.m3 == 2) return MatchClass::kExact2342;
    if (G.kf <= 2 && G.m1 <= 2 && G.m2 <= 2 && G.m3 <= 1) return MatchClass::kGuarded2221;
    return MatchClass::kGuarded4444;
}

// a kernel with `lds` bytes of dynamic LDS, past the 64 KB default
template <typename K, typename... Args>
inline void launch_lds(K kernel, int grid, int threads, size_t lds, hipStream_t st, Args... args) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    kernel<<<grid, threads, lds, st>>>(args...);
}

// ---- fragment layout -------------------------------------------------------------------------------

// channel of element j of lane half hh in k-step ks (the accumulator-as-operand k order)
__host__ __device__ __forceinline__ int frag_k(int ks, int hh, int j) { return 16 * ks + 8 * (j >> 2) + 4 * hh + (j & 3); }

// frag_k without the lane-half term: the wave-uniform part of a fragment element's channel
__device__ __forceinline__ int frag_k_uniform(int ks, int j) { return 16 * ks + 8 * (j >> 2) + (j & 3); }

// ---- weights -> A fragments ------------------------------------------------------------------------

// the matrices of the pack kernel: A[row][k] = src[row * row_stride + k * k_stride]; matrix m owns the
// fragments from first[m] up to the next matrix's first
struct PackDesc {
    const float* src[6];
    int row_stride[6], k_stride[6], ksteps[6], first[6];
};

// W1, W2, W3 (matrices 0..2) and, with two orientations, W1^T, W2^T, W3^T (3..5)
inline PackDesc match_pack_desc(const float* w1, const float* w2, const float* w3, int channels, int c1, int c2,
                                int c3, int orientations) {
    PackDesc D = {};
    const float* src[3] = {w1, w2, w3};
    const int cin[3] = {2 * channels, c1, c2}, cout[3] = {c1, c2, c3};
    int first = 0;
    for (int o = 0; o < orientations; ++o) {
        for (int l = 0; l < 3; ++l) {
            const int m = 3 * o + l;
            D.src[m] = src[l];
            D.row_stride[m] = o == 0 ? cin[l] : 1;          // plain: A = W_l; transposed: A[row][k] = W_l[k][row]
            D.k_stride[m] = o == 0 ? 1 : cin[l];
            D.ksteps[m] = (o == 0 ? cin[l] : cout[l]) / 16;
            D.first[m] = first;
            first += (cout[l] / 32) * (cin[l] / 16);
        }
    }
    return D;
}

// fragment (first[m] + mo * ksteps + ks), lane l = (row 32 mo + (l & 31), half l >> 5), element j:
// A[row][frag_k(ks, l >> 5, j)].  Parts of nfrag fragments each: plain hi, plain lo (if `lo`: the bf16 of the
// residual, for the three-product mode), then (ORIENTATIONS == 2) transposed hi, transposed lo.
template <int ORIENTATIONS>
__global__ void __launch_bounds__(256)
dicl_match_pack_kernel(PackDesc D, int nfrag, int lo, bf16x8* __restrict__ frags) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= ORIENTATIONS * nfrag * 64) return;
    const int fa = id >> 6, lane = id & 63;
    // the matrix that owns fragment fa (constant indices: the descriptor stays in scalar registers)
    const float* src = D.src[0];
    int row_stride = D.row_stride[0], k_stride = D.k_stride[0], ksteps = D.ksteps[0], first = 0;
#pragma unroll
    for (int m = 1; m < 3 * ORIENTATIONS; ++m) {
        if (fa >= D.first[m]) {
            src = D.src[m];
            row_stride = D.row_stride[m]; k_stride = D.k_stride[m]; ksteps = D.ksteps[m]; first = D.first[m];
        }
    }
    const int f = fa - first;
    const int mo = f / ksteps, ks = f - mo * ksteps;
    const float* row = src + (size_t)(32 * mo + (lane & 31)) * row_stride;
    bf16x8 hi, lopart;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = row[(size_t)frag_k(ks, lane >> 5, j) * k_stride];
        hi[j] = bf16_hi(v);
        lopart[j] = bf16_lo(v, hi[j]);
    }
    // first[3] == nfrag: plain fragments fill parts 0 / 1, transposed ones parts 2 / 3
    const int orient = fa >= nfrag ? 1 : 0;
    const size_t at = ((size_t)(2 * orient) * nfrag + (fa - orient * nfrag)) * 64 + lane;
    frags[at] = hi;
    if (lo) frags[at + (size_t)nfrag * 64] = lopart;
}

template <int ORIENTATIONS>
inline void match_pack(const PackDesc& D, int nfrag, bool lo, bf16x8* frags, hipStream_t st) {
    dicl_match_pack_kernel<ORIENTATIONS><<<(ORIENTATIONS * nfrag * 64 + 255) / 256, 256, 0, st>>>(D, nfrag, lo ? 1 : 0,
                                                                                                 frags);
}

// ---- device helpers --------------------------------------------------------------------------------

// torch's relu keeps NaN (fmaxf(x, 0) would drop it): IEEE maximum, one v_maximum3_f32
__device__ __forceinline__ float relu_nan(float x) { return __builtin_elementwise_maximum(x, 0.f); }

// a float at a 32-bit byte offset from a wave-uniform base (scalar base + vector offset addressing)
__device__ __forceinline__ float ld_off(const float* base, unsigned byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

// t1 | t2 | t3 | w4 into LDS, kMaxWidth floats each, zero past a layer's width (the caller synchronises)
__device__ __forceinline__ void stage_biases(float* sb, const float* __restrict__ t1, const float* __restrict__ t2,
                                             const float* __restrict__ t3, const float* __restrict__ w4, int m1, int m2,
                                             int m3, int tid, int threads) {
    for (int i = tid; i < 4 * kMaxWidth; i += threads) {
        const int which = i / kMaxWidth, c = i - which * kMaxWidth;
        const float* src = which == 0 ? t1 : which == 1 ? t2 : which == 2 ? t3 : w4;
        const int width = 32 * (which == 0 ? m1 : which == 1 ? m2 : m3);
        sb[i] = c < width ? src[c] : 0.f;
    }
}

// ---- the forward, up to the layer-2 activations ----------------------------------------------------
// KS, MO: compile-time bounds of the k-step / tile loops (register arrays); EXACT: they are the sizes
// themselves, else the run-time sizes guard.  afrag(f, part): A fragment f of part `part` for this lane.

// one output tile: acc += A[f0 .. f0 + ksteps) . b, A's hi part `part`, its lo part `part + 1`
template <int NP, bool EXACT, int KS, class AFrag>
__device__ __forceinline__ void mma_tile(f32x16& acc, const AFrag& afrag, int f0, int part, int ksteps,
                                         const bf16x8* bh, const bf16x8* bl) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (EXACT || ks < ksteps) {
            const int f = f0 + ks;
            mma<NP>(acc, afrag(f, part), NP == 3 ? afrag(f, part + 1) : bf16x8{}, bh[ks], bl[ks]);
        }
    }
}

// f1 of this lane's pixel (byte offset off1 into channel 4 hh) as layer-1 B fragments
template <int NP, bool EXACT, int KF>
__device__ __forceinline__ void f1_frags(const float* f1b, int n, unsigned off1, int kf, bf16x8* xh, bf16x8* xl) {
#pragma unroll
    for (int ks = 0; ks < KF; ++ks) {
        if (EXACT || ks < kf) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ld_off(f1b + (size_t)frag_k_uniform(ks, j) * n, off1);
            split<NP>(v, xh[ks], xl[ks]);
        }
    }
}

// layer-1 accumulators of the f1 half, plus t1: W1 x = W1a f1[p] + W1b f2sample, so every displacement of a
// strip starts from them
// (the scheduling barrier per tile is the backward's; the forward's once-per-strip loop had none.  With it the
// forward's registers are what they are without, and its fp32 4/4/4/4 instance spills 944 B instead of 992)
template <int NP, bool EXACT, int KF, int M1, class AFrag>
__device__ __forceinline__ void layer1_base(f32x16 (&base)[M1], const AFrag& afrag, const float* sb, int kf, int m1,
                                            int hh, const bf16x8* xh, const bf16x8* xl) {
#pragma unroll
    for (int mo = 0; mo < M1; ++mo) {
        if (EXACT || mo < m1) {
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = sb[32 * mo + acc_row(i, hh)];
            mma_tile<NP, EXACT, KF>(acc, afrag, mo * 2 * kf, 0, kf, xh, xl);
            base[mo] = acc;
        }
    }
}

// f2 half of the column: bilinear samples at the taps, straight into layer-1 B fragments
template <int NP, bool EXACT, int KF>
__device__ __forceinline__ void f2_frags(const float* f2b, int n, unsigned half_off, const Taps& t, int kf,
                                         bf16x8* xh, bf16x8* xl) {
    unsigned off2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) off2[k] = (half_off + (unsigned)t.idx[k]) * 4u;
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
            split<NP>(v, xh[ks], xl[ks]);
        }
    }
}

// a = relu(z) of one accumulator tile as the next layer's two B fragments; z = acc + bias (BIAS: the tile's
// 32 floats), else acc (the bias is in it already).  MASK: returns bit i = (z_i > 0) of register i, else 0.
template <int NP, bool BIAS, bool MASK>
__device__ __forceinline__ unsigned relu_frags(const f32x16& acc, const float* bias, int hh, bf16x8* ah, bf16x8* al) {
    unsigned m = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float z = BIAS ? acc[8 * s + j] + bias[acc_row(8 * s + j, hh)] : acc[8 * s + j];
            if constexpr (MASK) m |= (z > 0.f ? 1u : 0u) << (8 * s + j);
            v[j] = relu_nan(z);
        }
        split<NP>(v, ah[s], al[s]);
    }
    return m;
}

// layer 1 (the f2 half on top of base) -> layer-2 B fragments y
template <int NP, bool EXACT, bool MASK, int KF, int M1, class AFrag>
__device__ __forceinline__ void layer1(const f32x16 (&base)[M1], const AFrag& afrag, int kf, int m1, int hh,
                                       const bf16x8* xh, const bf16x8* xl, bf16x8* yh, bf16x8* yl, unsigned* mask) {
#pragma unroll
    for (int mo = 0; mo < M1; ++mo) {
        if (EXACT || mo < m1) {
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc = base[mo];
            mma_tile<NP, EXACT, KF>(acc, afrag, mo * 2 * kf + kf, 0, kf, xh, xl);
            const unsigned m = relu_frags<NP, false, MASK>(acc, nullptr, hh, yh + 2 * mo, yl + 2 * mo);
            if constexpr (MASK) mask[mo] = m;
        }
    }
}

// layer 2 (fragments from fb2 on, bias t2 at sb + kMaxWidth) -> layer-3 B fragments z
// (the backward's; the forward kernel keeps this loop in its own body, where it costs fewer registers)
template <int NP, bool EXACT, bool MASK, int M1, int M2, class AFrag>
__device__ __forceinline__ void layer2(const AFrag& afrag, const float* sb, int fb2, int m1, int m2, int hh,
                                       const bf16x8* yh, const bf16x8* yl, bf16x8* zh, bf16x8* zl, unsigned* mask) {
#pragma unroll
    for (int mo = 0; mo < M2; ++mo) {
        if (EXACT || mo < m2) {
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc = {};
            mma_tile<NP, EXACT, 2 * M1>(acc, afrag, fb2 + mo * 2 * m1, 0, 2 * m1, yh, yl);
            const unsigned m = relu_frags<NP, true, MASK>(acc, sb + kMaxWidth + 32 * mo, hh, zh + 2 * mo, zl + 2 * mo);
            if constexpr (MASK) mask[mo] = m;
        }
    }
}

}  // namespace rmd
