// mfma_bf16.h — the split-bf16 ("x3") MFMA arithmetic of every fp32-mode kernel, defined once.
//
// The contract.  A float v is carried as two bf16: hi = bf16(v) and lo = bf16(v - hi), both rounded to
// nearest even; hi + lo holds 16 of v's 24 significand bits, |v - hi - lo| <= 2^-17 |v|.  A product of two
// split operands is accumulated in fp32 on v_mfma_f32_32x32x16_bf16 as THREE bf16 products per k-step,
//
//     acc += a_lo . b_hi;   acc += a_hi . b_lo;   acc += a_hi . b_hi
//
// * Why three: the exact f32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 rate; three bf16
//   products cost 3/16 and give ~1e-5 of a float64 oracle (max-normalised) where one gives ~4e-3.
// * What is dropped: the a_lo . b_lo term, ~2^-16 relative to the product — at the level of the two
//   operands' own representation error (2^-17 each), so a fourth product would buy nothing.
// * Why the small terms first: the two cross terms are ~2^-8 of hi.hi.  Added to the accumulator before
//   it, they are rounded at their own magnitude; added after it, each would lose its low bits to the large
//   sum's rounding.  The order is part of the contract: the digest and exact-arithmetic tests pin it.
// * NP = 1 is the bf16 mode: hi.hi only, no lo part is computed or kept.
//
// The C/D register map of the 32x32 tile (16 fp32 registers per lane): lane l holds column l & 31;
// register i of lane half hh = l >> 5 holds row 8 (i >> 2) + 4 hh + (i & 3)  — acc_row(i, hh).  The A
// (B) operand of one k-step is 8 bf16 per lane: row (column) l & 31, k = 8 hh .. 8 hh + 7.
//
// Nothing here knows a kernel's shape.  A new MFMA kernel includes this header; it does not re-declare
// the types, the split or the product (tests/test_mfma_bf16_single_definition.py).
#pragma once

#include "rmd_common.h"

namespace rmd {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2;

// ---- the split ---------------------------------------------------------------------------------

__device__ __forceinline__ __bf16 bf16_hi(float v) { return (__bf16)v; }
// the bf16 of what hi = bf16_hi(v) leaves of v
__device__ __forceinline__ __bf16 bf16_lo(float v, __bf16 hi) { return (__bf16)(v - (float)hi); }

// v[0..N) -> hi, lo (N-element bf16 vectors), element by element; NP == 1 leaves lo untouched
template <int NP, int N>
__device__ __forceinline__ void split(const float* v, __bf16 __attribute__((ext_vector_type(N)))& hi,
                                      __bf16 __attribute__((ext_vector_type(N)))& lo) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        hi[j] = bf16_hi(v[j]);
        if constexpr (NP == 3) lo[j] = bf16_lo(v[j], hi[j]);
    }
}

// the same values, every hi before any lo: the grad GEMM's (corr_grad.hip) schedule depends on this order
template <int N>
__device__ __forceinline__ void split_hi_first(const float* v, __bf16 __attribute__((ext_vector_type(N)))& hi,
                                               __bf16 __attribute__((ext_vector_type(N)))& lo) {
#pragma unroll
    for (int j = 0; j < N; ++j) hi[j] = bf16_hi(v[j]);
#pragma unroll
    for (int j = 0; j < N; ++j) lo[j] = bf16_lo(v[j], hi[j]);
}

// ---- the product -------------------------------------------------------------------------------

// acc += A . B with NP bf16 products: hi.hi, and for NP == 3 first lo.hi and hi.lo
template <int NP>
__device__ __forceinline__ void mma(f32x16& acc, const bf16x8& ah, const bf16x8& al, const bf16x8& bh,
                                    const bf16x8& bl) {
    if constexpr (NP == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// ---- the accumulator map -----------------------------------------------------------------------

// row of accumulator register i for lane half hh (hh = 0: the wave-uniform part)
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

}  // namespace rmd
