// corr_pyramid_tiled.hip — the general correlation GEMM: any channel count, bf16 or exact-f32 MFMA, f32 or fp16
// pyramid in the row layout.  It is the fp32-exact mode's GEMM and the fallback of the other two modes; its
// operand prep (pixel-major, channel-contiguous (B, N, Cp)) also feeds corr_pyramid_stationary.
//
// 64 queries x 256 targets (a 16 x 16 block) per workgroup, K staged through LDS in 64-deep chunks; the epilogue
// is the in-lane pooling of corr_pyramid.hip's design comment, one store per level row piece.

#include "corr_pyramid.h"

namespace rmd {
namespace {

constexpr int kThreads = 256;
constexpr int kBQ = 64;      // queries per workgroup
constexpr int kNT = 256;     // targets per workgroup (16 x 16 block)

// operand element: bf16, or float for the exact f32 MFMA
template <bool F32> struct Operand { using T = __bf16; static constexpr int S = 2; };
template <> struct Operand<true> { using T = float; static constexpr int S = 4; };

// padded staging row: kKC elements + 16 B -> ds_read_b128 fragment reads are conflict-free
template <bool F32> constexpr int stage_stride() { return kKC * Operand<F32>::S + 16; }

// element offset of (b, query q, target row y, row-chunk x) at level l (rmd.h layout)
__device__ __forceinline__ size_t lvl_index(const PyrGeom& g, int l, int b, int y, int xc, int q, int N) {
    return (size_t)g.off[l] + ((((size_t)b * g.ty[l] + y) * g.tx[l] + xc) * N + q) * g.tw[l];
}

// ---------------------------------------------------------------------------------------------
// prep: (B, C, N) f32 -> (B, N, Cp) operand type, zero-padded channels.  64 px x 64 ch per block.
template <typename T>
__global__ void __launch_bounds__(kThreads)
prep_operand(const float* __restrict__ f, T* __restrict__ o, int C, int N, int Cp, float scale) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, t = threadIdx.x;
    const float* fb = f + (size_t)b * C * N;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = c0 + (t >> 6) + 4 * i, p = p0 + (t & 63);
        tile[(t >> 6) + 4 * i][t & 63] = (c < C && p < N) ? fb[(size_t)c * N + p] * scale : 0.f;
    }
    __syncthreads();
    const int p = p0 + (t >> 2);
    if (p >= N) return;
    const int cc = (t & 3) * 16;
    T vals[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) vals[j] = (T)tile[cc + j][t >> 2];
    uint4* dst = reinterpret_cast<uint4*>(o + ((size_t)b * N + p) * Cp + c0 + cc);
    const uint4* src = reinterpret_cast<const uint4*>(vals);
#pragma unroll
    for (int j = 0; j < (int)(16 * sizeof(T) / 16); ++j) dst[j] = src[j];
}

template <typename TOut> __device__ __forceinline__ TOut cvt_out(float v);
template <> __device__ __forceinline__ float cvt_out<float>(float v) { return v; }
template <> __device__ __forceinline__ __half cvt_out<__half>(float v) { return __float2half_rn(v); }

template <typename TOut, int NE>
__device__ __forceinline__ void put(TOut* p, const float* v) {
    TOut tmp[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) tmp[i] = cvt_out<TOut>(v[i]);
    constexpr int NB = NE * sizeof(TOut);
    if constexpr (NB == 16) *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(tmp);
    else if constexpr (NB == 8) *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(tmp);
    else if constexpr (NB == 4) *reinterpret_cast<unsigned*>(p) = *reinterpret_cast<const unsigned*>(tmp);
    else *p = tmp[0];
}

// ---------------------------------------------------------------------------------------------
// Workgroup = 4 waves = 16x16 targets x 64 queries; wave w owns the 8x8 target sub-block (rows 8*(w>>1)..,
// cols 8*(w&1)..) for all 64 queries (2x2 MFMA 32x32 tiles).
template <bool F32, typename TOut>
__global__ void __launch_bounds__(kThreads)
corr_pyramid_tiled(const typename Operand<F32>::T* __restrict__ opA,   // fmap2 (B, N, Cp)
                   const typename Operand<F32>::T* __restrict__ opB,   // fmap1 (B, N, Cp)
                   int Cp, float scale, PyrGeom g, TOut* __restrict__ pyr) {
    using T = typename Operand<F32>::T;
    constexpr int S = Operand<F32>::S;
    constexpr int SS = stage_stride<F32>();
    constexpr int PPR = kKC * S / 16;                       // 16-B pieces per staged row

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;
    unsigned char* sB = smem + kNT * SS;

    const int H = g.height, W = g.width, N = H * W;
    const int q0 = blockIdx.x * kBQ;
    const int ncb = (W + 15) >> 4;
    const int rb = blockIdx.y / ncb, cb = blockIdx.y - rb * ncb;
    const int b = blockIdx.z;
    const int ty0 = rb * 16, tx0 = cb * 16;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

    const T* gA = opA + (size_t)b * N * Cp;
    const T* gB = opB + (size_t)b * N * Cp;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // LDS row of this lane's A fragment for target tile tr (4 target rows x 8 target cols)
    int arow[2];
#pragma unroll
    for (int tr = 0; tr < 2; ++tr) arow[tr] = (8 * (w >> 1) + 4 * tr + (r >> 3)) * 16 + 8 * (w & 1) + (r & 7);

    for (int kc = 0; kc < Cp; kc += kKC) {
#pragma unroll 4
        for (int i = 0; i < kNT * PPR / kThreads; ++i) {
            const int id = tid + kThreads * i, row = id / PPR, pc = id - row * PPR;
            const int ty = ty0 + (row >> 4), tx = tx0 + (row & 15);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ty < H && tx < W)
                v = *reinterpret_cast<const uint4*>(gA + (size_t)(ty * W + tx) * Cp + kc + pc * (16 / S));
            *reinterpret_cast<uint4*>(sA + row * SS + pc * 16) = v;
        }
#pragma unroll
        for (int i = 0; i < kBQ * PPR / kThreads; ++i) {
            const int id = tid + kThreads * i, row = id / PPR, pc = id - row * PPR;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (q0 + row < N)
                v = *reinterpret_cast<const uint4*>(gB + (size_t)(q0 + row) * Cp + kc + pc * (16 / S));
            *reinterpret_cast<uint4*>(sB + row * SS + pc * 16) = v;
        }
        __syncthreads();

        if constexpr (!F32) {
#pragma unroll
            for (int s = 0; s < kKC / 16; ++s) {
                const int kb = (16 * s + 8 * h) * 2;
                bf16x8 a[2], q[2];
#pragma unroll
                for (int tr = 0; tr < 2; ++tr) a[tr] = *reinterpret_cast<const bf16x8*>(sA + arow[tr] * SS + kb);
#pragma unroll
                for (int tq = 0; tq < 2; ++tq) q[tq] = *reinterpret_cast<const bf16x8*>(sB + (32 * tq + r) * SS + kb);
#pragma unroll
                for (int tr = 0; tr < 2; ++tr)
#pragma unroll
                    for (int tq = 0; tq < 2; ++tq)
                        acc[tr][tq] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tr], q[tq], acc[tr][tq], 0, 0, 0);
            }
        } else {
            // exact f32 MFMA; k-slot h of every step walks k = 32h + 4m + u (same map for A and B)
#pragma unroll 2
            for (int m = 0; m < 8; ++m) {
                const int kb = (32 * h + 4 * m) * 4;
                f32x4 a[2], q[2];
#pragma unroll
                for (int tr = 0; tr < 2; ++tr) a[tr] = *reinterpret_cast<const f32x4*>(sA + arow[tr] * SS + kb);
#pragma unroll
                for (int tq = 0; tq < 2; ++tq) q[tq] = *reinterpret_cast<const f32x4*>(sB + (32 * tq + r) * SS + kb);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int tr = 0; tr < 2; ++tr)
#pragma unroll
                        for (int tq = 0; tq < 2; ++tq)
                            acc[tr][tq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tr][u], q[tq][u], acc[tr][tq], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- epilogue: scale, pool in-lane, store each level's row pieces from registers ------------
    const int levels = g.levels;
#pragma unroll
    for (int tq = 0; tq < 2; ++tq) {
        const int q = q0 + 32 * tq + r;
        if (q >= N) continue;
        float o[8][4];                                            // rows 0..7, cols 4h..4h+3
#pragma unroll
        for (int tr = 0; tr < 2; ++tr)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[4 * tr + (e >> 2)][e & 3] = acc[tr][tq][e] * scale;
        // level 0: wave block rows 16rb + 8(w>>1) + row, chunk 2cb + (w&1), elements 4h..4h+3
        {
            const int xc = 2 * cb + (w & 1);
            if (xc < g.tx[0]) {
#pragma unroll
                for (int row = 0; row < 8; ++row) {
                    const int y = 16 * rb + 8 * (w >> 1) + row;
                    if (y < g.ty[0]) put<TOut, 4>(pyr + lvl_index(g, 0, b, y, xc, q, N) + 4 * h, o[row]);
                }
            }
        }
        if (levels < 2) continue;
        float l1[4][2];
#pragma unroll
        for (int yy = 0; yy < 4; ++yy)
#pragma unroll
            for (int xx = 0; xx < 2; ++xx)
                l1[yy][xx] = 0.25f * ((o[2 * yy][2 * xx] + o[2 * yy][2 * xx + 1]) +
                                      (o[2 * yy + 1][2 * xx] + o[2 * yy + 1][2 * xx + 1]));
        if (cb < g.tx[1]) {
#pragma unroll
            for (int yy = 0; yy < 4; ++yy) {
                const int y = 8 * rb + 4 * (w >> 1) + yy;
                if (y < g.ty[1]) put<TOut, 2>(pyr + lvl_index(g, 1, b, y, cb, q, N) + 4 * (w & 1) + 2 * h, l1[yy]);
            }
        }
        if (levels < 3) continue;
        float l2[2];
#pragma unroll
        for (int yy = 0; yy < 2; ++yy)
            l2[yy] = 0.25f * ((l1[2 * yy][0] + l1[2 * yy][1]) + (l1[2 * yy + 1][0] + l1[2 * yy + 1][1]));
        if (cb < g.tx[2]) {
#pragma unroll
            for (int yy = 0; yy < 2; ++yy) {
                const int y = 4 * rb + 2 * (w >> 1) + yy;
                if (y < g.ty[2]) put<TOut, 1>(pyr + lvl_index(g, 2, b, y, cb, q, N) + 2 * (w & 1) + h, &l2[yy]);
            }
        }
        if (levels < 4) continue;
        float s3 = l2[0] + l2[1];
        s3 += __shfl_xor(s3, 32);
        s3 *= 0.25f;
        const int y3 = 2 * rb + (w >> 1);
        if (h == 0 && cb < g.tx[3] && y3 < g.ty[3]) put<TOut, 1>(pyr + lvl_index(g, 3, b, y3, cb, q, N) + (w & 1), &s3);
    }
}

// operands in the workspace: A = fmap2 (B, N, Cp), then B = fmap1 (B, N, Cp)
template <bool F32>
int launch_prepare(const float* f1, const float* f2, int C, float scale, const rmd_pyramid_desc& d, void* workspace,
                   hipStream_t st) {
    using T = typename Operand<F32>::T;
    const int N = d.height * d.width;
    const int Cp = padded_channels(C);
    T* opA = reinterpret_cast<T*>(workspace);
    T* opB = opA + (size_t)d.batch * N * Cp;
    dim3 pg((N + 63) / 64, Cp / 64, d.batch);
    // bf16: the scale (1/sqrt(C) for raft.CorrBlock) is folded into fmap2 before rounding (exact for a power of
    // two, e.g. C = 256 or raft_fs's 1); the f32 parity path scales the f32 accumulators in the epilogue
    const float prescale = F32 ? 1.0f : scale;
    prep_operand<T><<<pg, kThreads, 0, st>>>(f2, opA, C, N, Cp, prescale);
    prep_operand<T><<<pg, kThreads, 0, st>>>(f1, opB, C, N, Cp, 1.0f);
    return check_launch("rmd_corr_prepare");
}

template <bool F32, typename TOut>
int launch_pyramid(int C, float scale, const rmd_pyramid_desc& d, void* pyramid, void* workspace, hipStream_t st) {
    using T = typename Operand<F32>::T;
    const int N = d.height * d.width;
    const int Cp = padded_channels(C);
    T* opA = reinterpret_cast<T*>(workspace);
    T* opB = opA + (size_t)d.batch * N * Cp;
    constexpr int lds = (kNT + kBQ) * stage_stride<F32>();
    auto kern = corr_pyramid_tiled<F32, TOut>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    dim3 grid((N + kBQ - 1) / kBQ, ((d.height + 15) / 16) * ((d.width + 15) / 16), d.batch);
    kern<<<grid, kThreads, lds, st>>>(opA, opB, Cp, F32 ? scale : 1.0f, make_geom(d), reinterpret_cast<TOut*>(pyramid));
    return check_launch("rmd_corr_pyramid/gemm");
}

}  // namespace

namespace tiled {

int prepare(const float* fmap1, const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d, int compute,
            void* workspace, hipStream_t st) {
    return compute == RMD_BF16 ? launch_prepare<false>(fmap1, fmap2, channels, scale, d, workspace, st)
                               : launch_prepare<true>(fmap1, fmap2, channels, scale, d, workspace, st);
}

int pyramid(int channels, float scale, const rmd_pyramid_desc& d, int compute, void* pyramid, void* workspace,
            hipStream_t st) {
    if (compute == RMD_BF16)
        return d.storage == RMD_F16 ? launch_pyramid<false, __half>(channels, scale, d, pyramid, workspace, st)
                                    : launch_pyramid<false, float>(channels, scale, d, pyramid, workspace, st);
    return d.storage == RMD_F16 ? launch_pyramid<true, __half>(channels, scale, d, pyramid, workspace, st)
                                : launch_pyramid<true, float>(channels, scale, d, pyramid, workspace, st);
}

}  // namespace tiled
}  // namespace rmd
