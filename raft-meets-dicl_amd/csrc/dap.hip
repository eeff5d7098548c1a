// dap.hip — DICL displacement-aware projection (DAP): a 1x1 convolution over the displacement axis.
//
// Replaces (qzed/raft-meets-dicl v2):
//  * DisplacementAwareProjection 1x1 conv                    src/models/common/blocks/dicl.py:121-150
//    -> rmd_dap (forward; with transpose = 1 it is the input gradient W^T g)
//  * autograd of F.conv2d w.r.t. its weight                  src/models/common/blocks/dicl.py:137,147
//    -> rmd_dap_weight_grad

#include "mfma_bf16.h"

#include <algorithm>

namespace rmd {
namespace {

constexpr int kThreads = 256;

// ---- displacement-aware projection: out[b, o, p] = sum_i W[o, i] x[b, i, p] ------------------
// One lane per pixel, 16 output channels per pass held in registers; W rows broadcast from LDS.
constexpr int kDapOB = 16;

template <bool LDS_W>
__global__ void __launch_bounds__(kThreads)
dap_kernel(const float* __restrict__ x, const float* __restrict__ wgt, int D, int n, int transpose,
           float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sw[];     // D x D (row o, col i)
    if constexpr (LDS_W) {
        for (int k = threadIdx.x; k < D * D; k += kThreads) {
            const int o = k / D, i = k - o * D;
            sw[k] = transpose ? wgt[i * D + o] : wgt[k];
        }
        __syncthreads();
    }
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= n) return;
    const float* xb = x + (size_t)b * D * n + p;
    float* ob = out + (size_t)b * D * n + p;
    for (int o0 = 0; o0 < D; o0 += kDapOB) {
        float acc[kDapOB];
#pragma unroll
        for (int k = 0; k < kDapOB; ++k) acc[k] = 0.f;
        for (int i = 0; i < D; ++i) {
            const float xv = xb[(size_t)i * n];
#pragma unroll
            for (int k = 0; k < kDapOB; ++k) {
                const int o = min(o0 + k, D - 1);
                float wv;
                if constexpr (LDS_W) wv = sw[o * D + i];
                else wv = transpose ? wgt[i * D + o] : wgt[o * D + i];     // wave-uniform: scalar loads
                acc[k] = fmaf(wv, xv, acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kDapOB; ++k)
            if (o0 + k < D) ob[(size_t)(o0 + k) * n] = acc[k];
    }
}

// ---- DAP as a split-bf16 (x3) MFMA GEMM (product form) -----------------------------------------
// out_b (D x n) = W (D x D) . x_b (D x n), fp32 accuracy from the three bf16 products per k-step of
// mfma_bf16.h.  The exact f32 MFMA (v_mfma_f32_32x32x2_f32) held the round-1 kernel at ~25 % of even
// its own peak, 1/16 of the bf16 rate (0.27 ms at D = 324); here the 3 bf16 products cost 3/16.
// Geometry: a workgroup owns an M-block of MT x 32 output displacements (all of them when D <= 128)
// and one chunk of the batch image's 32-pixel tiles.  The block's W rows (or W^T rows, transpose)
// are split once into hi / lo bf16 in LDS — rows of 2 Kp + 16 bytes, an odd number of 16-B slots,
// so a ds_read_b128 lane group hits distinct bank slots; each wave then sweeps its tiles: x is read
// straight from HBM as the MFMA B operand (lane (r, h) holds rows 8h..8h+7 of k-step s at pixel r:
// eight coalesced 128-B row segments), split in registers, KC k-steps per chunk with the next chunk
// (or the next tile's first) in flight during the current chunk's MFMAs.  Rows >= D and pixels >= n
// fall outside the per-image buffer range (loads read 0, stores are dropped).  The M-blocks of one
// pixel chunk are consecutive workgroup ids (one XCD), so x is fetched from HBM once for all blocks.
// Output stores are non-temporal.  Measured (profiles/dap_ab_r02.json, b8): D = 49 10.1 us, D = 81
// 12.1 us, D = 324 62 us, vs 16.8 / 23.2 / 317 us for the exact-f32 MFMA form; error vs float64
// 1.5e-5 max-normalised.  At D = 324 the MFMA floor is ~19 us and the HBM floor ~27 us; PMC shows x
// fetched from HBM once (84 MB) and the x ring depth (3-8 chunks of prefetch) changes nothing, so the
// gap is in the per-CU issue of the 4x L2 re-reads of x and the single 8-wave workgroup per CU.
constexpr int kDapSG = 4;     // W staging: 4-element groups per thread in flight
constexpr int kDapStoreAux = 2;   // output store cache policy (gfx950 cpol: 2 = nt): 10-15 % at D <= 81
constexpr int kDapKC = 8, kDapNB = 2;   // x ring: NB buffers of KC k-steps

template <int MT, int NW, int AUX, int KC, int NB>
__global__ void __launch_bounds__(NW * 64, 2)
dap_x3_kernel(const float* __restrict__ x, const float* __restrict__ wgt, int D, int n, int transpose,
              int mblocks, int per, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int Kp = (D + 15) & ~15, nks = Kp >> 4;
    const int RB = 2 * Kp + 16;
    unsigned char* const sh = sm;                       // hi rows
    unsigned char* const sl = sm + MT * 32 * RB;        // lo rows
    int id = xcd_block(blockIdx.x, gridDim.x);
    const int mb = id % mblocks;
    id /= mblocks;
    const int pc = id % per, b = id / per;
    const int o0 = mb * 32 * MT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int ntile = (n + 31) >> 5;
    auto rsrc = [&](const void* base) {
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)base);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)base >> 32));
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uintptr_t)hi << 32) | lo), (short)0,
                                                 (int)((unsigned)D * (unsigned)n * 4u), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t xr = rsrc(x + (size_t)b * D * n);
    const __amdgpu_buffer_rsrc_t orr = rsrc(out + (size_t)b * D * n);
    const unsigned rowb = (unsigned)n * 4u;
    const unsigned aoff = (unsigned)(r * RB + 16 * h);
    const int nch = (nks + KC - 1) / KC;

    // x chunks stream through a ring of NB register buffers: step i = (tile t0 + (i / nch) tstride,
    // chunk i % nch) lives in buffer i % NB and is loaded NB - 1 steps before its use
    float xb[NB][KC * 8];
    // chunk c of tile tt: rows 16 (KC c + u) + 8 h + j at pixel 32 tt + r (out of range past n / D)
    auto load = [&](float (&v)[KC * 8], int tt, int c) {
        const int p = tt * 32 + r;
        const unsigned base = p < n ? (unsigned)(8 * h + 16 * KC * c) * rowb + (unsigned)p * 4u : 0x80000000u;
#pragma unroll
        for (int u = 0; u < KC; ++u)
            if (KC * c + u < nks)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v[u * 8 + j] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        xr, (int)(base + (unsigned)(16 * u + j) * rowb), 0, 0));
    };

    const int t0 = pc * NW + w, tstride = per * NW;
    const int mytiles = t0 < ntile ? (ntile - 1 - t0) / tstride + 1 : 0;
    const int nsteps = mytiles * nch;
#pragma unroll
    for (int u = 0; u < NB - 1; ++u)        // in flight while the workgroup stages W
        if (u < nsteps) load(xb[u], t0 + (u / nch) * tstride, u % nch);

    // stage the block's W rows as hi / lo bf16 (4 consecutive k per thread; W^T reads run along o),
    // kDapSG groups' loads in flight per thread before any is converted
    {
        constexpr int rows = MT * 32;
        const int kq = Kp >> 2, total = rows * kq;
        for (int e0 = tid; e0 < total; e0 += NW * 64 * kDapSG) {
            float v[kDapSG][4];
            int ro[kDapSG];
#pragma unroll
            for (int g = 0; g < kDapSG; ++g) {
                const int e = e0 + g * NW * 64;
                int rr, k;
                if (transpose) { rr = e % rows; k = 4 * (e / rows); }
                else { rr = e / kq; k = 4 * (e - rr * kq); }
                const int o = o0 + rr;
                ro[g] = e < total ? rr * RB + 2 * k : -1;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = k + q;
                    v[g][q] = (e < total && o < D && i < D) ? (transpose ? wgt[(size_t)i * D + o] : wgt[(size_t)o * D + i])
                                                            : 0.f;
                }
            }
#pragma unroll
            for (int g = 0; g < kDapSG; ++g) {
                if (ro[g] < 0) continue;
                bf16x4 hi, lo;
                split<3>(v[g], hi, lo);
                *reinterpret_cast<bf16x4*>(sh + ro[g]) = hi;
                *reinterpret_cast<bf16x4*>(sl + ro[g]) = lo;
            }
        }
    }
    __syncthreads();

    f32x16 acc[MT];
    for (int i0 = 0; i0 < nsteps; i0 += NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int i = i0 + u;
            if (i >= nsteps) break;
            const int ip = i + NB - 1;
            if (ip < nsteps) load(xb[(u + NB - 1) % NB], t0 + (ip / nch) * tstride, ip % nch);
            const int c = i % nch;
            if (c == 0) {
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = f32x16{};
            }
#pragma unroll
            for (int uu = 0; uu < KC; ++uu) {
                const int s = c * KC + uu;
                if (s < nks) {
                    bf16x8 bh, bl;
                    split<3>(xb[u] + uu * 8, bh, bl);
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const unsigned a = aoff + (unsigned)(m * 32 * RB + 32 * s);
                        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(sh + a);
                        const bf16x8 al = *reinterpret_cast<const bf16x8*>(sl + a);
                        mma<3>(acc[m], ah, al, bh, bl);
                    }
                }
            }
            if (c == nch - 1) {
                // C tile: lane (r, h) holds rows acc_row(e, h) of pixel column r; 4 h is in the lane offset
                const int p = (t0 + (i / nch) * tstride) * 32 + r;
                const unsigned so = p < n ? (unsigned)(4 * h) * rowb + (unsigned)p * 4u : 0x80000000u;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const unsigned row = (unsigned)(o0 + m * 32 + acc_row(e, 0));
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(acc[m][e]), orr, (int)(so + row * rowb),
                                                              0, AUX);
                    }
            }
        }
    }
}

// ---- DAP weight gradient ------------------------------------------------------------------------
// dW[o][i] = sum_b sum_p g[b][o][p] x[b][i][p]: the weight gradient of the 1x1 convolution
// (blocks/dicl.py:137,147; autograd of F.conv2d w.r.t. its weight).  M = N = D (tiny), K = B * pixels
// (large): K is split over workgroups (one image's pixel chunk each), every workgroup computes the
// full D x D partial with v_mfma_f32_32x32x16_bf16 on split operands (g = hi + lo, x = hi + lo:
// lo.hi + hi.lo + hi.hi, the forward DAP's split), a second kernel sums the partials in split order
// (deterministic).  Wave w of a workgroup owns a 2 x 2 block of 32 x 32 output tiles; A / B fragments
// are 8 consecutive pixels of one row (two float4 loads) split in registers.
constexpr int kWgPx = 16;                        // pixels per MFMA k-step

__device__ __forceinline__ void wg_frag(const float* __restrict__ row, bool rok, int p, int n, bf16x8& hi, bf16x8& lo) {
    float v[8];
    if (rok && p + 7 < n && ((reinterpret_cast<uintptr_t>(row + p) & 15) == 0)) {
        *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(row + p);
        *reinterpret_cast<float4*>(v + 4) = *reinterpret_cast<const float4*>(row + p + 4);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (rok && p + e < n) ? row[p + e] : 0.f;
    }
    split<3>(v, hi, lo);
}

// grid (B * nchunk, tile groups); 256 threads; part (splits, Dp, Dp)
__global__ void __launch_bounds__(256)
dap_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, int D, int n, int nchunk, int pchunk,
                 int Dp, float* __restrict__ part) {
    const int s = blockIdx.x, b = s / nchunk, c = s % nchunk;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int Dt = Dp / 32, Db = (Dt + 1) / 2;                   // 32-row tiles, 2x2 tile blocks per side
    const int tb = blockIdx.y * 4 + w;
    if (tb >= Db * Db) return;                                   // no barriers in this kernel
    const int ot0 = 2 * (tb / Db), it0 = 2 * (tb % Db);
    const int p0 = c * pchunk, p1 = min(n, p0 + pchunk);
    const float* gb = g + (size_t)b * D * n;
    const float* xb = x + (size_t)b * D * n;
    f32x16 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f32x16{};
    const int o[2] = {32 * ot0 + j, 32 * (ot0 + 1) + j}, i[2] = {32 * it0 + j, 32 * (it0 + 1) + j};
    for (int p = p0; p < p1; p += kWgPx) {
        bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            wg_frag(gb + (size_t)min(o[u], D - 1) * n, o[u] < D, p + 8 * h, p1, ah[u], al[u]);
            wg_frag(xb + (size_t)min(i[u], D - 1) * n, i[u] < D, p + 8 * h, p1, bh[u], bl[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) mma<3>(acc[u][v], ah[u], al[u], bh[v], bl[v]);
    }
    // lane (column j, half h): register r is row acc_row(r, h) of the tile (spelled out: through acc_row the
    // compiler swaps the operands of one v_or_b32)
    float* ps = part + (size_t)s * Dp * Dp;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (ot0 + u >= Dt || it0 + v >= Dt) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * (ot0 + u) + 8 * (r >> 2) + 4 * h + (r & 3);
                ps[(size_t)row * Dp + 32 * (it0 + v) + j] = acc[u][v][r];
            }
        }
}

// dW[o][i] = the sum over splits (fixed order: deterministic)
__global__ void __launch_bounds__(512)
dap_wgrad_reduce(const float* __restrict__ part, int splits, int D, int Dp, float* __restrict__ dw) {
    // 32 consecutive outputs x 16 split groups per 512-thread workgroup: thread (g, i) sums splits
    // g, g + 16, ... in order, then the 16 group sums are added in fixed order from LDS — the same
    // result for every launch (deterministic), with D^2 / 32 workgroups and coalesced 128-B reads
    __shared__ float red[16][33];
    const int t = threadIdx.x, i32 = t & 31, gsp = t >> 5;
    const int idx = blockIdx.x * 32 + i32;
    const bool ok = idx < D * D;
    const int o = ok ? idx / D : 0, i = ok ? idx % D : 0;
    const float* pp = part + (size_t)o * Dp + i;
    const size_t mat = (size_t)Dp * Dp;
    // the group's partials are summed in split order, 8 loads in flight at a time (the plain loop waited
    // for each strided load before the next add: latency-bound at ~20 splits per group)
    float s = 0.f;
    int k = gsp;
    for (; k + 16 * 7 < splits; k += 16 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = pp[(size_t)(k + 16 * u) * mat];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < splits; k += 16) s += pp[(size_t)k * mat];
    red[gsp][i32] = s;
    __syncthreads();
    if (gsp == 0 && ok) {
        float r = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) r += red[g][i32];
        dw[idx] = r;
    }
}

struct WgPlan {
    int Dp, groups, nchunk, pchunk, splits;
};

WgPlan wgrad_plan(int batch, int D, int n) {
    WgPlan w{};
    w.Dp = (D + 31) / 32 * 32;
    const int Db = (w.Dp / 32 + 1) / 2;
    w.groups = (Db * Db + 3) / 4;
    // about 256 workgroups in all (one per CU), at least 4 k-steps per split
    const int want = std::max(1, 256 / (w.groups * batch));
    const int steps = (n + kWgPx - 1) / kWgPx;
    const int per = std::max(4, (steps + want - 1) / want);
    w.pchunk = per * kWgPx;
    w.nchunk = (n + w.pchunk - 1) / w.pchunk;
    w.splits = batch * w.nchunk;
    return w;
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" size_t rmd_dap_weight_grad_workspace_bytes(int batch, int disp, int pixels) {
    if (batch <= 0 || disp <= 0 || pixels <= 0) return 0;
    const rmd::WgPlan w = rmd::wgrad_plan(batch, disp, pixels);
    return (size_t)w.splits * w.Dp * w.Dp * sizeof(float);
}

extern "C" int rmd_dap_weight_grad(const float* grad_out, const float* x, int batch, int disp, int pixels,
                                   float* grad_weight, void* workspace, void* stream) {
    RMD_REQUIRE(grad_out && x && grad_weight && workspace, RMD_ERR_ARG, "rmd_dap_weight_grad: null pointer");
    RMD_REQUIRE(batch > 0 && disp > 0 && pixels > 0, RMD_ERR_SHAPE, "rmd_dap_weight_grad: bad sizes");
    const rmd::WgPlan w = rmd::wgrad_plan(batch, disp, pixels);
    RMD_REQUIRE((long long)w.splits * w.groups < (1ll << 31) && w.groups < 65536, RMD_ERR_SHAPE,
                "rmd_dap_weight_grad: grid too large");
    hipStream_t st = rmd::as_stream(stream);
    float* part = static_cast<float*>(workspace);
    rmd::dap_wgrad_kernel<<<dim3(w.splits, w.groups), 256, 0, st>>>(grad_out, x, disp, pixels, w.nchunk, w.pchunk,
                                                                    w.Dp, part);
    int rc = rmd::check_launch("rmd_dap_weight_grad");
    if (rc) return rc;
    rmd::dap_wgrad_reduce<<<(disp * disp + 31) / 32, 512, 0, st>>>(part, w.splits, disp, w.Dp, grad_weight);
    return rmd::check_launch("rmd_dap_weight_grad reduce");
}

extern "C" int rmd_dap(const float* x, const float* weight, int batch, int disp, int pixels, int transpose,
                       float* out, void* stream) {
    RMD_REQUIRE(x && weight && out, RMD_ERR_ARG, "rmd_dap: null pointer");
    RMD_REQUIRE(batch > 0 && disp > 0 && pixels > 0, RMD_ERR_SHAPE, "rmd_dap: bad sizes");
    const int Kp = (disp + 15) & ~15;
    if (disp <= 1024 && (long long)(Kp + 16) * pixels * 4 < (1ll << 31)) {
        // split-bf16 MFMA form: M-block of MT row tiles = the largest (<= 4) whose hi / lo W rows fit in
        // 160 KB of LDS; 8 waves per workgroup when the block leaves room for only one workgroup per CU
        const int mt_all = (disp + 31) / 32;
        const size_t rowb = 2 * (size_t)(2 * Kp + 16);       // hi + lo bytes per W row
        int mt = mt_all < 4 ? mt_all : 4;
        while (mt > 1 && (size_t)32 * mt * rowb > 160 * 1024) --mt;
        const size_t lds = (size_t)32 * mt * rowb;
        constexpr int nw = 8;
        const int mblocks = (mt_all + mt - 1) / mt;
        const int ntile = (pixels + 31) / 32;
        // one round of workgroups over the chip: ~256 x (workgroups per CU) in all, at least one
        // 32-pixel tile per wave.  At 171-227 VGPRs a SIMD holds 2 waves, so a CU holds one 8-wave
        // workgroup (measured against 4-wave workgroups, 2-3 per CU: 11.5 vs 13.2 us at D = 49, 13.1 vs
        // 15.1 at D = 81, 62 vs 87 at D = 324 — fewer W stagings; profiles/dap_ab_r02.json)
        const int occ = 1;
        const long long units = (long long)mblocks * batch;
        int per = (int)std::min<long long>((256LL * occ + units - 1) / units, (ntile + nw - 1) / nw);
        per = std::max(per, 1);
        const long long nwg = units * per;
        RMD_REQUIRE(nwg < (1LL << 31), RMD_ERR_SHAPE, "rmd_dap: grid too large");
        hipStream_t st = as_stream(stream);
#define RMD_DAPX3_R(MT, NW, AUX, KC, NB)                                                                    \
        do {                                                                                                \
            /* the >64 KB LDS opt-in is per device: set before every launch */                           \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(dap_x3_kernel<MT, NW, AUX, KC, NB>),     \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);               \
            dap_x3_kernel<MT, NW, AUX, KC, NB><<<(unsigned)nwg, NW * 64, lds, st>>>(x, weight, disp, pixels, \
                                                                                  transpose, mblocks, per, out); \
        } while (0)
#define RMD_DAPX3(MT, NW) RMD_DAPX3_R(MT, NW, kDapStoreAux, kDapKC, kDapNB)
        switch (mt) {
            case 1: RMD_DAPX3(1, 8); break;
            case 2: RMD_DAPX3(2, 8); break;
            case 3: RMD_DAPX3(3, 8); break;
            default: RMD_DAPX3(4, 8); break;
        }
#undef RMD_DAPX3
#undef RMD_DAPX3_R
        return check_launch("rmd_dap/x3");
    }
    const size_t lds = sizeof(float) * (size_t)disp * disp;
    dim3 grid((pixels + kThreads - 1) / kThreads, batch);
    if (lds <= 64 * 1024) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(dap_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        dap_kernel<true><<<grid, kThreads, lds, as_stream(stream)>>>(x, weight, disp, pixels, transpose, out);
    } else {   // e.g. the 324x324 'full' DAP of raft_dicl_ml: W streamed through the scalar cache
        dap_kernel<false><<<grid, kThreads, 0, as_stream(stream)>>>(x, weight, disp, pixels, transpose, out);
    }
    return check_launch("rmd_dap");
}
