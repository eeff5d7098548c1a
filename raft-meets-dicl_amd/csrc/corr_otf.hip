// corr_otf.hip — on-the-fly windowed correlation lookup: no all-pairs volume in HBM.
//
// Replaces raft_fs.CorrBlock (qzed/raft-meets-dicl src/models/impls/raft_fs.py:13-87) — pooled
// fmap2 levels sampled on the (2r+1)^2 window of each query and dotted with fmap1, no 1/sqrt(C) —
// and, with one level and scale 1/sqrt(C), the window dot of corr/dot.py:25-57.  SURVEY.md §8(f)
// rank 1: memory O(B*C*N) instead of O(B*N^2).
//
// Operand layout (rmd_corr_otf_prepare): every map row is cut into segments of 16 pixels; a segment
// holds Cp channels of its 16 pixels as Cp/LSC load steps of exactly the 1 KiB one wave-instruction
// loads (16 B per lane), already in the lane order of the 16x16 MFMA operand (lane = 16*g + pixel):
//   bf16  16x16x32: lane (g, i) holds channels 32*ls + 8*g + e, e < 8           (one MFMA per step)
//   f32   16x16x4 : lane (g, i) holds channels 16*ls + 4*m + g, m < 4           (four MFMAs per step)
// so operand loads are whole 128-B lines (the row-per-lane gather of a pixel-major layout touches 32
// lines per instruction and halves the L1 rate).  Query rows (fmap1 * scale) use the same layout.
// compute RMD_BF16X3 (the fp32 precision mode) stores every value as a split bf16 pair v = hi + lo
// (hi = bf16(v), lo = bf16(v - hi)): each bf16 load step is followed by its lo step, and a task
// accumulates lo.hi + hi.lo + hi.hi with the 16x16x32 bf16 MFMA (the dropped lo.lo term is ~2^-16
// relative; same split as the fp32-mode GEMM), in the workspace bytes of f32 operands.  RMD_F32 keeps
// the exact f32 MFMA (fp32-exact).
//
// Lookup: one workgroup per (query block of QSY segments of 16 x 1 pixels, one below the other; batch),
// looping over the levels.  The block's queries' (2r+2)^2 integer patches at level l are bounded by one box
// (clipped to the map, widened to whole segments); every (box row, target segment) is one task: one
// 16x16 MFMA tile per query segment (16 targets x 16 queries), of whose products each lane keeps only
// those inside its query's own patch, in an LDS patch buffer per query (zero for targets off the map:
// zero padding per tap).  Each (query, x-offset) thread then interpolates its window exactly as
// rmd_corr_lookup does (shared bilinear weights, NaN for 1-pixel levels, zeroed masked levels).  A box
// of more than kMaxTasks segments (flow differing by hundreds of pixels inside one block) takes a
// per-query VALU patch path.
//
// The training backward of these lookups is corr_otf_backward.hip; corr_otf.h holds what both use.
#include "corr_otf.h"
#include "mfma_bf16.h"

namespace rmd {
namespace {

constexpr long long kWideBlocks = 4096;              // bf16: 16x4 query blocks from this many 16x2 blocks
constexpr int kMaxTasks = 1024;                      // box segments of the MFMA path (more: per-query VALU)
// Lookup launch shape per compute: query block of 16 x qsy pixels, workgroup threads, occupancy hint,
// query fragments in LDS (ql) or in registers.  cfg2 bf16, one box per comparison
// (profiles/otf_patch_ab_r03.jsonl, otf_ql_ab_r03.jsonl): 16x2 blocks with the query fragments in LDS
// 77.7 us; 16x1 with them in registers 87.5; 16x4 in registers 84.8; 16x4 in LDS 100.7 at 256 threads,
// 77.2 at 512.  Round 4, with the interleaved MFMA order (profiles/otf_put_ab_r04.json): bf16 16x2 LDS
// 256 threads 69-71 us (16x4 at 512 73-74, 16x1 88-91, 16x2 at 512 / 384 / 128 threads 75 / 86 / 83);
// split-bf16 16x2 LDS 512 threads 115-119 us (256 threads 136-139, register fragments 145-147).
struct LookShape {
    int qsy, threads, occ;
    bool ql;
};
constexpr LookShape kShapeBf16{2, 256, 2, true};
constexpr LookShape kShapeWide{4, 512, 2, true};     // bf16 on wide maps (kWideBlocks; figures at the dispatch)
constexpr LookShape kShapeSplit{2, 512, 2, true};
constexpr LookShape kShapeF32{2, 256, 1, false};     // f32: query fragments in registers
// LDS write of a task's products (put): true = every lane writes its 4 products, those outside its query's
// patch into a pad slot (no branches), false = only the products inside, under per-element branches.
// cfg2 A/B (profiles/otf_put_ab_r04.json): bf16 70.8-73.2 us with true vs 75.9-78.5 with false; split-bf16
// (two waves per SIMD) 150 with false vs 170 with true; f32 goes with split-bf16
constexpr bool kPutSelBf16 = true, kPutSelSplit = false;

template <typename T> struct Seg;
template <> struct Seg<__bf16> {
    static constexpr int LE = 8, LSC = 32;           // elements per lane, channels per load step
    typedef bf16x8 frag;
    static __device__ __forceinline__ void mma(f32x4& acc, const frag& a, const frag& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
    // (lane, element) of channel c within a load step
    static __host__ __device__ constexpr int lane_g(int c) { return (c >> 3) & 3; }
    static __host__ __device__ constexpr int elem(int c) { return c & 7; }
};
template <> struct Seg<float> {
    static constexpr int LE = 4, LSC = 16;
    typedef f32x4 frag;
    static __device__ __forceinline__ void mma(f32x4& acc, const frag& a, const frag& b) {
#pragma unroll
        for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[m], acc, 0, 0, 0);
    }
    static __host__ __device__ constexpr int lane_g(int c) { return c & 3; }
    static __host__ __device__ constexpr int elem(int c) { return (c >> 2) & 3; }
};

// Level l of fmap2 as the reference builds it (raft_fs.py:27-30): F.avg_pool2d(k=2, s=2) of level l-1.
// src / dst are (B, C, h, w) / (B, C, h/2, w/2) float32; one thread per output element.
__global__ void __launch_bounds__(kThreads)
otf_pool2_kernel(const float* __restrict__ src, int BC, int h, int w, float* __restrict__ dst) {
    const int h2 = h >> 1, w2 = w >> 1;
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long long)BC * h2 * w2) return;
    const int x = (int)(idx % w2);
    const long long r = idx / w2;
    const int y = (int)(r % h2);
    const long long bc = r / h2;
    const float* p = src + (size_t)bc * h * w + (size_t)(2 * y) * w + 2 * x;
    dst[idx] = (p[0] + p[1] + p[w] + p[w + 1]) * 0.25f;
}

// Segment operands: one thread per 16-B lane chunk (segment, load step, lane); a wave writes one
// contiguous 1-KiB load step, its reads run along x within each channel.
// levels = 1 and scale = s give the query operand (fmap1 * s).
template <typename T, bool X3>
__global__ void __launch_bounds__(kThreads)
otf_segments_kernel(LevelSrc src, OtfGeom g, float scale, T* __restrict__ seg) {
    static_assert(!X3 || sizeof(T) == 2, "split pairs are bf16");
    using S = Seg<T>;
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int nls = g.Cp / S::LSC;
    const long long total = (long long)g.B * g.TS * nls * 64;
    if (idx >= total) return;
    const int lane = (int)(idx & 63), gq = lane >> 4, i = lane & 15;
    const long long r = idx >> 6;
    const int ls = (int)(r % nls);
    const long long bs = r / nls;
    const long long s = bs % g.TS;
    const int b = (int)(bs / g.TS);
    int l = 0;
#pragma unroll
    for (int k = 1; k < RMD_MAX_LEVELS; ++k)
        if (k < g.L && s >= g.soff[k]) l = k;
    const int sl = (int)(s - g.soff[l]);
    const int y = sl / g.nsx[l], x = (sl - y * g.nsx[l]) * 16 + i;
    const size_t plane = (size_t)g.lh[l] * g.lw[l];
    const float* base = src.p[l] + (size_t)b * g.C * plane + (size_t)y * g.lw[l] + x;
    typedef __attribute__((ext_vector_type(S::LE))) T frag_t;
    frag_t v, vl;
#pragma unroll
    for (int e = 0; e < S::LE; ++e) {
        // channel of element e of lane group gq (inverse of Seg::lane_g / Seg::elem)
        const int c = S::LE == 8 ? ls * 32 + gq * 8 + e : ls * 16 + 4 * e + gq;
        const float f = x < g.lw[l] && c < g.C ? base[(size_t)c * plane] * scale : 0.f;
        v[e] = (T)f;
        if constexpr (X3) vl[e] = (T)(f - (float)v[e]);
    }
    if constexpr (X3) {
        // load step (r, hi) then (r, lo): r = idx >> 6 counts (segment, step) pairs
        T* o = seg + ((size_t)(idx >> 6) * 128 + lane) * S::LE;
        *reinterpret_cast<frag_t*>(o) = v;
        *reinterpret_cast<frag_t*>(o + 64 * S::LE) = vl;
    } else {
        (void)vl;
        *reinterpret_cast<frag_t*>(seg + (size_t)idx * S::LE) = v;
    }
}

// element (pixel i of segment, channel c) of a segment operand (X3: hi + lo)
template <typename T, bool X3>
__device__ __forceinline__ float seg_elem(const T* segbase, int i, int c) {
    using S = Seg<T>;
    constexpr int NP = X3 ? 2 : 1;
    const T* p = segbase + (c / S::LSC) * NP * 64 * S::LE + (S::lane_g(c) * 16 + i) * S::LE + S::elem(c);
    if constexpr (X3) return (float)p[0] + (float)p[64 * S::LE];
    return (float)p[0];
}

// one 16x16 tile's products of one load step: t / q point at the step's fragment(s)
template <typename T, bool X3>
__device__ __forceinline__ void seg_mma(f32x4& acc, const typename Seg<T>::frag* t, const typename Seg<T>::frag* q) {
    if constexpr (X3) {
        Seg<T>::mma(acc, t[1], q[0]);        // lo.hi, hi.lo first, hi.hi last
        Seg<T>::mma(acc, t[0], q[1]);
        Seg<T>::mma(acc, t[0], q[0]);
    } else {
        Seg<T>::mma(acc, t[0], q[0]);
    }
}

// Query block = QSY query segments (16 x 1 pixels each) one below the other: 16 x QSY queries.  Larger
// blocks load each target segment of their box once for more queries (the L2 -> CU operand traffic is
// the bound: every block re-reads its box), at the cost of MFMA tiles for targets outside a query's own
// window.  A 16 x 4 block (bf16) reads 2.5x fewer target bytes per query than 16 x 2.  A block is always
// one segment, 16 columns, wide.  Blocks grow downwards because that is the cheaper direction: one more
// query row adds one row to a box of 2r+2 rows and more, one more segment column a whole 16-target
// segment to every row of a box two or three segments wide.  So 16x1, 16x2 and 16x4 were measured
// (LookShape) and nothing wider; tools/otf_work_model.py counts the MFMA work of 32-wide blocks too.
// LDS floats per query patch: the (2r+2)^2 products, then the pad slot of put, rounded to an odd stride
constexpr int otf_patch_stride(int R) { return ((2 * R + 2) * (2 * R + 2) + 1) | 1; }

template <int QSY> struct QBlock {
    static constexpr int kQS = QSY, kBX = 16, kBY = QSY, kQ = kBX * kBY;
};

// 1-D grid over (batch, query block), XCD-aware: adjacent query blocks, whose target boxes overlap,
// run on the same XCD and share its L2.  One block runs every level of its queries, so the query
// staging, the coords load and the block's fixed start-up cost are paid once, not once per level.
// CPT = compiled Cp (0: runtime multiple of 128).
template <typename T, bool X3, int R, int CPT, int QSY, int OCC, bool QL, int kLookThreads>
__global__ void __launch_bounds__(kLookThreads, OCC)
otf_lookup_kernel(const T* __restrict__ qseg, const T* __restrict__ tseg, OtfGeom g,
                  const float* __restrict__ coords, unsigned zmask, float* __restrict__ out) {
    using SG = Seg<T>;
    using frag = typename SG::frag;
    using QB = QBlock<QSY>;
    constexpr int kQS = QB::kQS, kBX = QB::kBX, kBY = QB::kBY, kQ = QB::kQ;
    constexpr int kWaves = kLookThreads / 64;
    constexpr int D = 2 * R + 1, K = 2 * R + 2, KK = K * K, KKp = otf_patch_stride(R);   // odd: queries spread over banks
    constexpr bool kPutSel = sizeof(T) == 2 && !X3 ? kPutSelBf16 : kPutSelSplit;
    extern __shared__ float S[];                       // [kQ][KKp]: every query's (2r+2)^2 patch
    // every level's window origins / fractions and the block's bounding box per level, computed once
    // before the level loop (no per-level reduction barriers)
    __shared__ int box[RMD_MAX_LEVELS][4];             // x0, x1, y0, y1 (min / max)
    __shared__ int sxs[RMD_MAX_LEVELS][kQ], sys[RMD_MAX_LEVELS][kQ];
    __shared__ float sfx[RMD_MAX_LEVELS][kQ], sfy[RMD_MAX_LEVELS][kQ];
    const int nbx = (g.W + kBX - 1) / kBX, nqb = nbx * ((g.H + kBY - 1) / kBY);
    const int lid = xcd_block(blockIdx.x, gridDim.x);
    const int qb = lid % nqb, b = lid / nqb;
    const int qx0 = (qb % nbx) * kBX, qy0 = (qb / nbx) * kBY;
    const int N = g.H * g.W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: task indices in SGPRs
    constexpr int NP = X3 ? 2 : 1;                      // load steps per channel step (X3: hi, lo)
    const int cp = CPT > 0 ? CPT : g.Cp;
    const int nls = cp / SG::LSC;
    const size_t segsz = (size_t)16 * cp * NP;
    // query segment s = row s of the block: its operand rows (clamped at the map edge)
    const T* qsb[kQS];
#pragma unroll
    for (int s = 0; s < kQS; ++s)
        qsb[s] = qseg + ((size_t)b * g.QS + (size_t)min(qy0 + s, g.H - 1) * g.qnsx + min(qx0 >> 4, g.qnsx - 1)) * segsz;

    // the block's query fragments (CPT > 0): each wave keeps them in registers for every level and
    // target segment (a load step is one coalesced 1-KiB read per instruction), or (QL) one copy in
    // LDS behind the patch buffers, read per MFMA (fewer VGPRs: more waves and target loads in flight)
    constexpr int NLS = CPT > 0 ? CPT / SG::LSC * NP : 1;                 // load steps per segment
    constexpr bool QREG = CPT > 0 && !QL;
    frag qf[QREG ? kQS : 1][QREG ? NLS : 1];
    const frag* qlds = reinterpret_cast<const frag*>(S + kQ * KKp);
    if constexpr (QREG) {
#pragma unroll
        for (int s = 0; s < kQS; ++s)
#pragma unroll
            for (int ls = 0; ls < NLS; ++ls) qf[s][ls] = *reinterpret_cast<const frag*>(qsb[s] + ((size_t)ls * 64 + lane) * SG::LE);
    } else if constexpr (CPT > 0) {
        constexpr int QV = 16 * CPT * NP * (int)sizeof(T) / 16;            // 16-B vectors per segment
        uint4* dst = reinterpret_cast<uint4*>(S + kQ * KKp);
#pragma unroll
        for (int s = 0; s < kQS; ++s) {
            const uint4* src = reinterpret_cast<const uint4*>(qsb[s]);
            for (int v = tid; v < QV; v += kLookThreads) dst[s * QV + v] = src[v];
        }
    }
    // query fragments (s, load steps ls .. ls + NP - 1) of this lane
    auto qget = [&](frag (&u)[NP], int s, int ls) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if constexpr (QREG) u[p] = qf[s][ls + p];
            else u[p] = qlds[(s * NLS + ls + p) * 64 + lane];
        }
    };
    if (tid < RMD_MAX_LEVELS * 4) box[tid >> 2][tid & 3] = (tid & 1) ? -(1 << 30) : (1 << 30);
    __syncthreads();
    // thread (level, query) items: every level's window origin (coords clamped as rmd_corr_lookup does)
    for (int it = tid; it < kQ * g.L; it += kLookThreads) {
        const int q = it % kQ, L = it / kQ;
        const int y = min(qy0 + q / kBX, g.H - 1), x = min(qx0 + q % kBX, g.W - 1);
        const float cx0 = coords[((size_t)b * 2 + 0) * N + y * g.W + x];
        const float cy0 = coords[((size_t)b * 2 + 1) * N + y * g.W + x];
        const float inv = 1.0f / (float)(1 << L);
        const float rx = cx0 * inv, ry = cy0 * inv;
        const float cx = fminf(fmaxf(rx, -1.0e6f), 1.0e6f);
        const float cy = fminf(fmaxf(ry, -1.0e6f), 1.0e6f);
        const float fx0 = floorf(cx), fy0 = floorf(cy);
        const int xs = (int)fx0 - R, ys = (int)fy0 - R;
        sxs[L][q] = xs;
        sys[L][q] = ys;
        sfx[L][q] = rx - floorf(rx);                // NaN / inf coordinate -> NaN window (grid_sample)
        sfy[L][q] = ry - floorf(ry);
        atomicMin(&box[L][0], xs);
        atomicMax(&box[L][1], xs + K - 1);
        atomicMin(&box[L][2], ys);
        atomicMax(&box[L][3], ys + K - 1);
    }
    __syncthreads();                                   // boxes complete
    // thread items (q, a): query q, window x-offset a; hx[i][jj] = row jj of the window, x-interpolated
    constexpr int ITEMS = (kQ * D + kLookThreads - 1) / kLookThreads;

    for (int L = 0; L < g.L; ++L) {
        const int lh = g.lh[L], lw = g.lw[L];
        float* ob = out + ((size_t)b * g.L + L) * D * D * (size_t)N;
        // masked / degenerate level: constant output (raft_fs.py:77-78; 1-pixel levels divide by zero)
        const bool masked = (zmask >> L) & 1u;
        if (masked || lh < 2 || lw < 2) {
            const float v = masked ? 0.f : __builtin_nanf("");
            for (int idx = tid; idx < kQ * D * D; idx += kLookThreads) {
                const int q = idx % kQ, c = idx / kQ;
                const int y = qy0 + q / kBX, x = qx0 + q % kBX;
                if (y < g.H && x < g.W) ob[(size_t)c * N + y * g.W + x] = v;
            }
            continue;
        }
        const int bx0 = max(box[L][0], 0), bx1 = min(box[L][1], lw - 1);
        const int by0 = max(box[L][2], 0), by1 = min(box[L][3], lh - 1);
        const int th = max(by1 - by0 + 1, 0);
        const int sa = bx0 >> 4, nseg = bx1 >= bx0 ? (bx1 >> 4) - sa + 1 : 0;
        const int ntask = th * nseg;                   // (box row, target segment) MFMA tasks
        const T* tlev = tseg + ((size_t)b * g.TS + g.soff[L]) * segsz;

        float hx[ITEMS][K];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
#pragma unroll
            for (int jj = 0; jj < K; ++jj) hx[i][jj] = 0.f;

        if (ntask > 0 && ntask <= kMaxTasks) {
            // every query's (2r+2)^2 patch in LDS, zero where the target is off the map (zero padding)
            for (int i = tid; i < kQ * KKp; i += kLookThreads) S[i] = 0.f;
            // the lane's query in each query segment: its window origin at this level
            int wx[kQS], wy[kQS], wq[kQS];
#pragma unroll
            for (int s = 0; s < kQS; ++s) {
                wq[s] = s * kBX + (lane & 15);
                wx[s] = sxs[L][wq[s]];
                wy[s] = sys[L][wq[s]];
            }
            __syncthreads();
            // C[target 4*(lane>>4)+e][query lane&15] of task (box row r, target segment column c): keep the
            // products inside the query's own patch (kPutSel: the others go to a pad slot of the query,
            // never read, so the four LDS writes carry no branches)
            auto put = [&](const f32x4& acc, int s, int r, int c) {
                const int dy = by0 + r - wy[s];
                const int dx0 = c * 16 + 4 * (lane >> 4) - wx[s];
                const bool rok = (unsigned)dy < (unsigned)K;
                float* P = S + wq[s] * KKp;
                if constexpr (kPutSel) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) P[rok && (unsigned)(dx0 + e) < (unsigned)K ? dy * K + dx0 + e : KK] = acc[e];
                } else if (rok) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((unsigned)(dx0 + e) < (unsigned)K) P[dy * K + dx0 + e] = acc[e];
                }
            };
            auto tptr = [&](int r, int c) {
                return tlev + ((size_t)(by0 + r) * g.nsx[L] + c) * segsz + (size_t)lane * SG::LE;
            };
            // the wave's tasks w, w + kWaves, ... as (box row, segment column), advanced without division
            int tr = w / nseg, tcol = sa + w - tr * nseg;
            auto advance = [&](int& r, int& c) {
                c += kWaves;
                while (c >= sa + nseg) {
                    c -= nseg;
                    ++r;
                }
            };
            if constexpr (CPT > 0) {
                frag tc[NLS];
                for (int task = w; task < ntask; task += kWaves, advance(tr, tcol)) {
                    const T* tsb = tptr(tr, tcol);
#pragma unroll
                    for (int ls = 0; ls < NLS; ++ls) tc[ls] = *reinterpret_cast<const frag*>(tsb + (size_t)ls * 64 * SG::LE);
                    // load step outer, query segment inner: kQS independent accumulator chains interleave
                    f32x4 acc[kQS];
#pragma unroll
                    for (int s = 0; s < kQS; ++s) acc[s] = f32x4{};
#pragma unroll
                    for (int ls = 0; ls < NLS; ls += NP)
#pragma unroll
                        for (int s = 0; s < kQS; ++s) {
                            frag u[NP];
                            qget(u, s, ls);
                            seg_mma<T, X3>(acc[s], tc + ls, u);
                        }
#pragma unroll
                    for (int s = 0; s < kQS; ++s) put(acc[s], s, tr, tcol);
                }
            } else {
                for (int task = w; task < ntask; task += kWaves, advance(tr, tcol)) {
                    const T* tsb = tptr(tr, tcol);
                    f32x4 acc[kQS];
#pragma unroll
                    for (int s = 0; s < kQS; ++s) acc[s] = f32x4{};
                    for (int ls = 0; ls < nls * NP; ls += NP) {
                        frag t[NP];
#pragma unroll
                        for (int p = 0; p < NP; ++p) t[p] = *reinterpret_cast<const frag*>(tsb + (size_t)(ls + p) * 64 * SG::LE);
#pragma unroll
                        for (int s = 0; s < kQS; ++s) {
                            frag u[NP];
#pragma unroll
                            for (int p = 0; p < NP; ++p)
                                u[p] = *reinterpret_cast<const frag*>(qsb[s] + ((size_t)(ls + p) * 64 + lane) * SG::LE);
                            seg_mma<T, X3>(acc[s], t, u);
                        }
                    }
#pragma unroll
                    for (int s = 0; s < kQS; ++s) put(acc[s], s, tr, tcol);
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const int idx = tid + i * kLookThreads;
                if (idx >= kQ * D) break;
                const int q = idx % kQ, a = idx / kQ;
                const float fx = sfx[L][q];
                const float* P = S + q * KKp + a;
#pragma unroll
                for (int jj = 0; jj < K; ++jj) hx[i][jj] = fmaf(fx, P[jj * K + 1] - P[jj * K], P[jj * K]);
            }
            __syncthreads();                           // S is free for the next level
        } else if (ntask > 0) {
            // a box of more than kMaxTasks segments (flow differing by hundreds of pixels inside one
            // block): each query's own (2r+2)^2 patch, one dot product per thread
            for (int idx = tid; idx < kQ * KK; idx += kLookThreads) {
                const int q = idx / KK, r = idx - q * KK;
                const int ty = sys[L][q] + r / K, tx = sxs[L][q] + r % K;
                float acc = 0.f;
                if (ty >= 0 && ty < lh && tx >= 0 && tx < lw) {
                    const T* qs = qsb[q / kBX];
                    const T* ts = tlev + ((size_t)ty * g.nsx[L] + (tx >> 4)) * segsz;
                    for (int c = 0; c < g.C; ++c)
                        acc = fmaf(seg_elem<T, X3>(qs, q % kBX, c), seg_elem<T, X3>(ts, tx & 15, c), acc);
                }
                S[q * KKp + r] = acc;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const int idx = tid + i * kLookThreads;
                if (idx >= kQ * D) break;
                const int q = idx % kQ, a = idx / kQ;
                const float fx = sfx[L][q];
                const float* P = S + q * KKp + a;
#pragma unroll
                for (int jj = 0; jj < K; ++jj) hx[i][jj] = fmaf(fx, P[jj * K + 1] - P[jj * K], P[jj * K]);
            }
            __syncthreads();                           // S is free for the next level
        }

        // y-interpolation and the (a, b)-major output planes
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int idx = tid + i * kLookThreads;
            if (idx >= kQ * D) break;
            const int q = idx % kQ, a = idx / kQ;
            const int y = qy0 + q / kBX, x = qx0 + q % kBX;
            if (y >= g.H || x >= g.W) continue;
            const float fy = sfy[L][q] + (sfx[L][q] - sfx[L][q]);   // a NaN x weight reaches rows outside the band too
            float* o = ob + (size_t)(a * D) * N + y * g.W + x;
#pragma unroll
            for (int bb = 0; bb < D; ++bb) o[(size_t)bb * N] = fmaf(fy, hx[i][bb + 1] - hx[i][bb], hx[i][bb]);
        }
    }
}

template <typename T, bool X3>
void launch_segments(const LevelSrc& src, const OtfGeom& g, float scale, T* seg, hipStream_t st) {
    const long long n = (long long)g.B * g.TS * (g.Cp / Seg<T>::LSC) * 64;
    otf_segments_kernel<T, X3><<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, st>>>(src, g, scale, seg);
}

// One lookup over workspace ws in launch shape SH, at the radius and the compiled channel count cpt (0: the
// runtime loop) that the entry point chose: 8 radii x 5 channel counts per shape
template <typename T, bool X3, const LookShape& SH>
int launch_lookup(const void* ws, const OtfGeom& g, int radius, int cpt, const float* coords, unsigned zmask,
                  float* out, hipStream_t st) {
    using QB = QBlock<SH.qsy>;
    constexpr size_t NP = X3 ? 2 : 1;                // operand elements per value (X3: split pairs)
    const long long nblk = (long long)((g.W + QB::kBX - 1) / QB::kBX) * ((g.H + QB::kBY - 1) / QB::kBY) * g.B;
    RMD_REQUIRE(nblk < (1ll << 31), RMD_ERR_SHAPE, "rmd_corr_otf_lookup: grid too large");
    const T* q = reinterpret_cast<const T*>(ws);
    return otf_dispatch_radius(radius, [&](auto r) -> int {
        return otf_dispatch<32, 64, 128, 256, 0>(cpt, [&](auto c) -> int {
            constexpr int R = decltype(r)::value, CPT = decltype(c)::value;
            auto k = otf_lookup_kernel<T, X3, R, CPT, SH.qsy, SH.occ, SH.ql, SH.threads>;
            const size_t lds = sizeof(float) * QB::kQ * otf_patch_stride(R) +
                               (SH.ql && CPT > 0 ? (size_t)QB::kQS * 16 * CPT * NP * sizeof(T) : 0);
            RMD_REQUIRE(lds <= 160 * 1024, RMD_ERR_SHAPE, "rmd_corr_otf_lookup: %zu B of LDS per block", lds);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
            k<<<(unsigned)nblk, SH.threads, lds, st>>>(q, q + otf_query_elems(g) * NP, g, coords, zmask, out);
            return RMD_OK;
        });
    });
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" size_t rmd_corr_otf_workspace_bytes(int batch, int channels, int height, int width, int levels,
                                               int compute) {
    if (check_otf(batch, channels, height, width, levels, compute)) return 0;
    const OtfGeom g = make_otf_geom(batch, channels, height, width, levels);
    return otf_scratch_offset(g, otf_elem_bytes(compute)) + otf_scratch_elems(g) * 4;
}

extern "C" int rmd_corr_otf_prepare(const float* fmap1, const float* fmap2, int batch, int channels, int height,
                                    int width, int levels, float scale, int compute, void* workspace, void* stream) {
    RMD_REQUIRE(fmap1 && fmap2 && workspace, RMD_ERR_ARG, "rmd_corr_otf_prepare: null pointer");
    int rc = check_otf(batch, channels, height, width, levels, compute);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const OtfGeom g = make_otf_geom(batch, channels, height, width, levels);
    const OtfGeom g1 = make_otf_geom(batch, channels, height, width, 1);   // query segments: TS = QS
    LevelSrc lq{};
    lq.p[0] = fmap1;
    const LevelSrc lt = otf_level_sources(fmap2, workspace, g, compute);   // levels 1..: pooled here, in the scratch
    for (int l = 1; l < levels; ++l) {
        const long long n = (long long)batch * channels * g.lh[l] * g.lw[l];
        otf_pool2_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, st>>>(
            lt.p[l - 1], batch * channels, g.lh[l - 1], g.lw[l - 1], const_cast<float*>(lt.p[l]));
    }
    const size_t qn = otf_query_elems(g);
    if (compute == RMD_BF16) {
        __bf16* q = reinterpret_cast<__bf16*>(workspace);
        launch_segments<__bf16, false>(lq, g1, scale, q, st);
        launch_segments<__bf16, false>(lt, g, 1.0f, q + qn, st);
    } else if (compute == RMD_BF16X3) {
        __bf16* q = reinterpret_cast<__bf16*>(workspace);          // split pairs: 2 x qn bf16 = qn floats
        launch_segments<__bf16, true>(lq, g1, scale, q, st);
        launch_segments<__bf16, true>(lt, g, 1.0f, q + 2 * qn, st);
    } else {
        float* q = reinterpret_cast<float*>(workspace);
        launch_segments<float, false>(lq, g1, scale, q, st);
        launch_segments<float, false>(lt, g, 1.0f, q + qn, st);
    }
    return check_launch("rmd_corr_otf_prepare");
}

extern "C" int rmd_corr_otf_lookup(const void* workspace, int batch, int channels, int height, int width, int levels,
                                   int compute, const float* coords, int radius, unsigned zero_level_mask, float* out,
                                   void* stream) {
    RMD_REQUIRE(workspace && coords && out, RMD_ERR_ARG, "rmd_corr_otf_lookup: null pointer");
    int rc = check_otf(batch, channels, height, width, levels, compute);
    if (rc) return rc;
    RMD_REQUIRE(radius >= 1 && radius <= 8, RMD_ERR_SHAPE, "rmd_corr_otf_lookup: radius %d not in 1..8", radius);
    hipStream_t st = as_stream(stream);
    const OtfGeom g = make_otf_geom(batch, channels, height, width, levels);
    // compiled channel counts keep the query segments in registers; f32 operands of >= 128 channels
    // would not fit and take the runtime loop
    const int cpt = (compute == RMD_F32 && g.Cp >= 128) || g.Cp > 256 ? 0 : g.Cp;
    // bf16 on wide maps (at least kWideBlocks 16x2 query blocks): 16x4 blocks at 512 threads read 45 %
    // fewer target bytes per query; at the 4K map (b2, 270x480) 362 us vs 396 us per lookup, at cfg2
    // (1,792 blocks) 77 vs 73 us (profiles/otf_put_ab_r04.json, box r04t)
    const long long blocks16x2 = (long long)((width + 15) / 16) * ((height + 1) / 2) * batch;
    if (compute == RMD_BF16 && blocks16x2 >= kWideBlocks)
        rc = launch_lookup<__bf16, false, kShapeWide>(workspace, g, radius, cpt, coords, zero_level_mask, out, st);
    else if (compute == RMD_BF16)
        rc = launch_lookup<__bf16, false, kShapeBf16>(workspace, g, radius, cpt, coords, zero_level_mask, out, st);
    else if (compute == RMD_BF16X3)
        rc = launch_lookup<__bf16, true, kShapeSplit>(workspace, g, radius, cpt, coords, zero_level_mask, out, st);
    else
        rc = launch_lookup<float, false, kShapeF32>(workspace, g, radius, cpt, coords, zero_level_mask, out, st);
    if (rc) return rc;
    return check_launch("rmd_corr_otf_lookup");
}
