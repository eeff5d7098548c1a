// corr_pyramid_stationary.hip — the bf16 correlation GEMM with 64-bit store addressing (fp16 pyramid in the row
// layout, C <= 256): the route of maps whose level spans pass 1 GiB (4K frames), which corr_pyramid_w8's 32-bit
// buffer offsets cannot reach.  Operands come from corr_pyramid_tiled.hip's prep.
//
// One workgroup = 4 waves (one per SIMD, 512-register budget) owns a 16x16 block of target pixels: its A operand
// (256 targets x 256 bf16 = 128 KiB) is loaded into LDS once, 16-B chunks XOR-swizzled by row so the
// 16 rows a ds_read_b128 lane group reads hit distinct banks.  Each wave sweeps 32-query tiles:
// 8 MFMA 32x32x16 tiles per k-step (all 256 targets x 32 queries), then pools in-lane and stores
// every level straight from registers.  v_permlane32_swap pairs the two half-waves' 8-byte row
// halves into full 16-byte row chunks, so one store instruction writes two contiguous 512-byte runs.
// The next tile's B fragments load during the epilogue.  (An 8-wave form, two waves per SIMD with 8 target
// rows each, and two diagnostic ablations are in git history.)

#include "corr_pyramid.h"

namespace rmd {
namespace {

constexpr int kWaves = 4;        // one per SIMD: each owns all 16 target rows of the block, and every 4th query tile
constexpr int kThreads = 64 * kWaves;
constexpr int kTiles = 8;        // MFMA 32x32 tiles per wave
// Stores per lane per 32-query tile: 16 + 4 + 2 + 1 over levels 0-3.  The load window's wait (s_load_b_asm)
// counts on exactly this many; tests/test_asm_audit.py checks it in the compiled kernel.
constexpr int kStores = 23;

// LDS swizzle of the A block (256 target rows x 32 16-B chunks): chunk' = chunk ^ swz(row).
// A ds_read_b128 fragment read serves the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (and
// +32) in one LDS cycle each iff their 16 addresses fall in distinct 16-B bank slots.  The lanes
// of a fragment read rows base + 16*(j>>3) + (j&7) (j = lane & 31) at one chunk, so the slot must
// separate j&7 AND the parity of j>>3: swz = (row & 7) | ((row >> 4) & 1) << 3.  (row & 15 alone
// maps j and j+8 to one slot: a 2-way conflict on every fragment read.)
__device__ __forceinline__ int a_swz(int row) { return (row & 7) | ((row >> 1) & 8); }

// per-wave store geometry: element offsets of the wave's first row/chunk on every level, row and
// chunk strides, valid rows/chunks; a store address is base + uniform constant + per-lane offset
struct SCtx {
    int N;
    size_t base[4];     // level offset + row/chunk origin of this wave's rows (elements)
    size_t rs[4];       // row stride (elements)
    size_t cs[4];       // chunk stride = N * chunk width (elements)
    int rows[4];        // valid rows of this wave per level
    int chunks[4];      // valid chunks of this block per level (<= 2, 1, 1, 1)
};

// B-fragment loads in inline asm, retired by ONE hand-placed `s_waitcnt vmcnt(kStores)`: between a
// tile's loads and that wait the wave issues exactly kStores compiler stores (the epilogue, every
// store unconditional) and no other vector-memory op (no compiler-visible global loads in the
// loop, no spills: checked in the .s by tests/test_asm_audit.py), so the wait retires the loads
// while the previous stores stay in flight.  hipcc does not count asm loads, so it never inserts
// its own draining vmcnt(0).
__device__ __forceinline__ void s_load_b_asm(bf16x8 (&bq)[16], const __bf16* src) {
#define RMD_GLD(S) asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(bq[S]) : "v"(src), "i"((S) * 32) : "memory")
    RMD_GLD(0); RMD_GLD(1); RMD_GLD(2); RMD_GLD(3); RMD_GLD(4); RMD_GLD(5); RMD_GLD(6); RMD_GLD(7);
    RMD_GLD(8); RMD_GLD(9); RMD_GLD(10); RMD_GLD(11); RMD_GLD(12); RMD_GLD(13); RMD_GLD(14); RMD_GLD(15);
#undef RMD_GLD
}

template <int N>
__device__ __forceinline__ void s_wait_b(bf16x8 (&bq)[16]) {
    asm volatile("s_waitcnt vmcnt(%16)"
                 : "+v"(bq[0]), "+v"(bq[1]), "+v"(bq[2]), "+v"(bq[3]), "+v"(bq[4]), "+v"(bq[5]), "+v"(bq[6]),
                   "+v"(bq[7]), "+v"(bq[8]), "+v"(bq[9]), "+v"(bq[10]), "+v"(bq[11]), "+v"(bq[12]), "+v"(bq[13]),
                   "+v"(bq[14]), "+v"(bq[15])
                 : "i"(N)
                 : "memory");
}

__device__ __forceinline__ void s_lda(bf16x8 (&a)[kTiles], const unsigned char* smem, const int (&arow)[kTiles], int s, int h) {
    constexpr int Cp = 256;
#pragma unroll
    for (int ti = 0; ti < kTiles; ++ti) {
        const int row = arow[ti];
        a[ti] = *reinterpret_cast<const bf16x8*>(smem + (size_t)row * Cp * 2 + (((2 * s + h) ^ a_swz(row)) << 4));
    }
}

// 16 k-steps x 8 MFMA tiles; the A fragments of step s+1 are read from LDS while step s's MFMAs run
__device__ __forceinline__ void s_mma(f32x16 (&acc)[kTiles], const bf16x8 (&bq)[16], const unsigned char* smem,
                                      const int (&arow)[kTiles], int h) {
#pragma unroll
    for (int ti = 0; ti < kTiles; ++ti)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ti][e] = 0.f;
    bf16x8 a0[kTiles], a1[kTiles];
    s_lda(a0, smem, arow, 0, h);
#pragma unroll
    for (int s = 0; s < 16; s += 2) {
        s_lda(a1, smem, arow, s + 1, h);
#pragma unroll
        for (int ti = 0; ti < kTiles; ++ti) acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[ti], bq[s], acc[ti], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < 16) s_lda(a0, smem, arow, s + 2, h);
#pragma unroll
        for (int ti = 0; ti < kTiles; ++ti) acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[ti], bq[s + 1], acc[ti], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Every store is unconditional: an invalid one (query past N, row or chunk outside a level, a
// level beyond g.levels) goes to `trash`, this lane's own 16-B slot, so each tile issues exactly
// kStores stores (see s_load_b_asm).  The address is computed either way and then selected: no branch.
__device__ __forceinline__ __half* sel(bool ok, __half* p, __half* trash) { return ok ? p : trash; }

__device__ __forceinline__ void s_epilogue(const f32x16 (&acc)[kTiles], const SCtx& c, int q, int h,
                                           __half* __restrict__ pyr, __half* __restrict__ trash) {
    const bool qv = q < c.N;
    // per-lane parts of the addresses: query offset and the half-wave's row (h)
    __half* p0 = pyr + c.base[0] + (size_t)q * 8 + h * c.rs[0];
    __half* p1 = pyr + c.base[1] + (size_t)q * 8 + h * c.rs[1];
    // V(row, cg 0..1, k 0..3) = level-0 value at the block's target row, col 8cg + 4h + k (the
    // 1/sqrt(C) scale is folded into the operands by the prep)
#define V(row, cg, k) RMD_ACC(acc, row, cg, k)
    // level 0: rows 2m + h after the swap; chunk tc
#pragma unroll
    for (int tc = 0; tc < 2; ++tc) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int r0 = 2 * m;
            unsigned x0 = pack_half2(V(r0, tc, 0), V(r0, tc, 1));
            unsigned x1 = pack_half2(V(r0, tc, 2), V(r0, tc, 3));
            unsigned y0 = pack_half2(V(r0 + 1, tc, 0), V(r0 + 1, tc, 1));
            unsigned y1 = pack_half2(V(r0 + 1, tc, 2), V(r0 + 1, tc, 3));
            swap32(x0, y0);
            swap32(x1, y1);
            const bool ok = qv && r0 + h < c.rows[0] && tc < c.chunks[0];
            *reinterpret_cast<uint4*>(sel(ok, p0 + r0 * c.rs[0] + tc * c.cs[0], trash)) = make_uint4(x0, x1, y0, y1);
        }
    }
    // level 1: lane h holds cols {2h, 2h+1} (cg 0) and {4+2h, 5+2h} (cg 1) of 8 rows
    float l1[8][2][2];
#pragma unroll
    for (int yy = 0; yy < 8; ++yy)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                l1[yy][cg][u] = 0.25f * ((V(2 * yy, cg, 2 * u) + V(2 * yy, cg, 2 * u + 1)) +
                                         (V(2 * yy + 1, cg, 2 * u) + V(2 * yy + 1, cg, 2 * u + 1)));
#undef V
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        unsigned x0 = pack_half2(l1[2 * m][0][0], l1[2 * m][0][1]);
        unsigned x1 = pack_half2(l1[2 * m][1][0], l1[2 * m][1][1]);
        unsigned y0 = pack_half2(l1[2 * m + 1][0][0], l1[2 * m + 1][0][1]);
        unsigned y1 = pack_half2(l1[2 * m + 1][1][0], l1[2 * m + 1][1][1]);
        swap32(x0, y0);
        swap32(x1, y1);
        const bool ok = qv && 2 * m + h < c.rows[1] && c.chunks[1] > 0;
        *reinterpret_cast<uint4*>(sel(ok, p1 + 2 * m * c.rs[1], trash)) = make_uint4(x0, y0, x1, y1);
    }
    // level 2: lane h holds cols {h, 2+h} of 4 rows; it stores rows 2h, 2h + 1
    float l2[4][2];
#pragma unroll
    for (int yy = 0; yy < 4; ++yy)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg)
            l2[yy][cg] = 0.25f * ((l1[2 * yy][cg][0] + l1[2 * yy][cg][1]) + (l1[2 * yy + 1][cg][0] + l1[2 * yy + 1][cg][1]));
    {
        unsigned mine[4], other[4];
#pragma unroll
        for (int yy = 0; yy < 4; ++yy) {
            mine[yy] = pack_half2(l2[yy][0], l2[yy][1]);          // (col h, col 2+h)
            other[yy] = __shfl_xor(mine[yy], 32);
        }
        __half* p2 = pyr + c.base[2] + (size_t)q * 4 + 2 * h * c.rs[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            // row 2h + k, selected with compile-time indices (a runtime index would go to scratch)
            const unsigned mk = h ? mine[2 + k] : mine[k];
            const unsigned ok_ = h ? other[2 + k] : other[k];
            const unsigned e0 = h ? ok_ : mk;      // cols 0 and 2 (held by h = 0)
            const unsigned e1 = h ? mk : ok_;      // cols 1 and 3 (held by h = 1)
            const bool ok = qv && 2 * h + k < c.rows[2] && c.chunks[2] > 0;
            *reinterpret_cast<uint2*>(sel(ok, p2 + k * c.rs[2], trash)) =
                make_uint2((e0 & 0xffffu) | (e1 << 16), (e0 >> 16) | (e1 & 0xffff0000u));
        }
    }
    // level 3: 2 rows of 2 cols; lane h stores row h
    {
        float t3[2][2];
#pragma unroll
        for (int yy = 0; yy < 2; ++yy)
#pragma unroll
            for (int cg = 0; cg < 2; ++cg) {
                const float s_ = l2[2 * yy][cg] + l2[2 * yy + 1][cg];
                t3[yy][cg] = 0.25f * (s_ + __shfl_xor(s_, 32));
            }
        const unsigned v = h ? pack_half2(t3[1][0], t3[1][1]) : pack_half2(t3[0][0], t3[0][1]);
        const bool ok = qv && h < c.rows[3] && c.chunks[3] > 0;
        *reinterpret_cast<unsigned*>(sel(ok, pyr + c.base[3] + (size_t)q * 2 + h * c.rs[3], trash)) = v;
    }
}

__global__ void __launch_bounds__(kThreads, 1)
corr_pyramid_stationary(const __bf16* __restrict__ opA, const __bf16* __restrict__ opB, PyrGeom g, int qsplit,
                        __half* __restrict__ pyr, __half* __restrict__ trash_base) {
    constexpr int Cp = 256, CPR = Cp / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int H = g.height, W = g.width, N = H * W;
    const int ncb = (W + 15) >> 4;
    const int nblk = ((H + 15) >> 4) * ncb;
    const int lid = xcd_block(blockIdx.x, gridDim.x);  // consecutive logical blocks (same batch) share an XCD's L2
    const int tb = lid % nblk;
    const int rest = lid / nblk;
    const int split = rest % qsplit;
    const int b = rest / qsplit;
    const int rb = tb / ncb, cb = tb - rb * ncb;
    const int ty0 = rb * 16, tx0 = cb * 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);    // wave-uniform: scalar loop control
    const int j = lane & 31, h = lane >> 5;
    __half* trash = trash_base + lane * 8;            // 16 B per lane (stores of all waves may collide)

    // ---- A block -> LDS (zero rows for targets outside the image) ------------------------------
    const __bf16* gA = opA + (size_t)b * N * Cp;
    for (int id = tid; id < 256 * CPR; id += kThreads) {
        const int row = id / CPR, c = id - row * CPR;
        const int ty = ty0 + (row >> 4), tx = tx0 + (row & 15);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ty < H && tx < W) v = *reinterpret_cast<const uint4*>(gA + (size_t)(ty * W + tx) * Cp + c * 8);
        *reinterpret_cast<uint4*>(smem + (size_t)row * Cp * 2 + ((c ^ a_swz(row)) << 4)) = v;
    }
    __syncthreads();

    // LDS row of this lane's A fragment for tile ti (4 target rows x 8 target cols)
    int arow[kTiles];
#pragma unroll
    for (int ti = 0; ti < kTiles; ++ti) arow[ti] = (4 * (ti >> 1) + (j >> 3)) * 16 + 8 * (ti & 1) + (j & 7);

    SCtx c;
    c.N = N;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int cw = g.tw[l], span = 16 >> l, nch = l == 0 ? 2 : 1;   // rows of the block at level l
        const int y0 = rb * span, xc0 = cb * nch;
        const bool lv = l < g.levels;
        c.cs[l] = (size_t)N * cw;
        c.rs[l] = lv ? (size_t)g.tx[l] * N * cw : 0;
        c.base[l] = lv ? (size_t)g.off[l] + (((size_t)b * g.ty[l] + y0) * g.tx[l] + xc0) * N * cw : 0;
        c.rows[l] = lv ? max(0, min(span, g.ty[l] - y0)) : 0;
        c.chunks[l] = lv ? max(0, min(nch, g.tx[l] - xc0)) : 0;
    }

    const __bf16* gB = opB + (size_t)b * N * Cp;
    const int nqt = (N + 31) >> 5;
    const int stride = kWaves * qsplit;
    int qt = split * kWaves + w;
    if (qt >= nqt) return;
    // software pipeline: tile t+1's B fragments load right after tile t's MFMAs (their registers
    // are free then) and land while tile t's epilogue runs; one B buffer, one explicit wait
    bf16x8 bq[16];
    f32x16 acc[kTiles];
    const int last = nqt - 1;
    const size_t hoff = 8 * h;
    s_load_b_asm(bq, gB + (size_t)min(qt * 32 + j, N - 1) * Cp + hoff);
    s_wait_b<0>(bq);
    while (true) {
        const int qn = qt + stride;
        s_mma(acc, bq, smem, arow, h);
        s_load_b_asm(bq, gB + (size_t)min(min(qn, last) * 32 + j, N - 1) * Cp + hoff);
        s_epilogue(acc, c, qt * 32 + j, h, pyr, trash);
        s_wait_b<kStores>(bq);
        if (qn >= nqt) break;
        qt = qn;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

namespace stationary {

bool eligible(const rmd_pyramid_desc& d, int channels) {
    return d.storage == RMD_F16 && padded_channels(channels) == 256;
}

int pyramid(const rmd_pyramid_desc& d, void* pyramid, void* workspace, hipStream_t st) {
    constexpr int Cp = 256;
    const int N = d.height * d.width;
    __bf16* opA = reinterpret_cast<__bf16*>(workspace);
    __bf16* opB = opA + (size_t)d.batch * N * Cp;
    const int nblk = ((d.height + 15) / 16) * ((d.width + 15) / 16);
    const int nqt = (N + 31) / 32;
    // query tiles split over workgroups only when the blocks alone do not fill the chip's 256 CUs
    int qsplit = 1;
    while (nblk * d.batch * qsplit < 256 && qsplit * 16 <= nqt) qsplit *= 2;
    const int lds = 256 * Cp * 2;
    const int nwg = nblk * d.batch * qsplit;
    // the lanes' trash slots: the workspace's tail, behind the B operand padded to whole query tiles
    __half* trash = reinterpret_cast<__half*>(opB + (size_t)d.batch * nqt * 32 * Cp);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(corr_pyramid_stationary),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    corr_pyramid_stationary<<<nwg, kThreads, lds, st>>>(opA, opB, make_geom(d), qsplit,
                                                       reinterpret_cast<__half*>(pyramid), trash);
    return check_launch("rmd_corr_pyramid/gemm-stationary");
}

}  // namespace stationary
}  // namespace rmd
