// corr_pyramid_w8.hip — the bf16 correlation GEMM of the performance path (bf16 operands, fp16 pyramid in the
// tiles layout of rmd.h, C <= 256, 32-bit store offsets) and its operand prep, in two forms: corr_pyramid_w8 reads
// both operands from the workspace (prep_pair), corr_pyramid_w8_f32 only the queries (prep_queries) and builds its
// target tiles from fp32 fmap2 (stage_a_f32).
//
// One workgroup (8 waves, two per SIMD) owns a 16x16 block of level-0 target pixels; its A operand
// (256 targets x 256 channels bf16) stays in LDS while the waves sweep their own 32-query tiles
// (query slots 32 qt .. 32 qt + 31 of the tiles layout: a 2 x 16 patch of query pixels).  Per tile
// a wave runs 16 k-steps x 8 MFMA 32x32x16 tiles into 128 accumulator VGPRs, then the epilogue pools
// in-lane and stores every level straight from registers:
//  * in the 32x32 accumulator layout lane (j, h) holds, for query slot j, target rows 4i..4i+3 x
//    columns 8cg + 4h .. +3 of MFMA tile (i, cg): a 2 x 4 level-0 chunk of the tiles layout is one
//    lane's own 8 values (one 16-B store, lanes h = 0/1 writing neighbouring quads: each store
//    instruction writes two contiguous 512-B runs); level-1 2 x 4 chunks and level-2 1 x 4 chunks
//    need one v_permlane32_swap per row pair, level 3 one lane exchange;
//  * stores are raw buffer stores through one descriptor per level covering the block's valid chunk
//    rows: the per-lane 32-bit offset = slot * chunk bytes + quad * chunk stride (a 1 GiB bias for a
//    quad past the level), rows past the level fall outside num_records and are dropped by the
//    hardware range check — no predication, no redirect.  Slots of no pixel (x >= W) compute and
//    store a clamped query's values into their own slot, so every 128-B line is written whole.

#include "corr_pyramid.h"

namespace rmd {
namespace {

// prep (prep_pair: both operands in one launch, the bf16-staging GEMM's; prep_queries: the B operand alone, the
// fp32-staging GEMM's): grid (128-element tiles, B, 2).  z = 0: fmap2 ->
// A operand (B, N, 256) bf16 * scale over raster pixels; z = 1: fmap1 -> B operand over the query
// slots of the tiles layout (rmd.h), in MFMA B-fragment order
//   o[b][qt][s][lane][8]  (lane = j + 32h: channels 16s + 8h .. +7 of slot 32 qt + j),
// so each of a wave's 16 B-fragment loads per 32-query tile is one contiguous 1 KiB read.  Read
// phase: a thread loads 8 channels x 4 pixels (a slot quad is 4 consecutive pixels of one row:
// float4 per channel row), converts, and writes the 4 pixels' 16-B channel octets into a bf16 LDS
// tile.  Write phase: one 16-B fragment per lane-store, the tile's output is one contiguous 64 KiB
// block for either operand.  Slots of no pixel take a clamped pixel's features.
constexpr int kPrepPx = 128, kPrepStride = 256 * 2 + 16;     // LDS row: 256 bf16 + 16 B pad

// One 128-element tile of operand `which` of image b = blockIdx.y, tile blockIdx.x.
__device__ __forceinline__ void prep_tile(const int which, const float* f1, const float* f2, __bf16* opA, __bf16* opB,
                                          int C, int H, int W, int S, int nqt, float scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.y;
    const int N = H * W;
    const float* f = which ? f1 : f2;
    const float s = which ? 1.0f : scale;
    const int t = threadIdx.x;
    const int p0 = blockIdx.x * kPrepPx;
    if (p0 >= (which ? S : N)) return;               // block-uniform
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int item = it * 512 + t;               // (channel octet cg, element quad q), q fastest
        const int q = item & 31, cg = item >> 5;
        // the quad's first pixel (y1, x1) and whether all 4 are in the map and 16-B aligned
        int y1, x1;
        if (which) {
            tiles_pixel(p0 + 4 * q, H, W, y1, x1);
        } else {
            y1 = 0;
            x1 = p0 + 4 * q;                         // raster: row 0 of a 1 x N map
        }
        const int lim = which ? W : N;
        const bool full = (which ? y1 < H : true) && x1 + 3 < lim && (lim & 3) == 0;
        const int yc = which ? min(y1, H - 1) : 0;
        const float* src = f + ((size_t)b * C) * N + (size_t)yc * (which ? W : 0);
        float v[8][4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = cg * 8 + e;
            const float* row = src + (size_t)c * N;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < C) {
                if (full) {
                    x = *reinterpret_cast<const float4*>(row + x1);
                } else {
                    x.x = row[min(x1 + 0, lim - 1)];
                    x.y = row[min(x1 + 1, lim - 1)];
                    x.z = row[min(x1 + 2, lim - 1)];
                    x.w = row[min(x1 + 3, lim - 1)];
                }
            }
            v[e][0] = x.x * s;
            v[e][1] = x.y * s;
            v[e][2] = x.z * s;
            v[e][3] = x.w * s;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e][i];
            *reinterpret_cast<bf16x8*>(lds + (size_t)(4 * q + i) * kPrepStride + cg * 16) = o;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int k = it * 512 + t;                  // 16-B output chunk of the tile's 64 KiB block
        int px, c0;
        if (which) {                                 // fragment order per 32-pixel tile: k = (tile, s, lane)
            const int L = k & 63, st = (k >> 6) & 15;
            px = (k >> 10) * 32 + (L & 31);
            c0 = 16 * st + 8 * (L >> 5);
        } else {                                     // pixel-major: k = px * 32 + octet
            px = k >> 5;
            c0 = (k & 31) * 8;
        }
        const bf16x8 o = *reinterpret_cast<const bf16x8*>(lds + (size_t)px * kPrepStride + c0 * 2);
        if (which) {
            const int qt = blockIdx.x * 4 + (k >> 10);
            if (qt < nqt) *reinterpret_cast<bf16x8*>(opB + (((size_t)b * nqt + qt) * 1024 + (k & 1023)) * 8) = o;
        } else if (p0 + px < N) {
            *reinterpret_cast<bf16x8*>(opA + ((size_t)b * N + p0) * 256 + (size_t)k * 8) = o;
        }
    }
}

__global__ void __launch_bounds__(512)
prep_pair(const float* __restrict__ f1, const float* __restrict__ f2, __bf16* __restrict__ opA,
          __bf16* __restrict__ opB, int C, int H, int W, int S, int nqt, float scale) {
    prep_tile(blockIdx.z, f1, f2, opA, opB, C, H, W, S, nqt, scale);
}

// The z = 1 half alone, grid (tiles, B): the fp32-staging GEMM (corr_pyramid_w8_f32) reads fmap2 itself.
__global__ void __launch_bounds__(512)
prep_queries(const float* __restrict__ f1, __bf16* __restrict__ opB, int C, int H, int W, int S, int nqt) {
    prep_tile(1, f1, nullptr, nullptr, opB, C, H, W, S, nqt, 1.0f);
}

// ---- the pooled epilogue, in 16 pieces -----------------------------------------------------------

constexpr unsigned kBig = 0x40000000u;    // offset bias that lands beyond every level's range

// Cache-policy bits of every pyramid store: 2 = non-temporal (the pyramid is re-read a whole GEMM later).
// Plain stores: 0.305-0.309 vs 0.213-0.216 ms (profiles/gemm_ab_r02_cpol.json); temporal stores on levels 1-3
// only: lookups 26.0 vs 27.6 us but the GEMM 0.258-0.274 vs 0.211 ms (profiles/w8_store_policy_ab_r06.json).
constexpr int kStoreAux = 2;

struct Lvl {
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned rs;      // chunk-row stride (bytes)
    unsigned cs;      // chunk stride (bytes): next quad / chunk of the same chunk row
    unsigned hd;      // paired block (corr_pyramid_w8): added to the offsets of the block's second row
                      // half, which holds the NEXT column block's rows: chunks per block * cs - half rows * rs
    int nq;           // valid chunks of this block's chunk rows (level 0: 0..4, 1: 0..2, 2-3: 0..1)
};

struct Ctx {
    Lvl l[4];
};

// lane-dependent parts of the store offsets of query slot q (bytes)
struct LaneOff {
    unsigned o0[2];   // level 0, column group tc: quad 2 tc + h
    unsigned o1;      // level 1: quad h
    unsigned o2;      // level 2: chunk row h of each stored pair
    unsigned o3;      // level 3: chunk row h
};

__device__ __forceinline__ LaneOff lane_offsets(const Ctx& c, int q, int h) {
    LaneOff r;
    const unsigned uq = (unsigned)q;
#pragma unroll
    for (int tc = 0; tc < 2; ++tc)
        r.o0[tc] = 2 * tc + h < c.l[0].nq ? uq * 16u + (unsigned)(2 * tc + h) * c.l[0].cs : kBig;
    r.o1 = h < c.l[1].nq ? uq * 16u + (unsigned)h * c.l[1].cs : kBig;
    r.o2 = c.l[2].nq > 0 ? uq * 8u + (unsigned)h * c.l[2].rs : kBig;
    r.o3 = c.l[3].nq > 0 ? uq * 4u + (unsigned)h * (c.l[3].rs + c.l[3].hd) : kBig;
    return r;
}

// per-tile running sums of the epilogue (unscaled: level-l sums are 4^l x the average)
struct EpiState {
    float s1[8][2][2];    // level-1 row yy (0..7), col group cg, pair u
    float s2[4][2];       // level-2 row, col group
};

#define V(row, cg, k) RMD_ACC(acc, row, cg, k)

// Epilogue piece s (0..15) of one tile, from accumulator set `acc`: level-0 chunk row m = s/2 of
// column group tc = s%2, the level-1 sums of those rows, and every 4th / 8th / 16th piece the level-1
// / level-2 / level-3 stores — so the pieces can ride along the k-steps of the next tile.
template <int S>
__device__ __forceinline__ void epi_piece(const f32x16 (&acc)[8], const Ctx& c, const LaneOff& lo, EpiState& st) {
    constexpr int m = S >> 1, tc = S & 1;
    // level 0: chunk rows 2m, 2m+1 x cols 8 tc + 4h .. +3 — this lane's own values
    {
        const i32x4 d = {(int)pack_half2(V(2 * m, tc, 0), V(2 * m, tc, 1)),
                         (int)pack_half2(V(2 * m, tc, 2), V(2 * m, tc, 3)),
                         (int)pack_half2(V(2 * m + 1, tc, 0), V(2 * m + 1, tc, 1)),
                         (int)pack_half2(V(2 * m + 1, tc, 2), V(2 * m + 1, tc, 3))};
        __builtin_amdgcn_raw_buffer_store_b128(d, c.l[0].rsrc,
                                               (int)(lo.o0[tc] + (unsigned)m * c.l[0].rs + (m >= 4 ? c.l[0].hd : 0u)),
                                               0, kStoreAux);
    }
    // level-1 sums of level-1 row m, col group tc: cols {2h, 2h+1} (tc 0) / {4+2h, 5+2h} (tc 1)
#pragma unroll
    for (int u = 0; u < 2; ++u)
        st.s1[m][tc][u] = (V(2 * m, tc, 2 * u) + V(2 * m, tc, 2 * u + 1)) +
                          (V(2 * m + 1, tc, 2 * u) + V(2 * m + 1, tc, 2 * u + 1));
    if constexpr ((S & 3) == 3) {
        // level-1 chunk row p (rows 2p, 2p+1) complete: lane h stores quad h (cols 4h .. 4h+3).  Per
        // row, x = cols {2h, 2h+1}, y = cols {4+2h, 5+2h}; the swap leaves lanes h = 0 with cols 0-3
        // and lanes h = 1 with cols 4-7 as (x, y)
        constexpr int p = S >> 2;
        unsigned x0 = pack_half2(0.25f * st.s1[2 * p][0][0], 0.25f * st.s1[2 * p][0][1]);
        unsigned y0 = pack_half2(0.25f * st.s1[2 * p][1][0], 0.25f * st.s1[2 * p][1][1]);
        unsigned x1 = pack_half2(0.25f * st.s1[2 * p + 1][0][0], 0.25f * st.s1[2 * p + 1][0][1]);
        unsigned y1 = pack_half2(0.25f * st.s1[2 * p + 1][1][0], 0.25f * st.s1[2 * p + 1][1][1]);
        swap32(x0, y0);
        swap32(x1, y1);
        const i32x4 d = {(int)x0, (int)y0, (int)x1, (int)y1};
        __builtin_amdgcn_raw_buffer_store_b128(d, c.l[1].rsrc,
                                               (int)(lo.o1 + (unsigned)p * c.l[1].rs + (p >= 2 ? c.l[1].hd : 0u)), 0, kStoreAux);
        // level-2 sums of level-2 row p: lane h holds cols {h, 2+h}
#pragma unroll
        for (int cg = 0; cg < 2; ++cg)
            st.s2[p][cg] = (st.s1[2 * p][cg][0] + st.s1[2 * p][cg][1]) + (st.s1[2 * p + 1][cg][0] + st.s1[2 * p + 1][cg][1]);
    }
    if constexpr ((S & 7) == 7) {
        // level-2 rows 2k, 2k+1 complete (k = S >> 3): lanes h -> row 2k+h, 4 cols (8 B)
        constexpr int k = S >> 3;
        unsigned x = pack_half2(0.0625f * st.s2[2 * k][0], 0.0625f * st.s2[2 * k][1]);          // row 2k:   cols h, 2+h
        unsigned y = pack_half2(0.0625f * st.s2[2 * k + 1][0], 0.0625f * st.s2[2 * k + 1][1]);  // row 2k+1: cols h, 2+h
        swap32(x, y);       // lane h now holds row 2k+h: x = cols {0,2}, y = cols {1,3}
        const i32x2 d = {(int)__builtin_amdgcn_perm(y, x, 0x05040100u), (int)__builtin_amdgcn_perm(y, x, 0x07060302u)};
        __builtin_amdgcn_raw_buffer_store_b64(d, c.l[2].rsrc,
                                              (int)(lo.o2 + (unsigned)(2 * k) * c.l[2].rs + (k >= 1 ? c.l[2].hd : 0u)), 0, kStoreAux);
    }
    if constexpr (S == 15) {
        // level 3: rows 0, 1 (level-2 rows 0-1 / 2-3), cols 0, 1 (level-2 cols {0,1} / {2,3});
        // own partial of col cg is level-2 col 2cg+h; the swap adds the other half's
        float a0[2], a1[2];
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
            a0[cg] = st.s2[0][cg] + st.s2[1][cg];
            a1[cg] = st.s2[2][cg] + st.s2[3][cg];
        }
        unsigned x0 = __float_as_uint(a0[0]), y0 = __float_as_uint(a1[0]);
        unsigned x1 = __float_as_uint(a0[1]), y1 = __float_as_uint(a1[1]);
        swap32(x0, y0);     // lane h: x0 + y0 = full row-h sum of col 0
        swap32(x1, y1);
        const float inv = 1.0f / 64.0f;
        const unsigned v = pack_half2(inv * (__uint_as_float(x0) + __uint_as_float(y0)),
                                      inv * (__uint_as_float(x1) + __uint_as_float(y1)));
        __builtin_amdgcn_raw_buffer_store_b32((int)v, c.l[3].rsrc, (int)lo.o3, 0, kStoreAux);
    }
}
#undef V

// ---- padded, swizzle-free A layout -------------------------------------------------------------
// LDS row of block target (y, x) = (x>>3)*128 + y*8 + (x&7), rows 528 B apart (256 bf16 + 16 B pad).
// The 32 targets of MFMA tile ti (4 rows x 8 cols) are then the consecutive LDS rows
// (ti&1)*128 + (ti>>1)*32 + j, so lane (j, h)'s fragment of tile ti at k-step s sits at
//   base[ti&1] + (ti>>1)*32*528 + 32*s,   base[e] = (e*128 + j)*528 + 16h:
// two address VGPRs for the whole tile loop, everything else an instruction immediate (<= 51168).
// Banks: 528 B = 33 x 16 B, so a ds_read_b128 lane group's 16 rows land in 16-B slots (row + chunk)
// mod 16 = j mod 16 over lanes {0-3,12-15,20-27} and {4-11,16-19,28-31}: conflict-free, no XOR.
constexpr unsigned kPadRow = 528;

__device__ __forceinline__ int pad_row(int y, int x) { return ((x >> 3) << 7) + (y << 3) + (x & 7); }

// ---- B-fragment register ring ------------------------------------------------------------------
// k-step s of every tile lives in slot s % 8 and is loaded 7 k-steps (56 MFMAs) ahead — the previous
// tile's k-steps 9-15 load this tile's 0-6 — instead of all 16 (64 VGPRs) being held for the whole
// tile; the 32 VGPRs freed double-buffer the A fragments: k-step s+1's 8 fragments are read at the
// top of k-step s.  One scheduling region per k-step keeps both sets of loads where they are issued.
constexpr int kEpiStores = 24;  // buffer stores of one ping-pong epilogue (23 in the .s), for vmcnt_pad_n
constexpr int kRing = 8;

template <int S>
__device__ __forceinline__ void read_a8(bf16x8 (&a)[8], const unsigned char* smem, unsigned b0, unsigned b1) {
#pragma unroll
    for (int ti = 0; ti < 8; ++ti)
        a[ti] = *reinterpret_cast<const bf16x8*>(smem + ((ti & 1) ? b1 : b0) + (unsigned)((ti >> 1) * 32 * kPadRow + 32 * S));
}

template <int S>
__device__ __forceinline__ void ksteps_ring(f32x16 (&acc)[8], bf16x8 (&acur)[8], bf16x8 (&anext)[8],
                                            bf16x8 (&ring)[kRing], const unsigned char* smem, unsigned b0,
                                            unsigned b1, const __bf16* cur, const __bf16* nxt) {
    if constexpr (S < 16) {
        if constexpr (S + 1 < 16) read_a8<S + 1>(anext, smem, b0, b1);
        {
            constexpr int T = S + kRing - 1;
            ring[T % kRing] = *reinterpret_cast<const bf16x8*>((T < 16 ? cur : nxt) + 512 * (T & 15));
        }
        const f32x16 zero = {};
#pragma unroll
        for (int ti = 0; ti < 8; ++ti)
            acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(acur[ti], ring[S % kRing], S == 0 ? zero : acc[ti], 0, 0, 0);
        // order inside the region: the 8 LDS reads of k-step S+1 and the ring load first, then the MFMAs
        if constexpr (S + 1 < 16) __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        __builtin_amdgcn_sched_barrier(0);
        ksteps_ring<S + 1>(acc, anext, acur, ring, smem, b0, b1, cur, nxt);
    }
}

template <int S>
__device__ __forceinline__ void epilogue(const f32x16 (&acc)[8], const Ctx& c, const LaneOff& lo, EpiState& st) {
    if constexpr (S < 16) {
        epi_piece<S>(acc, c, lo, st);
        epilogue<S + 1>(acc, c, lo, st);
    }
}

// ---- A staging from fp32 -----------------------------------------------------------------------
// The LDS A image of one workgroup built from fmap2 itself (f2: this image's (C, H, W) fp32) instead of from
// opA.  Items (target row y, channel octet cg, column quad xq) = 16 x 32 x 4, four per thread, xq and the low
// four bits of cg over a wave's lanes: a load instruction reads the 64-B row pieces of 16 channels (the other
// half of each 128-B line is the neighbouring column block's, whose workgroup xcd_block puts on the same XCD),
// and an item's four 16-B LDS writes fall into all sixteen 16-B slots ((row + cg) mod 16 over a lane group).
// Values as prep_pair + the bf16 staging give them: bf16(x * scale), channels >= C bf16(0 * scale), targets
// off the map +0.
struct StageItem {
    int xq, cg, y;    // column quad, channel octet, (virtual) block row
    int ty, tx;       // the quad's first target pixel
};

__device__ __forceinline__ StageItem stage_item(int id, int ty0, int tx0, bool paired) {
    StageItem t;
    t.xq = id & 3, t.cg = (id >> 2) & 31, t.y = id >> 7;
    // virtual row y >= 8 of a paired block = row y - 8 of the next column block
    const bool second = paired && t.y >= 8;
    t.ty = ty0 + t.y - (second ? 8 : 0), t.tx = tx0 + 4 * t.xq + (second ? 16 : 0);
    return t;
}

// pixel i of the item's quad: its 8 channels -> one 16-B channel octet of the LDS image
__device__ __forceinline__ void stage_write_px(unsigned char* smem, const StageItem& t, int i, const float (&p)[8], int C,
                                               int H, int W, float scale) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)(t.ty < H && t.tx + i < W ? (t.cg * 8 + e < C ? p[e] : 0.0f) * scale : 0.0f);
    *reinterpret_cast<bf16x8*>(smem + (size_t)pad_row(t.y, 4 * t.xq + i) * kPadRow + t.cg * 16) = o;
}

__device__ __forceinline__ void stage_a_f32(unsigned char* smem, const float* __restrict__ f2, int C, int H, int W,
                                            float scale, int ty0, int tx0, bool paired, int tid) {
    constexpr int kItems = 4;
    const int N = H * W;
    // a quad starts at a multiple of 4 columns, so float4 loads need W % 4 == 0 (then N % 4 == 0) and an aligned base;
    // N < 2^22 keeps a 256-channel image's byte offsets in 32 bits
    if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(f2) & 15) == 0 && N < (1 << 22)) {
        // One item's 8 float4 in flight per thread (64 KiB per workgroup: the start-up is all workgroups reading
        // at once, bound by bandwidth and not by the depth of one thread's queue), in a rolled loop.  The
        // compiler schedules the tile loop's epilogue by the register pressure it has met in the function so
        // far: with two items in flight (86 VGPRs here against the bf16 staging's 70) that schedule changes, and
        // with four it interleaves the loads and the writes by itself.  No load is predicated: a quad off the
        // map or a channel >= C reads a clamped one that stage_write_px drops, so the loads are one straight
        // block of uniform base + 32-bit lane offset.
#pragma unroll 1
        for (int it = 0; it < kItems; ++it) {
            const StageItem t = stage_item(it * 512 + tid, ty0, tx0, paired);
            const unsigned pix = (unsigned)(min(t.ty, H - 1) * W + min(t.tx, W - 4));
            float4 x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned c = (unsigned)min(t.cg * 8 + e, C - 1);
                x[e] = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(f2) +
                                                        (size_t)((c * (unsigned)N + pix) * 4u));
            }
            stage_write_px(smem, t, 0, {x[0].x, x[1].x, x[2].x, x[3].x, x[4].x, x[5].x, x[6].x, x[7].x}, C, H, W, scale);
            stage_write_px(smem, t, 1, {x[0].y, x[1].y, x[2].y, x[3].y, x[4].y, x[5].y, x[6].y, x[7].y}, C, H, W, scale);
            stage_write_px(smem, t, 2, {x[0].z, x[1].z, x[2].z, x[3].z, x[4].z, x[5].z, x[6].z, x[7].z}, C, H, W, scale);
            stage_write_px(smem, t, 3, {x[0].w, x[1].w, x[2].w, x[3].w, x[4].w, x[5].w, x[6].w, x[7].w}, C, H, W, scale);
        }
        return;
    }
    // otherwise scalar loads, clamped as prep_pair clamps its partial quads, one pixel's 8 channels at a time
#pragma unroll 1
    for (int k = 0; k < 4 * kItems; ++k) {
        const StageItem t = stage_item((k >> 2) * 512 + tid, ty0, tx0, paired);
        const int i = k & 3;
        const float* px = f2 + (size_t)min(t.ty, H - 1) * W + min(t.tx + i, W - 1);
        float p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = px[(size_t)min(t.cg * 8 + e, C - 1) * N];
        stage_write_px(smem, t, i, p, C, H, W, scale);
    }
}

// Paired last block row (host: w8_balance): the last block row has at most 8 valid target rows and
// W % 32 == 0, so two horizontally adjacent last-row blocks share one workgroup: rows 0-7 of its virtual
// 16x16 block are block cb's rows, rows 8-15 block cb+1's (A staging and the stores' second-half delta
// Lvl::hd follow), and no workgroup spends half its MFMAs on rows past the map (cfg2: 55 = 3 x 16 + 7).
struct Bal {
    int pair;        // last block row paired
    int nwg;         // workgroups = the grid (blocks x batch x qsplit; a pair counts once)
};

// Ping-pong phases: the two waves of each SIMD (w and w + 4) alternate an MFMA phase and an epilogue
// phase, separated by workgroup barriers, so one wave's pooling VALU and stores run while its partner
// owns the matrix pipe (free-running partners drift into lock step: PMC of the free-running kernel
// showed VALU co-issued with MFMA in a third of its VALU cycles; 0.221 vs 0.242 ms,
// profiles/gemm_ab_r02_pp.json).
//
// A staging, two modes sharing everything else (kF32 is compile time: no branch reaches the tile loop):
//  * bf16 (corr_pyramid_w8, after prep_pair): the block's rows of opA = bf16(fmap2 * scale), copied;
//  * fp32 (corr_pyramid_w8_f32, after prep_queries): the LDS image built from fmap2 itself (stage_a_f32), bit
//    for bit the same image, so opA's 2 x 28.8 MB round trip (cfg2) and half of the prep pass go away.
template <bool kF32>
__device__ __forceinline__ void w8_body(const void* srcA, int C, float scale, const __bf16* opB, const PyrGeom& g,
                                        int qsplit, __half* pyr, const Bal& bal) {
    constexpr int Cp = 256, CPR = Cp / 8, WAVES = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int H = g.height, W = g.width, N = H * W;
    const int ncb = (W + 15) >> 4;
    const int nrb = (H + 15) >> 4;
    const int nqt = g.slots >> 5;                 // query tiles (tiles layout: slots % 32 == 0)
    // blocks per image: full blocks, then (pair) the last row's blocks two per workgroup
    const int nfull = bal.pair ? (nrb - 1) * ncb : nrb * ncb;
    const int nblk = nfull + (bal.pair ? ncb / 2 : 0);
    const int lid = xcd_block(blockIdx.x, bal.nwg);     // consecutive logical blocks (same batch) share an XCD's L2
    const int ib = lid % nblk;
    const int rest = lid / nblk;
    const int split = rest % qsplit;
    const int b = rest / qsplit;
    const bool paired = ib >= nfull;
    const int tb = paired ? (nrb - 1) * ncb + 2 * (ib - nfull) : ib;
    const int rb = tb / ncb, cb = tb - rb * ncb;
    const int ty0 = rb * 16, tx0 = cb * 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;

    if constexpr (kF32) {
        stage_a_f32(smem, static_cast<const float*>(srcA) + (size_t)b * C * N, C, H, W, scale, ty0, tx0, paired, tid);
    } else {
        const __bf16* gA = static_cast<const __bf16*>(srcA) + (size_t)b * N * Cp;
        // 16 pieces per thread, all loads in flight before the first LDS store (a load-store loop pays one
        // HBM round trip per piece before the first MFMA)
        constexpr int kPieces = 256 * CPR / (64 * WAVES);
        uint4 av[kPieces];
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int id = tid + i * 64 * WAVES;
            const int row = id / CPR, c = id - row * CPR;
            // virtual row y >= 8 of a paired block = row y - 8 of the next column block
            const bool second = paired && (row >> 4) >= 8;
            const int ty = ty0 + (row >> 4) - (second ? 8 : 0), tx = tx0 + (row & 15) + (second ? 16 : 0);
            av[i] = make_uint4(0, 0, 0, 0);
            if (ty < H && tx < W) av[i] = *reinterpret_cast<const uint4*>(gA + (size_t)(ty * W + tx) * Cp + c * 8);
        }
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const int id = tid + i * 64 * WAVES;
            const int row = id / CPR, c = id - row * CPR;
            *reinterpret_cast<uint4*>(smem + (size_t)pad_row(row >> 4, row & 15) * kPadRow + c * 16) = av[i];
        }
    }
    __syncthreads();

    const unsigned pb0 = (unsigned)j * kPadRow + 16u * h, pb1 = pb0 + 128u * kPadRow;

    // store context per level: chunk rows cr0 .. of this block (th = 2, 2, 1, 1 target rows each),
    // chunks cc0 .. (tw = 4, 4, 4, 2 columns)
    Ctx c;
    const unsigned S = (unsigned)g.slots;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int crows = l <= 1 ? 8 >> l : 4 >> (l - 2);       // chunk rows per 16-row block: 8, 4, 4, 2
        const int cpb = l == 0 ? 4 : (l == 1 ? 2 : 1);          // chunks per 16-column block
        const int cbytes = l <= 1 ? 16 : (l == 2 ? 8 : 4);      // chunk bytes
        const int cr0 = rb * crows, cc0 = cb * cpb;
        const bool lv = l < g.levels;
        const int rows = lv ? max(0, min(crows, g.ty[l] - cr0)) : 0;
        const unsigned cs = S * (unsigned)cbytes;
        const unsigned rs = lv ? (unsigned)g.tx[l] * cs : 0u;
        const size_t base = lv ? ((size_t)g.off[l] * 2 + (((size_t)b * g.ty[l] + cr0) * g.tx[l] + cc0) * (size_t)cs) : 0;
        const unsigned char* bp = reinterpret_cast<const unsigned char*>(pyr) + base;
        const unsigned lo32 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)bp);
        const unsigned hi32 = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)bp >> 32));
        c.l[l].rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uintptr_t)hi32 << 32) | lo32), (short)0,
                                                        (int)__builtin_amdgcn_readfirstlane((unsigned)rows * rs), 0x00020000);
        c.l[l].rs = __builtin_amdgcn_readfirstlane(rs);
        c.l[l].cs = __builtin_amdgcn_readfirstlane(cs);
        c.l[l].nq = __builtin_amdgcn_readfirstlane(lv ? max(0, min(cpb, g.tx[l] - cc0)) : 0);
        c.l[l].hd = paired ? __builtin_amdgcn_readfirstlane((unsigned)cpb * cs - (unsigned)(crows / 2) * rs) : 0u;
    }

    // B operand in fragment order (prep_pair): tile qt, k-step s = 1 KiB at ((b nqt + qt) 16 + s) KiB
    const __bf16* gB = opB + ((size_t)b * nqt * 1024 + lane) * 8;
    const int stride = WAVES * qsplit;
    // this workgroup's query tiles: every stride-th from f0 + w; waves 4-7 start one phase late; every wave
    // runs 2 * nmax + 1 barriers
    const int f0 = split * WAVES;
    int qt = f0 + w;
    const int nmax = f0 < nqt ? (nqt - f0 + stride - 1) / stride : 0;
    const int nw = qt < nqt ? (nqt - qt + stride - 1) / stride : 0;
    const bool late = w >= 4;
    unsigned b0 = pb0, b1 = pb1;
    asm volatile("" : "+v"(b0), "+v"(b1));
    bf16x8 ring[kRing];
    if (nw > 0) {
#pragma unroll
        for (int s = 0; s < kRing - 1; ++s) ring[s] = *reinterpret_cast<const bf16x8*>(gB + (size_t)qt * 8192 + 512 * s);
    }
    vmcnt_pad_n<kEpiStores>(pyr);
    if (late) __builtin_amdgcn_s_barrier();
    for (int k = 0; k < nmax; ++k) {
        f32x16 acc[8];
        const int qn = qt + stride;
        if (k < nw) {
            // both phases in one wave-uniform branch: every path that loads ring fragments issues
            // the epilogue stores after them (vmcnt_pad_n, rmd_common.h)
            bf16x8 a0[8], a1[8];
            read_a8<0>(a0, smem, b0, b1);
            ksteps_ring<0>(acc, a0, a1, ring, smem, b0, b1, gB + (size_t)qt * 8192,
                           gB + (size_t)min(qn, nqt - 1) * 8192);
            __builtin_amdgcn_s_barrier();
            const LaneOff lo = lane_offsets(c, qt * 32 + j, h);
            EpiState st;
            epilogue<0>(acc, c, lo, st);
            __builtin_amdgcn_s_barrier();
            qt = qn;
            continue;
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_barrier();
        qt = qn;
    }
    if (!late) __builtin_amdgcn_s_barrier();
}

__global__ void __launch_bounds__(512, 1)
corr_pyramid_w8(const __bf16* __restrict__ opA, const __bf16* __restrict__ opB, PyrGeom g, int qsplit,
                __half* __restrict__ pyr, Bal bal) {
    w8_body<false>(opA, 0, 0.0f, opB, g, qsplit, pyr, bal);
}

__global__ void __launch_bounds__(512, 1)
corr_pyramid_w8_f32(const float* __restrict__ f2, const __bf16* __restrict__ opB, PyrGeom g, int qsplit,
                    __half* __restrict__ pyr, Bal bal, int C, float scale) {
    w8_body<true>(f2, C, scale, opB, g, qsplit, pyr, bal);
}

// query slots of the tiles layout for an H x W map (rmd.h)
long long tiles_slots(int H, int W) {
    return (long long)(H / 2) * ((W + 15) / 16) * 32 + ((H & 1) ? (long long)(W + 31) / 32 * 32 : 0);
}

// The schedule of a launch (Bal): the last block row is paired when it holds at most 8 target rows and the
// query tiles are not split (qs == 1).  Measured at cfg2 (profiles/gemm_ab_r02_bal.json): 0.2280 (off) /
// 0.2257 (pairing) / 0.2271 ms (pairing + one helper workgroup per block running its tail query tiles on the
// CUs left free), all bitwise identical — evening out the per-CU work does not move the kernel: it is bound
// by the chip-wide pyramid write stream, not by any CU's share.  Pairing stays (the same time for 12.5 %
// fewer MFMAs, 224 instead of 256 workgroups); the helper schedule is in git history.
Bal w8_balance(const rmd_pyramid_desc& d, int qs) {
    const int nrb = (d.height + 15) / 16, ncb = (d.width + 15) / 16;
    const int rows_last = d.height - 16 * (nrb - 1);
    if (qs == 1 && nrb >= 2 && rows_last <= 8 && d.width % 32 == 0) return {1, ((nrb - 1) * ncb + ncb / 2) * d.batch};
    return {0, nrb * ncb * d.batch * qs};
}

}  // namespace

namespace w8 {

bool eligible(const rmd_pyramid_desc& d, int channels) {
    if (d.storage != RMD_F16 || padded_channels(channels) != 256) return false;
    // 32-bit store offsets: one 16-row band of level 0 (bytes) stays below 1 GiB
    const double slots = (double)tiles_slots(d.height, d.width);
    const double span0 = 16.0 * ((d.width + 7) / 8 * 8) * slots * 2;
    return span0 < (double)(1u << 30);
}

// operands in the workspace: A = fmap2 (B, N, 256) raster, then B = fmap1 in fragment order over the query slots
int prepare(const float* fmap1, const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d,
            void* workspace, hipStream_t st) {
    const int N = d.height * d.width;
    __bf16* opA = reinterpret_cast<__bf16*>(workspace);
    __bf16* opB = opA + (size_t)d.batch * N * 256;
    const int S = d.query_slots;
    const int nqt = S / 32;
    const int lds = kPrepPx * kPrepStride;
    const int nx = ((N > S ? N : S) + kPrepPx - 1) / kPrepPx;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prep_pair), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    // the scale (1/sqrt(C) for raft.CorrBlock) is folded into fmap2 before rounding (exact for a power of two)
    prep_pair<<<dim3(nx, d.batch, 2), 512, lds, st>>>(fmap1, fmap2, opA, opB, channels, d.height, d.width, S, nqt, scale);
    return check_launch("rmd_corr_prepare");
}

// the B operand alone, at the offset prepare() puts it: what pyramid_staged() reads from the workspace
int prepare_queries(const float* fmap1, int channels, const rmd_pyramid_desc& d, void* workspace, hipStream_t st) {
    const int N = d.height * d.width;
    __bf16* opB = reinterpret_cast<__bf16*>(workspace) + (size_t)d.batch * N * 256;
    const int S = d.query_slots;
    const int lds = kPrepPx * kPrepStride;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prep_queries), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    prep_queries<<<dim3((S + kPrepPx - 1) / kPrepPx, d.batch), 512, lds, st>>>(fmap1, opB, channels, d.height, d.width, S,
                                                                                S / 32);
    return check_launch("rmd_corr_prepare_queries");
}

namespace {

// fmap2 == nullptr: A from the workspace (prepare()); otherwise staged from fmap2 (prepare_queries())
int launch_gemm(const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d, void* pyramid, void* workspace,
                hipStream_t st) {
    const int N = d.height * d.width;
    __bf16* opA = reinterpret_cast<__bf16*>(workspace);
    __bf16* opB = opA + (size_t)d.batch * N * 256;
    const int nblk = ((d.height + 15) / 16) * ((d.width + 15) / 16);
    // query tiles split over workgroups only when the blocks alone do not fill the chip's 256 CUs
    const int nqt = d.query_slots / 32;
    int qs = 1;
    while (nblk * d.batch * qs < 256 && qs * 32 <= nqt) qs *= 2;
    const int lds = 256 * (int)kPadRow;
    const Bal bal = w8_balance(d, qs);
    if (fmap2) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(corr_pyramid_w8_f32),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        corr_pyramid_w8_f32<<<bal.nwg, 512, lds, st>>>(fmap2, opB, make_geom(d), qs, reinterpret_cast<__half*>(pyramid), bal,
                                                       channels, scale);
        return check_launch("rmd_corr_pyramid/gemm-w8-f32");
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(corr_pyramid_w8), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    corr_pyramid_w8<<<bal.nwg, 512, lds, st>>>(opA, opB, make_geom(d), qs, reinterpret_cast<__half*>(pyramid), bal);
    return check_launch("rmd_corr_pyramid/gemm-w8");
}

}  // namespace

int pyramid(const rmd_pyramid_desc& d, void* pyramid, void* workspace, hipStream_t st) {
    return launch_gemm(nullptr, 0, 0.0f, d, pyramid, workspace, st);
}

int pyramid_staged(const float* fmap2, int channels, float scale, const rmd_pyramid_desc& d, void* pyramid,
                   void* workspace, hipStream_t st) {
    return launch_gemm(fmap2, channels, scale, d, pyramid, workspace, st);
}

}  // namespace w8
}  // namespace rmd
