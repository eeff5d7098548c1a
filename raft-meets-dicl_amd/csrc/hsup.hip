// hsup.hip — local cross-attention of the hidden-state upsampler HUpCrossAttn
// (qzed/raft-meets-dicl src/models/common/hsup.py:71-92).
//
// Every fine pixel (y, x) of q (B, ck, h, w) attends over the wy x wx coarse cells around its parent
// cell (y / fy, x / fx) of k (B, ck, h2, w2) and v (B, cv, h2, w2):
//   s_j = sum_c q[c] k[c, cell_j],  a = softmax(s),  out[c] = sum_j a_j v[c, cell_j]
// with cells outside the map read as zero keys / values that take part in the softmax (the zero
// padding of F.unfold, hsup.py:71, :76).  The reference expands K and V to (B, c, wy*wx, h, w) first;
// here a block stages the coarse K / V tile of its pixels with the zero halo in LDS, a channel chunk
// at a time, and reads q once and writes out once: one launch, q + out + (tile halo overhead) K, V
// bytes.
//
// Layout of a block: 256 threads = 4 waves.  A lane owns one fine column x (consecutive lanes on
// consecutive x: q loads and out stores are coalesced 256-B rows); a wave owns one fine row, or, where
// the factors are compile-time constants (the 3x3 window at factor 2x2 of the models), the FY fine
// rows of one coarse row, so that one LDS read of a key / value serves FY pixels.  The LDS reads of a
// wave touch one tile row at consecutive or equal cells: conflict-free (equal addresses broadcast).
//
// Backward: a pixel pass recomputes the softmax, writes a and ds = a (da - sum a da) to the caller's
// workspace (B, 2 wy wx, h, w) and d q; a gather pass per coarse cell then adds, in a fixed order, the
// wy*wx neighbour cells x fy*fx fine pixels that read the cell.  No atomics: bitwise repeatable.
// A weight is always multiplied with its value (0 * inf = NaN as in the reference).  All arithmetic is
// float32, all global offsets 64-bit.

#include <cmath>

#include "rmd_common.h"

namespace rmd {
namespace {

constexpr int kAttnThreads = 256;
constexpr int kAttnRows = kAttnThreads / 64;    // waves of a block = coarse (fast) or fine (generic) rows of its tile
constexpr int kAttnCols = 64;                   // fine columns of a block's tile: one per lane
constexpr int kAttnMaxFactor = 64;
constexpr int kGatherChannels = 8;              // channels a gather thread accumulates

struct AttnGeom {
    int ck, cv, h, w, h2, w2, fy, fx;
};

// FY = FX = 0: run-time factors, one pixel per lane.  Otherwise a lane owns the FY fine rows of its coarse row.
template <int WY, int WX, int FY, int FX>
struct AttnTile {
    static constexpr int W = WY * WX;
    static constexpr int PY = FY > 0 ? FY : 1;
    static constexpr int TH = kAttnRows + WY - 1;                                  // tile rows incl. halo
    static constexpr int TW = (FX > 0 ? kAttnCols / FX : kAttnCols) + WX - 1;      // tile columns incl. halo
    static constexpr int kPlane = TH * TW;
    static constexpr int kChunk = kPlane > 256 ? 8 : 16;                           // channels staged in LDS at a time
    static constexpr int kStage = (kChunk * kPlane + kAttnThreads - 1) / kAttnThreads;     // staged values per thread
};

// the thread's pixels and its place in the block's coarse tile; coordinates of lanes outside the
// map are clamped into it (they compute a copy of a border pixel and store nothing)
template <int WY, int WX, int FY, int FX>
struct AttnThread {
    using T = AttnTile<WY, WX, FY, FX>;
    int b, x, y[T::PY];
    int cy0, cx0;       // map coordinates of the tile's first (halo) cell
    int ry, rx;         // tile coordinates of the window's first cell
    bool valid;

    __device__ __forceinline__ AttnThread(const AttnGeom& g) {
        const int fy = FY > 0 ? FY : g.fy, fx = FX > 0 ? FX : g.fx;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        b = blockIdx.z;
        const int x0 = blockIdx.x * kAttnCols, y0 = blockIdx.y * kAttnRows * T::PY;
        const int xr = x0 + lane, yr = y0 + wv * T::PY;
        valid = xr < g.w && yr < g.h;           // h is a multiple of fy: the PY rows of a coarse row are in or out together
        x = min(xr, g.w - 1);
#pragma unroll
        for (int p = 0; p < T::PY; ++p) y[p] = min(yr + p, g.h - 1);
        const int ty0 = min(y0, g.h - 1) / fy, tx0 = x0 / fx;      // first parent cell of the tile (x0 < w, y0 < h by the grid)
        cy0 = ty0 - WY / 2;
        cx0 = tx0 - WX / 2;
        ry = y[0] / fy - ty0;
        rx = x / fx - tx0;
    }
};

// Staging is a two-stage pipeline: the values of chunk i + 1 travel from global memory to registers
// (attn_stage_load) while chunk i is consumed from LDS, and go to the other LDS buffer afterwards
// (attn_stage_store): one barrier per chunk, and the load latency hides behind the arithmetic.
template <class T>
__device__ __forceinline__ void attn_stage_load(float (&r)[T::kStage], const float* __restrict__ src, int b, int C,
                                                int c0, int cy0, int cx0, const AttnGeom& g) {
#pragma unroll
    for (int n = 0; n < T::kStage; ++n) {
        const int i = threadIdx.x + n * kAttnThreads;
        const int c = i / T::kPlane, rem = i - c * T::kPlane;
        const int ty = rem / T::TW, tx = rem - ty * T::TW;
        const int gy = cy0 + ty, gx = cx0 + tx, gc = c0 + c;
        float val = 0.0f;       // outside the map, past the last channel
        if (i < T::kChunk * T::kPlane && gc < C && gy >= 0 && gy < g.h2 && gx >= 0 && gx < g.w2)
            val = src[(((size_t)b * C + gc) * g.h2 + gy) * g.w2 + gx];
        r[n] = val;
    }
}

template <class T>
__device__ __forceinline__ void attn_stage_store(float* __restrict__ lds, const float (&r)[T::kStage]) {
#pragma unroll
    for (int n = 0; n < T::kStage; ++n) {
        const int i = threadIdx.x + n * kAttnThreads;
        if (i < T::kChunk * T::kPlane) lds[i] = r[n];
    }
}

// Run body(tile, c0) over the channel chunks of src (B, C, h2, w2), `tile` the LDS image of channels
// [c0, c0 + kChunk) of the block's coarse tile.  next(c0) is called before the body of the chunk in
// front of c0 (the caller's own prefetch), take() at the start of a chunk (to accept what next fetched).
// Every thread of the block must call this; on return all reads of both buffers are done.
template <class T, class Thread, class Next, class Take, class Body>
__device__ __forceinline__ void attn_chunks(float* __restrict__ lds, const float* __restrict__ src, int C,
                                            const Thread& t, const AttnGeom& g, Next&& next, Take&& take,
                                            Body&& body) {
    float r[T::kStage];
    const int n = (C + T::kChunk - 1) / T::kChunk;
    attn_stage_load<T>(r, src, t.b, C, 0, t.cy0, t.cx0, g);
    next(0);
    attn_stage_store<T>(lds, r);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        take();
        if (i + 1 < n) {
            attn_stage_load<T>(r, src, t.b, C, (i + 1) * T::kChunk, t.cy0, t.cx0, g);
            next((i + 1) * T::kChunk);
        }
        body(lds + (i & 1) * T::kChunk * T::kPlane, i * T::kChunk);
        if (i + 1 < n) attn_stage_store<T>(lds + ((i + 1) & 1) * T::kChunk * T::kPlane, r);
        __syncthreads();
    }
}

// channels [c0, c0 + kChunk) of src (B, C, h, w) at the thread's pixels; 0 past the last channel
template <class T, class Thread>
__device__ __forceinline__ void attn_fetch(float (&r)[T::kChunk][T::PY], const float* __restrict__ src, int C, int c0,
                                           const Thread& t, const AttnGeom& g) {
#pragma unroll
    for (int c = 0; c < T::kChunk; ++c)
#pragma unroll
        for (int p = 0; p < T::PY; ++p)
            r[c][p] = c0 + c < C ? src[(((size_t)t.b * C + c0 + c) * g.h + t.y[p]) * g.w + t.x] : 0.0f;
}

// acc[p][j] += sum over the chunk's channels of f[c][p] * tile[c, cell_j].  Channels past the last one
// are zero on both sides.
template <class T, int WY, int WX, class Thread>
__device__ __forceinline__ void attn_window_fma(float (&acc)[T::PY][WY * WX], const float (&f)[T::kChunk][T::PY],
                                                const float* __restrict__ tile, const Thread& t) {
#pragma unroll
    for (int c = 0; c < T::kChunk; ++c) {
        const float* tc = tile + c * T::kPlane + t.ry * T::TW + t.rx;
#pragma unroll
        for (int jy = 0; jy < WY; ++jy)
#pragma unroll
            for (int jx = 0; jx < WX; ++jx) {
                const float tv = tc[jy * T::TW + jx];
#pragma unroll
                for (int p = 0; p < T::PY; ++p) acc[p][jy * WX + jx] = fmaf(f[c][p], tv, acc[p][jy * WX + jx]);
            }
    }
}

// dst[c, pixel] = sum_j wgt[p][j] * tile[c, cell_j] for the chunk's channels below C
template <class T, int WY, int WX, class Thread>
__device__ __forceinline__ void attn_window_dot(float* __restrict__ dst, int C, int c0,
                                                const float (&wgt)[T::PY][WY * WX], const float* __restrict__ tile,
                                                const Thread& t, const AttnGeom& g) {
#pragma unroll
    for (int c = 0; c < T::kChunk; ++c) {
        const float* tc = tile + c * T::kPlane + t.ry * T::TW + t.rx;
        float acc[T::PY];
#pragma unroll
        for (int p = 0; p < T::PY; ++p) acc[p] = 0.0f;
#pragma unroll
        for (int jy = 0; jy < WY; ++jy)
#pragma unroll
            for (int jx = 0; jx < WX; ++jx) {
                const float tv = tc[jy * T::TW + jx];
#pragma unroll
                for (int p = 0; p < T::PY; ++p) acc[p] = fmaf(wgt[p][jy * WX + jx], tv, acc[p]);
            }
        if (t.valid && c0 + c < C) {
#pragma unroll
            for (int p = 0; p < T::PY; ++p) dst[(((size_t)t.b * C + c0 + c) * g.h + t.y[p]) * g.w + t.x] = acc[p];
        }
    }
}

// acc[p][j] = sum_c f[c] tile_src[c, cell_j] over all C channels: the logits (f = q, src = k) and da (f = grad, src = v)
template <int WY, int WX, int FY, int FX>
__device__ __forceinline__ void attn_window_sums(float* __restrict__ lds, const float* __restrict__ f,
                                                 const float* __restrict__ src, int C, const AttnGeom& g,
                                                 const AttnThread<WY, WX, FY, FX>& t,
                                                 float (&acc)[AttnTile<WY, WX, FY, FX>::PY][WY * WX]) {
    using T = AttnTile<WY, WX, FY, FX>;
#pragma unroll
    for (int p = 0; p < T::PY; ++p)
#pragma unroll
        for (int j = 0; j < T::W; ++j) acc[p][j] = 0.0f;
    float cur[T::kChunk][T::PY], nxt[T::kChunk][T::PY];
    attn_chunks<T>(
        lds, src, C, t, g, [&](int c0) { attn_fetch<T>(nxt, f, C, c0, t, g); },
        [&]() {
#pragma unroll
            for (int c = 0; c < T::kChunk; ++c)
#pragma unroll
                for (int p = 0; p < T::PY; ++p) cur[c][p] = nxt[c][p];
        },
        [&](const float* tile, int) { attn_window_fma<T, WY, WX>(acc, cur, tile, t); });
}

// s -> softmax(s) in place, the maximum subtracted.  A NaN or +inf logit makes the whole pixel NaN, as torch's softmax.
template <int W>
__device__ __forceinline__ void attn_softmax(float (&s)[W]) {
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < W; ++j) mx = s[j] > mx ? s[j] : mx;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        s[j] = expf(s[j] - mx);
        sum += s[j];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int j = 0; j < W; ++j) s[j] *= inv;
}

template <int WY, int WX, int FY, int FX>
__global__ void __launch_bounds__(kAttnThreads) local_cross_attn_kernel(const float* __restrict__ q,
                                                                        const float* __restrict__ k,
                                                                        const float* __restrict__ v, AttnGeom g,
                                                                        float* __restrict__ out) {
    using T = AttnTile<WY, WX, FY, FX>;
    __shared__ float lds[2 * T::kChunk * T::kPlane];
    const AttnThread<WY, WX, FY, FX> t(g);
    float a[T::PY][T::W];
    attn_window_sums<WY, WX, FY, FX>(lds, q, k, g.ck, g, t, a);
#pragma unroll
    for (int p = 0; p < T::PY; ++p) attn_softmax<T::W>(a[p]);
    attn_chunks<T>(
        lds, v, g.cv, t, g, [](int) {}, []() {},
        [&](const float* tile, int c0) { attn_window_dot<T, WY, WX>(out, g.cv, c0, a, tile, t, g); });
}

// Backward, pixel pass: a and ds to the workspace planes [0, W) and [W, 2 W) of (B, 2 W, h, w), and d q.
template <int WY, int WX, int FY, int FX>
__global__ void __launch_bounds__(kAttnThreads) local_cross_attn_backward_pixel_kernel(
    const float* __restrict__ grad, const float* __restrict__ q, const float* __restrict__ k,
    const float* __restrict__ v, AttnGeom g, float* __restrict__ ws, float* __restrict__ grad_q) {
    using T = AttnTile<WY, WX, FY, FX>;
    __shared__ float lds[2 * T::kChunk * T::kPlane];
    const AttnThread<WY, WX, FY, FX> t(g);
    float a[T::PY][T::W], da[T::PY][T::W];
    attn_window_sums<WY, WX, FY, FX>(lds, q, k, g.ck, g, t, a);
#pragma unroll
    for (int p = 0; p < T::PY; ++p) attn_softmax<T::W>(a[p]);
    attn_window_sums<WY, WX, FY, FX>(lds, grad, v, g.cv, g, t, da);          // da_j = sum_c g[c] v[c, cell_j]
    // ds_j = a_j (da_j - sum_i a_i da_i), kept in da
#pragma unroll
    for (int p = 0; p < T::PY; ++p) {
        float dot = 0.0f;
#pragma unroll
        for (int j = 0; j < T::W; ++j) dot = fmaf(a[p][j], da[p][j], dot);
#pragma unroll
        for (int j = 0; j < T::W; ++j) da[p][j] = a[p][j] * (da[p][j] - dot);
        if (t.valid) {
            const size_t plane = (size_t)g.h * g.w;
            float* o = ws + (size_t)t.b * 2 * T::W * plane + (size_t)t.y[p] * g.w + t.x;
#pragma unroll
            for (int j = 0; j < T::W; ++j) {
                o[(size_t)j * plane] = a[p][j];
                o[(size_t)(T::W + j) * plane] = da[p][j];
            }
        }
    }
    // d q[c] = sum_j ds_j k[c, cell_j]
    attn_chunks<T>(
        lds, k, g.ck, t, g, [](int) {}, []() {},
        [&](const float* tile, int c0) { attn_window_dot<T, WY, WX>(grad_q, g.ck, c0, da, tile, t, g); });
}

// Backward, gather pass.  A thread owns one coarse cell and kGatherChannels channels of d k (weights ds,
// features q) or of d v (weights a, features grad): blockIdx.z = (image, channel group), the groups of
// d k first.  The cell (Y, X) is window entry (jy, jx) of the parent cell (Y - jy + wy/2, X - jx + wx/2);
// the terms are added in the order jy, jx, fine row, fine column.  WY = 0: run-time sizes.
template <int WY, int WX, int FY, int FX>
__global__ void __launch_bounds__(kAttnThreads) local_cross_attn_backward_gather_kernel(
    const float* __restrict__ grad, const float* __restrict__ q, const float* __restrict__ ws, AttnGeom g, int wy_,
    int wx_, float* __restrict__ grad_k, float* __restrict__ grad_v) {
    const int wy = WY > 0 ? WY : wy_, wx = WX > 0 ? WX : wx_;
    const int fy = FY > 0 ? FY : g.fy, fx = FX > 0 ? FX : g.fx;
    const int kgroups = (g.ck + kGatherChannels - 1) / kGatherChannels;
    const int vgroups = (g.cv + kGatherChannels - 1) / kGatherChannels;
    const int b = blockIdx.z / (kgroups + vgroups);
    int grp = blockIdx.z - b * (kgroups + vgroups);
    const bool is_v = grp >= kgroups;           // block-uniform
    grp -= is_v ? kgroups : 0;
    const int C = is_v ? g.cv : g.ck, c0 = grp * kGatherChannels, nc = min(kGatherChannels, C - c0);
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * kAttnRows + (threadIdx.x >> 6);
    if (X >= g.w2 || Y >= g.h2) return;
    const size_t plane = (size_t)g.h * g.w;
    const float* wgt = ws + ((size_t)b * 2 + (is_v ? 0 : 1)) * wy * wx * plane;
    const float* feat = (is_v ? grad : q) + ((size_t)b * C + c0) * plane;
    float acc[kGatherChannels];
#pragma unroll
    for (int i = 0; i < kGatherChannels; ++i) acc[i] = 0.0f;
    constexpr int kUnrollY = WY > 0 ? WY : 1, kUnrollX = WX > 0 ? WX : 1, kUnrollF = FY > 0 ? FY : 1;   // 1: run-time trip counts
    // Branch-free, so that the loads of all terms can be in flight together: a parent cell outside the
    // map has no term; its (clamped, in-range) loads are discarded by a select, never multiplied.
#pragma unroll kUnrollY
    for (int jy = 0; jy < wy; ++jy) {
        const int yp = Y - jy + wy / 2, ypc = min(max(yp, 0), g.h2 - 1);
#pragma unroll kUnrollX
        for (int jx = 0; jx < wx; ++jx) {
            const int xp = X - jx + wx / 2, xpc = min(max(xp, 0), g.w2 - 1);
            const bool ok = yp == ypc && xp == xpc;
            const float* wj = wgt + (size_t)(jy * wx + jx) * plane;
#pragma unroll kUnrollF
            for (int py = 0; py < fy; ++py) {
                const size_t row = (size_t)(ypc * fy + py) * g.w + (size_t)xpc * fx;
                if constexpr (FX == 2) {        // both fine pixels of the row in one 8-byte load (w = 2 w2: even offsets)
                    const float2 wv = *reinterpret_cast<const float2*>(wj + row);
#pragma unroll
                    for (int i = 0; i < kGatherChannels; ++i) {
                        const float2 f = *reinterpret_cast<const float2*>(feat + (size_t)min(i, nc - 1) * plane + row);
                        acc[i] = ok ? fmaf(wv.y, f.y, fmaf(wv.x, f.x, acc[i])) : acc[i];
                    }
                } else {
                    for (int px = 0; px < fx; ++px) {
                        const float wv = wj[row + px];
#pragma unroll
                        for (int i = 0; i < kGatherChannels; ++i) {
                            const float f = feat[(size_t)min(i, nc - 1) * plane + row + px];
                            acc[i] = ok ? fmaf(wv, f, acc[i]) : acc[i];
                        }
                    }
                }
            }
        }
    }
    float* dst = (is_v ? grad_v : grad_k) + (((size_t)b * C + c0) * g.h2 + Y) * g.w2 + X;
#pragma unroll
    for (int i = 0; i < kGatherChannels; ++i)
        if (i < nc) dst[(size_t)i * g.h2 * g.w2] = acc[i];
}

inline int attn_check(const char* what, int batch, int ck, int cv, int h, int w, int h2, int w2, int wy, int wx,
                      AttnGeom& g) {
    RMD_REQUIRE(batch >= 1 && ck >= 1 && cv >= 1 && h >= 1 && w >= 1 && h2 >= 1 && w2 >= 1, RMD_ERR_SHAPE,
                "%s: bad sizes (batch=%d ck=%d cv=%d fine %dx%d coarse %dx%d)", what, batch, ck, cv, h, w, h2, w2);
    RMD_REQUIRE((wy == 1 || wy == 3 || wy == 5) && (wx == 1 || wx == 3 || wx == 5), RMD_ERR_SHAPE,
                "%s: window %dx%d: sizes must be 1, 3 or 5", what, wy, wx);
    RMD_REQUIRE(h % h2 == 0 && w % w2 == 0, RMD_ERR_SHAPE,
                "%s: fine size %dx%d is not an integer multiple of the coarse size %dx%d", what, h, w, h2, w2);
    RMD_REQUIRE(h / h2 <= kAttnMaxFactor && w / w2 <= kAttnMaxFactor, RMD_ERR_SHAPE,
                "%s: factors %dx%d above %d are not supported", what, h / h2, w / w2, kAttnMaxFactor);
    const long long groups = (ck + kGatherChannels - 1) / kGatherChannels + (cv + kGatherChannels - 1) / kGatherChannels;
    RMD_REQUIRE(batch * groups <= 65535 && (h + kAttnRows - 1) / kAttnRows <= 65535, RMD_ERR_SHAPE,
                "%s: batch=%d ck=%d cv=%d h=%d exceed the launch grid", what, batch, ck, cv, h);
    g = AttnGeom{ck, cv, h, w, h2, w2, h / h2, w / w2};
    return RMD_OK;
}

inline bool attn_fast(const AttnGeom& g, int wy, int wx) { return wy == 3 && wx == 3 && g.fy == 2 && g.fx == 2; }

template <int FY>
inline dim3 attn_grid(const AttnGeom& g, int batch) {
    const int rows = kAttnRows * (FY > 0 ? FY : 1);
    return dim3((unsigned)((g.w + kAttnCols - 1) / kAttnCols), (unsigned)((g.h + rows - 1) / rows), (unsigned)batch);
}

}  // namespace
}  // namespace rmd

using namespace rmd;

#define RMD_ATTN_WINDOWS(X) X(1, 1) X(1, 3) X(1, 5) X(3, 1) X(3, 3) X(3, 5) X(5, 1) X(5, 3) X(5, 5)

extern "C" const char* rmd_local_cross_attn_kernel(int batch, int ck, int cv, int h, int w, int h2, int w2, int wy,
                                                   int wx) {
    AttnGeom g;
    if (attn_check("rmd_local_cross_attn_kernel", batch, ck, cv, h, w, h2, w2, wy, wx, g)) return "invalid";
    clear_error();
    return attn_fast(g, wy, wx) ? "w3x3_f2x2" : "generic";
}

extern "C" size_t rmd_local_cross_attn_workspace_bytes(int batch, int h, int w, int wy, int wx) {
    if (batch < 1 || h < 1 || w < 1 || wy < 1 || wx < 1) return 0;
    return (size_t)batch * 2 * wy * wx * h * w * sizeof(float);
}

extern "C" int rmd_local_cross_attn(const float* q, const float* k, const float* v, int batch, int ck, int cv, int h,
                                    int w, int h2, int w2, int wy, int wx, float* out, void* stream) {
    RMD_REQUIRE(q && k && v && out, RMD_ERR_ARG, "rmd_local_cross_attn: null pointer");
    AttnGeom g;
    const int rc = attn_check("rmd_local_cross_attn", batch, ck, cv, h, w, h2, w2, wy, wx, g);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    if (attn_fast(g, wy, wx)) {
        local_cross_attn_kernel<3, 3, 2, 2><<<attn_grid<2>(g, batch), kAttnThreads, 0, st>>>(q, k, v, g, out);
    } else {
#define RMD_ATTN(WY, WX)                                                                                      \
    if (wy == WY && wx == WX)                                                                                 \
        local_cross_attn_kernel<WY, WX, 0, 0><<<attn_grid<0>(g, batch), kAttnThreads, 0, st>>>(q, k, v, g, out);
        RMD_ATTN_WINDOWS(RMD_ATTN)
#undef RMD_ATTN
    }
    return check_launch("rmd_local_cross_attn");
}

extern "C" int rmd_local_cross_attn_backward(const float* grad_out, const float* q, const float* k, const float* v,
                                             int batch, int ck, int cv, int h, int w, int h2, int w2, int wy, int wx,
                                             float* grad_q, float* grad_k, float* grad_v, void* workspace,
                                             void* stream) {
    RMD_REQUIRE(grad_out && q && k && v && grad_q && grad_k && grad_v && workspace, RMD_ERR_ARG,
                "rmd_local_cross_attn_backward: null pointer");
    AttnGeom g;
    const int rc = attn_check("rmd_local_cross_attn_backward", batch, ck, cv, h, w, h2, w2, wy, wx, g);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(workspace);
    const int groups = (ck + kGatherChannels - 1) / kGatherChannels + (cv + kGatherChannels - 1) / kGatherChannels;
    const dim3 ggrid((unsigned)((w2 + 63) / 64), (unsigned)((h2 + kAttnRows - 1) / kAttnRows), (unsigned)(batch * groups));
    if (attn_fast(g, wy, wx)) {
        local_cross_attn_backward_pixel_kernel<3, 3, 2, 2>
            <<<attn_grid<2>(g, batch), kAttnThreads, 0, st>>>(grad_out, q, k, v, g, ws, grad_q);
        local_cross_attn_backward_gather_kernel<3, 3, 2, 2>
            <<<ggrid, kAttnThreads, 0, st>>>(grad_out, q, ws, g, wy, wx, grad_k, grad_v);
    } else {
#define RMD_ATTN(WY, WX)                                                                      \
    if (wy == WY && wx == WX)                                                                 \
        local_cross_attn_backward_pixel_kernel<WY, WX, 0, 0>                                  \
            <<<attn_grid<0>(g, batch), kAttnThreads, 0, st>>>(grad_out, q, k, v, g, ws, grad_q);
        RMD_ATTN_WINDOWS(RMD_ATTN)
#undef RMD_ATTN
        local_cross_attn_backward_gather_kernel<0, 0, 0, 0>
            <<<ggrid, kAttnThreads, 0, st>>>(grad_out, q, ws, g, wy, wx, grad_k, grad_v);
    }
    return check_launch("rmd_local_cross_attn_backward");
}
