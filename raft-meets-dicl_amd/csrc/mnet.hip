// mnet.hip — the k x k DICL MatchingNet (inference) without MIOpen: its last two layers as one kernel, and the whole
// network as five launches per group of images over one workspace.
//
// Replaces (qzed/raft-meets-dicl v2) MatchingNet (src/models/common/blocks/dicl.py:93-118) for the norm types
// 'none' and — folded into the weights by the caller — eval-mode 'batch'.  Layers 1-4 (3 x 3 at stride 1, 2, 1, 1
// with ReLU) are encoder.hip's sconv_kernel, reached through encoder.h on weights packed once per call.
//
// The tail: layer 5, ConvTranspose2d(c3, c4, 4, stride 2, padding 1) + ReLU, and layer 6, Conv2d(c4, 1, 3,
// padding 1) with bias,
//   u[o, Y, X] = relu(t5[o] + sum_{c,ky,kx} W5'[c, o, ky, kx] x[c, iy, ix]),  Y = 2 iy - 1 + ky, X = 2 ix - 1 + kx
//   cost[Y, X] = b6 + sum_{o,i,j} w6[o, i, j] u[o, Y + i - 1, X + j - 1],      u zero outside the map
// Output parity class (py, px) = (Y & 1, X & 1) of layer 5 is a 2 x 2-tap convolution of x: class pixel (m, n) =
// u[., 2 m + py, 2 n + px] reads x at (m + py - a, n + px - b) through tap (ky, kx) = (1 - py + 2 a, 1 - px + 2 b),
// a, b in {0, 1}.  So layer 5 is four implicit GEMMs (M = c4: one 32-row MFMA tile, K = 4 c3, N = pixels) on
// v_mfma_f32_32x32x16_bf16 with the split-bf16 arithmetic of mfma_bf16.h, the weights packed into A fragments
// (fragment ((class 4 + tap) ks + k), rows and channels zero-padded: nothing need be a multiple of 16).
//
// Tile.  A workgroup (256 threads, one wave per parity class) owns 6 x 62 cost pixels of one image.  It stages the
// 5 x 33 positions of x its taps read (position-major, 16 ks + 8 bf16 per position: an odd number of 16-byte
// slots; hi part and — three-product mode — the part of the residual; positions outside the map zero), computes
// per class 4 x 32 pixels of u — the tile plus a one-pixel ring, 8 x 64 in all, recomputed by the neighbours, not
// exchanged — and, once every wave has read its last B fragment, writes relu(acc + t5) over the staged x as fp32
// u[o][8][64]; ring positions outside the map are written as zero, not relu(t5): they are layer 6's padding.
// Layer 6 runs in fp32 on the VALU from LDS (channel, tap row, tap column: one order), and the cost is stored once;
// the c4-channel map never reaches memory.
// LDS: max(parts 165 (16 ks + 8) 2, c4 8 64 4) bytes = 65,536 at c3 = 64, c4 = 32 in either mode (the u tile; the
// staged x takes 47,520 with three products): two workgroups per CU.  The compiler's register, scratch and LDS
// figures are recorded in profiles/mnet_r18.json.
//
// Every output's summation order is fixed and depends on nothing but its own image: results are bitwise
// repeatable, per-sample independent, and independent of how the composite launcher groups the images.

#include "encoder.h"
#include "mfma_bf16.h"

namespace rmd {
namespace {

constexpr int kThreads = 256;
constexpr int kRY = 3, kRX = 31;                    // x positions (= class pixels less the ring) a tile advances by
constexpr int kXR = kRY + 2, kXC = kRX + 2;         // staged x rows, columns
constexpr int kSlots = kXR * kXC;
constexpr int kCR = kRY + 1;                        // class rows of a tile; a class row is kRX + 1 = 32 pixels
constexpr int kUR = 2 * kRY + 2, kUC = 2 * kRX + 2; // the u tile: 8 x 64
constexpr int kOutR = 2 * kRY, kOutC = 2 * kRX;     // the cost tile: 6 x 62
constexpr int kMaxC3 = 64, kMaxC4 = 32;
constexpr int kAlign = 256;
constexpr int kLayers = 6;

struct TailGeom {
    int N, c3, c4, h2, w2;
    int ks;                 // 16-channel k-steps
    int tiles_x, tiles_y;
    int nfrag;              // A fragments of one part: 16 ks
};

inline bool tail_supported(int c3, int c4, long long h2, long long w2) {
    return c3 >= 1 && c3 <= kMaxC3 && c4 >= 1 && c4 <= kMaxC4 && h2 >= 1 && w2 >= 1 && h2 * w2 * c3 < (1ll << 30);
}

// W5' (c3, c4, 4, 4) -> fragment ((cl 4 + t) ks + k), lane l = (row o = l & 31, half l >> 5), element j:
// W5'[16 k + 8 (l >> 5) + j][o][1 - py + 2 a][1 - px + 2 b], cl = 2 py + px, t = 2 a + b; zero for o >= c4 or a
// channel >= c3; nfrag hi fragments, then (if `lo`) nfrag fragments of the bf16 of the residual
__global__ void __launch_bounds__(256)
mnet_tail_pack_kernel(const float* __restrict__ w5, int c3, int c4, int ks, int nfrag, int lo,
                      bf16x8* __restrict__ frags) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= nfrag * 64) return;
    const int lane = id & 63, f = id >> 6;
    const int k = f % ks, ct = f / ks, t = ct & 3, cl = ct >> 2;
    const int ky = 1 - (cl >> 1) + 2 * (t >> 1), kx = 1 - (cl & 1) + 2 * (t & 1);
    const int o = lane & 31, c = 16 * k + 8 * (lane >> 5);
    bf16x8 hi, lopart;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = (o < c4 && c + j < c3) ? w5[(((size_t)(c + j) * c4 + o) * 4 + ky) * 4 + kx] : 0.f;
        hi[j] = bf16_hi(v);
        lopart[j] = bf16_lo(v, hi[j]);
    }
    frags[id] = hi;
    if (lo) frags[id + (size_t)nfrag * 64] = lopart;
}

template <int NP>
__global__ void __launch_bounds__(kThreads, 2)
mnet_tail_kernel(const float* __restrict__ x, const bf16x8* __restrict__ frags, const float* __restrict__ t5,
                 const float* __restrict__ w6, const float* __restrict__ b6, float* __restrict__ cost, TailGeom P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __bf16* sm = reinterpret_cast<__bf16*>(smem);           // the staged x: PARTS * kSlots * stride
    float* us = reinterpret_cast<float*>(smem);             // then u[c4][kUR][kUC]
    const int stride = 16 * P.ks + 8;

    const int tid = threadIdx.x, lane = tid & 63;
    const int cl = __builtin_amdgcn_readfirstlane(tid >> 6);        // the wave's parity class
    const int py = cl >> 1, px = cl & 1;
    const int r = lane & 31, hh = lane >> 5;
    int blk = blockIdx.x;
    const int tx = blk % P.tiles_x; blk /= P.tiles_x;
    const int ty = blk % P.tiles_y;
    const int n = blk / P.tiles_y;
    const int y0 = ty * kRY, x0 = tx * kRX;                 // x position under the tile's first cost pixel
    const int HW = P.h2 * P.w2;
    const float* ib = x + (size_t)n * P.c3 * HW;            // 32-bit offsets inside an image
    const int lopart = kSlots * stride;

    for (int id = tid; id < 2 * P.ks * kSlots; id += kThreads) {
        const int grp = id / kSlots, s = id - grp * kSlots;
        const int sy = s / kXC, sx = s - sy * kXC;          // neighbouring lanes, neighbouring x
        const int yy = y0 - 1 + sy, xx = x0 - 1 + sx;
        const bool inside = yy >= 0 && yy < P.h2 && xx >= 0 && xx < P.w2;
        const int c = 8 * grp;
        const int at = inside ? yy * P.w2 + xx : 0;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (inside && c + j < P.c3) ? ib[(c + j) * HW + at] : 0.f;
        bf16x8 hi, lo;
        split<NP>(v, hi, lo);
        *reinterpret_cast<bf16x8*>(&sm[s * stride + 8 * grp]) = hi;
        if constexpr (NP == 3) *reinterpret_cast<bf16x8*>(&sm[lopart + s * stride + 8 * grp]) = lo;
    }
    __syncthreads();

    // layer 5: class pixel (m, r) of this wave's class reads staged position (m + 1 - a, r + 1 - b) through tap (a, b)
    f32x16 acc[kCR];
#pragma unroll
    for (int m = 0; m < kCR; ++m) acc[m] = f32x16{};
    for (int t = 0; t < 4; ++t) {
        const int a = t >> 1, b = t & 1;
        for (int k = 0; k < P.ks; ++k) {
            const size_t f = ((size_t)(cl * 4 + t) * P.ks + k) * 64 + lane;
            const bf16x8 ah = frags[f];
            const bf16x8 al = NP == 3 ? frags[f + (size_t)P.nfrag * 64] : bf16x8{};
#pragma unroll
            for (int m = 0; m < kCR; ++m) {
                const __bf16* p = &sm[((m + 1 - a) * kXC + r + 1 - b) * stride + 16 * k + 8 * hh];
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(p);
                const bf16x8 bl = NP == 3 ? *reinterpret_cast<const bf16x8*>(p + lopart) : bf16x8{};
                mma<NP>(acc[m], ah, al, bh, bl);
            }
        }
    }
    __syncthreads();                                        // every wave has read its last B fragment: x is dead

    // u: register i of lane (r, hh) is channel acc_row(i, hh) of class pixel (m, r) = u tile (2 m + 1 - py, 2 r + 1 - px),
    // which is map position (2 y0 - 1, 2 x0 - 1) + that
    const int Ho = 2 * P.h2, Wo = 2 * P.w2;
    const int ux = 2 * r + 1 - px, gx = 2 * x0 - 1 + ux;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int o = acc_row(i, hh);
        if (o >= P.c4) continue;
        const float bv = t5[o];
#pragma unroll
        for (int m = 0; m < kCR; ++m) {
            const int uy = 2 * m + 1 - py, gy = 2 * y0 - 1 + uy;
            float v = acc[m][i] + bv;
            v = v < 0.f ? 0.f : v;                          // keeps NaN, as torch.relu
            if (gy < 0 || gy >= Ho || gx < 0 || gx >= Wo) v = 0.f;  // layer 6's padding, not relu(t5)
            us[(o * kUR + uy) * kUC + ux] = v;
        }
    }
    __syncthreads();

    // layer 6, fp32: cost tile pixel (yo, xo) reads u tile (yo + i, xo + j)
    const float bias = b6[0];
    float* ob = cost + (size_t)n * Ho * Wo;
    for (int pix = tid; pix < kOutR * kOutC; pix += kThreads) {
        const int yo = pix / kOutC, xo = pix - yo * kOutC;
        const int gy = 2 * y0 + yo, gxo = 2 * x0 + xo;
        if (gy >= Ho || gxo >= Wo) continue;
        float s = 0.f;
        for (int o = 0; o < P.c4; ++o) {
            const float* up = &us[(o * kUR + yo) * kUC + xo];
            const float* wp = w6 + o * 9;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) s += wp[i * 3 + j] * up[i * kUC + j];
        }
        ob[(size_t)gy * Wo + gxo] = bias + s;
    }
}

// ---- host --------------------------------------------------------------------------------------------

TailGeom tail_geom(int n, int c3, int c4, int h2, int w2) {
    TailGeom P;
    P.N = n; P.c3 = c3; P.c4 = c4; P.h2 = h2; P.w2 = w2;
    P.ks = (c3 + 15) / 16;
    P.tiles_x = (w2 + kRX - 1) / kRX; P.tiles_y = (h2 + kRY - 1) / kRY;
    P.nfrag = 16 * P.ks;
    return P;
}

// bytes of the tail's packed fragments: both parts, a multiple of kAlign
size_t tail_frag_bytes(int c3) { return (size_t)16 * ((c3 + 15) / 16) * 64 * sizeof(bf16x8) * 2; }

size_t tail_lds_bytes(const TailGeom& P, int compute) {
    const size_t xb = (size_t)(compute == RMD_BF16X3 ? 2 : 1) * kSlots * (16 * P.ks + 8) * sizeof(__bf16);
    const size_t ub = (size_t)P.c4 * kUR * kUC * sizeof(float);
    return xb > ub ? xb : ub;                               // at most 65,536
}

void tail_pack(const float* w5, void* frags, int c3, int c4, int compute, hipStream_t st) {
    const TailGeom P = tail_geom(1, c3, c4, 1, 1);
    mnet_tail_pack_kernel<<<(P.nfrag * 64 + 255) / 256, 256, 0, st>>>(w5, c3, c4, P.ks, P.nfrag,
                                                                      compute == RMD_BF16X3 ? 1 : 0,
                                                                      reinterpret_cast<bf16x8*>(frags));
}

void tail_packed(const float* x, const void* frags, const float* t5, const float* w6, const float* b6, float* cost,
                 const TailGeom& P, int compute, hipStream_t st) {
    const int grid = P.N * P.tiles_y * P.tiles_x;
    const size_t lds = tail_lds_bytes(P, compute);
    const bf16x8* fr = reinterpret_cast<const bf16x8*>(frags);
    if (compute == RMD_BF16X3) mnet_tail_kernel<3><<<grid, kThreads, lds, st>>>(x, fr, t5, w6, b6, cost, P);
    else mnet_tail_kernel<1><<<grid, kThreads, lds, st>>>(x, fr, t5, w6, b6, cost, P);
}

int tail_check_shape(const char* name, int n, int c3, int c4, int h2, int w2) {
    RMD_REQUIRE(n > 0 && h2 > 0 && w2 > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(tail_supported(c3, c4, h2, w2), RMD_ERR_SHAPE,
                "%s: unsupported tail (channels %d -> %d on %d x %d): c3 in 1..64, c4 in 1..32, c3 h2 w2 < 2^30", name, c3,
                c4, h2, w2);
    const TailGeom P = tail_geom(n, c3, c4, h2, w2);
    RMD_REQUIRE((long long)n * P.tiles_y * P.tiles_x <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: too many pixel tiles (images=%d h2=%d w2=%d)", name, n, h2, w2);
    return RMD_OK;
}

// ---- the whole network ---------------------------------------------------------------------------------

struct NetShape {
    int c[kLayers];         // input channels of layers 1-6: c_in, c1, c2, c2, c3, c4
    int h, w, h2, w2;
};

NetShape net_shape(int c_in, int c1, int c2, int c3, int c4, int h, int w) {
    return {{c_in, c1, c2, c2, c3, c4}, h, w, h / 2, w / 2};
}

inline bool net_supported(int c_in, int c1, int c2, int c3, int c4, long long h, long long w) {
    if (h < 2 || w < 2 || (h & 1) || (w & 1)) return false;         // the reference's view fails on odd sides
    const int cin[4] = {c_in, c1, c2, c2}, cout[4] = {c1, c2, c2, c3};
    for (int l = 0; l < 4; ++l)
        if (cin[l] < 1 || cin[l] > 512 || cout[l] < 1 || cout[l] > 1024) return false;
    if (!tail_supported(c3, c4, h / 2, w / 2)) return false;
    const long long n = h * w, n2 = n / 4;
    return n * c_in < (1ll << 30) && n * c1 < (1ll << 30) && n2 * c2 < (1ll << 30);
}

struct NetWork {
    char* frags[5];         // the packed weights of layers 1-4 and of the tail
    float* map[4];          // one group's results of layers 1-4
    size_t bytes;
};

// the carve-up of the workspace from `base` (already aligned)
NetWork net_carve(char* base, int group, const NetShape& S) {
    NetWork Wk;
    size_t at = 0;
    for (int l = 0; l < 4; ++l) {
        Wk.frags[l] = base + at;
        at += sconv_frag_bytes(S.c[l], S.c[l + 1], 3, 3);
    }
    Wk.frags[4] = base + at;
    at += tail_frag_bytes(S.c[4]);
    for (int l = 0; l < 4; ++l) {
        const size_t px = l == 0 ? (size_t)S.h * S.w : (size_t)S.h2 * S.w2;
        Wk.map[l] = reinterpret_cast<float*>(base + at);
        at += align256((size_t)group * S.c[l + 1] * px * sizeof(float));
    }
    Wk.bytes = at;
    return Wk;
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" int rmd_mnet_tail_supported(int c3, int c4, int h2, int w2) { return tail_supported(c3, c4, h2, w2) ? 1 : 0; }

extern "C" size_t rmd_mnet_tail_workspace_bytes(int c3, int c4) {
    if (!tail_supported(c3, c4, 1, 1)) return 0;
    return tail_frag_bytes(c3) + kAlign;
}

extern "C" int rmd_mnet_tail(const float* x, const float* weight5, const float* bias5, const float* weight6,
                             const float* bias6, float* cost, void* workspace, int images, int c3, int c4, int h2,
                             int w2, int compute, void* stream) {
    const char* name = "rmd_mnet_tail";
    RMD_REQUIRE(x && weight5 && bias5 && weight6 && bias6 && cost && workspace, RMD_ERR_ARG, "%s: null pointer", name);
    RMD_REQUIRE(compute == RMD_BF16X3 || compute == RMD_BF16, RMD_ERR_ARG,
                "%s: compute must be RMD_BF16X3 or RMD_BF16, got %d", name, compute);
    if (int rc = tail_check_shape(name, images, c3, c4, h2, w2)) return rc;
    const size_t wbytes = rmd_mnet_tail_workspace_bytes(c3, c4);
    const size_t xbytes = (size_t)images * c3 * h2 * w2 * sizeof(float);
    const size_t obytes = (size_t)images * 4 * h2 * w2 * sizeof(float);
    const void* par[4] = {weight5, bias5, weight6, bias6};
    const size_t pbytes[4] = {(size_t)c3 * c4 * 16 * sizeof(float), c4 * sizeof(float), (size_t)c4 * 9 * sizeof(float),
                              sizeof(float)};
    RMD_REQUIRE(!overlap(cost, obytes, x, xbytes) && !overlap(workspace, wbytes, x, xbytes) &&
                    !overlap(workspace, wbytes, cost, obytes), RMD_ERR_ARG, "%s: cost, x and workspace overlap", name);
    for (int g = 0; g < 4; ++g)
        RMD_REQUIRE(!overlap(workspace, wbytes, par[g], pbytes[g]) && !overlap(cost, obytes, par[g], pbytes[g]),
                    RMD_ERR_ARG, "%s: workspace or cost overlaps a parameter", name);
    void* frags = reinterpret_cast<void*>(align256(reinterpret_cast<size_t>(workspace)));
    hipStream_t st = as_stream(stream);
    tail_pack(weight5, frags, c3, c4, compute, st);
    tail_packed(x, frags, bias5, weight6, bias6, cost, tail_geom(images, c3, c4, h2, w2), compute, st);
    return check_launch(name);
}

extern "C" int rmd_matching_net_supported(int c_in, int c1, int c2, int c3, int c4, int h, int w) {
    return net_supported(c_in, c1, c2, c3, c4, h, w) ? 1 : 0;
}

extern "C" size_t rmd_matching_net_workspace_bytes(int group, int c_in, int c1, int c2, int c3, int c4, int h, int w) {
    if (group < 1 || !net_supported(c_in, c1, c2, c3, c4, h, w)) return 0;
    return net_carve(nullptr, group, net_shape(c_in, c1, c2, c3, c4, h, w)).bytes + kAlign;
}

extern "C" int rmd_matching_net(const float* mvol, const float* const* weights, const float* const* biases, float* cost,
                                void* workspace, int images, int group, int c_in, int c1, int c2, int c3, int c4, int h,
                                int w, int compute, void* stream) {
    const char* name = "rmd_matching_net";
    RMD_REQUIRE(mvol && weights && biases && cost && workspace, RMD_ERR_ARG, "%s: null pointer", name);
    for (int g = 0; g < kLayers; ++g)
        RMD_REQUIRE(weights[g] && biases[g], RMD_ERR_ARG, "%s: null weight or bias %d", name, g);
    RMD_REQUIRE(compute == RMD_BF16X3 || compute == RMD_BF16, RMD_ERR_ARG,
                "%s: compute must be RMD_BF16X3 or RMD_BF16, got %d", name, compute);
    RMD_REQUIRE(group >= 1, RMD_ERR_ARG, "%s: group must be at least 1, got %d", name, group);
    RMD_REQUIRE(images > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(net_supported(c_in, c1, c2, c3, c4, h, w), RMD_ERR_SHAPE,
                "%s: unsupported (channels %d -> %d, %d, %d, %d on %d x %d): sides even, layer inputs <= 512 channels, "
                "c3 in 1..64, c4 in 1..32, channels x H x W < 2^30", name, c_in, c1, c2, c3, c4, h, w);
    if (group > images) group = images;
    const NetShape S = net_shape(c_in, c1, c2, c3, c4, h, w);
    const int strides[4] = {1, 2, 1, 1};
    for (int l = 0; l < 4; ++l)         // layers 1 and 2 read full-resolution maps, 3 and 4 the halved ones
        if (int rc = sconv_check_shape(name, group, S.c[l], S.c[l + 1], 3, 3, l < 2 ? h : S.h2, l < 2 ? w : S.w2,
                                       strides[l]))
            return rc;
    if (int rc = tail_check_shape(name, group, c3, c4, S.h2, S.w2)) return rc;
    const size_t wbytes = rmd_matching_net_workspace_bytes(group, c_in, c1, c2, c3, c4, h, w);
    const size_t xbytes = (size_t)images * c_in * h * w * sizeof(float), obytes = (size_t)images * h * w * sizeof(float);
    RMD_REQUIRE(!overlap(cost, obytes, mvol, xbytes) && !overlap(workspace, wbytes, mvol, xbytes) &&
                    !overlap(workspace, wbytes, cost, obytes), RMD_ERR_ARG, "%s: cost, mvol and workspace overlap", name);
    for (int g = 0; g < kLayers; ++g) {
        const size_t pw = (g < 4 ? (size_t)S.c[g + 1] * S.c[g] * 9 : g == 4 ? (size_t)c3 * c4 * 16 : (size_t)c4 * 9) *
                          sizeof(float);
        const size_t pb = (g < 5 ? S.c[g + 1] : 1) * sizeof(float);
        RMD_REQUIRE(!overlap(workspace, wbytes, weights[g], pw) && !overlap(workspace, wbytes, biases[g], pb) &&
                        !overlap(cost, obytes, weights[g], pw) && !overlap(cost, obytes, biases[g], pb),
                    RMD_ERR_ARG, "%s: workspace or cost overlaps weight or bias %d", name, g);
    }
    const NetWork Wk = net_carve(reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(workspace))), group, S);
    hipStream_t st = as_stream(stream);
    for (int l = 0; l < 4; ++l) sconv_pack(weights[l], Wk.frags[l], S.c[l], S.c[l + 1], 3, 3, compute, st);
    tail_pack(weights[4], Wk.frags[4], c3, c4, compute, st);
    const size_t in_img = (size_t)c_in * h * w, out_img = (size_t)h * w;
    for (int first = 0; first < images; first += group) {
        const int g = images - first < group ? images - first : group;
        sconv_packed(mvol + first * in_img, Wk.frags[0], biases[0], Wk.map[0], g, c_in, c1, 3, 3, h, w, 1, 1, compute, st);
        sconv_packed(Wk.map[0], Wk.frags[1], biases[1], Wk.map[1], g, c1, c2, 3, 3, h, w, 2, 1, compute, st);
        sconv_packed(Wk.map[1], Wk.frags[2], biases[2], Wk.map[2], g, c2, c2, 3, 3, S.h2, S.w2, 1, 1, compute, st);
        sconv_packed(Wk.map[2], Wk.frags[3], biases[3], Wk.map[3], g, c2, c3, 3, 3, S.h2, S.w2, 1, 1, compute, st);
        tail_packed(Wk.map[3], Wk.frags[4], biases[4], weights[5], biases[5], cost + first * out_img,
                    tail_geom(g, c3, c4, S.h2, S.w2), compute, st);
    }
    return check_launch(name);
}
