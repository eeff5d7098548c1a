// encoder.hip — the RAFT feature / context encoder (inference) without MIOpen: a strided, normalising k x k
// convolution as one MFMA implicit GEMM, the instance-norm statistics of a map, the residual join, and the whole
// s3 FeatureEncoder forward over one workspace.
//
// Replaces (qzed/raft-meets-dicl v2) FeatureEncoder (src/models/common/encoders/raft/s3.py:8-72) and ResidualBlock
// (src/models/common/blocks/raft.py:13-46) for the norm types 'none', 'instance' and — folded into the weights by
// the caller — eval-mode 'batch'.
//
// The convolution is conv.hip's GEMM (M = output channels, N = pixels, K = kh kw C; v_mfma_f32_32x32x16_bf16, the
// weights packed into A fragments, the split-bf16 arithmetic of mfma_bf16.h, fp32 NCHW in and out) with three
// additions:
//   stride s = 1 or 2   out[b, o, y, x] = sum W[o, c, i, j] in'[b, c, s y + i - kh/2, s x + j - kw/2], zero outside;
//                       the output side is (H - 1) / s + 1
//   load transform      in'[b, c, p] = relu(in[b, c, p] a[b, c] + d[b, c]) — the instance norm and ReLU of the
//                       producing convolution, applied in fp32 before the bf16 split while the chunk is staged.
//                       Positions outside the map stay zero: they pad the normalised map
//   residual            v = act(acc + bias); with a residual v = relu(v + res[b, o, y, x]): relu3(x + relu2(.)) of
//                       the block in the store of its second convolution
//
// Tile and chunk.  A workgroup owns NR x 32 output pixels of one image and stages, per chunk of KC input
// channels, the ((NR - 1) s + kh) x (31 s + kw) positions its taps read (along a kernel side of 1 only every s-th
// row or column is read, and only those are staged: a strided 1 x 1 projection stages NR x 32), position-major
// with KC + 8 bf16 per position (an odd number of 16-byte slots), hi part and — three-product mode — the part of the residual.  At
// stride 2 a lane's B fragment would move two positions per lane (an even number of slots: two-way bank
// conflicts), so the even and the odd staged columns of a row are kept as two planes: tap (i, j) of output column
// r reads plane j & 1 at r + (j >> 1), one position per lane again.  NR and KC are the largest that fit 64 KiB (two
// workgroups per CU) in the three-product mode: NR = 4 with KC = 64 (1 x 1 at either stride, 3 x 3 at stride 1),
// 32 (up to 7 x 7 at stride 1), 16 (3 x 3 at stride 2: 9 x 65 positions, 56,160 bytes), else NR = 2 with KC = 16 (5 x 5 and 7 x 7 at
// stride 2: the stem's 9 x 69 positions, 59,616 bytes).  The stem (Cin = 3) fills 3 of a k-step's 16 K lanes per
// tap, as convf1 of the motion encoder fills 2; taps are not packed together.
//
// The statistics are two passes over a plane by one workgroup of 1024 threads — the mean, then the centred
// squares — accumulated in float64 per thread and reduced over a fixed tree: no atomics, one order, nothing shared
// between planes.
//
// Every output's summation order is fixed (channel chunk, tap row, tap column, k-step; small products first) and
// depends on nothing but its own image: results are bitwise repeatable and per-sample independent.

#include "encoder.h"
#include "mfma_bf16.h"

namespace rmd {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kCols = 32;                   // output pixels of a tile row: one MFMA pixel tile
constexpr int kLdsBytes = 64 * 1024;        // dynamic LDS of a workgroup: two workgroups per CU
constexpr int kMaxK = 7, kMaxC = 512, kMaxCout = 1024;
constexpr int kAlign = 256;

struct SConvGeom {
    int B, C, Cout, kh, kw, stride, H, W, Ho, Wo;
    int act;                // 0: none, 1: ReLU
    int mo, ks, taps;       // 32-row tiles, 16-channel k-steps of one tap, taps
    int rows;               // output rows of a tile (NR)
    int tiles_x, tiles_y, mpass;
    int sy, sx;             // staged rows / positions between two output rows / columns: the stride, or 1 along a
                            // side of the kernel that is 1 (only every stride-th row / column is read: only those
                            // are staged)
    int iy, ix;             // input rows / columns between two staged ones: 1, or the stride along such a side
    int sh, sw;             // staged rows, staged positions of a row
    int pw0;                // positions of a staged row's even-column plane (sx = 2)
    int slots;              // staged positions
    int kc;                 // channels per staged chunk
    int nfrag;              // A fragments of one part (hi or lo)
};

inline bool sconv_supported(int kh, int kw, int stride, int c, int cout) {
    return kh >= 1 && kh <= kMaxK && (kh & 1) && kw >= 1 && kw <= kMaxK && (kw & 1) && (stride == 1 || stride == 2) &&
           c >= 1 && c <= kMaxC && cout >= 1 && cout <= kMaxCout;
}

// ---- weights -> A fragments: conv.hip's order ----------------------------------------------------------

// fragment (m * taps + t) * ks + k, lane l = (row 32 m + (l & 31), half l >> 5), element j:
// W[row][16 k + 8 (l >> 5) + j][tap t], zero for row >= Cout or a channel >= C; nfrag hi fragments, then (if `lo`)
// nfrag fragments of the bf16 of the residual
__global__ void __launch_bounds__(256)
sconv_pack_kernel(const float* __restrict__ w, int cout, int C, int taps, int mo, int ks, int nfrag, int lo,
                  bf16x8* __restrict__ frags) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    const int groups = 2 * ks;
    if (id >= mo * 32 * groups) return;
    const int row = id / groups, grp = id - row * groups;
    const int m = row >> 5, k = grp >> 1, half = grp & 1;
    const int c = 8 * grp;
    const float* src = w + ((size_t)row * C + c) * taps;
    for (int t = 0; t < taps; ++t) {
        bf16x8 hi, lopart;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = (row < cout && c + j < C) ? src[j * taps + t] : 0.f;
            hi[j] = bf16_hi(v);
            lopart[j] = bf16_lo(v, hi[j]);
        }
        const size_t at = ((size_t)(m * taps + t) * ks + k) * 64 + 32 * half + (row & 31);
        frags[at] = hi;
        if (lo) frags[at + (size_t)nfrag * 64] = lopart;
    }
}

// ---- the GEMM kernel ---------------------------------------------------------------------------------

template <int NP, int MT, int NR, int KC>
__global__ void __launch_bounds__(kThreads, 2)
sconv_kernel(const float* __restrict__ in, const float* __restrict__ scale, const float* __restrict__ shift,
             const bf16x8* __restrict__ frags, const float* __restrict__ bias, const float* __restrict__ res,
             float* __restrict__ out, SConvGeom P) {
    extern __shared__ __attribute__((aligned(16))) __bf16 sm[];      // PARTS * slots * kStride
    constexpr int kStride = KC + 8;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    int blk = blockIdx.x;
    const int pass = blk % P.mpass; blk /= P.mpass;
    const int tx = blk % P.tiles_x; blk /= P.tiles_x;
    const int ty = blk % P.tiles_y;
    const int b = blk / P.tiles_y;
    const int x0 = tx * kCols, y0 = ty * NR;                // first output pixel of the tile
    const int HW = P.H * P.W, HWo = P.Ho * P.Wo;
    const int sw = P.sw, st = P.stride;
    const int yb = st * y0 - (P.kh >> 1), xb = st * x0 - (P.kw >> 1);     // input position of staged (0, 0)
    const float* ib = in + (size_t)b * P.C * HW;            // wave-uniform bases, 32-bit offsets inside an image
    const float* ab = scale ? scale + (size_t)b * P.C : nullptr;
    const float* db = scale ? shift + (size_t)b * P.C : nullptr;
    // wave -> 32-row output tiles and pixel rows, as conv.hip: four tiles or more in a pass give a wave MT tiles
    // for all NR rows; one or two tiles (Cout <= 64) split the rows over the waves instead
    const bool split_rows = MT == 1 && P.mo <= 2;
    const int rpg = max(1, NR * P.mo / kWaves);            // rows of a wave when the rows are split
    const int m0 = split_rows ? wave % P.mo : (pass * kWaves + wave) * MT;
    const int nlo = split_rows ? wave / P.mo * rpg : 0, nhi = split_rows ? nlo + rpg : NR;
    const bool active = m0 < P.mo && nlo < NR;
    const int lopart = P.slots * kStride;

    f32x16 acc[MT][NR];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NR; ++n) acc[m][n] = f32x16{};

    for (int c0 = 0; c0 < P.C; c0 += KC) {
        const int ksteps = (min(KC, P.C - c0) + 15) >> 4;
        __syncthreads();                                    // the previous chunk's reads are done
        for (int id = tid; id < 2 * ksteps * P.slots; id += kThreads) {
            const int grp = id / P.slots, s = id - grp * P.slots;
            const int sy = s / sw, sx = s - sy * sw;        // in the map's order: neighbouring lanes, neighbouring x
            const int yy = yb + sy * P.iy, xx = xb + sx * P.ix;
            const bool inside = yy >= 0 && yy < P.H && xx >= 0 && xx < P.W;
            const int c = c0 + 8 * grp;
            const int at = inside ? yy * P.W + xx : 0;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int cc = c + j;                       // the last group may hold the padded tail
                const bool have = inside && cc < P.C;
                float t = have ? ib[cc * HW + at] : 0.f;
                if (ab && have) {                           // padding stays zero: it pads the normalised map
                    t = t * ab[cc] + db[cc];
                    t = t < 0.f ? 0.f : t;                  // keeps NaN
                }
                v[j] = t;
            }
            bf16x8 hi, lo;
            split<NP>(v, hi, lo);
            const int slot = sy * sw + (P.sx == 2 ? (sx & 1) * P.pw0 + (sx >> 1) : sx);
            *reinterpret_cast<bf16x8*>(&sm[slot * kStride + 8 * grp]) = hi;
            if constexpr (NP == 3) *reinterpret_cast<bf16x8*>(&sm[lopart + slot * kStride + 8 * grp]) = lo;
        }
        __syncthreads();
        if (!active) continue;
        const int kbase = c0 >> 4;
        for (int i = 0; i < P.kh; ++i) {
            for (int j = 0; j < P.kw; ++j) {
                const int t = i * P.kw + j;
                const int joff = P.sx == 2 ? (j & 1) * P.pw0 + (j >> 1) : j;
#pragma unroll
                for (int k = 0; k < KC / 16; ++k) {
                    if (k < ksteps) {
                        bf16x8 ah[MT], al[MT];
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            const int mm = min(m0 + m, P.mo - 1);       // a tile past the last one is never stored
                            const size_t f = ((size_t)(mm * P.taps + t) * P.ks + kbase + k) * 64 + lane;
                            ah[m] = frags[f];
                            al[m] = NP == 3 ? frags[f + (size_t)P.nfrag * 64] : bf16x8{};
                        }
#pragma unroll
                        for (int n = 0; n < NR; ++n) {
                            if (n >= nlo && n < nhi && (n == 0 || y0 + n < P.Ho)) {
                                const __bf16* p = &sm[((n * P.sy + i) * sw + joff + r) * kStride + 16 * k + 8 * hh];
                                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(p);
                                const bf16x8 bl = NP == 3 ? *reinterpret_cast<const bf16x8*>(p + lopart) : bf16x8{};
#pragma unroll
                                for (int m = 0; m < MT; ++m) mma<NP>(acc[m][n], ah[m], al[m], bh, bl);
                            }
                        }
                    }
                }
            }
        }
    }
    if (!active) return;

    // epilogue: register i of lane (r, hh) is channel 32 (m0 + m) + acc_row(i, hh) of pixel (y0 + n, x0 + r)
    const int x = x0 + r;
    if (x >= P.Wo) return;
    float* ob = out + (size_t)b * P.Cout * HWo;
    const float* rb = res ? res + (size_t)b * P.Cout * HWo : nullptr;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ch = 32 * (m0 + m) + acc_row(i, hh);
            if (ch >= P.Cout) continue;
            const float bv = bias[ch];
#pragma unroll
            for (int n = 0; n < NR; ++n) {
                if (n < nlo || n >= nhi || y0 + n >= P.Ho) continue;
                const int at = ch * HWo + (y0 + n) * P.Wo + x;
                float v = acc[m][n][i] + bv;
                if (P.act) v = v < 0.f ? 0.f : v;           // keeps NaN, as torch.relu (fmaxf would not)
                if (rb) {
                    v += rb[at];
                    v = v < 0.f ? 0.f : v;
                }
                ob[at] = v;
            }
        }
    }
}

// ---- instance statistics -----------------------------------------------------------------------------

constexpr int kStatThreads = 1024;          // 16 waves per plane: a batch of 8 at 64 channels still fills the CUs

// the sum of every thread's v, to every thread; a fixed tree over `red`
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                        // the previous sum's reads are done
    red[tid] = v;
    __syncthreads();
    for (int s = kStatThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// elements 4 q .. 4 q + 3 of the plane (zero past its end, `have` of them real): one 16-byte load where the plane
// allows it.  Which thread adds which element, and in which order, does not depend on that: a view at an odd
// offset gives the bits of its aligned copy
__device__ __forceinline__ int load_quad(const float* p, int q, int HW, bool vec, float* v) {
    const int have = min(4, HW - 4 * q);
    if (vec && have == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = t[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < have ? p[4 * q + j] : 0.f;
    }
    return have;
}

// plane (b, c) of x -> a = 1 / sqrt(var + eps), d = -mean a; biased variance.  One workgroup per plane: the mean,
// then the centred squares (the second pass re-reads the plane from L2)
__global__ void __launch_bounds__(kStatThreads)
inst_stats_kernel(const float* __restrict__ x, int HW, float eps, float* __restrict__ a, float* __restrict__ d) {
    __shared__ double red[kStatThreads];
    const int tid = threadIdx.x;
    const float* p = x + (size_t)blockIdx.x * HW;
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    const int quads = (HW + 3) >> 2;
    float v[4];
    double s = 0.0;
    for (int q = tid; q < quads; q += kStatThreads) {
        load_quad(p, q, HW, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += (double)v[j];      // the zeros past the end add nothing
    }
    const double mean = block_sum(s, red) / HW;
    double sq = 0.0;
    for (int q = tid; q < quads; q += kStatThreads) {
        const int have = load_quad(p, q, HW, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double t = (double)v[j] - mean;
            if (j < have) sq += t * t;
        }
    }
    const double var = block_sum(sq, red) / HW;
    if (tid == 0) {
        const double aa = 1.0 / sqrt(var + (double)eps);
        a[blockIdx.x] = (float)aa;
        d[blockIdx.x] = (float)(-mean * aa);
    }
}

// ---- residual join -------------------------------------------------------------------------------------

// out = relu(xs + relu(y ya + yd)), xs = x, x xa + xd or (x absent) 0; the statistics are per plane.  out may be y
__global__ void __launch_bounds__(256)
join_kernel(const float* y, const float* __restrict__ ya, const float* __restrict__ yd, const float* __restrict__ x,
            const float* __restrict__ xa, const float* __restrict__ xd, float* out, int HW, long long total) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const long long plane = id / HW;
    float v = y[id];
    if (ya) v = v * ya[plane] + yd[plane];
    v = v < 0.f ? 0.f : v;                                  // keeps NaN
    if (x) {
        float xs = x[id];
        if (xa) xs = xs * xa[plane] + xd[plane];
        v += xs;
        v = v < 0.f ? 0.f : v;
    }
    out[id] = v;
}

// ---- host --------------------------------------------------------------------------------------------

inline int out_side(int n, int stride) { return (n - 1) / stride + 1; }

inline size_t lds_bytes(int slots, int kc) { return (size_t)2 * slots * (kc + 8) * sizeof(__bf16); }

SConvGeom sconv_geom(int batch, int c, int cout, int kh, int kw, int stride, int height, int width, int act) {
    SConvGeom P;
    P.B = batch; P.C = c; P.Cout = cout; P.kh = kh; P.kw = kw; P.stride = stride; P.H = height; P.W = width;
    P.Ho = out_side(height, stride); P.Wo = out_side(width, stride); P.act = act;
    P.mo = (cout + 31) / 32; P.ks = (c + 15) / 16; P.taps = kh * kw;
    P.sy = kh == 1 ? 1 : stride; P.iy = kh == 1 ? stride : 1;
    P.sx = kw == 1 ? 1 : stride; P.ix = kw == 1 ? stride : 1;
    P.sw = (kCols - 1) * P.sx + kw;
    P.pw0 = (P.sw + 1) / 2;
    // the largest tile and chunk whose two staged parts fit kLdsBytes (both modes take the same)
    P.rows = 4; P.kc = 0;
    for (int kc = 64; kc >= 16 && !P.kc; kc >>= 1)
        if (lds_bytes((3 * P.sy + kh) * P.sw, kc) <= (size_t)kLdsBytes) P.kc = kc;
    if (!P.kc) { P.rows = 2; P.kc = 16; }                   // 7 x 7 at stride 2: 9 x 69 positions, 59,616 bytes
    P.sh = (P.rows - 1) * P.sy + kh;
    P.slots = P.sh * P.sw;
    P.tiles_x = (P.Wo + kCols - 1) / kCols; P.tiles_y = (P.Ho + P.rows - 1) / P.rows;
    const int per_pass = kWaves * (cout <= 32 * kWaves ? 1 : 2);
    P.mpass = (P.mo + per_pass - 1) / per_pass;
    P.nfrag = P.mo * P.taps * P.ks;
    return P;
}

// bytes of the packed weights of one convolution: both parts, a multiple of kAlign
size_t sconv_packed_bytes(int c, int cout, int kh, int kw) {
    const size_t nfrag = (size_t)((cout + 31) / 32) * kh * kw * ((c + 15) / 16);
    return nfrag * 64 * sizeof(bf16x8) * 2;
}

// the shape checks of one convolution of entry point `name`
int sconv_shape(const char* name, int batch, int c, int cout, int kh, int kw, int height, int width, int stride) {
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(sconv_supported(kh, kw, stride, c, cout), RMD_ERR_SHAPE,
                "%s: unsupported (kernel %dx%d, stride %d, channels %d -> %d): kernel sides odd in 1..7, stride 1 or 2, "
                "C in 1..512, Cout in 1..1024", name, kh, kw, stride, c, cout);
    const long long n = (long long)height * width;
    const long long no = (long long)out_side(height, stride) * out_side(width, stride);
    // 32-bit lane offsets into one image's maps, 64-bit everywhere else
    RMD_REQUIRE(n * c < (1ll << 30) && no * cout < (1ll << 30), RMD_ERR_SHAPE,
                "%s: %lld pixels x %d channels in, %lld x %d out per image", name, n, c, no, cout);
    const SConvGeom P = sconv_geom(batch, c, cout, kh, kw, stride, height, width, 0);
    RMD_REQUIRE((long long)batch * P.tiles_y * P.tiles_x * P.mpass <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: too many pixel tiles (batch=%d height=%d width=%d)", name, batch, height, width);
    return RMD_OK;
}

// the checks of one convolution of entry point `name`, before any launch
int sconv_check(const char* name, const float* in, const float* scale, const float* shift, const float* weight,
                const float* bias, const float* res, const float* out, int batch, int c, int cout, int kh, int kw,
                int height, int width, int stride, int act, int compute) {
    RMD_REQUIRE(in && weight && bias && out, RMD_ERR_ARG, "%s: null pointer", name);
    RMD_REQUIRE((scale == nullptr) == (shift == nullptr), RMD_ERR_ARG, "%s: scale and shift are given together", name);
    RMD_REQUIRE(compute == RMD_BF16X3 || compute == RMD_BF16, RMD_ERR_ARG,
                "%s: compute must be RMD_BF16X3 or RMD_BF16, got %d", name, compute);
    RMD_REQUIRE(act == 0 || act == 1, RMD_ERR_ARG, "%s: act must be 0 (none) or 1 (ReLU), got %d", name, act);
    if (int rc = sconv_shape(name, batch, c, cout, kh, kw, height, width, stride)) return rc;
    const long long n = (long long)height * width;
    const long long no = (long long)out_side(height, stride) * out_side(width, stride);
    const size_t obytes = (size_t)batch * cout * no * sizeof(float);
    const size_t ibytes = (size_t)batch * c * n * sizeof(float), sbytes = (size_t)batch * c * sizeof(float);
    const size_t wbytes = (size_t)cout * c * kh * kw * sizeof(float);
    RMD_REQUIRE(!overlap(out, obytes, in, ibytes) && !overlap(out, obytes, weight, wbytes) &&
                    !overlap(out, obytes, bias, cout * sizeof(float)) && !(res && overlap(out, obytes, res, obytes)) &&
                    !(scale && (overlap(out, obytes, scale, sbytes) || overlap(out, obytes, shift, sbytes))),
                RMD_ERR_ARG, "%s: out overlaps an input", name);
    return RMD_OK;
}

template <int NP, int NR, int KC>
void sconv_launch(const float* in, const float* scale, const float* shift, const bf16x8* frags, const float* bias,
                  const float* res, float* out, const SConvGeom& P, hipStream_t st) {
    const int grid = P.B * P.tiles_y * P.tiles_x * P.mpass;
    const size_t lds = (size_t)(NP == 3 ? 2 : 1) * P.slots * (KC + 8) * sizeof(__bf16);     // at most kLdsBytes
    if (P.Cout <= 32 * kWaves)
        sconv_kernel<NP, 1, NR, KC><<<grid, kThreads, lds, st>>>(in, scale, shift, frags, bias, res, out, P);
    else
        sconv_kernel<NP, 2, NR, KC><<<grid, kThreads, lds, st>>>(in, scale, shift, frags, bias, res, out, P);
}

template <int NP>
void sconv_dispatch(const float* in, const float* scale, const float* shift, const bf16x8* fr, const float* bias,
                    const float* res, float* out, const SConvGeom& P, hipStream_t st) {
    if (P.rows == 2) sconv_launch<NP, 2, 16>(in, scale, shift, fr, bias, res, out, P, st);
    else if (P.kc == 64) sconv_launch<NP, 4, 64>(in, scale, shift, fr, bias, res, out, P, st);
    else if (P.kc == 32) sconv_launch<NP, 4, 32>(in, scale, shift, fr, bias, res, out, P, st);
    else sconv_launch<NP, 4, 16>(in, scale, shift, fr, bias, res, out, P, st);
}

// packs `weight` at `frags`
void sconv_pack_run(const float* weight, void* frags, const SConvGeom& P, int compute, hipStream_t st) {
    const int threads = P.mo * 32 * 2 * P.ks;
    sconv_pack_kernel<<<(threads + 255) / 256, 256, 0, st>>>(weight, P.Cout, P.C, P.taps, P.mo, P.ks, P.nfrag,
                                                            compute == RMD_BF16X3 ? 1 : 0,
                                                            reinterpret_cast<bf16x8*>(frags));
}

// runs the convolution on the fragments sconv_pack_run wrote for `compute`
void sconv_packed_run(const float* in, const float* scale, const float* shift, const void* frags, const float* bias,
                      const float* res, float* out, const SConvGeom& P, int compute, hipStream_t st) {
    const bf16x8* fr = reinterpret_cast<const bf16x8*>(frags);
    if (compute == RMD_BF16X3) sconv_dispatch<3>(in, scale, shift, fr, bias, res, out, P, st);
    else sconv_dispatch<1>(in, scale, shift, fr, bias, res, out, P, st);
}

// packs `weight` at `frags` and runs the convolution
void sconv_run(const float* in, const float* scale, const float* shift, const float* weight, const float* bias,
               const float* res, float* out, void* frags, const SConvGeom& P, int compute, hipStream_t st) {
    sconv_pack_run(weight, frags, P, compute, st);
    sconv_packed_run(in, scale, shift, frags, bias, res, out, P, compute, st);
}

void stats_run(const float* x, int planes, int hw, float eps, float* a, float* d, hipStream_t st) {
    inst_stats_kernel<<<planes, kStatThreads, 0, st>>>(x, hw, eps, a, d);
}

void join_run(const float* y, const float* ya, const float* yd, const float* x, const float* xa, const float* xd,
              float* out, long long planes, int hw, hipStream_t st) {
    const long long total = planes * hw;
    join_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(y, ya, yd, x, xa, xd, out, hw, total);
}

// ---- FeatureEncoder (s3.py:8-72) -----------------------------------------------------------------------

constexpr int kEncConvs = 16, kEncIn = 3, kEncMaxC = 128;

struct EncConv {
    int c, cout, k, stride;
};

// the 16 convolutions in module order: conv1; per block conv1, conv2 and (stride 2) downsample.0; conv2
void enc_convs(int output_dim, EncConv* cv) {
    int n = 0;
    cv[n++] = {kEncIn, 64, 7, 2};
    const int widths[3] = {64, 96, 128};
    int cin = 64;
    for (int l = 0; l < 3; ++l) {
        const int w = widths[l], s = l ? 2 : 1;
        cv[n++] = {cin, w, 3, s};
        cv[n++] = {w, w, 3, 1};
        if (s == 2) cv[n++] = {cin, w, 1, 2};
        cv[n++] = {w, w, 3, 1};
        cv[n++] = {w, w, 3, 1};
        cin = w;
    }
    cv[n++] = {128, output_dim, 1, 1};
}

struct EncWork {
    char* frags[kEncConvs];
    float* stat[6];         // a, d of the three norms of a block, (B, 128) each
    float* map[3];          // the block's input, conv1's and conv2's results
    float* proj;            // the projection's result
    size_t map_bytes, proj_bytes;       // of one map, of the projection's
    size_t bytes;
};

// floats of one image's largest map among the layers from `first` on: 64 H2 W2, 96 H4 W4, 128 H8 W8.  The first is
// the largest wherever the sides still halve, but a side of 1 stays 1 while the channels grow
size_t enc_map_floats(int height, int width, int first) {
    const int widths[3] = {64, 96, 128};
    size_t most = 0;
    int h = height, w = width;
    for (int l = 0; l < 3; ++l) {
        h = out_side(h, 2); w = out_side(w, 2);
        const size_t n = (size_t)widths[l] * h * w;
        if (l >= first && n > most) most = n;
    }
    return most;
}

// the carve-up of the encoder's workspace from `base` (already aligned)
EncWork enc_carve(char* base, int batch, int height, int width, int output_dim) {
    EncConv cv[kEncConvs];
    enc_convs(output_dim, cv);
    EncWork Wk;
    size_t at = 0;
    for (int i = 0; i < kEncConvs; ++i) {
        Wk.frags[i] = base + at;
        at += sconv_packed_bytes(cv[i].c, cv[i].cout, cv[i].k, cv[i].k);
    }
    for (int i = 0; i < 6; ++i) {
        Wk.stat[i] = reinterpret_cast<float*>(base + at);
        at += align256((size_t)batch * kEncMaxC * sizeof(float));
    }
    // every layer's maps rotate through the same three regions, both projections use the fourth
    Wk.map_bytes = align256((size_t)batch * enc_map_floats(height, width, 0) * sizeof(float));
    Wk.proj_bytes = align256((size_t)batch * enc_map_floats(height, width, 1) * sizeof(float));
    for (int i = 0; i < 3; ++i) {
        Wk.map[i] = reinterpret_cast<float*>(base + at);
        at += Wk.map_bytes;
    }
    Wk.proj = reinterpret_cast<float*>(base + at);
    at += Wk.proj_bytes;
    Wk.bytes = at;
    return Wk;
}

inline bool enc_supported(int output_dim, int norm) {
    return output_dim >= 1 && output_dim <= kMaxCout && (norm == RMD_NORM_NONE || norm == RMD_NORM_INSTANCE);
}

}  // namespace

// ---- encoder.h: the convolution's two steps for other launchers -------------------------------------------

size_t sconv_frag_bytes(int c, int cout, int kh, int kw) { return sconv_packed_bytes(c, cout, kh, kw); }

int sconv_check_shape(const char* name, int batch, int c, int cout, int kh, int kw, int height, int width, int stride) {
    return sconv_shape(name, batch, c, cout, kh, kw, height, width, stride);
}

void sconv_pack(const float* weight, void* frags, int c, int cout, int kh, int kw, int compute, hipStream_t st) {
    sconv_pack_run(weight, frags, sconv_geom(1, c, cout, kh, kw, 1, 1, 1, 0), compute, st);
}

void sconv_packed(const float* in, const void* frags, const float* bias, float* out, int batch, int c, int cout, int kh,
                  int kw, int height, int width, int stride, int act, int compute, hipStream_t st) {
    sconv_packed_run(in, nullptr, nullptr, frags, bias, nullptr, out,
                     sconv_geom(batch, c, cout, kh, kw, stride, height, width, act), compute, st);
}

}  // namespace rmd

using namespace rmd;

extern "C" int rmd_conv2d_strided_supported(int kh, int kw, int stride, int c, int cout) {
    return sconv_supported(kh, kw, stride, c, cout) ? 1 : 0;
}

extern "C" size_t rmd_conv2d_strided_workspace_bytes(int c, int cout, int kh, int kw) {
    if (!sconv_supported(kh, kw, 1, c, cout)) return 0;
    return sconv_packed_bytes(c, cout, kh, kw) + kAlign;
}

extern "C" int rmd_conv2d_strided(const float* in, const float* scale, const float* shift, const float* weight,
                                  const float* bias, const float* residual, float* out, void* workspace, int batch,
                                  int c, int cout, int kh, int kw, int height, int width, int stride, int act,
                                  int compute, void* stream) {
    const char* name = "rmd_conv2d_strided";
    RMD_REQUIRE(workspace, RMD_ERR_ARG, "%s: null workspace", name);
    if (int rc = sconv_check(name, in, scale, shift, weight, bias, residual, out, batch, c, cout, kh, kw, height, width,
                             stride, act, compute))
        return rc;
    const SConvGeom P = sconv_geom(batch, c, cout, kh, kw, stride, height, width, act);
    const size_t wbytes = rmd_conv2d_strided_workspace_bytes(c, cout, kh, kw);
    const size_t ibytes = (size_t)batch * c * height * width * sizeof(float);
    const size_t obytes = (size_t)batch * cout * P.Ho * P.Wo * sizeof(float), sbytes = (size_t)batch * c * sizeof(float);
    RMD_REQUIRE(!overlap(workspace, wbytes, in, ibytes) && !overlap(workspace, wbytes, out, obytes) &&
                    !overlap(workspace, wbytes, weight, (size_t)cout * c * kh * kw * sizeof(float)) &&
                    !overlap(workspace, wbytes, bias, cout * sizeof(float)) &&
                    !(residual && overlap(workspace, wbytes, residual, obytes)) &&
                    !(scale && (overlap(workspace, wbytes, scale, sbytes) || overlap(workspace, wbytes, shift, sbytes))),
                RMD_ERR_ARG, "%s: workspace overlaps a tensor", name);
    sconv_run(in, scale, shift, weight, bias, residual, out,
              reinterpret_cast<void*>(align256(reinterpret_cast<size_t>(workspace))), P, compute, as_stream(stream));
    return check_launch(name);
}

extern "C" int rmd_instance_stats(const float* x, float* scale, float* shift, int batch, int channels, int height,
                                  int width, float eps, void* stream) {
    const char* name = "rmd_instance_stats";
    RMD_REQUIRE(x && scale && shift, RMD_ERR_ARG, "%s: null pointer", name);
    RMD_REQUIRE(batch > 0 && channels > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    const long long n = (long long)height * width, planes = (long long)batch * channels;
    RMD_REQUIRE(n > 1, RMD_ERR_SHAPE, "%s: a plane of one pixel has no variance (nn.InstanceNorm2d raises too)", name);
    RMD_REQUIRE(n < (1ll << 30) && planes <= 0x7fffffffll, RMD_ERR_SHAPE, "%s: %lld pixels per plane, %lld planes", name,
                n, planes);
    RMD_REQUIRE(eps >= 0.f, RMD_ERR_ARG, "%s: eps must not be negative", name);
    const size_t xbytes = (size_t)planes * n * sizeof(float), sbytes = (size_t)planes * sizeof(float);
    RMD_REQUIRE(!overlap(scale, sbytes, x, xbytes) && !overlap(shift, sbytes, x, xbytes) &&
                    !overlap(scale, sbytes, shift, sbytes), RMD_ERR_ARG, "%s: the outputs overlap x or each other", name);
    stats_run(x, (int)planes, (int)n, eps, scale, shift, as_stream(stream));
    return check_launch(name);
}

extern "C" int rmd_residual_join(const float* y, const float* y_scale, const float* y_shift, const float* x,
                                 const float* x_scale, const float* x_shift, float* out, int batch, int channels,
                                 int height, int width, void* stream) {
    const char* name = "rmd_residual_join";
    RMD_REQUIRE(y && x && out, RMD_ERR_ARG, "%s: null pointer", name);
    RMD_REQUIRE((y_scale == nullptr) == (y_shift == nullptr) && (x_scale == nullptr) == (x_shift == nullptr), RMD_ERR_ARG,
                "%s: a scale and its shift are given together", name);
    RMD_REQUIRE(batch > 0 && channels > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    const long long n = (long long)height * width, planes = (long long)batch * channels;
    RMD_REQUIRE(n < (1ll << 30) && (planes * n + 255) / 256 <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: %lld pixels per plane, %lld planes", name, n, planes);
    const size_t bytes = (size_t)planes * n * sizeof(float), sbytes = (size_t)planes * sizeof(float);
    const float* stats[4] = {y_scale, y_shift, x_scale, x_shift};
    RMD_REQUIRE(!overlap(out, bytes, y, bytes) && !overlap(out, bytes, x, bytes), RMD_ERR_ARG,
                "%s: out overlaps an input", name);
    for (const float* s : stats)
        RMD_REQUIRE(!(s && overlap(out, bytes, s, sbytes)), RMD_ERR_ARG, "%s: out overlaps the statistics", name);
    join_run(y, y_scale, y_shift, x, x_scale, x_shift, out, planes, (int)n, as_stream(stream));
    return check_launch(name);
}

extern "C" int rmd_feature_encoder_supported(int output_dim, int norm) { return enc_supported(output_dim, norm) ? 1 : 0; }

extern "C" size_t rmd_feature_encoder_workspace_bytes(int batch, int height, int width, int output_dim) {
    if (batch < 1 || height < 1 || width < 1 || !enc_supported(output_dim, RMD_NORM_NONE)) return 0;
    return enc_carve(nullptr, batch, height, width, output_dim).bytes + kAlign;
}

extern "C" int rmd_feature_encoder_workspace_regions(int batch, int height, int width, int output_dim, size_t* regions) {
    const char* name = "rmd_feature_encoder_workspace_regions";
    RMD_REQUIRE(regions, RMD_ERR_ARG, "%s: null pointer", name);
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0 && enc_supported(output_dim, RMD_NORM_NONE), RMD_ERR_SHAPE,
                "%s: bad sizes", name);
    const EncWork Wk = enc_carve(nullptr, batch, height, width, output_dim);
    regions[0] = static_cast<size_t>(Wk.frags[kEncConvs - 1] - Wk.frags[0]) +
                 sconv_packed_bytes(128, output_dim, 1, 1);
    regions[1] = align256((size_t)batch * kEncMaxC * sizeof(float));
    regions[2] = Wk.map_bytes;
    regions[3] = Wk.proj_bytes;
    clear_error();
    return RMD_OK;
}

extern "C" int rmd_feature_encoder(const float* x, const float* const* weights, const float* const* biases, float* out,
                                   void* workspace, int batch, int height, int width, int output_dim, int norm, float eps,
                                   int compute, void* stream) {
    const char* name = "rmd_feature_encoder";
    RMD_REQUIRE(x && weights && biases && out && workspace, RMD_ERR_ARG, "%s: null pointer", name);
    for (int g = 0; g < kEncConvs; ++g)
        RMD_REQUIRE(weights[g] && biases[g], RMD_ERR_ARG, "%s: null weight or bias %d", name, g);
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(enc_supported(output_dim, norm), RMD_ERR_SHAPE,
                "%s: output_dim %d not in 1..1024 or norm %d not RMD_NORM_NONE / RMD_NORM_INSTANCE", name, output_dim, norm);
    RMD_REQUIRE(compute == RMD_BF16X3 || compute == RMD_BF16, RMD_ERR_ARG,
                "%s: compute must be RMD_BF16X3 or RMD_BF16, got %d", name, compute);
    RMD_REQUIRE(eps >= 0.f, RMD_ERR_ARG, "%s: eps must not be negative", name);
    const bool inst = norm == RMD_NORM_INSTANCE;
    EncConv cv[kEncConvs];
    enc_convs(output_dim, cv);
    const int h2 = out_side(height, 2), w2 = out_side(width, 2), h4 = out_side(h2, 2), w4 = out_side(w2, 2);
    const int h8 = out_side(h4, 2), w8 = out_side(w4, 2);
    RMD_REQUIRE(!inst || (long long)h8 * w8 > 1, RMD_ERR_SHAPE,
                "%s: a 1/8-resolution plane of one pixel has no variance (nn.InstanceNorm2d raises too)", name);
    RMD_REQUIRE((long long)height * width * kEncIn < (1ll << 30) &&
                    (long long)enc_map_floats(height, width, 0) < (1ll << 30) &&
                    (long long)h8 * w8 * output_dim < (1ll << 30), RMD_ERR_SHAPE, "%s: image too large (%d x %d)", name,
                height, width);
    const size_t wbytes = rmd_feature_encoder_workspace_bytes(batch, height, width, output_dim);
    const size_t xbytes = (size_t)batch * kEncIn * height * width * sizeof(float);
    const size_t obytes = (size_t)batch * output_dim * h8 * w8 * sizeof(float);
    RMD_REQUIRE(!overlap(out, obytes, x, xbytes) && !overlap(workspace, wbytes, x, xbytes) &&
                    !overlap(workspace, wbytes, out, obytes), RMD_ERR_ARG, "%s: out, x and workspace overlap", name);
    for (int g = 0; g < kEncConvs; ++g) {
        const size_t pw = (size_t)cv[g].cout * cv[g].c * cv[g].k * cv[g].k * sizeof(float), pb = cv[g].cout * sizeof(float);
        RMD_REQUIRE(!overlap(workspace, wbytes, weights[g], pw) && !overlap(workspace, wbytes, biases[g], pb) &&
                        !overlap(out, obytes, weights[g], pw) && !overlap(out, obytes, biases[g], pb),
                    RMD_ERR_ARG, "%s: workspace or out overlaps weight or bias %d", name, g);
    }
    const EncWork Wk = enc_carve(reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(workspace))), batch, height,
                                 width, output_dim);
    // the stem's 2 x 32 tiles of the 1/2-resolution map are the largest grid but for the last convolution's passes
    // (at most 8, on a map 16 times smaller)
    RMD_REQUIRE((long long)batch * ((h2 + 1) / 2) * ((w2 + kCols - 1) / kCols) * 8 <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: too many pixel tiles (batch=%d height=%d width=%d)", name, batch, height, width);
    hipStream_t st = as_stream(stream);
    float *X = Wk.map[0], *Y1 = Wk.map[1], *Y2 = Wk.map[2];
    float *a1 = Wk.stat[0], *d1 = Wk.stat[1], *a2 = Wk.stat[2], *d2 = Wk.stat[3], *a3 = Wk.stat[4], *d3 = Wk.stat[5];
    auto conv = [&](int g, const float* in, const float* sc, const float* sh, const float* res, float* dst, int h, int w,
                    int act) {
        const SConvGeom P = sconv_geom(batch, cv[g].c, cv[g].cout, cv[g].k, cv[g].k, cv[g].stride, h, w, act);
        sconv_run(in, sc, sh, weights[g], biases[g], res, dst, Wk.frags[g], P, compute, st);
    };
    // the stem: relu1(norm1(conv1(x)))
    int h = h2, w = w2, g = 0;
    if (inst) {
        conv(g, x, nullptr, nullptr, nullptr, Y1, height, width, 0);
        stats_run(Y1, batch * 64, h * w, eps, a1, d1, st);
        join_run(Y1, a1, d1, nullptr, nullptr, nullptr, X, (long long)batch * 64, h * w, st);
    } else {
        conv(g, x, nullptr, nullptr, nullptr, X, height, width, 1);
    }
    ++g;
    for (int blk = 0; blk < 6; ++blk) {
        const int s = cv[g].stride, co = cv[g].cout;
        const int ho = out_side(h, s), wo = out_side(w, s);
        const int g1 = g, g2 = g + 1, gd = s == 2 ? g + 2 : -1;
        const long long planes = (long long)batch * co;
        if (inst) {
            // conv1 raw -> statistics -> conv2 normalising on load -> statistics -> the projection's -> join
            conv(g1, X, nullptr, nullptr, nullptr, Y1, h, w, 0);
            stats_run(Y1, (int)planes, ho * wo, eps, a1, d1, st);
            conv(g2, Y1, a1, d1, nullptr, Y2, ho, wo, 0);
            stats_run(Y2, (int)planes, ho * wo, eps, a2, d2, st);
            if (gd >= 0) {
                conv(gd, X, nullptr, nullptr, nullptr, Wk.proj, h, w, 0);
                stats_run(Wk.proj, (int)planes, ho * wo, eps, a3, d3, st);
                join_run(Y2, a2, d2, Wk.proj, a3, d3, Y2, planes, ho * wo, st);
            } else {
                join_run(Y2, a2, d2, X, nullptr, nullptr, Y2, planes, ho * wo, st);
            }
        } else {
            // the projection, conv1 with ReLU, conv2 with the ReLU-and-residual epilogue
            if (gd >= 0) conv(gd, X, nullptr, nullptr, nullptr, Wk.proj, h, w, 0);
            conv(g1, X, nullptr, nullptr, nullptr, Y1, h, w, 1);
            conv(g2, Y1, nullptr, nullptr, gd >= 0 ? Wk.proj : X, Y2, ho, wo, 1);
        }
        float* t = X; X = Y2; Y2 = t;                       // the block's result is the next one's input
        h = ho; w = wo;
        g += s == 2 ? 3 : 2;
    }
    conv(g, X, nullptr, nullptr, nullptr, out, h, w, 0);
    return check_launch(name);
}
