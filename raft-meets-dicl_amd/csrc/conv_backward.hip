// conv_backward.hip — the backward of conv.hip's fused k x k convolution: with x = cat(in0, in1),
// y = act(conv(x, W) + b), g = dL/dy and gm = g [y > 0] (ReLU) or g (no activation),
//   gb[o]          = sum_{b,y,x} gm[b, o, y, x]
//   gx[b, c, y, x] = sum_{o,i,j} W[o, c, i, j] gm[b, o, y - i + kh/2, x - j + kw/2]
//   gW[o, c, i, j] = sum_{b,y,x} gm[b, o, y, x] x[b, c, y + i - kh/2, x + j - kw/2]        (zero outside the map)
//
// Replaces (qzed/raft-meets-dicl v2), under autograd, the backward of the convolutions next to the recurrent unit:
// BasicMotionEncoder (src/models/impls/raft.py:193-225), FlowHead (raft.py:262-273) and the mask head of
// Up8Network (raft.py:299-331).  Three split-bf16 products throughout (mfma_bf16.h), fp32 accumulators.
//
// Mask and bias gradient, one pass (conv_mask_bias_kernel): one workgroup per output channel walks the B planes of
// that channel in order, writes gm and keeps float64 partial sums per thread, combined by a fixed tree.  The mask
// is !(y <= 0), so a NaN in y keeps the gradient as torch.relu's backward does; a masked position is exactly 0
// whatever g holds.  Without an activation gm is g itself and the pass runs only where gb is wanted.
//
// Data gradient: a stride-1 "same" convolution of gm with W'[c, o, i, j] = W[o, c, kh-1-i, kw-1-j], which is
// conv.hip's conv_kernel<3, MT, KC> unchanged (conv_internal.h) behind conv_pack_transposed_kernel, which writes
// the A fragments of W' for the channel range of one source; gx0 and gx1 are two launches into two tensors.  The
// contraction runs over Cout (up to 1024: see conv_internal.h on why conv.hip's 512 does not bind here).
//
// Weight gradient (conv_wgrad_kernel): a GEMM with M = Cout, N = C per tap and K = B H W on
// v_mfma_f32_32x32x16_bf16, gm as the A operand and x as the B operand; both are K-contiguous in NCHW memory
// because pixels run along a row.
// * The K unit is a segment of kKP = 64 pixels of one map row (four k-steps).  A workgroup stages, as bf16 hi and
//   lo parts, the segment of gm for its 128 output channels ([channel][pixel], 72 bf16 per channel: an odd number
//   of 16-byte slots) and the segment of x of ONE tap row with its kw - 1 halo for its 32 input channels
//   ([channel][position], 72 per channel).  Tap (i, j) is the B fragment of the staged row y + i - kh/2 read
//   j positions further: a 16-byte read at a 2-byte-aligned address, which the compiler splits as the target
//   needs.  The A fragment of a k-step is read once and used for the kw taps.
// * A workgroup owns 128 output channels (one 32-row tile per wave) x 32 input channels x the kw taps of one tap
//   row x one slice of the (image, row) list: kw <= 7 accumulators of 16 registers per wave, so 7 x 7 needs no
//   spill, and only one row of x is staged at a time.  A map row whose tap row falls outside the map is skipped.
//   The price: gm is staged once per input-channel tile and tap row.  It is the simplest partition that fits every
//   supported shape; nothing here is tuned yet.
// * The (image, row) list is cut into nslices = min(B H, 32, ceil(1024 / workgroups of one slice)) slices of
//   equal length, a function of the shapes alone.  Every slice writes its own full (Cout, C, kh, kw) partial to the
//   workspace; conv_wgrad_reduce_kernel adds them in slice order.  No atomics: bitwise repeatable.
// * Pixels past the row's end, positions outside the map, channels past C and rows past Cout are staged as zeros.
//   A NaN in gm[b, o] therefore reaches every element of gW[o] (0 x NaN), as it does with a padded input.

#include <algorithm>
#include <cstring>

#include "conv_internal.h"
#include "mfma_bf16.h"

namespace rmd {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kKP = 64;                         // pixels of a staged row segment
constexpr int kGS = kKP + 8, kXS = kKP + 8;     // bf16 per staged channel: gm, x (64 + kw - 1 <= 70 positions)
constexpr int kOT = 32 * kWaves, kCT = 32;      // output / input channels of a workgroup
constexpr int kMaxSlices = 32, kTargetGroups = 1024;

struct WgradGeom {
    int B, C0, C1, C, Cout, kh, H, W;
    int mog, ctiles, nslices, rps;              // 128-row groups, 32-channel tiles, slices, (image, row)s per slice
};

// ---- mask + bias gradient ----------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads)
conv_mask_bias_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ gm,
                      float* __restrict__ gb, int B, int Cout, int HW) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x, o = blockIdx.x;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const size_t base = ((size_t)b * Cout + o) * HW;
        for (int p = tid; p < HW; p += kThreads) {
            float v = g[base + p];
            if (y) v = !(y[base + p] <= 0.f) ? v : 0.f;
            if (gm) gm[base + p] = v;
            s += (double)v;
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int n = kThreads / 2; n > 0; n >>= 1) {
        if (tid < n) red[tid] += red[tid + n];
        __syncthreads();
    }
    if (gb && tid == 0) gb[o] = (float)red[0];
}

// ---- W -> A fragments of W' for one source ---------------------------------------------------------------

// conv.hip's fragment layout for the (c_n, Cout, kh, kw) weight W'[row, o, t] = W[o, c_off + row, taps - 1 - t]:
// fragment (m taps + t) ks + k, lane (row 32 m + (l & 31), half l >> 5), element j: contraction channel
// o = 16 k + 8 half + j; zero for row >= c_n or o >= Cout.  Also zeroes the 32 mo floats of the bias the forward
// kernel adds.  One thread per (row, group of 8 contraction channels).
__global__ void __launch_bounds__(256)
conv_pack_transposed_kernel(const float* __restrict__ w, int cout, int C, int c_off, int c_n, int taps, int mo, int ks,
                            int nfrag, bf16x8* __restrict__ frags, float* __restrict__ zero_bias) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < mo * 32) zero_bias[id] = 0.f;
    const int groups = 2 * ks;
    if (id >= mo * 32 * groups) return;
    const int row = id / groups, grp = id - row * groups;
    const int m = row >> 5, k = grp >> 1, half = grp & 1;
    const int o = 8 * grp;
    for (int t = 0; t < taps; ++t) {
        bf16x8 hi, lopart;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = (row < c_n && o + j < cout) ? w[((size_t)(o + j) * C + c_off + row) * taps + (taps - 1 - t)]
                                                        : 0.f;
            hi[j] = bf16_hi(v);
            lopart[j] = bf16_lo(v, hi[j]);
        }
        const size_t at = ((size_t)(m * taps + t) * ks + k) * 64 + 32 * half + (row & 31);
        frags[at] = hi;
        frags[at + (size_t)nfrag * 64] = lopart;
    }
}

// ---- weight gradient -------------------------------------------------------------------------------------

template <int KW>
__global__ void __launch_bounds__(kThreads)
conv_wgrad_kernel(const float* __restrict__ gm, const float* __restrict__ in0, const float* __restrict__ in1,
                  float* __restrict__ partial, WgradGeom P) {
    __shared__ __attribute__((aligned(16))) __bf16 sg[2 * kOT * kGS];       // hi part, lo part
    __shared__ __attribute__((aligned(16))) __bf16 sx[2 * kCT * kXS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    int blk = blockIdx.x;
    const int ct = blk % P.ctiles; blk /= P.ctiles;
    const int og = blk % P.mog; blk /= P.mog;
    const int ti = blk % P.kh;
    const int s = blk / P.kh;
    const int HW = P.H * P.W;
    const int ph = P.kh >> 1, pw = KW >> 1;
    const int o0 = og * kOT, c0 = ct * kCT;
    const bool active = o0 + 32 * wave < P.Cout;

    f32x16 acc[KW];
#pragma unroll
    for (int j = 0; j < KW; ++j) acc[j] = f32x16{};

    const int rows = P.B * P.H;
    const int row_end = min(rows, (s + 1) * P.rps);
    for (int row = s * P.rps; row < row_end; ++row) {
        const int b = row / P.H, y = row - b * P.H;
        const int yy = y + ti - ph;
        if (yy < 0 || yy >= P.H) continue;                  // block-uniform: this tap row reads padding only
        const float* gb = gm + (size_t)b * P.Cout * HW + y * P.W;           // 32-bit offsets inside an image
        const float* b0 = in0 + (size_t)b * P.C0 * HW + yy * P.W;
        const float* b1 = P.C1 ? in1 + (size_t)b * P.C1 * HW + yy * P.W : in0;
        for (int x0 = 0; x0 < P.W; x0 += kKP) {
            __syncthreads();                                // the previous segment's reads are done
            for (int id = tid; id < kOT * (kKP / 2); id += kThreads) {
                const int ol = id / (kKP / 2), p = 2 * (id - ol * (kKP / 2));
                const int o = o0 + ol;
                float v[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int xx = x0 + p + j;
                    v[j] = (o < P.Cout && xx < P.W) ? gb[o * HW + xx] : 0.f;
                }
                bf16x2 hi, lo;
                split<3>(v, hi, lo);
                *reinterpret_cast<bf16x2*>(&sg[ol * kGS + p]) = hi;
                *reinterpret_cast<bf16x2*>(&sg[kOT * kGS + ol * kGS + p]) = lo;
            }
            for (int id = tid; id < kCT * (kXS / 2); id += kThreads) {
                const int cl = id / (kXS / 2), q = 2 * (id - cl * (kXS / 2));
                const int c = c0 + cl;
                float v[2] = {0.f, 0.f};
                if (c < P.C) {
                    const float* src = c < P.C0 ? b0 + c * HW : b1 + (c - P.C0) * HW;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int xx = x0 + q + j - pw;
                        if (xx >= 0 && xx < P.W) v[j] = src[xx];
                    }
                }
                bf16x2 hi, lo;
                split<3>(v, hi, lo);
                *reinterpret_cast<bf16x2*>(&sx[cl * kXS + q]) = hi;
                *reinterpret_cast<bf16x2*>(&sx[kCT * kXS + cl * kXS + q]) = lo;
            }
            __syncthreads();
            if (!active) continue;
            const int ksteps = (min(kKP, P.W - x0) + 15) >> 4;
            for (int k = 0; k < ksteps; ++k) {
                const __bf16* pa = &sg[(32 * wave + r) * kGS + 16 * k + 8 * hh];
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(pa);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(pa + kOT * kGS);
#pragma unroll
                for (int j = 0; j < KW; ++j) {
                    const __bf16* pb = &sx[r * kXS + 16 * k + 8 * hh + j];  // last element read: 72 r + 69
                    bf16x8 bh, bl;
                    memcpy(&bh, pb, sizeof(bh));                            // 2-byte aligned
                    memcpy(&bl, pb + kCT * kXS, sizeof(bl));
                    mma<3>(acc[j], ah, al, bh, bl);
                }
            }
        }
    }
    if (!active) return;

    // register i of lane (r, hh): output channel o0 + 32 wave + acc_row(i, hh), input channel c0 + r
    const int c = c0 + r;
    if (c >= P.C) return;
    const int taps = P.kh * KW;
    float* pp = partial + (size_t)s * P.Cout * P.C * taps;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int o = o0 + 32 * wave + acc_row(i, hh);
        if (o >= P.Cout) continue;
        float* dst = pp + ((size_t)o * P.C + c) * taps + ti * KW;
#pragma unroll
        for (int j = 0; j < KW; ++j) dst[j] = acc[j][i];
    }
}

// gW[e] = the partials of element e in slice order
__global__ void __launch_bounds__(256)
conv_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gw, int nslices, long long total) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = partial[e];
    for (int n = 1; n < nslices; ++n) s += partial[(size_t)n * total + e];
    gw[e] = s;
}

// ---- host --------------------------------------------------------------------------------------------

int wgrad_slices(int batch, int c, int cout, int kh, int height) {
    const long long per = (long long)((cout + kOT - 1) / kOT) * ((c + kCT - 1) / kCT) * kh;
    const long long want = (kTargetGroups + per - 1) / per;
    const long long rows = (long long)batch * height;
    return (int)std::max(1ll, std::min(std::min(rows, (long long)kMaxSlices), want));
}

struct BwdWork {
    float* gm;
    char* frags[2];
    float* zero[2];
    float* partial;
    size_t bytes;
};

// the carve-up of the workspace from `base` (already aligned): gm, per source the packed W' and its zero bias, the
// weight gradient's partials
BwdWork bwd_carve(char* base, int batch, int c0, int c1, int cout, int kh, int kw, int height, int width) {
    BwdWork Wk{};
    const size_t n = (size_t)height * width;
    size_t at = 0;
    Wk.gm = reinterpret_cast<float*>(base + at); at += align256((size_t)batch * cout * n * sizeof(float));
    const int cs[2] = {c0, c1};
    for (int s = 0; s < 2; ++s) {
        if (!cs[s]) continue;
        Wk.frags[s] = base + at; at += conv_fragment_bytes(cout, cs[s], kh, kw);
        Wk.zero[s] = reinterpret_cast<float*>(base + at); at += align256((size_t)(cs[s] + 31) / 32 * 32 * sizeof(float));
    }
    Wk.partial = reinterpret_cast<float*>(base + at);
    at += align256((size_t)wgrad_slices(batch, c0 + c1, cout, kh, height) * cout * (c0 + c1) * kh * kw * sizeof(float));
    Wk.bytes = at;
    return Wk;
}

// which kernels a call launches: the mask / bias pass (and whether it writes gm), the data gradient of each
// source, the weight gradient.  rmd_conv2d_backward and rmd_conv2d_backward_kernels both read it.
struct BwdPlan {
    bool mask, write_gm, gx[2], gw;
};

BwdPlan bwd_plan(bool want_in0, bool want_in1, bool want_weight, bool want_bias, int act) {
    BwdPlan pl;
    const bool need_gm = want_in0 || want_in1 || want_weight;
    pl.write_gm = act && need_gm;
    pl.mask = pl.write_gm || want_bias;
    pl.gx[0] = want_in0; pl.gx[1] = want_in1; pl.gw = want_weight;
    return pl;
}

template <int KW>
void wgrad_launch(const float* gm, const float* in0, const float* in1, float* partial, const WgradGeom& P,
                  hipStream_t st) {
    const int grid = P.ctiles * P.mog * P.kh * P.nslices;
    conv_wgrad_kernel<KW><<<grid, kThreads, 0, st>>>(gm, in0, in1, partial, P);
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" int rmd_conv2d_backward_supported(int kh, int kw, int c0, int c1, int cout) {
    return rmd_conv2d_supported(kh, kw, c0, c1, cout);
}

extern "C" size_t rmd_conv2d_backward_workspace_bytes(int batch, int c0, int c1, int cout, int kh, int kw, int height,
                                                      int width) {
    if (batch < 1 || height < 1 || width < 1 || !rmd_conv2d_backward_supported(kh, kw, c0, c1, cout)) return 0;
    return bwd_carve(nullptr, batch, c0, c1, cout, kh, kw, height, width).bytes + 256;
}

extern "C" const char* rmd_conv2d_backward_kernels(int want_in0, int want_in1, int want_weight, int want_bias, int act) {
    static thread_local char text[160];
    const BwdPlan pl = bwd_plan(want_in0, want_in1, want_weight, want_bias, act);
    snprintf(text, sizeof(text), "%s%s%s%s", pl.mask ? (pl.write_gm ? "mask_bias+gm " : "mask_bias ") : "",
             pl.gx[0] ? "pack0 conv0 " : "", pl.gx[1] ? "pack1 conv1 " : "", pl.gw ? "wgrad reduce " : "");
    const size_t n = strlen(text);
    if (n) text[n - 1] = 0;
    return text;
}

// The backward, under autograd, of the convolutions of raft.py:193-225, 262-273, 299-331.
extern "C" int rmd_conv2d_backward(const float* grad, const float* y, const float* in0, const float* in1,
                                   const float* weight, float* grad_in0, float* grad_in1, float* grad_weight,
                                   float* grad_bias, void* workspace, int batch, int c0, int c1, int cout, int kh,
                                   int kw, int height, int width, int act, void* stream) {
    const char* name = "rmd_conv2d_backward";
    RMD_REQUIRE(grad && in0 && weight && workspace, RMD_ERR_ARG, "%s: null pointer", name);
    RMD_REQUIRE(act == 0 || act == 1, RMD_ERR_ARG, "%s: act must be 0 (none) or 1 (ReLU), got %d", name, act);
    RMD_REQUIRE((act == 0) == (y == nullptr), RMD_ERR_ARG, "%s: y must be given exactly when act is 1 (ReLU)", name);
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0 && (long long)batch * height <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: bad sizes", name);
    RMD_REQUIRE(rmd_conv2d_backward_supported(kh, kw, c0, c1, cout), RMD_ERR_SHAPE,
                "%s: unsupported (kernel %dx%d, channels %d + %d -> %d): kernel sides odd in 1..7, C0 >= 1, "
                "C1 >= 0, C0 + C1 <= 512, Cout in 1..1024", name, kh, kw, c0, c1, cout);
    RMD_REQUIRE((c1 == 0) == (in1 == nullptr), RMD_ERR_ARG, "%s: in1 must be given exactly when C1 > 0", name);
    RMD_REQUIRE(c1 > 0 || !grad_in1, RMD_ERR_ARG, "%s: grad_in1 without a second source (C1 = 0)", name);
    const int c = c0 + c1;
    const long long n = (long long)height * width;
    // 32-bit lane offsets into one image's maps, 64-bit everywhere else
    RMD_REQUIRE(n * c < (1ll << 30) && n * cout < (1ll << 30), RMD_ERR_SHAPE, "%s: %lld pixels x %d (%d) channels per image",
                name, n, c, cout);
    const long long tiles = (long long)batch * ((height + 3) / 4) * ((width + 31) / 32);
    RMD_REQUIRE(tiles * ((c + 127) / 128) <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: too many pixel tiles (batch=%d height=%d width=%d)", name, batch, height, width);
    const size_t fb = sizeof(float);
    const size_t gbytes = (size_t)batch * cout * n * fb, b0 = (size_t)batch * c0 * n * fb, b1 = (size_t)batch * c1 * n * fb;
    const size_t wbytes = (size_t)cout * c * kh * kw * fb, bbytes = (size_t)cout * fb;
    const size_t work = rmd_conv2d_backward_workspace_bytes(batch, c0, c1, cout, kh, kw, height, width);
    struct Span {
        const void* p;
        size_t bytes;
    };
    const Span ins[5] = {{grad, gbytes}, {y, gbytes}, {in0, b0}, {in1, b1}, {weight, wbytes}};
    const Span outs[5] = {{grad_in0, b0}, {grad_in1, b1}, {grad_weight, wbytes}, {grad_bias, bbytes}, {workspace, work}};
    for (int o = 0; o < 5; ++o) {
        if (!outs[o].p) continue;
        for (int i = 0; i < 5; ++i)
            RMD_REQUIRE(!(ins[i].p && overlap(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes)), RMD_ERR_ARG,
                        "%s: %s overlaps an input", name, o == 4 ? "workspace" : "a gradient");
        for (int q = o + 1; q < 5; ++q)
            RMD_REQUIRE(!(outs[q].p && overlap(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes)), RMD_ERR_ARG,
                        "%s: %s overlaps a gradient", name, q == 4 ? "workspace" : "a gradient");
    }
    if (!grad_in0 && !grad_in1 && !grad_weight && !grad_bias) {
        clear_error();
        return RMD_OK;
    }

    hipStream_t st = as_stream(stream);
    const BwdWork Wk = bwd_carve(reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(workspace))), batch, c0, c1,
                                 cout, kh, kw, height, width);
    const BwdPlan pl = bwd_plan(grad_in0, grad_in1, grad_weight, grad_bias, act);
    const float* gm = pl.write_gm ? Wk.gm : grad;
    if (pl.mask)
        conv_mask_bias_kernel<<<cout, kThreads, 0, st>>>(grad, y, pl.write_gm ? Wk.gm : nullptr, grad_bias, batch, cout,
                                                         (int)n);
    float* gx[2] = {grad_in0, grad_in1};
    const int cs[2] = {c0, c1}, offs[2] = {0, c0};
    const int taps = kh * kw;
    for (int s = 0; s < 2; ++s) {
        if (!gx[s]) continue;
        const int mo = (cs[s] + 31) / 32, ks = (cout + 15) / 16, nfrag = mo * taps * ks;
        const int threads = mo * 32 * 2 * ks;
        conv_pack_transposed_kernel<<<(threads + 255) / 256, 256, 0, st>>>(
            weight, cout, c, offs[s], cs[s], taps, mo, ks, nfrag, reinterpret_cast<bf16x8*>(Wk.frags[s]), Wk.zero[s]);
        conv_run_prepacked(gm, Wk.frags[s], Wk.zero[s], gx[s], batch, cout, cs[s], kh, kw, height, width, st);
    }
    if (grad_weight) {
        WgradGeom P;
        P.B = batch; P.C0 = c0; P.C1 = c1; P.C = c; P.Cout = cout; P.kh = kh; P.H = height; P.W = width;
        P.mog = (cout + kOT - 1) / kOT; P.ctiles = (c + kCT - 1) / kCT;
        P.nslices = wgrad_slices(batch, c, cout, kh, height);
        P.rps = (batch * height + P.nslices - 1) / P.nslices;
        switch (kw) {
            case 1: wgrad_launch<1>(gm, in0, in1, Wk.partial, P, st); break;
            case 3: wgrad_launch<3>(gm, in0, in1, Wk.partial, P, st); break;
            case 5: wgrad_launch<5>(gm, in0, in1, Wk.partial, P, st); break;
            default: wgrad_launch<7>(gm, in0, in1, Wk.partial, P, st); break;
        }
        const long long total = (long long)cout * c * taps;
        conv_wgrad_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(Wk.partial, grad_weight, P.nslices,
                                                                                total);
    }
    return check_launch(name);
}
