// conv.hip — fused k x k convolution (inference): a stride-1, "same"-padded dense convolution over the channel
// concatenation of up to two fp32 NCHW maps as one MFMA implicit GEMM, bias and ReLU in its epilogue, written
// into a channel slice of an fp32 NCHW destination.
//
// Replaces (qzed/raft-meets-dicl v2) the convolutions next to the recurrent unit in every iteration:
// BasicMotionEncoder (src/models/impls/raft.py:193-225), FlowHead (raft.py:262-273) and the mask head of
// Up8Network (raft.py:299-331).
//   out[b, off + o, y, x] = act(bias[o] + sum_{c,i,j} W[o, c, i, j] in[b, c, y + i - kh/2, x + j - kw/2])
//   in = cat(in0 (C0 channels), in1 (C1 channels, may be absent)), zero outside the map
// Neither the concatenation, an unfolded tensor nor a pre-activation is written to memory, and because the
// destination is a channel slice, the concatenation of two convolutions' results is never made either.
//
// The GEMM is that of gru.hip generalised: M = output channels, N = pixels, K = kh kw C; v_mfma_f32_32x32x16_bf16
// with the weights as the A operand, the pixels on the MFMA column (lane & 31) and the split-bf16 arithmetic of
// mfma_bf16.h.  A workgroup owns a kRows x 32 pixel tile of one image (each row of it is one MFMA pixel tile) and
// stages, per chunk of KC input channels, the (kRows + kh - 1) x (32 + kw - 1) positions its taps read through
// LDS as bf16 (hi, and the bf16 of the residual in the three-product mode), position-major with the channels of a
// position contiguous: a lane's B fragment of a k-step is one 16-byte LDS read, and tap (i, j) is the same read
// shifted by i staged rows and j positions.  A 3 x 3 kernel so stages 6 x 34 = 1.6 x its 128 outputs (a 1 x 64
// row segment would stage 3 x 66 = 3.1 x).  Positions outside the map and channels past C0 + C1 are staged as
// zeros: the former is the convolution's padding, the latter meets the zero weights the pack kernel writes for
// the padded part of the last k-step.  No channel count needs to be a multiple of anything.
//
// The weights are packed once per call into A fragments in (32-row tile, tap, k-step) order, zero rows past Cout,
// and read from global memory (L2).  Wave w of a workgroup owns MT 32-row tiles (MT = 1: Cout <= 128, MT = 2
// otherwise) for all kRows x 32 pixels, so a fragment is loaded once per workgroup and used for kRows pixel
// tiles; a workgroup covers 128 MT output channels and wider convolutions take several workgroups per pixel tile.
// A convolution of at most 64 output channels (one or two 32-row tiles) splits the pixel rows over the waves.
//
// The summation order of an output is fixed (channel chunk, tap row, tap column, k-step; small products first)
// and does not depend on the batch, on the other tiles or on the slice offset: results are bitwise repeatable
// and per-sample independent.

#include "conv_internal.h"
#include "mfma_bf16.h"

namespace rmd {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRows = 4, kCols = 32;        // pixel tile of a workgroup: kRows MFMA pixel tiles of one row each
// channels per staged chunk KC: 64 (four k-steps) where both staged parts of it fit kLdsBytes — up to 3 x 5 taps,
// so every 1 x 1 and 3 x 3 convolution: half the barriers per MFMA of KC = 32 —, else 32 (5 x 3 up to 7 x 7).  A
// position holds KC + 8 bf16: an odd number of 16-byte slots (see gru.hip)
constexpr int kLdsBytes = 64 * 1024;        // dynamic LDS of a workgroup: two workgroups per CU
constexpr int kMaxK = 7, kMaxC = 512, kMaxCout = 1024;
constexpr int kAlign = 256;

struct ConvGeom {
    int B, C0, C1, C, Cout, kh, kw, H, W;
    int out_total, off;     // channels of the destination, first channel of the slice
    int act;                // 0: none, 1: ReLU
    int mo, ks;             // 32-row tiles, 16-channel k-steps of one tap
    int taps;
    int tiles_x, tiles_y, mpass;
    int slots;              // staged positions
    int kc;                 // channels per staged chunk
    int nfrag;              // A fragments of one part (hi or lo)
};

inline bool conv_supported(int kh, int kw, int c0, int c1, int cout) {
    return kh >= 1 && kh <= kMaxK && (kh & 1) && kw >= 1 && kw <= kMaxK && (kw & 1) && c0 >= 1 && c1 >= 0 &&
           c0 + c1 <= kMaxC && cout >= 1 && cout <= kMaxCout;
}

// ---- weights -> A fragments --------------------------------------------------------------------------

// fragment (m * taps + t) * ks + k, lane l = (row 32 m + (l & 31), half l >> 5), element j:
// W[row][16 k + 8 (l >> 5) + j][tap t] of the (Cout, C, kh, kw) weight, zero for row >= Cout or a channel >= C.
// nfrag hi fragments, then (if `lo`) nfrag fragments of the bf16 of the residual.  One thread per (row, group of
// 8 channels): it reads the 8 taps floats of its group, which are contiguous in memory and follow those of the
// previous thread's group.
__global__ void __launch_bounds__(256)
conv_pack_kernel(const float* __restrict__ w, int cout, int C, int taps, int mo, int ks, int nfrag, int lo,
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

template <int NP, int MT, int KC>
__global__ void __launch_bounds__(kThreads, 2)
conv_kernel(const float* __restrict__ in0, const float* __restrict__ in1, const bf16x8* __restrict__ frags,
            const float* __restrict__ bias, float* __restrict__ out, ConvGeom P) {
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
    const int x0 = tx * kCols, y0 = ty * kRows;
    const int HW = P.H * P.W;
    const int sw = kCols + P.kw - 1;                        // staged positions of a row
    const int py = P.kh >> 1, px = P.kw >> 1;
    const float* b0 = in0 + (size_t)b * P.C0 * HW;         // wave-uniform bases, 32-bit offsets inside an image
    const float* b1 = P.C1 ? in1 + (size_t)b * P.C1 * HW : in0;
    // wave -> 32-row output tiles and pixel rows.  With four tiles or more in a pass a wave owns MT tiles for all
    // kRows rows; a convolution of one or two tiles (Cout <= 64) splits the rows over the waves instead of leaving
    // three or two of them idle: tile wave % mo, rows mo (wave / mo) .. + mo.  An output's summation is the same.
    const bool split_rows = MT == 1 && P.mo <= 2;
    const int m0 = split_rows ? wave % P.mo : (pass * kWaves + wave) * MT;      // first 32-row tile of this wave
    const int nlo = split_rows ? wave / P.mo * P.mo : 0, nhi = split_rows ? nlo + P.mo : kRows;
    const bool active = m0 < P.mo;
    const int lopart = P.slots * kStride;

    f32x16 acc[MT][kRows];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < kRows; ++n) acc[m][n] = f32x16{};

    for (int c0 = 0; c0 < P.C; c0 += KC) {
        const int ksteps = (min(KC, P.C - c0) + 15) >> 4;
        __syncthreads();                                    // the previous chunk's reads are done
        for (int id = tid; id < 2 * ksteps * P.slots; id += kThreads) {
            const int grp = id / P.slots, s = id - grp * P.slots;
            const int sy = s / sw, sx = s - sy * sw;
            const int yy = y0 + sy - py, xx = x0 + sx - px;
            const bool inside = yy >= 0 && yy < P.H && xx >= 0 && xx < P.W;
            const int c = c0 + 8 * grp;
            const int at = inside ? yy * P.W + xx : 0;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int cc = c + j;                       // a group may hold the seam and the padded tail
                const bool have = inside && cc < P.C;
                const float* src = cc < P.C0 ? b0 + cc * HW : b1 + (cc - P.C0) * HW;
                v[j] = have ? src[at] : 0.f;
            }
            bf16x8 hi, lo;
            split<NP>(v, hi, lo);
            *reinterpret_cast<bf16x8*>(&sm[s * kStride + 8 * grp]) = hi;
            if constexpr (NP == 3) *reinterpret_cast<bf16x8*>(&sm[lopart + s * kStride + 8 * grp]) = lo;
        }
        __syncthreads();
        if (!active) continue;
        const int kbase = c0 >> 4;
        for (int i = 0; i < P.kh; ++i) {
            for (int j = 0; j < P.kw; ++j) {
                const int t = i * P.kw + j;
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
                        for (int n = 0; n < kRows; ++n) {
                            if (n >= nlo && n < nhi && (n == 0 || y0 + n < P.H)) {
                                const __bf16* p = &sm[((n + i) * sw + r + j) * kStride + 16 * k + 8 * hh];
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
    if (x >= P.W) return;
    float* ob = out + ((size_t)b * P.out_total + P.off) * HW;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ch = 32 * (m0 + m) + acc_row(i, hh);
            if (ch >= P.Cout) continue;
            const float bv = bias[ch];
#pragma unroll
            for (int n = 0; n < kRows; ++n) {
                if (n < nlo || n >= nhi || y0 + n >= P.H) continue;
                float v = acc[m][n][i] + bv;
                if (P.act) v = v < 0.f ? 0.f : v;           // keeps NaN, as torch.relu (fmaxf would not)
                ob[(size_t)ch * HW + (y0 + n) * P.W + x] = v;
            }
        }
    }
}

// out[b, off + c] = src[b, c] for the nc channels of src: the copy of `flow` into the encoder's result
__global__ void __launch_bounds__(256)
conv_copy_kernel(const float* __restrict__ src, float* __restrict__ out, int nc, int HW, int out_total, int off,
                 long long total) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const long long per = (long long)nc * HW;
    const long long b = id / per, rest = id - b * per;
    out[(b * out_total + off) * HW + rest] = src[id];
}

ConvGeom conv_geom(int batch, int c0, int c1, int cout, int kh, int kw, int height, int width, int out_total,
                   int off, int act) {
    ConvGeom P;
    P.B = batch; P.C0 = c0; P.C1 = c1; P.C = c0 + c1; P.Cout = cout; P.kh = kh; P.kw = kw; P.H = height; P.W = width;
    P.out_total = out_total; P.off = off; P.act = act;
    P.mo = (cout + 31) / 32; P.ks = (P.C + 15) / 16; P.taps = kh * kw;
    P.tiles_x = (width + kCols - 1) / kCols; P.tiles_y = (height + kRows - 1) / kRows;
    const int per_pass = kWaves * (cout <= 32 * kWaves ? 1 : 2);
    P.mpass = (P.mo + per_pass - 1) / per_pass;
    P.slots = (kRows + kh - 1) * (kCols + kw - 1);
    P.kc = 2 * P.slots * (64 + 8) * (int)sizeof(__bf16) <= kLdsBytes ? 64 : 32;
    P.nfrag = P.mo * P.taps * P.ks;
    return P;
}

// bytes of the packed weights of one convolution: both parts, a multiple of kAlign
size_t conv_packed_bytes(int c, int cout, int kh, int kw) {
    const size_t nfrag = (size_t)((cout + 31) / 32) * kh * kw * ((c + 15) / 16);
    return nfrag * 64 * sizeof(bf16x8) * 2;
}

// the checks of one convolution of entry point `name`, before any launch
int conv_check(const char* name, const float* in0, const float* in1, const float* weight, const float* bias,
               const float* out, int batch, int c0, int c1, int cout, int kh, int kw, int height, int width,
               int out_total, int off, int act, int compute) {
    RMD_REQUIRE(in0 && weight && bias && out, RMD_ERR_ARG, "%s: null pointer", name);
    RMD_REQUIRE(compute == RMD_BF16X3 || compute == RMD_BF16, RMD_ERR_ARG,
                "%s: compute must be RMD_BF16X3 or RMD_BF16, got %d", name, compute);
    RMD_REQUIRE(act == 0 || act == 1, RMD_ERR_ARG, "%s: act must be 0 (none) or 1 (ReLU), got %d", name, act);
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(conv_supported(kh, kw, c0, c1, cout), RMD_ERR_SHAPE,
                "%s: unsupported (kernel %dx%d, channels %d + %d -> %d): kernel sides odd in 1..7, C0 >= 1, "
                "C1 >= 0, C0 + C1 <= 512, Cout in 1..1024", name, kh, kw, c0, c1, cout);
    RMD_REQUIRE((c1 == 0) == (in1 == nullptr), RMD_ERR_ARG, "%s: in1 must be given exactly when C1 > 0", name);
    RMD_REQUIRE(off >= 0 && out_total >= off + cout, RMD_ERR_SHAPE,
                "%s: the slice %d..%d does not fit the destination's %d channels", name, off, off + cout, out_total);
    const long long n = (long long)height * width;
    // 32-bit lane offsets into one image's maps, 64-bit everywhere else
    RMD_REQUIRE(n * (c0 + c1) < (1ll << 30) && n * out_total < (1ll << 30), RMD_ERR_SHAPE,
                "%s: %lld pixels x %d (%d) channels per image", name, n, c0 + c1, out_total);
    const long long tiles = (long long)batch * ((height + kRows - 1) / kRows) * ((width + kCols - 1) / kCols);
    RMD_REQUIRE(tiles * ((cout + 127) / 128) <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: too many pixel tiles (batch=%d height=%d width=%d)", name, batch, height, width);
    const size_t obytes = (size_t)batch * out_total * n * sizeof(float);
    const size_t b0 = (size_t)batch * c0 * n * sizeof(float), b1 = (size_t)batch * c1 * n * sizeof(float);
    const size_t wbytes = (size_t)cout * (c0 + c1) * kh * kw * sizeof(float);
    RMD_REQUIRE(!overlap(out, obytes, in0, b0) && !(in1 && overlap(out, obytes, in1, b1)) &&
                    !overlap(out, obytes, weight, wbytes) && !overlap(out, obytes, bias, cout * sizeof(float)),
                RMD_ERR_ARG, "%s: out overlaps an input", name);
    return RMD_OK;
}

template <int NP, int KC>
void conv_launch(const float* in0, const float* in1, const bf16x8* frags, const float* bias, float* out,
                 const ConvGeom& P, hipStream_t st) {
    const int grid = P.B * P.tiles_y * P.tiles_x * P.mpass;
    // at most kLdsBytes: conv_geom's choice for KC = 64, 2 x 380 x 40 x 2 = 60800 bytes for 7 x 7 with KC = 32
    const size_t lds = (size_t)(NP == 3 ? 2 : 1) * P.slots * (KC + 8) * sizeof(__bf16);
    if (P.Cout <= 32 * kWaves) conv_kernel<NP, 1, KC><<<grid, kThreads, lds, st>>>(in0, in1, frags, bias, out, P);
    else conv_kernel<NP, 2, KC><<<grid, kThreads, lds, st>>>(in0, in1, frags, bias, out, P);
}

// packs `weight` at `frags` and runs the convolution
void conv_run(const float* in0, const float* in1, const float* weight, const float* bias, float* out, void* frags,
              const ConvGeom& P, int compute, hipStream_t st) {
    const bool lo = compute == RMD_BF16X3;
    bf16x8* fr = reinterpret_cast<bf16x8*>(frags);
    const int threads = P.mo * 32 * 2 * P.ks;
    conv_pack_kernel<<<(threads + 255) / 256, 256, 0, st>>>(weight, P.Cout, P.C, P.taps, P.mo, P.ks, P.nfrag,
                                                           lo ? 1 : 0, fr);
    if (lo) {
        if (P.kc == 64) conv_launch<3, 64>(in0, in1, fr, bias, out, P, st);
        else conv_launch<3, 32>(in0, in1, fr, bias, out, P, st);
    } else {
        if (P.kc == 64) conv_launch<1, 64>(in0, in1, fr, bias, out, P, st);
        else conv_launch<1, 32>(in0, in1, fr, bias, out, P, st);
    }
}

// ---- BasicMotionEncoder (raft.py:193-225) ------------------------------------------------------------

constexpr int kEncC1 = 256, kEncC2 = 192, kEncF1 = 128, kEncF2 = 64, kEncOut = 126, kEncFlow = 2;
constexpr int kEncMid = kEncC2 + kEncF2, kEncTotal = kEncOut + kEncFlow;

struct EncWork {
    char* frags[5];
    float *cor, *flo, *mid;
    size_t bytes;
};

// the carve-up of the encoder's workspace from `base` (already aligned): five packed weights, then the maps
EncWork enc_carve(char* base, int batch, int corr_planes, int height, int width) {
    const size_t n = (size_t)batch * height * width * sizeof(float);
    const size_t packed[5] = {conv_packed_bytes(corr_planes, kEncC1, 1, 1), conv_packed_bytes(kEncC1, kEncC2, 3, 3),
                              conv_packed_bytes(kEncFlow, kEncF1, 7, 7), conv_packed_bytes(kEncF1, kEncF2, 3, 3),
                              conv_packed_bytes(kEncMid, kEncOut, 3, 3)};
    EncWork Wk;
    size_t at = 0;
    for (int i = 0; i < 5; ++i) {
        Wk.frags[i] = base + at;
        at += packed[i];
    }
    Wk.cor = reinterpret_cast<float*>(base + at); at += align256(n * kEncC1);
    Wk.flo = reinterpret_cast<float*>(base + at); at += align256(n * kEncF1);
    Wk.mid = reinterpret_cast<float*>(base + at); at += align256(n * kEncMid);
    Wk.bytes = at;
    return Wk;
}

}  // namespace

// ---- the door of conv_backward.hip (conv_internal.h) -------------------------------------------------

size_t conv_fragment_bytes(int c, int cout, int kh, int kw) { return conv_packed_bytes(c, cout, kh, kw); }

void conv_run_prepacked(const float* in, const void* frags, const float* bias, float* out, int batch, int c, int cout,
                        int kh, int kw, int height, int width, hipStream_t st) {
    const ConvGeom P = conv_geom(batch, c, 0, cout, kh, kw, height, width, cout, 0, 0);
    const bf16x8* fr = reinterpret_cast<const bf16x8*>(frags);
    if (P.kc == 64) conv_launch<3, 64>(in, nullptr, fr, bias, out, P, st);
    else conv_launch<3, 32>(in, nullptr, fr, bias, out, P, st);
}

}  // namespace rmd

using namespace rmd;

extern "C" int rmd_conv2d_supported(int kh, int kw, int c0, int c1, int cout) {
    return conv_supported(kh, kw, c0, c1, cout) ? 1 : 0;
}

extern "C" size_t rmd_conv2d_workspace_bytes(int c0, int c1, int cout, int kh, int kw) {
    if (!conv_supported(kh, kw, c0, c1, cout)) return 0;
    return conv_packed_bytes(c0 + c1, cout, kh, kw) + kAlign;
}

extern "C" int rmd_conv2d(const float* in0, const float* in1, const float* weight, const float* bias, float* out,
                          void* workspace, int batch, int c0, int c1, int cout, int kh, int kw, int height, int width,
                          int out_channels_total, int out_offset, int act, int compute, void* stream) {
    RMD_REQUIRE(workspace, RMD_ERR_ARG, "rmd_conv2d: null workspace");
    if (int rc = conv_check("rmd_conv2d", in0, in1, weight, bias, out, batch, c0, c1, cout, kh, kw, height, width,
                            out_channels_total, out_offset, act, compute))
        return rc;
    const size_t n = (size_t)height * width * sizeof(float);
    const size_t wbytes = rmd_conv2d_workspace_bytes(c0, c1, cout, kh, kw);
    RMD_REQUIRE(!overlap(workspace, wbytes, in0, batch * c0 * n) && !(in1 && overlap(workspace, wbytes, in1, batch * c1 * n)) &&
                    !overlap(workspace, wbytes, out, batch * out_channels_total * n) &&
                    !overlap(workspace, wbytes, weight, (size_t)cout * (c0 + c1) * kh * kw * sizeof(float)) &&
                    !overlap(workspace, wbytes, bias, cout * sizeof(float)),
                RMD_ERR_ARG, "rmd_conv2d: workspace overlaps a tensor");
    const ConvGeom P = conv_geom(batch, c0, c1, cout, kh, kw, height, width, out_channels_total, out_offset, act);
    conv_run(in0, in1, weight, bias, out, reinterpret_cast<void*>(align256(reinterpret_cast<size_t>(workspace))), P,
             compute, as_stream(stream));
    return check_launch("rmd_conv2d");
}

extern "C" size_t rmd_motion_encoder_workspace_bytes(int batch, int corr_planes, int height, int width) {
    if (batch < 1 || height < 1 || width < 1 || !conv_supported(1, 1, corr_planes, 0, kEncC1)) return 0;
    return enc_carve(nullptr, batch, corr_planes, height, width).bytes + kAlign;
}

extern "C" int rmd_motion_encoder(const float* flow, const float* corr, const float* const* weights,
                                  const float* const* biases, float* out, void* workspace, int batch, int corr_planes,
                                  int height, int width, int compute, void* stream) {
    const char* name = "rmd_motion_encoder";
    RMD_REQUIRE(flow && corr && weights && biases && out && workspace, RMD_ERR_ARG, "%s: null pointer", name);
    for (int g = 0; g < 5; ++g) RMD_REQUIRE(weights[g] && biases[g], RMD_ERR_ARG, "%s: null weight or bias %d", name, g);
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(conv_supported(1, 1, corr_planes, 0, kEncC1), RMD_ERR_SHAPE, "%s: corr_planes %d not in 1..512", name,
                corr_planes);
    const size_t n = (size_t)batch * height * width * sizeof(float);
    const size_t wbytes = rmd_motion_encoder_workspace_bytes(batch, corr_planes, height, width);
    const EncWork Wk = enc_carve(reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(workspace))), batch,
                                 corr_planes, height, width);
    // the five convolutions: in0, in1, C0, C1, Cout, k, destination, its channels, slice offset
    struct Step {
        const float *in0, *in1;
        int c0, c1, cout, k;
        float* dst;
        int total, off;
    } steps[5] = {
        {corr, nullptr, corr_planes, 0, kEncC1, 1, Wk.cor, kEncC1, 0},
        {Wk.cor, nullptr, kEncC1, 0, kEncC2, 3, Wk.mid, kEncMid, 0},
        {flow, nullptr, kEncFlow, 0, kEncF1, 7, Wk.flo, kEncF1, 0},
        {Wk.flo, nullptr, kEncF1, 0, kEncF2, 3, Wk.mid, kEncMid, kEncC2},
        {Wk.mid, nullptr, kEncMid, 0, kEncOut, 3, out, kEncTotal, 0},
    };
    for (int g = 0; g < 5; ++g) {
        const Step& s = steps[g];
        if (int rc = conv_check(name, s.in0, s.in1, weights[g], biases[g], s.dst, batch, s.c0, s.c1, s.cout, s.k, s.k,
                                height, width, s.total, s.off, 1, compute))
            return rc;
        RMD_REQUIRE(!overlap(workspace, wbytes, weights[g], (size_t)s.cout * (s.c0 + s.c1) * s.k * s.k * sizeof(float)) &&
                        !overlap(workspace, wbytes, biases[g], s.cout * sizeof(float)),
                    RMD_ERR_ARG, "%s: workspace overlaps weight or bias %d", name, g);
    }
    RMD_REQUIRE(!overlap(out, n * kEncTotal, flow, n * kEncFlow) && !overlap(out, n * kEncTotal, corr, n * corr_planes),
                RMD_ERR_ARG, "%s: out overlaps an input", name);
    RMD_REQUIRE(!overlap(workspace, wbytes, flow, n * kEncFlow) && !overlap(workspace, wbytes, corr, n * corr_planes) &&
                    !overlap(workspace, wbytes, out, n * kEncTotal),
                RMD_ERR_ARG, "%s: workspace overlaps a tensor", name);
    hipStream_t st = as_stream(stream);
    for (int g = 0; g < 5; ++g) {
        const Step& s = steps[g];
        const ConvGeom P = conv_geom(batch, s.c0, s.c1, s.cout, s.k, s.k, height, width, s.total, s.off, 1);
        conv_run(s.in0, s.in1, weights[g], biases[g], s.dst, Wk.frags[g], P, compute, st);
    }
    const long long total = (long long)batch * kEncFlow * height * width;
    conv_copy_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(flow, out, kEncFlow, height * width, kEncTotal,
                                                                      kEncOut, total);
    return check_launch(name);
}
