// gru.hip — fused SepConvGRU (inference): the six 1x5 / 5x1 convolutions of the recurrent unit as MFMA
// implicit GEMMs with the sigmoid / tanh / gating in their epilogues.
//
// Replaces (qzed/raft-meets-dicl v2) SepConvGru.forward (src/models/impls/raft.py:228-259).  One half-step
// along one axis (axis 0: 1x5 along W, padding (0, 2); axis 1: 5x1 along H, padding (2, 0)):
//   hx = [h ; x]    z = sigmoid(Wz * hx + bz)    r = sigmoid(Wr * hx + br)
//   q = tanh(Wq * [r.h ; x] + bq)                h' = (1 - z) h + z q
// Neither cat(h, x), an unfolded tensor nor a pre-activation is written to memory; between the gate kernel
// (z and r together) and the candidate kernel (q and the gating) only z and r.h pass through the workspace.
//
// Each convolution is a GEMM with M = output channels, N = pixels, K = 5 (Hd + Xd); v_mfma_f32_32x32x16_bf16
// with the weights as the A operand and the pixels on the MFMA column (lane & 31), the split-bf16 arithmetic
// of mfma_bf16.h.  The B operand is an implicit im2col: a workgroup owns a segment of kTile
// pixels of one image row and stages, per chunk of KC input channels, the positions its five taps read
// (kTile + 4 along the row for axis 0, five row segments for axis 1) through LDS as bf16 (hi, and the bf16
// of the residual in the three-product mode), position-major with the channels of a position contiguous:
// a lane's B fragment of a k-step (channels 8 hh .. 8 hh + 7 of 16) is one 16-byte LDS read, and tap t is
// the same read shifted by t positions (axis 0) or t row segments (axis 1).  Positions outside the map are
// staged as zeros, which is the convolution's padding.  The weights are packed once per call into A
// fragments in (gate, 32-row tile, tap, k-step) order and read from global memory (L2): wave w of a
// workgroup owns output channels 32 w .. 32 w + 31 of both gates for all kTile pixels, so a fragment is
// loaded once per workgroup and used for kTile / 32 pixel tiles.
//
// The summation order of an output is fixed (channel chunk, tap, k-step; small products first) and does not
// depend on the batch or on the other tiles: results are bitwise repeatable and per-sample independent.

#include "mfma_bf16.h"

namespace rmd {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;     // wave w: output channels 32 w ..; Hd <= 128
constexpr int kTile = 64, kSub = kTile / 32;              // pixels of a workgroup; 32-pixel MFMA tiles of it
constexpr int kTaps = 5;
constexpr int kAlign = 256;

struct GruGeom {
    int B, Hd, Xd, H, W;
    int C;          // Hd + Xd
    int mo, ks;     // 32-row tiles of one gate, 16-channel k-steps of one tap
    int tiles_x;    // workgroups per image row
    int nfrag;      // A fragments of one part (hi or lo) of the packed gates of this call
};

inline bool gru_supported(int hd, int xd) {
    return hd >= 32 && hd <= 32 * kWaves && hd % 32 == 0 && xd >= 16 && xd % 16 == 0 && hd + xd <= 512;
}

// ---- weights -> A fragments --------------------------------------------------------------------------

struct GruWeights {
    const float* w[6];
};

// fragment ((g * mo + m) * 5 + t) * ks + k, lane l = (row 32 m + (l & 31), half l >> 5), element j:
// W_g[row][16 k + 8 (l >> 5) + j][tap t] of the (Hd, C, 1, 5) or (Hd, C, 5, 1) weight (both are [row][c][t]
// in memory).  nfrag hi fragments, then (if `lo`) nfrag fragments of the bf16 of the residual.
__global__ void __launch_bounds__(256)
gru_pack_kernel(GruWeights Wt, int ngates, int mo, int ks, int C, int nfrag, int lo, bf16x8* __restrict__ frags) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= nfrag * 64) return;
    const int fa = id >> 6, lane = id & 63;
    const int k = fa % ks, t = (fa / ks) % kTaps, m = (fa / (ks * kTaps)) % mo, g = fa / (ks * kTaps * mo);
    const float* src = Wt.w[0];
#pragma unroll
    for (int i = 1; i < 6; ++i)
        if (i < ngates && g == i) src = Wt.w[i];
    const float* row = src + ((size_t)(32 * m + (lane & 31)) * C + 16 * k + 8 * (lane >> 5)) * kTaps + t;
    bf16x8 hi, lopart;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = row[j * kTaps];
        hi[j] = bf16_hi(v);
        lopart[j] = bf16_lo(v, hi[j]);
    }
    frags[id] = hi;
    if (lo) frags[id + (size_t)nfrag * 64] = lopart;
}

// ---- the GEMM kernels --------------------------------------------------------------------------------

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

template <int AXIS> struct Stage {
    static constexpr int KC = AXIS == 0 ? 64 : 32;                       // channels per staged chunk
    static constexpr int SLOTS = AXIS == 0 ? kTile + 4 : kTaps * kTile;   // staged positions
    static constexpr int STRIDE = KC + 8;     // bf16 per position: an odd number of 16-byte slots, so the
                                              // 16-byte reads of consecutive positions fall on distinct banks
};

// NG = 2: the gate kernel.  Rows of gates g0 (z) and g0 + 1 (r) over [hsrc ; x]; writes z to zbuf and
//         r . h to out.
// NG = 1: the candidate kernel.  Rows of gate g0 (q) over [hsrc = r . h ; x]; reads z from zbuf and writes
//         h' = (1 - z) h + z q to out.
template <int NP, int AXIS, int NG>
__global__ void __launch_bounds__(kThreads)
gru_kernel(const float* __restrict__ hsrc, const float* __restrict__ x, const bf16x8* __restrict__ frags, int g0,
           const float* __restrict__ bias0, const float* __restrict__ bias1, const float* __restrict__ h,
           float* __restrict__ zbuf, float* __restrict__ out, GruGeom P) {
    using S = Stage<AXIS>;
    constexpr int PARTS = NP == 3 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) __bf16 sm[PARTS * S::SLOTS * S::STRIDE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int tx = blockIdx.x % P.tiles_x, row = blockIdx.x / P.tiles_x;
    const int y = row % P.H, b = row / P.H;
    const int x0 = tx * kTile;
    const int HW = P.H * P.W;
    const float* hb = hsrc + (size_t)b * P.Hd * HW;       // wave-uniform bases, 32-bit offsets inside an image
    const float* xb = x + (size_t)b * P.Xd * HW;
    const bool active = wave < P.mo;

    f32x16 acc[NG][kSub];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int n = 0; n < kSub; ++n) acc[g][n] = f32x16{};

    for (int c0 = 0; c0 < P.C; c0 += S::KC) {
        const int kc = min(S::KC, P.C - c0);              // a multiple of 16
        __syncthreads();                                   // the previous chunk's reads are done
        for (int id = tid; id < (kc >> 3) * S::SLOTS; id += kThreads) {
            const int grp = id / S::SLOTS, s = id - grp * S::SLOTS;
            int yy, xx;
            if constexpr (AXIS == 0) {
                yy = y; xx = x0 - 2 + s;
            } else {
                const int t = s / kTile;
                yy = y + t - 2; xx = x0 + (s - t * kTile);
            }
            const bool inside = yy >= 0 && yy < P.H && xx >= 0 && xx < P.W;
            const int c = c0 + 8 * grp;                    // Hd is a multiple of 8: a group is all h or all x
            const float* src = (c < P.Hd ? hb + c * HW : xb + (c - P.Hd) * HW) + (inside ? yy * P.W + xx : 0);
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = inside ? src[j * HW] : 0.f;
            bf16x8 hi, lo;
            split<NP>(v, hi, lo);
            *reinterpret_cast<bf16x8*>(&sm[s * S::STRIDE + 8 * grp]) = hi;
            if constexpr (NP == 3) *reinterpret_cast<bf16x8*>(&sm[(S::SLOTS + s) * S::STRIDE + 8 * grp]) = lo;
        }
        __syncthreads();
        if (!active) continue;
        const int ksteps = kc >> 4, kbase = c0 >> 4;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
#pragma unroll
            for (int k = 0; k < S::KC / 16; ++k) {
                if (k < ksteps) {
                    bf16x8 ah[NG], al[NG];
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const size_t f = ((size_t)(((g0 + g) * P.mo + wave) * kTaps + t) * P.ks + kbase + k) * 64 + lane;
                        ah[g] = frags[f];
                        al[g] = NP == 3 ? frags[f + (size_t)P.nfrag * 64] : bf16x8{};
                    }
#pragma unroll
                    for (int n = 0; n < kSub; ++n) {
                        if (n == 0 || x0 + 32 * n < P.W) {
                            const int slot = AXIS == 0 ? 32 * n + r + t : t * kTile + 32 * n + r;
                            const __bf16* p = &sm[slot * S::STRIDE + 16 * k + 8 * hh];
                            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(p);
                            const bf16x8 bl = NP == 3 ? *reinterpret_cast<const bf16x8*>(p + S::SLOTS * S::STRIDE)
                                                      : bf16x8{};
#pragma unroll
                            for (int g = 0; g < NG; ++g) mma<NP>(acc[g][n], ah[g], al[g], bh, bl);
                        }
                    }
                }
            }
        }
    }
    if (!active) return;

    // epilogue: register i of lane (r, hh) is channel 32 wave + acc_row(i, hh) of pixel x0 + 32 n + r
    const size_t img = (size_t)b * P.Hd * HW;
#pragma unroll
    for (int n = 0; n < kSub; ++n) {
        const int px = x0 + 32 * n + r;
        if (px >= P.W) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ch = 32 * wave + acc_row(i, hh);
            const size_t at = img + (size_t)(ch * HW + y * P.W + px);
            if constexpr (NG == 2) {
                zbuf[at] = sigmoidf(acc[0][n][i] + bias0[ch]);
                out[at] = sigmoidf(acc[1][n][i] + bias1[ch]) * h[at];
            } else {
                const float q = tanhf(acc[0][n][i] + bias0[ch]);
                const float z = zbuf[at], hv = h[at];
                out[at] = (1.f - z) * hv + z * q;
            }
        }
    }
}

// one half-step: gates g0 .. g0 + 2 of the packed fragments (z, r, q), h -> out
template <int NP, int AXIS>
void launch_half(const float* h, const float* x, const bf16x8* frags, int g0, const float* const* biases, float* zbuf,
                 float* rh, float* out, const GruGeom& P, hipStream_t st) {
    const int grid = P.B * P.H * P.tiles_x;
    gru_kernel<NP, AXIS, 2><<<grid, kThreads, 0, st>>>(h, x, frags, g0, biases[0], biases[1], h, zbuf, rh, P);
    gru_kernel<NP, AXIS, 1><<<grid, kThreads, 0, st>>>(rh, x, frags, g0 + 2, biases[2], nullptr, h, zbuf, out, P);
}

void run_half(int np, int axis, const float* h, const float* x, const bf16x8* frags, int g0,
              const float* const* biases, float* zbuf, float* rh, float* out, const GruGeom& P, hipStream_t st) {
    if (np == 3) {
        if (axis == 0) launch_half<3, 0>(h, x, frags, g0, biases, zbuf, rh, out, P, st);
        else launch_half<3, 1>(h, x, frags, g0, biases, zbuf, rh, out, P, st);
    } else {
        if (axis == 0) launch_half<1, 0>(h, x, frags, g0, biases, zbuf, rh, out, P, st);
        else launch_half<1, 1>(h, x, frags, g0, biases, zbuf, rh, out, P, st);
    }
}

size_t gru_workspace_bytes(int batch, int hd, int xd, int height, int width) {
    const size_t packed = (size_t)6 * hd * kTaps * (hd + xd) * 2 * sizeof(__bf16);
    const size_t map = (size_t)batch * hd * height * width * sizeof(float);
    return packed + 3 * map + 4 * kAlign;
}

// the checks of entry point `name` (ngates weights and biases), before any launch
int gru_check(const char* name, const float* h, const float* x, const float* const* weights,
              const float* const* biases, int ngates, const float* out, const void* workspace, int batch, int hd,
              int xd, int height, int width, int compute) {
    RMD_REQUIRE(h && x && weights && biases && out && workspace, RMD_ERR_ARG, "%s: null pointer", name);
    for (int g = 0; g < ngates; ++g)
        RMD_REQUIRE(weights[g] && biases[g], RMD_ERR_ARG, "%s: null weight or bias %d", name, g);
    RMD_REQUIRE(compute == RMD_BF16X3 || compute == RMD_BF16, RMD_ERR_ARG,
                "%s: compute must be RMD_BF16X3 or RMD_BF16, got %d", name, compute);
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes", name);
    RMD_REQUIRE(gru_supported(hd, xd), RMD_ERR_SHAPE,
                "%s: unsupported (hidden=%d input=%d): hidden a multiple of 32 in 32..128, input a multiple of 16, "
                "hidden + input <= 512", name, hd, xd);
    const long long n = (long long)height * width;
    // 32-bit lane offsets into one image's maps, 64-bit everywhere else
    RMD_REQUIRE(n * (hd + xd) < (1ll << 30), RMD_ERR_SHAPE, "%s: %lld pixels x %d channels per image", name, n,
                hd + xd);
    RMD_REQUIRE((long long)batch * height * ((width + kTile - 1) / kTile) <= 0x7fffffffll, RMD_ERR_SHAPE,
                "%s: too many row segments (batch=%d height=%d width=%d)", name, batch, height, width);
    const size_t hbytes = (size_t)batch * hd * n * sizeof(float), xbytes = (size_t)batch * xd * n * sizeof(float);
    const size_t wbytes = gru_workspace_bytes(batch, hd, xd, height, width);
    RMD_REQUIRE(!overlap(out, hbytes, h, hbytes) && !overlap(out, hbytes, x, xbytes), RMD_ERR_ARG,
                "%s: out overlaps an input", name);
    RMD_REQUIRE(!overlap(workspace, wbytes, h, hbytes) && !overlap(workspace, wbytes, x, xbytes) &&
                    !overlap(workspace, wbytes, out, hbytes),
                RMD_ERR_ARG, "%s: workspace overlaps a tensor", name);
    return RMD_OK;
}

GruGeom gru_geom(int batch, int hd, int xd, int height, int width, int ngates) {
    GruGeom P;
    P.B = batch; P.Hd = hd; P.Xd = xd; P.H = height; P.W = width;
    P.C = hd + xd; P.mo = hd / 32; P.ks = P.C / 16;
    P.tiles_x = (width + kTile - 1) / kTile;
    P.nfrag = ngates * P.mo * kTaps * P.ks;
    return P;
}

// packs `ngates` weights into the workspace and carves the three maps; returns the fragments
struct GruWork {
    bf16x8* frags;
    float *zbuf, *rh, *mid;
};

GruWork gru_prepare(const float* const* weights, int ngates, void* workspace, const GruGeom& P, bool lo,
                    hipStream_t st) {
    char* base = reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(workspace)));
    const size_t packed = (size_t)6 * P.Hd * kTaps * P.C * 2 * sizeof(__bf16);       // a multiple of kAlign
    const size_t map = align256((size_t)P.B * P.Hd * P.H * P.W * sizeof(float));
    GruWork Wk;
    Wk.frags = reinterpret_cast<bf16x8*>(base);
    Wk.zbuf = reinterpret_cast<float*>(base + packed);
    Wk.rh = reinterpret_cast<float*>(base + packed + map);
    Wk.mid = reinterpret_cast<float*>(base + packed + 2 * map);
    GruWeights Wt = {};
    for (int g = 0; g < ngates; ++g) Wt.w[g] = weights[g];
    gru_pack_kernel<<<(P.nfrag * 64 + 255) / 256, 256, 0, st>>>(Wt, ngates, P.mo, P.ks, P.C, P.nfrag, lo ? 1 : 0,
                                                                 Wk.frags);
    return Wk;
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" int rmd_sepconv_gru_supported(int hidden, int input) { return gru_supported(hidden, input) ? 1 : 0; }

extern "C" size_t rmd_sepconv_gru_workspace_bytes(int batch, int hidden, int input, int height, int width) {
    if (!gru_supported(hidden, input) || batch < 1 || height < 1 || width < 1) return 0;
    return gru_workspace_bytes(batch, hidden, input, height, width);
}

extern "C" int rmd_sepconv_gru_half(const float* h, const float* x, const float* const* weights,
                                    const float* const* biases, float* out, void* workspace, int batch, int hidden,
                                    int input, int height, int width, int axis, int compute, void* stream) {
    RMD_REQUIRE(axis == 0 || axis == 1, RMD_ERR_ARG, "rmd_sepconv_gru_half: axis must be 0 (1x5) or 1 (5x1), got %d",
                axis);
    if (int rc = gru_check("rmd_sepconv_gru_half", h, x, weights, biases, 3, out, workspace, batch, hidden, input,
                           height, width, compute))
        return rc;
    const GruGeom P = gru_geom(batch, hidden, input, height, width, 3);
    hipStream_t st = as_stream(stream);
    const int np = compute == RMD_BF16X3 ? 3 : 1;
    const GruWork Wk = gru_prepare(weights, 3, workspace, P, np == 3, st);
    run_half(np, axis, h, x, Wk.frags, 0, biases, Wk.zbuf, Wk.rh, out, P, st);
    return check_launch("rmd_sepconv_gru_half");
}

extern "C" int rmd_sepconv_gru(const float* h, const float* x, const float* const* weights,
                               const float* const* biases, float* out, void* workspace, int batch, int hidden,
                               int input, int height, int width, int compute, void* stream) {
    if (int rc = gru_check("rmd_sepconv_gru", h, x, weights, biases, 6, out, workspace, batch, hidden, input, height,
                           width, compute))
        return rc;
    const GruGeom P = gru_geom(batch, hidden, input, height, width, 6);
    hipStream_t st = as_stream(stream);
    const int np = compute == RMD_BF16X3 ? 3 : 1;
    const GruWork Wk = gru_prepare(weights, 6, workspace, P, np == 3, st);
    run_half(np, 0, h, x, Wk.frags, 0, biases, Wk.zbuf, Wk.rh, Wk.mid, P, st);
    run_half(np, 1, Wk.mid, x, Wk.frags, 3, biases + 3, Wk.zbuf, Wk.rh, out, P, st);
    return check_launch("rmd_sepconv_gru");
}
