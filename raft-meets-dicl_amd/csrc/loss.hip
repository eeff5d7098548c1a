// loss.hip — the sequence losses of a training step, fused: every prediction of a call against one
// target in one streaming pass, and a recomputing, deterministic backward.
//
// Replaces (qzed/raft-meets-dicl v2):
//  * SequenceLoss.compute                        src/models/impls/raft.py:616-644
//  * MultiLevelSequenceLoss.compute / upsample   src/models/common/loss/mlseq.py:34-67
//  * RestrictedMultiLevelSequenceLoss.compute    src/models/impls/raft_dicl_ctf_l3.py:430-473 (masks built by the caller)
//  * MultiscaleLoss.compute / upsample           src/models/impls/dicl.py:436-472 (masks built by the caller)
// -> rmd_sequence_loss, rmd_sequence_loss_backward
//
// Forward: a work item is 4 adjacent pixels of a row (16-B loads; 1 pixel when W % 4 != 0 or a base
// pointer is not 16-B aligned).  A thread loads target and validity of its item once and loops over
// the K predictions of the table (passed by value); its K running sums and counts live in LDS
// ([k][thread], private until the block reduction), so K is a run-time loop.  Each block writes K
// double sums and K counts to the workspace with plain stores; a one-block kernel adds them in a
// fixed order and forms the loss.  No atomics anywhere: bitwise run-to-run reproducible.
//
// Backward: nothing is saved; d = f - target is recomputed.  Full-resolution predictions: one pass
// writes every requested gradient (target and validity loaded once per item).  Upsampled
// predictions: the transpose of the bilinear map in gather form, one wave per coarse pixel, lanes
// over the fine footprint (a conservative index range, membership tested with the forward's own
// index expressions), shuffle-tree sum in a fixed order.

#include "rmd_common.h"

namespace rmd {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;       // bounded grid: 8 blocks per CU on 256 CUs

struct LossEntry {
    const float* flow;
    const unsigned char* mask;         // own (B, H, W) mask or nullptr: the shared one
    float* grad;                       // backward only
    int h, w;
    int index;                         // position in the call's counts array
    float weight;
    float ry, rx;                      // ATen's align_corners source scale (in - 1) / (out - 1), 0 for out == 1
    float sy, sx;                      // size ratios H / h, W / w applied to components 1, 0
};

struct LossTable {
    LossEntry e[RMD_LOSS_MAX_PREDICTIONS];
    int n;
};

struct LossWeights {
    float w[RMD_LOSS_MAX_PREDICTIONS];
    int n;
};

// ATen's bilinear align_corners index rule (UpSample.h area_pixel_compute_source_index +
// guard_index_and_lambda): source = scale * dst in fp32, i0 = floor, i1 = i0 + (i0 < in - 1)
__device__ __forceinline__ void src_index(int dst, float rs, int in, int& i0, int& i1, float& lam) {
    const float s = rs * (float)dst;
    i0 = min((int)floorf(s), in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    lam = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

// upsampled flow of entry e at fine pixel (b, y, x): mlseq.py:59-67 (interpolate, then the size ratios)
__device__ __forceinline__ void up_value(const LossEntry& e, int b, int y0, int y1, float ly, int x0, int x1, float lx,
                                         float& f0, float& f1) {
    const size_t plane = (size_t)e.h * e.w;
    const float* p = e.flow + (size_t)b * 2 * plane;
    const size_t o00 = (size_t)y0 * e.w + x0, o01 = (size_t)y0 * e.w + x1;
    const size_t o10 = (size_t)y1 * e.w + x0, o11 = (size_t)y1 * e.w + x1;
    const float wy0 = 1.f - ly, wx0 = 1.f - lx;
    f0 = (wy0 * (wx0 * p[o00] + lx * p[o01]) + ly * (wx0 * p[o10] + lx * p[o11])) * e.sx;
    p += plane;
    f1 = (wy0 * (wx0 * p[o00] + lx * p[o01]) + ly * (wx0 * p[o10] + lx * p[o11])) * e.sy;
}

template <int NORM>
__device__ __forceinline__ float dist(float d0, float d1) {
    if (NORM == RMD_LOSS_L2) return sqrtf(d0 * d0 + d1 * d1);
    const float a = fabsf(d0) + fabsf(d1);
    if (NORM == RMD_LOSS_ABSMEAN) return 0.5f * a;
    if (NORM == RMD_LOSS_ROBUST) return powf(a + 1e-8f, 0.4f);            // dicl.py:451
    return a;
}

__device__ __forceinline__ float sgn(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }

// d dist / d d_c; the zero norm of ord 2 is masked as torch's norm backward masks it
template <int NORM>
__device__ __forceinline__ void dist_grad(float d0, float d1, float& g0, float& g1) {
    if (NORM == RMD_LOSS_L2) {
        const float n = sqrtf(d0 * d0 + d1 * d1);
        g0 = n == 0.f ? 0.f : d0 / n;
        g1 = n == 0.f ? 0.f : d1 / n;
        return;
    }
    float c = 1.f;
    if (NORM == RMD_LOSS_ABSMEAN) c = 0.5f;
    if (NORM == RMD_LOSS_ROBUST) c = 0.4f * powf(fabsf(d0) + fabsf(d1) + 1e-8f, -0.6f);
    g0 = c * sgn(d0);
    g1 = c * sgn(d1);
}

template <int VEC>
__device__ __forceinline__ void load_f(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}

template <int VEC>
__device__ __forceinline__ void store_f(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

template <int VEC>
__device__ __forceinline__ void load_m(const unsigned char* p, bool (&m)[VEC]) {
    if constexpr (VEC == 4) {
        const unsigned u = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
        for (int v = 0; v < VEC; ++v) m[v] = ((u >> (8 * v)) & 0xffu) != 0;
    } else {
        m[0] = *p != 0;
    }
}

// grid: bounded, grid-stride over items of VEC pixels.  Dynamic LDS: n * 256 * (float + int).
template <int NORM, int VEC>
__global__ void __launch_bounds__(kThreads)
loss_forward_kernel(LossTable t, const float* __restrict__ target, const unsigned char* __restrict__ valid, int B,
                    int H, int W, int include_invalid, double* __restrict__ psum, long long* __restrict__ pcnt) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* ssum = smem;
    int* scnt = reinterpret_cast<int*>(smem + t.n * kThreads);
    const int tid = threadIdx.x;
    for (int k = 0; k < t.n; ++k) {
        ssum[k * kThreads + tid] = 0.f;
        scnt[k * kThreads + tid] = 0;
    }
    const long long plane = (long long)H * W;
    const long long items = (long long)B * plane / VEC;
    for (long long it = (long long)blockIdx.x * kThreads + tid; it < items; it += (long long)gridDim.x * kThreads) {
        const long long p = it * VEC;
        const int b = (int)(p / plane);
        const long long q = p - (long long)b * plane;
        const int y = (int)(q / W), x = (int)(q - (long long)y * W);
        float t0[VEC], t1[VEC];
        bool m[VEC];
        load_f<VEC>(target + (size_t)b * 2 * plane + q, t0);
        load_f<VEC>(target + (size_t)b * 2 * plane + plane + q, t1);
        load_m<VEC>(valid + p, m);
        for (int k = 0; k < t.n; ++k) {
            const LossEntry& e = t.e[k];
            bool mk[VEC];
            if (e.mask) {
                load_m<VEC>(e.mask + p, mk);
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) mk[v] = m[v];
            }
            float f0[VEC], f1[VEC];
            if (e.h == H && e.w == W) {
                load_f<VEC>(e.flow + (size_t)b * 2 * plane + q, f0);
                load_f<VEC>(e.flow + (size_t)b * 2 * plane + plane + q, f1);
            } else {
                int y0, y1;
                float ly;
                src_index(y, e.ry, e.h, y0, y1, ly);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    int x0, x1;
                    float lx;
                    src_index(x + v, e.rx, e.w, x0, x1, lx);
                    up_value(e, b, y0, y1, ly, x0, x1, lx, f0[v], f1[v]);
                }
            }
            float s = 0.f;
            int c = 0;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float dd = dist<NORM>(f0[v] - t0[v], f1[v] - t1[v]);
                if (include_invalid) {
                    s += dd * (mk[v] ? 1.f : 0.f);       // raft.py:633: a product, NaN * 0 stays NaN
                } else if (mk[v]) {                      // raft.py:639: a selection
                    s += dd;
                    ++c;
                }
            }
            ssum[k * kThreads + tid] += s;
            scnt[k * kThreads + tid] += c;
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = wave; k < t.n; k += kThreads / 64) {
        const float* sp = ssum + k * kThreads;
        const int* cp = scnt + k * kThreads;
        double a = ((double)sp[lane] + (double)sp[lane + 64]) + ((double)sp[lane + 128] + (double)sp[lane + 192]);
        long long c = (long long)cp[lane] + cp[lane + 64] + cp[lane + 128] + cp[lane + 192];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            a += __shfl_down(a, off);
            c += __shfl_down(c, off);
        }
        if (lane == 0) {
            psum[(size_t)blockIdx.x * t.n + k] = a;
            pcnt[(size_t)blockIdx.x * t.n + k] = c;
        }
    }
}

// one block: the partials of every prediction in a fixed order, the K means, the loss
__global__ void __launch_bounds__(kThreads)
loss_final_kernel(LossWeights wt, const double* __restrict__ psum, const long long* __restrict__ pcnt, int nblocks,
                  long long full_count, int include_invalid, int skip_empty, float scale, float* __restrict__ loss,
                  long long* __restrict__ counts) {
    __shared__ double sd[kThreads];
    __shared__ long long sc[kThreads];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int k = 0; k < wt.n; ++k) {
        double a = 0.0;
        long long c = 0;
        for (int i = tid; i < nblocks; i += kThreads) {
            a += psum[(size_t)i * wt.n + k];
            c += pcnt[(size_t)i * wt.n + k];
        }
        sd[tid] = a;
        sc[tid] = c;
        __syncthreads();
        for (int s = kThreads / 2; s >= 1; s >>= 1) {
            if (tid < s) {
                sd[tid] += sd[tid + s];
                sc[tid] += sc[tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const long long n = include_invalid ? full_count : sc[0];
            counts[k] = n;
            // mean() of an empty selection is NaN (0 / 0); skip_empty: `if torch.any(valid_lvl)`
            if (!(n == 0 && skip_empty)) total += (double)wt.w[k] * (sd[0] / (double)n);
        }
        __syncthreads();
    }
    if (tid == 0) *loss = (float)(total * (double)scale);
}

__device__ __forceinline__ float loss_coef(const LossEntry& e, float g, float scale, const long long* counts) {
    const long long n = counts[e.index];
    return n > 0 ? g * scale * e.weight / (float)n : 0.f;
}

// full-resolution predictions: one item per thread, every requested gradient in one pass
template <int NORM, int VEC>
__global__ void __launch_bounds__(kThreads)
loss_backward_full_kernel(LossTable t, const float* __restrict__ target, const unsigned char* __restrict__ valid,
                          int B, int H, int W, int include_invalid, float scale, const float* __restrict__ gloss,
                          const long long* __restrict__ counts) {
    const long long plane = (long long)H * W;
    const long long items = (long long)B * plane / VEC;
    const long long it = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (it >= items) return;
    const long long p = it * VEC;
    const int b = (int)(p / plane);
    const long long q = p - (long long)b * plane;
    const float g = *gloss;
    float t0[VEC], t1[VEC];
    bool m[VEC];
    load_f<VEC>(target + (size_t)b * 2 * plane + q, t0);
    load_f<VEC>(target + (size_t)b * 2 * plane + plane + q, t1);
    load_m<VEC>(valid + p, m);
    for (int k = 0; k < t.n; ++k) {
        const LossEntry& e = t.e[k];
        const float coef = loss_coef(e, g, scale, counts);
        bool mk[VEC];
        if (e.mask) {
            load_m<VEC>(e.mask + p, mk);
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) mk[v] = m[v];
        }
        float f0[VEC], f1[VEC], g0[VEC], g1[VEC];
        load_f<VEC>(e.flow + (size_t)b * 2 * plane + q, f0);
        load_f<VEC>(e.flow + (size_t)b * 2 * plane + plane + q, f1);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            float a0, a1;
            dist_grad<NORM>(f0[v] - t0[v], f1[v] - t1[v], a0, a1);
            if (include_invalid) {
                const float mf = mk[v] ? 1.f : 0.f;
                g0[v] = coef * mf * a0;
                g1[v] = coef * mf * a1;
            } else {
                g0[v] = mk[v] ? coef * a0 : 0.f;
                g1[v] = mk[v] ? coef * a1 : 0.f;
            }
        }
        store_f<VEC>(e.grad + (size_t)b * 2 * plane + q, g0);
        store_f<VEC>(e.grad + (size_t)b * 2 * plane + plane + q, g1);
    }
}

// fine index range whose i0 / i1 can select coarse index c (i0 in {c - 1, c}), one pixel of margin
__device__ __forceinline__ void footprint(int c, float rs, int out, int& lo, int& hi) {
    lo = 0;
    hi = out - 1;
    if (rs > 0.f) {
        const float inv = 1.f / rs;
        lo = max(0, (int)floorf((float)(c - 1) * inv) - 1);
        hi = min(out - 1, (int)ceilf((float)(c + 1) * inv) + 1);
    }
}

// upsampled predictions: grid (ceil(max coarse pixels / 4), entries); one wave per coarse pixel
template <int NORM>
__global__ void __launch_bounds__(kThreads)
loss_backward_up_kernel(LossTable t, const float* __restrict__ target, const unsigned char* __restrict__ valid, int B,
                        int H, int W, int include_invalid, float scale, const float* __restrict__ gloss,
                        const long long* __restrict__ counts) {
    const LossEntry& e = t.e[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long cplane = (long long)e.h * e.w;
    const long long cp = (long long)blockIdx.x * (kThreads / 64) + wave;
    if (cp >= (long long)B * cplane) return;
    const int b = (int)(cp / cplane);
    const int r = (int)(cp - (long long)b * cplane);
    const int yc = r / e.w, xc = r - yc * e.w;
    const float coef = loss_coef(e, *gloss, scale, counts);
    const size_t plane = (size_t)H * W;
    const unsigned char* mp = (e.mask ? e.mask : valid) + (size_t)b * plane;
    const float* tp = target + (size_t)b * 2 * plane;
    float g0 = 0.f, g1 = 0.f;
    if (coef != 0.f) {
        int ylo, yhi, xlo, xhi;
        footprint(yc, e.ry, H, ylo, yhi);
        footprint(xc, e.rx, W, xlo, xhi);
        const int fw = xhi - xlo + 1, cnt = fw * (yhi - ylo + 1);
        for (int j = lane; j < cnt; j += 64) {
            const int y = ylo + j / fw, x = xlo + j % fw;
            int y0, y1, x0, x1;
            float ly, lx;
            src_index(y, e.ry, e.h, y0, y1, ly);
            src_index(x, e.rx, e.w, x0, x1, lx);
            if ((y0 != yc && y1 != yc) || (x0 != xc && x1 != xc)) continue;
            const bool m = mp[(size_t)y * W + x] != 0;
            if (!include_invalid && !m) continue;
            float f0, f1, a0, a1;
            up_value(e, b, y0, y1, ly, x0, x1, lx, f0, f1);
            dist_grad<NORM>(f0 - tp[(size_t)y * W + x], f1 - tp[plane + (size_t)y * W + x], a0, a1);
            const float wy = (y0 == yc ? 1.f - ly : 0.f) + (y1 == yc ? ly : 0.f);
            const float wx = (x0 == xc ? 1.f - lx : 0.f) + (x1 == xc ? lx : 0.f);
            const float wgt = wy * wx * (m ? 1.f : 0.f);
            g0 += wgt * a0;
            g1 += wgt * a1;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            g0 += __shfl_xor(g0, off);
            g1 += __shfl_xor(g1, off);
        }
    }
    if (lane == 0) {
        float* gp = e.grad + (size_t)b * 2 * cplane + r;
        gp[0] = coef * e.sx * g0;
        gp[cplane] = coef * e.sy * g1;
    }
}

inline int forward_blocks(int batch, int height, int width) {
    const long long items = (long long)batch * height * width;       // the scalar path's item count (the larger)
    const long long blocks = (items + kThreads - 1) / kThreads;
    return (int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

int check_common(const char* what, const rmd_loss_prediction* preds, int npred, const float* target,
                 const unsigned char* valid, int batch, int height, int width, int norm) {
    RMD_REQUIRE(preds && target && valid, RMD_ERR_ARG, "%s: null pointer", what);
    RMD_REQUIRE(npred >= 1 && npred <= RMD_LOSS_MAX_PREDICTIONS, RMD_ERR_ARG,
                "%s: %d predictions (1..%d per call; chunk longer lists)", what, npred, RMD_LOSS_MAX_PREDICTIONS);
    RMD_REQUIRE(norm >= RMD_LOSS_L1 && norm <= RMD_LOSS_ROBUST, RMD_ERR_ARG,
                "%s: bad norm %d (RMD_LOSS_L1, RMD_LOSS_L2, RMD_LOSS_ABSMEAN or RMD_LOSS_ROBUST)", what, norm);
    RMD_REQUIRE(batch > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "%s: bad sizes (batch=%d height=%d width=%d)",
                what, batch, height, width);
    for (int k = 0; k < npred; ++k) {
        RMD_REQUIRE(preds[k].flow, RMD_ERR_ARG, "%s: prediction %d: null flow", what, k);
        RMD_REQUIRE(preds[k].height > 0 && preds[k].width > 0, RMD_ERR_SHAPE, "%s: prediction %d: bad sizes (%d x %d)",
                    what, k, preds[k].height, preds[k].width);
    }
    return RMD_OK;
}

LossEntry make_entry(const rmd_loss_prediction& p, int index, int height, int width) {
    LossEntry e{};
    e.flow = p.flow;
    e.mask = p.mask;
    e.grad = p.grad;
    e.h = p.height;
    e.w = p.width;
    e.index = index;
    e.weight = p.weight;
    e.ry = height > 1 ? (float)(p.height - 1) / (float)(height - 1) : 0.f;
    e.rx = width > 1 ? (float)(p.width - 1) / (float)(width - 1) : 0.f;
    e.sy = (float)((double)height / p.height);
    e.sx = (float)((double)width / p.width);
    return e;
}

// 4-pixel items need W % 4 == 0 (items stay inside a row, plane offsets stay aligned) and aligned bases
bool can_vector(const LossTable& t, const float* target, const unsigned char* valid, int height, int width,
                bool grads) {
    if (width % 4 || !aligned(target, 16) || !aligned(valid, 4)) return false;
    for (int k = 0; k < t.n; ++k) {
        const LossEntry& e = t.e[k];
        if (e.mask && !aligned(e.mask, 4)) return false;
        if (e.h == height && e.w == width && (!aligned(e.flow, 16) || (grads && !aligned(e.grad, 16)))) return false;
    }
    return true;
}

template <int NORM>
void launch_forward(bool vec, int grid, size_t lds, hipStream_t s, const LossTable& t, const float* target,
                    const unsigned char* valid, int b, int h, int w, int inc, double* psum, long long* pcnt) {
    if (vec) loss_forward_kernel<NORM, 4><<<grid, kThreads, lds, s>>>(t, target, valid, b, h, w, inc, psum, pcnt);
    else loss_forward_kernel<NORM, 1><<<grid, kThreads, lds, s>>>(t, target, valid, b, h, w, inc, psum, pcnt);
}

template <int NORM>
void launch_backward(bool vec, hipStream_t s, const LossTable& full, const LossTable& up, long long up_pixels,
                     const float* target, const unsigned char* valid, int b, int h, int w, int inc, float scale,
                     const float* gloss, const long long* counts) {
    if (full.n) {
        const long long items = (long long)b * h * w / (vec ? 4 : 1);
        const unsigned grid = (unsigned)((items + kThreads - 1) / kThreads);
        if (vec) loss_backward_full_kernel<NORM, 4><<<grid, kThreads, 0, s>>>(full, target, valid, b, h, w, inc, scale, gloss, counts);
        else loss_backward_full_kernel<NORM, 1><<<grid, kThreads, 0, s>>>(full, target, valid, b, h, w, inc, scale, gloss, counts);
    }
    if (up.n) {
        const int per = kThreads / 64;
        dim3 grid((unsigned)((up_pixels + per - 1) / per), up.n);
        loss_backward_up_kernel<NORM><<<grid, kThreads, 0, s>>>(up, target, valid, b, h, w, inc, scale, gloss, counts);
    }
}

}  // namespace
}  // namespace rmd

using namespace rmd;

extern "C" size_t rmd_sequence_loss_workspace_bytes(int batch, int height, int width, int npred) {
    if (batch < 1 || height < 1 || width < 1 || npred < 1 || npred > RMD_LOSS_MAX_PREDICTIONS) return 0;
    return (size_t)forward_blocks(batch, height, width) * npred * (sizeof(double) + sizeof(long long));
}

extern "C" int rmd_sequence_loss(const rmd_loss_prediction* preds, int npred, const float* target,
                                 const unsigned char* valid, int batch, int height, int width, int norm,
                                 int include_invalid, int skip_empty, float scale, float* loss, long long* counts,
                                 void* workspace, void* stream) {
    const int rc = check_common("rmd_sequence_loss", preds, npred, target, valid, batch, height, width, norm);
    if (rc != RMD_OK) return rc;
    RMD_REQUIRE(loss && counts && workspace, RMD_ERR_ARG, "rmd_sequence_loss: null output or workspace");
    RMD_REQUIRE((long long)batch * height * width <= 0x7fffffffLL * 4, RMD_ERR_SHAPE,
                "rmd_sequence_loss: %lld pixels", (long long)batch * height * width);
    LossTable t{};
    LossWeights wt{};
    t.n = wt.n = npred;
    for (int k = 0; k < npred; ++k) {
        t.e[k] = make_entry(preds[k], k, height, width);
        wt.w[k] = preds[k].weight;
    }
    const bool vec = can_vector(t, target, valid, height, width, false);
    const int grid = forward_blocks(batch, height, width);
    const size_t lds = (size_t)npred * kThreads * (sizeof(float) + sizeof(int));
    double* psum = static_cast<double*>(workspace);
    long long* pcnt = reinterpret_cast<long long*>(psum + (size_t)grid * npred);
    hipStream_t s = as_stream(stream);
    switch (norm) {
        case RMD_LOSS_L1: launch_forward<RMD_LOSS_L1>(vec, grid, lds, s, t, target, valid, batch, height, width, include_invalid, psum, pcnt); break;
        case RMD_LOSS_L2: launch_forward<RMD_LOSS_L2>(vec, grid, lds, s, t, target, valid, batch, height, width, include_invalid, psum, pcnt); break;
        case RMD_LOSS_ABSMEAN: launch_forward<RMD_LOSS_ABSMEAN>(vec, grid, lds, s, t, target, valid, batch, height, width, include_invalid, psum, pcnt); break;
        default: launch_forward<RMD_LOSS_ROBUST>(vec, grid, lds, s, t, target, valid, batch, height, width, include_invalid, psum, pcnt); break;
    }
    loss_final_kernel<<<1, kThreads, 0, s>>>(wt, psum, pcnt, grid, (long long)batch * height * width, include_invalid,
                                            skip_empty, scale, loss, counts);
    return check_launch("rmd_sequence_loss");
}

extern "C" int rmd_sequence_loss_backward(const rmd_loss_prediction* preds, int npred, const float* target,
                                          const unsigned char* valid, int batch, int height, int width, int norm,
                                          int include_invalid, float scale, const float* grad_loss,
                                          const long long* counts, void* stream) {
    const int rc = check_common("rmd_sequence_loss_backward", preds, npred, target, valid, batch, height, width, norm);
    if (rc != RMD_OK) return rc;
    RMD_REQUIRE(grad_loss && counts, RMD_ERR_ARG, "rmd_sequence_loss_backward: null grad_loss or counts");
    LossTable full{}, up{}, all{};
    long long up_pixels = 0;
    for (int k = 0; k < npred; ++k) {
        if (!preds[k].grad) continue;                    // no gradient required: skipped
        const LossEntry e = make_entry(preds[k], k, height, width);
        all.e[all.n++] = e;
        if (e.h == height && e.w == width) {
            full.e[full.n++] = e;
        } else {
            up.e[up.n++] = e;
            const long long px = (long long)batch * e.h * e.w;
            up_pixels = px > up_pixels ? px : up_pixels;
        }
    }
    RMD_REQUIRE(up_pixels <= 0x7fffffffLL, RMD_ERR_SHAPE, "rmd_sequence_loss_backward: %lld coarse pixels", up_pixels);
    const bool vec = can_vector(all, target, valid, height, width, true);
    hipStream_t s = as_stream(stream);
    switch (norm) {
        case RMD_LOSS_L1: launch_backward<RMD_LOSS_L1>(vec, s, full, up, up_pixels, target, valid, batch, height, width, include_invalid, scale, grad_loss, counts); break;
        case RMD_LOSS_L2: launch_backward<RMD_LOSS_L2>(vec, s, full, up, up_pixels, target, valid, batch, height, width, include_invalid, scale, grad_loss, counts); break;
        case RMD_LOSS_ABSMEAN: launch_backward<RMD_LOSS_ABSMEAN>(vec, s, full, up, up_pixels, target, valid, batch, height, width, include_invalid, scale, grad_loss, counts); break;
        default: launch_backward<RMD_LOSS_ROBUST>(vec, s, full, up, up_pixels, target, valid, batch, height, width, include_invalid, scale, grad_loss, counts); break;
    }
    return check_launch("rmd_sequence_loss_backward");
}
