// corr_otf.h — internal interface between the on-the-fly lookup (corr_otf.hip) and its training backward
// (corr_otf_backward.hip): the map geometry, the forward workspace's carve-up, the argument check and the
// radius dispatch.  Host code and plain structs only; everything has internal linkage, as have the kernels of
// both sources that take these structs by value.
#pragma once

#include "rmd_common.h"

#include <type_traits>

namespace rmd {
namespace {

constexpr int kThreads = 256;                        // prepare kernels (one thread per element)

struct OtfGeom {
    int B, C, Cp, H, W, L;
    int lh[RMD_MAX_LEVELS], lw[RMD_MAX_LEVELS], nsx[RMD_MAX_LEVELS];
    long long soff[RMD_MAX_LEVELS], TS;               // target segments: level offsets, per batch
    int qnsx;
    long long QS;                                     // query segments per batch
};

// operand channel padding: one of the compiled channel counts, else a multiple of 128
inline int otf_cp(int C) {
    for (int c : {32, 64, 128, 256})
        if (C <= c) return c;
    return (C + 127) / 128 * 128;
}

inline OtfGeom make_otf_geom(int B, int C, int H, int W, int L) {
    OtfGeom g{};
    g.B = B;
    g.C = C;
    g.Cp = otf_cp(C);
    g.H = H;
    g.W = W;
    g.L = L;
    long long s = 0;
    for (int l = 0; l < L; ++l) {
        g.lh[l] = H >> l;
        g.lw[l] = W >> l;
        g.nsx[l] = (g.lw[l] + 15) / 16;
        g.soff[l] = s;
        s += (long long)g.lh[l] * g.nsx[l];
    }
    g.TS = s;
    g.qnsx = (W + 15) / 16;
    g.QS = (long long)H * g.qnsx;
    return g;
}

// bytes per operand element of the forward workspace (BF16X3: a (hi, lo) bf16 pair)
inline size_t otf_elem_bytes(int compute) { return compute == RMD_BF16 ? 2 : 4; }

// forward workspace: query segments (B, QS) | target segments (B, TS) | f32 scratch of levels 1.. (B, C, lh, lw)
inline size_t otf_query_elems(const OtfGeom& g) { return (size_t)g.B * g.QS * 16 * g.Cp; }
inline size_t otf_scratch_elems(const OtfGeom& g) {
    size_t n = 0;
    for (int l = 1; l < g.L; ++l) n += (size_t)g.B * g.C * g.lh[l] * g.lw[l];
    return n;
}
inline size_t otf_scratch_offset(const OtfGeom& g, size_t es) {
    return align256((size_t)g.B * (g.QS + g.TS) * 16 * g.Cp * es);
}

struct LevelSrc {
    const float* p[RMD_MAX_LEVELS];      // (B, C, lh, lw) float32 per level
};

struct LevelOff {
    long long o[RMD_MAX_LEVELS];
};

// fmap2 and its pooled levels 1.. in the scratch of forward workspace `ws` (prepare pools into these)
inline LevelSrc otf_level_sources(const float* fmap2, const void* ws, const OtfGeom& g, int compute) {
    LevelSrc s{};
    s.p[0] = fmap2;
    const float* scratch = reinterpret_cast<const float*>(static_cast<const char*>(ws) +
                                                          otf_scratch_offset(g, otf_elem_bytes(compute)));
    for (int l = 1; l < g.L; ++l) {
        s.p[l] = scratch;
        scratch += (size_t)g.B * g.C * g.lh[l] * g.lw[l];
    }
    return s;
}

// Run-time value -> template argument: f(std::integral_constant<int, V>{}) for the V of Vs that equals v, and
// its return code (the callers check v first; no match is RMD_ERR_ARG).  f is instantiated for every V.
template <int... Vs, typename F>
inline int otf_dispatch(int v, F&& f) {
    int rc = RMD_ERR_ARG;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}
template <typename F>
inline int otf_dispatch_radius(int radius, F&& f) {
    return otf_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(radius, f);
}

inline int check_otf(int batch, int channels, int height, int width, int levels, int compute) {
    RMD_REQUIRE(batch > 0 && channels > 0 && height > 0 && width > 0, RMD_ERR_SHAPE, "rmd_corr_otf: bad sizes");
    RMD_REQUIRE(levels >= 1 && levels <= RMD_MAX_LEVELS, RMD_ERR_SHAPE, "rmd_corr_otf: bad levels");
    RMD_REQUIRE((height >> (levels - 1)) >= 1 && (width >> (levels - 1)) >= 1, RMD_ERR_SHAPE,
                "rmd_corr_otf: level %d of a %dx%d map is empty", levels - 1, height, width);
    RMD_REQUIRE(compute == RMD_F32 || compute == RMD_BF16 || compute == RMD_BF16X3, RMD_ERR_ARG,
                "rmd_corr_otf: compute must be F32, BF16 or BF16X3");
    return RMD_OK;
}

}  // namespace
}  // namespace rmd
