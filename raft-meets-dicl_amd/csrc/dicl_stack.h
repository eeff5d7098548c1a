// dicl_stack.h — what the forward (dicl_stack.hip) and the backward (dicl_stack_backward.hip) of the DICL
// bilinear displacement stack share: the sample geometry, the vector store helpers and the routing, i.e.
// which kernel a call runs.  dicl_int.hip takes kThreads and st4 from here.
#pragma once

#include "dicl_taps.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace rmd {
namespace {

constexpr int kThreads = 256;

// sample position of displacement (a, bb) for pixel p: the reference adds the integer offset to
// coords/2^level, normalises with (wn-1),(hn-1) and grid_sample un-normalises with (wl-1),(hl-1)
struct StackParams {
    int B, C, h, w, hl, wl, radius, extra;     // extra = 2 adds the displacement channels (dicl_emb)
    float inv_scale;                            // 1 / 2^level
    float sx, sy;                               // (wl-1)/(wn-1), (hl-1)/(hn-1)
};

typedef __attribute__((ext_vector_type(4))) float f4_t;

template <bool NT>
__device__ __forceinline__ void st4(float* p, f4_t v) {
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<f4_t*>(p));
    else *reinterpret_cast<f4_t*>(p) = v;
}

template <int PX> struct FVec;
template <> struct FVec<4> { typedef __attribute__((ext_vector_type(4))) float T; };
template <> struct FVec<2> { typedef __attribute__((ext_vector_type(2))) float T; };
template <> struct FVec<1> { typedef __attribute__((ext_vector_type(1))) float T; };

template <bool NT, typename V>
__device__ __forceinline__ void stv(float* p, V v) {
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
    else *reinterpret_cast<V*>(p) = v;
}

// LDS window of the backward kernels (dicl_stack_window.h); stack_small_window() chooses between the two
constexpr int kWinFloats = 12288;      // 48 KiB LDS window
constexpr int kWinSmall = 4096;        // 16 KiB LDS window (narrow maps, see rmd_dicl_stack_backward)

int stack_params(StackParams& P, int B, int C, int h, int w, int hl, int wl, int radius, int level, int nh, int nw,
                 int extra) {
    RMD_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && hl > 0 && wl > 0, RMD_ERR_SHAPE, "rmd_dicl_stack: bad sizes");
    RMD_REQUIRE(radius >= 0 && radius <= 32, RMD_ERR_SHAPE, "rmd_dicl_stack: radius %d out of range", radius);
    RMD_REQUIRE((h * w) % 4 == 0, RMD_ERR_SHAPE, "rmd_dicl_stack: h*w must be a multiple of 4 (MatchingNet needs even h, w)");
    RMD_REQUIRE(level >= 0 && level < 16, RMD_ERR_SHAPE, "rmd_dicl_stack: bad level");
    P.B = B; P.C = C; P.h = h; P.w = w; P.hl = hl; P.wl = wl; P.radius = radius; P.extra = extra ? 2 : 0;
    P.inv_scale = 1.0f / (float)(1 << level);
    // (wl-1)/(wn-1): 0/0 -> NaN exactly as the reference's normalisation does for 1-pixel maps
    P.sx = (float)(wl - 1) / (float)(nw - 1);
    P.sy = (float)(hl - 1) / (float)(nh - 1);
    return RMD_OK;
}

// ---- kernel routing ------------------------------------------------------------------------------
// Which kernel a stack call runs: decided here, once, for the launchers and for the
// rmd_dicl_stack_kernel query alike (host only, no GPU call).
constexpr double kImageBytesMax = 4294967296.0;   // 32-bit lane offsets inside one image's stack

double stack_image_bytes(const StackParams& P) {
    const int d = 2 * P.radius + 1;
    return 4.0 * d * d * (2.0 * P.C + P.extra) * P.h * P.w;
}

bool scale_in_01(const StackParams& P) {       // both scales finite and in [0, 1]
    return std::isfinite(P.sx) && std::isfinite(P.sy) && P.sx >= 0.f && P.sy >= 0.f && P.sx <= 1.f && P.sy <= 1.f;
}

// separable patch edge: floor(span) + 1 tap offsets + 1 for the right/bottom tap + 1 for fp32 rounding, even
int sep_patch_edge(const StackParams& P) {
    const float span = 2.0f * P.radius * std::max(P.sx, P.sy);
    return ((int)std::floor(span * (1.0f + 1e-5f) + 1e-4f) + 3 + 1) & ~1;
}

enum class StackFamily { Patch, Separable, General };
struct StackRoute {
    StackFamily family;
    int R, K;                                     // Patch: R; Separable: R, K
};

StackRoute stack_route(const StackParams& P) {
    const bool fits32 = stack_image_bytes(P) < kImageBytesMax;
    if (P.sx == 1.0f && P.sy == 1.0f && P.radius >= 1 && P.radius <= 4 && fits32)
        return {StackFamily::Patch, P.radius, 0};
    if ((P.radius == 3 || P.radius == 4) && scale_in_01(P) && fits32) {
        const int k = sep_patch_edge(P);
        if (k == 4 || k == 6 || k == 8) return {StackFamily::Separable, P.radius, k};
    }
    return {StackFamily::General, 0, 0};
}

enum class StackBwdFamily { Patch2, Patch1, Separable2, Separable1, General, Fallback };
struct StackBwdRoute {
    StackBwdFamily family;
    int R, K;                                     // Patch*: R; Separable*: K
    bool small;                                   // LDS window: kWinSmall (16 KiB) or kWinFloats (48 KiB)
};

// LDS window: a workgroup's 256 pixels (512 with two pixels per lane) cover ~256/w + 1 rows; with the
// patch (<= 2r+2 rows at unit steps) and some flow spread, 4096 floats (16 KiB) hold them for w up to
// ~170 and leave room for 9 workgroups per CU instead of 3 (48 KiB); rows past the window still go to
// global atomics, so the choice only affects speed.
bool stack_small_window(const StackParams& P, int pixels) {
    const float rows = 2.0f * P.radius * std::max(P.sy, 1.0f) + (float)pixels / P.w * std::max(P.sy, 0.5f) + 10.0f;
    return rows * P.wl <= (float)kWinSmall;
}

StackBwdRoute stack_backward_route(const StackParams& P) {
    if (P.sx == 1.0f && P.sy == 1.0f && P.radius >= 1 && P.radius <= 4) {
        // two pixels per lane: the general two-pixel merge over the joint patch box + the cross-lane chain
        // (0.55 vs 0.75 ms smooth flow, 0.77 vs 0.96 ms steep flow at cfg4 against the round-1 per-pixel
        // adds, profiles/dicl_bwd_ab_r02.json); one pixel per lane for images past 4 GiB of stack
        if (stack_image_bytes(P) < kImageBytesMax)
            return {StackBwdFamily::Patch2, P.radius, 0, stack_small_window(P, 512)};
        return {StackBwdFamily::Patch1, P.radius, 0, stack_small_window(P, 256)};
    }
    if (P.wl <= kWinFloats && scale_in_01(P)) {
        // two pixels per lane with the merged / chained patch adds (K <= 8: 0.50 vs 0.68 ms smooth, 0.52 vs
        // 0.61 ms steep flow at cfg4 level 1 against one pixel per lane); K = 10 one pixel per lane
        const int k = sep_patch_edge(P);
        if (k <= 8) return {StackBwdFamily::Separable2, 0, k, stack_small_window(P, 512)};   // k = 4, 6, 8
        if (k == 10) return {StackBwdFamily::Separable1, 0, k, stack_small_window(P, 256)};
    }
    if (P.wl <= kWinFloats && std::isfinite(P.sx) && std::isfinite(P.sy) && P.sy >= 0.f)
        return {StackBwdFamily::General, 0, 0, stack_small_window(P, 256)};
    return {StackBwdFamily::Fallback, 0, 0, false};
}

std::string route_name(const StackRoute& r) {
    switch (r.family) {
        case StackFamily::Patch: return "patch/" + std::to_string(r.R);
        case StackFamily::Separable: return "separable/" + std::to_string(r.R) + "/" + std::to_string(r.K);
        default: return "general";
    }
}

std::string route_name(const StackBwdRoute& r) {
    const char* win = r.small ? "/small" : "/large";
    switch (r.family) {
        case StackBwdFamily::Patch2: return "patch2/" + std::to_string(r.R) + win;
        case StackBwdFamily::Patch1: return "patch1/" + std::to_string(r.R) + win;
        case StackBwdFamily::Separable2: return "separable2/" + std::to_string(r.K) + win;
        case StackBwdFamily::Separable1: return "separable1/" + std::to_string(r.K) + win;
        case StackBwdFamily::General: return std::string("general") + win;
        default: return "fallback";
    }
}

// every route the two functions above can return, in dispatch order; the strings live for the
// life of the library, so the queries hand out pointers into them
struct RouteNames {
    std::vector<std::string> names;
    std::string joined;
    void add(const std::string& s) {
        names.push_back(s);
        joined += (joined.empty() ? "" : ",") + s;
    }
    const char* find(const std::string& s) const {
        for (const std::string& n : names)
            if (n == s) return n.c_str();
        return nullptr;
    }
};

const RouteNames& route_names(bool backward) {
    static const RouteNames fwd = [] {
        RouteNames t;
        for (int r = 1; r <= 4; ++r) t.add(route_name(StackRoute{StackFamily::Patch, r, 0}));
        for (int r = 3; r <= 4; ++r)
            for (int k = 4; k <= 8; k += 2) t.add(route_name(StackRoute{StackFamily::Separable, r, k}));
        t.add(route_name(StackRoute{StackFamily::General, 0, 0}));
        return t;
    }();
    static const RouteNames bwd = [] {
        RouteNames t;
        for (StackBwdFamily f : {StackBwdFamily::Patch2, StackBwdFamily::Patch1})
            for (int r = 1; r <= 4; ++r)
                for (bool small : {true, false}) t.add(route_name(StackBwdRoute{f, r, 0, small}));
        for (int k = 4; k <= 8; k += 2)
            for (bool small : {true, false}) t.add(route_name(StackBwdRoute{StackBwdFamily::Separable2, 0, k, small}));
        for (bool small : {true, false}) t.add(route_name(StackBwdRoute{StackBwdFamily::Separable1, 0, 10, small}));
        for (bool small : {true, false}) t.add(route_name(StackBwdRoute{StackBwdFamily::General, 0, 0, small}));
        t.add(route_name(StackBwdRoute{StackBwdFamily::Fallback, 0, 0, false}));
        return t;
    }();
    return backward ? bwd : fwd;
}

}  // namespace
}  // namespace rmd

