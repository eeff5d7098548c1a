// corr_pyramid.hip — all-pairs correlation GEMM with the pooled pyramid fused into its epilogue: the routing of a
// call to one of four GEMMs and the C entry points.  No kernel lives here.
//
// Replaces raft.CorrBlock.__init__ (qzed/raft-meets-dicl src/models/impls/raft.py:18-47):
//   corr0[b,p,q] = sum_c f1[b,c,p] f2[b,c,q] / sqrt(C);  level l = avg_pool2d(level l-1, 2, 2)
//
// gfx950 design, common to the four.  Targets (fmap2 pixels) are the MFMA row side, queries
// (fmap1 pixels) the column side, and one 32-target MFMA tile is a 4 x 8 block of target pixels.  In the
// 32x32 accumulator layout lane (h = lane>>5, j = lane&31) then holds, for query j, a 4-row x
// 4-column patch of targets (columns 4h..4h+3) per tile, so the 2x2 average pools of levels 1-2
// are in-lane adds and level 3 needs one xor-32 lane exchange.  Every level is written from the
// f32 accumulators straight from registers, query-minor: the lanes of a store instruction are consecutive
// queries, so each instruction writes whole contiguous 512 B runs.
//
// Who routes where (gemm_path; rmd_corr_gemm_kernel names the answer):
//  * x3          corr_pyramid_x3.hip          compute BF16X3 (the fp32 parity mode), C <= 256, f32 / S24 rows
//  * w8          corr_pyramid_w8.hip          compute BF16, fp16 storage, C <= 256: the performance path, the
//                                             only one that writes the tiles layout
//  * stationary  corr_pyramid_stationary.hip  the same calls when a level-0 band passes 1 GiB (4K frames) and
//                                             w8's 32-bit store offsets no longer reach: 64-bit addressing, rows
//  * tiled       corr_pyramid_tiled.hip       everything else: compute F32 (exact f32 MFMA, fp32-exact), any C,
//                                             BF16 with f32 storage, BF16X3 with C > 256 (as F32); rows
// Each GEMM reads operands that a prep kernel of its own wrote into the caller's workspace (stationary reads
// tiled's), so rmd_corr_prepare routes the same way.  rmd_corr_pyramid_fused (the torch operator's entry) differs
// on w8 only: prep_queries writes the query operand alone and the GEMM stages its targets from fp32 fmap2
// (rmd_corr_prepare_queries + rmd_corr_pyramid_staged are its halves); the pyramid is bit-identical.

#include "corr_pyramid.h"

namespace rmd {
namespace {

enum class Path { W8, STATIONARY, TILED, X3 };

Path gemm_path(const rmd_pyramid_desc& d, int C, int compute) {
    if (compute == RMD_BF16X3) return x3::eligible(d, C) ? Path::X3 : Path::TILED;     // TILED: exact f32
    if (compute == RMD_BF16) {
        if (w8::eligible(d, C)) return Path::W8;
        if (stationary::eligible(d, C)) return Path::STATIONARY;
    }
    return Path::TILED;
}

// the pyramid layout the GEMM of a call writes
int path_layout(Path p) { return p == Path::W8 ? RMD_LAYOUT_TILES : RMD_LAYOUT_ROWS; }

// the compute mode the tiled GEMM runs a call in: BF16X3 calls it could not take as x3 run exact f32
int tiled_compute(int compute) { return compute == RMD_BF16X3 ? RMD_F32 : compute; }

int check_args(const rmd_pyramid_desc* d, int channels, int compute) {
    RMD_REQUIRE(d, RMD_ERR_ARG, "rmd_corr_pyramid: null desc");
    RMD_REQUIRE(channels > 0, RMD_ERR_SHAPE, "rmd_corr_pyramid: channels must be > 0");
    RMD_REQUIRE(d->levels >= 1 && d->levels <= RMD_MAX_LEVELS, RMD_ERR_SHAPE, "rmd_corr_pyramid: bad levels");
    RMD_REQUIRE(compute == RMD_F32 || compute == RMD_BF16 || compute == RMD_BF16X3, RMD_ERR_ARG,
                "rmd_corr_pyramid: compute must be F32, BF16 or BF16X3");
    RMD_REQUIRE(d->storage == RMD_F32 || d->storage == RMD_F16 || d->storage == RMD_S24, RMD_ERR_ARG,
                "rmd_corr_pyramid: storage must be F32, F16 or S24");
    RMD_REQUIRE(d->storage != RMD_S24 || gemm_path(*d, channels, compute) == Path::X3, RMD_ERR_ARG,
                "rmd_corr_pyramid: S24 storage is written by the BF16X3 GEMM only (C <= 256; describe with "
                "rmd_pyramid_describe_for)");
    const int want = path_layout(gemm_path(*d, channels, compute));
    RMD_REQUIRE(d->layout == want, RMD_ERR_ARG,
                "rmd_corr_pyramid: the %s GEMM writes layout %d, desc has layout %d (describe with rmd_pyramid_describe_for)",
                want == RMD_LAYOUT_TILES ? "w8" : "selected", want, d->layout);
    return RMD_OK;
}

}  // namespace
}  // namespace rmd

extern "C" int rmd_pyramid_describe_for(int batch, int height, int width, int levels, int storage, int channels,
                                        int compute, rmd_pyramid_desc* d) {
    int rc = rmd_pyramid_describe_layout(batch, height, width, levels, storage, RMD_LAYOUT_ROWS, d);
    if (rc || channels <= 0) return rc;
    // S24 is an output format of the x3 GEMM: any other GEMM of this call stores F32
    if (storage == RMD_S24 && rmd::gemm_path(*d, channels, compute) != rmd::Path::X3)
        return rmd_pyramid_describe_layout(batch, height, width, levels, RMD_F32, RMD_LAYOUT_ROWS, d);
    if (rmd::gemm_path(*d, channels, compute) == rmd::Path::W8)
        rc = rmd_pyramid_describe_layout(batch, height, width, levels, storage, RMD_LAYOUT_TILES, d);
    return rc;
}

extern "C" size_t rmd_corr_pyramid_workspace_bytes(const rmd_pyramid_desc* d, int channels, int compute) {
    if (!d || channels <= 0) return 0;
    if (compute == RMD_BF16X3) {
        if (rmd::x3::eligible(*d, channels)) return rmd::x3::workspace_bytes(*d);
        compute = RMD_F32;
    }
    const size_t Cp = (size_t)rmd::padded_channels(channels);
    const size_t es = compute == RMD_F32 ? 4 : 2;
    const size_t N = (size_t)d->height * d->width;
    const size_t S = d->query_slots > 0 && (size_t)d->query_slots > N ? (size_t)d->query_slots : N;
    const size_t Npad = (S + 31) / 32 * 32;                         // B operand padded to 32-query tiles
    return (size_t)d->batch * (N + Npad) * Cp * es + 32 * 1024;     // + trash slots (<= 32 x 1 KiB)
}

extern "C" const char* rmd_corr_gemm_kernel(const rmd_pyramid_desc* d, int channels, int compute) {
    if (!d || channels <= 0) return "invalid";
    switch (rmd::gemm_path(*d, channels, compute)) {
        case rmd::Path::W8: return "w8";
        case rmd::Path::STATIONARY: return "stationary";
        case rmd::Path::X3: return "x3";
        default: return "tiled";
    }
}

extern "C" int rmd_corr_prepare(const float* fmap1, const float* fmap2, int channels, float scale,
                                const rmd_pyramid_desc* d, int compute, void* workspace, void* stream) {
    RMD_REQUIRE(fmap1 && fmap2 && workspace, RMD_ERR_ARG, "rmd_corr_prepare: null pointer");
    int rc = rmd::check_args(d, channels, compute);
    if (rc) return rc;
    hipStream_t st = rmd::as_stream(stream);
    switch (rmd::gemm_path(*d, channels, compute)) {
        case rmd::Path::X3: return rmd::x3::prepare(fmap1, fmap2, channels, scale, *d, workspace, st);
        case rmd::Path::W8: return rmd::w8::prepare(fmap1, fmap2, channels, scale, *d, workspace, st);
        default: return rmd::tiled::prepare(fmap1, fmap2, channels, scale, *d, rmd::tiled_compute(compute), workspace, st);
    }
}

extern "C" int rmd_corr_pyramid_prepared(int channels, float scale, const rmd_pyramid_desc* d, int compute,
                                         void* pyramid, void* workspace, void* stream) {
    RMD_REQUIRE(pyramid && workspace, RMD_ERR_ARG, "rmd_corr_pyramid_prepared: null pointer");
    int rc = rmd::check_args(d, channels, compute);
    if (rc) return rc;
    hipStream_t st = rmd::as_stream(stream);
    switch (rmd::gemm_path(*d, channels, compute)) {
        case rmd::Path::X3: return rmd::x3::pyramid(*d, pyramid, workspace, st);
        case rmd::Path::W8: return rmd::w8::pyramid(*d, pyramid, workspace, st);
        case rmd::Path::STATIONARY: return rmd::stationary::pyramid(*d, pyramid, workspace, st);
        default: return rmd::tiled::pyramid(channels, scale, *d, rmd::tiled_compute(compute), pyramid, workspace, st);
    }
}

extern "C" int rmd_corr_prepare_queries(const float* fmap1, int channels, const rmd_pyramid_desc* d, int compute,
                                        void* workspace, void* stream) {
    RMD_REQUIRE(fmap1 && workspace, RMD_ERR_ARG, "rmd_corr_prepare_queries: null pointer");
    int rc = rmd::check_args(d, channels, compute);
    if (rc) return rc;
    RMD_REQUIRE(rmd::gemm_path(*d, channels, compute) == rmd::Path::W8, RMD_ERR_ARG,
                "rmd_corr_prepare_queries: the w8 GEMM only (see rmd_corr_gemm_kernel)");
    return rmd::w8::prepare_queries(fmap1, channels, *d, workspace, rmd::as_stream(stream));
}

extern "C" int rmd_corr_pyramid_staged(const float* fmap2, int channels, float scale, const rmd_pyramid_desc* d,
                                       int compute, void* pyramid, void* workspace, void* stream) {
    RMD_REQUIRE(fmap2 && pyramid && workspace, RMD_ERR_ARG, "rmd_corr_pyramid_staged: null pointer");
    int rc = rmd::check_args(d, channels, compute);
    if (rc) return rc;
    RMD_REQUIRE(rmd::gemm_path(*d, channels, compute) == rmd::Path::W8, RMD_ERR_ARG,
                "rmd_corr_pyramid_staged: the w8 GEMM only (see rmd_corr_gemm_kernel)");
    return rmd::w8::pyramid_staged(fmap2, channels, scale, *d, pyramid, workspace, rmd::as_stream(stream));
}

extern "C" int rmd_corr_pyramid_fused(const float* fmap1, const float* fmap2, int channels, float scale,
                                      const rmd_pyramid_desc* d, int compute, void* pyramid, void* workspace,
                                      void* stream) {
    RMD_REQUIRE(fmap1 && fmap2 && pyramid && workspace, RMD_ERR_ARG, "rmd_corr_pyramid_fused: null pointer");
    int rc = rmd::check_args(d, channels, compute);
    if (rc) return rc;
    if (rmd::gemm_path(*d, channels, compute) != rmd::Path::W8)
        return rmd_corr_pyramid(fmap1, fmap2, channels, scale, d, compute, pyramid, workspace, stream);
    rc = rmd::w8::prepare_queries(fmap1, channels, *d, workspace, rmd::as_stream(stream));
    if (rc) return rc;
    return rmd::w8::pyramid_staged(fmap2, channels, scale, *d, pyramid, workspace, rmd::as_stream(stream));
}

extern "C" int rmd_corr_pyramid(const float* fmap1, const float* fmap2, int channels, float scale,
                                const rmd_pyramid_desc* d, int compute, void* pyramid, void* workspace, void* stream) {
    int rc = rmd_corr_prepare(fmap1, fmap2, channels, scale, d, compute, workspace, stream);
    if (rc) return rc;
    return rmd_corr_pyramid_prepared(channels, scale, d, compute, pyramid, workspace, stream);
}
