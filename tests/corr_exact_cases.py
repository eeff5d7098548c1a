"""Inputs and exact expectations of the RAFT correlation forward in every compute mode (numpy only).

tests/test_corr_exact.py checks this module itself (preconditions, the restated rounding rules, the
wrapper against the reference's golden outputs, the comparators against planted errors);
tests/test_gpu_corr_exact.py compares the HIP kernels with it.

Why the expectations are exact
------------------------------
Every feature is an integer over a power of two and every scale a power of two.  With n1, n2 the integer
numerators and pmax = max|n1| * max|n2|, a level-l element is (sum of C * 4^l integer products) times a
power of two.  While C * pmax * 4^(L-1) <= 2^24 (check_exact(), asserted for every case, never assumed)

  * every bf16 operand is exact (families below), every split-bf16 operand hi + lo is exact, and at most
    one operand of a product has a low part, so the dropped lo.lo term is zero;
  * every product and every fp32 partial sum, in any order, is an integer below 2^24 in the common unit:
    the MFMA accumulation is exact whatever the k order, and so are the running unscaled sums of the
    stationary / w8 epilogues and the successive 0.25f * (a + b + c + d) form of the others;
  * the value a GEMM must store is therefore the float64 level, rounded ONCE by the storage rule:
    fp16 round-to-nearest-even, RMD_S24 (include/rmd.h: add 0x80 to the fp32 word, keep its top three
    bytes; NaN stays quiet), or nothing for f32.  The pyramid assertion is bit equality.

The on-the-fly lookup is the same lookup on a virtual pyramid: level l = (fmap1 * scale)^T P_l with P_l
the successive 2x2 averages of fmap2.  rmd_corr_otf_prepare pools in fp32 (otf_pool2_kernel: exact for
these inputs), scales the QUERY rows and converts both operands (otf_segments_kernel: targets with scale
1, queries with `scale`; (T)f is bf16 round-to-nearest-even).  In the fp32 (split-bf16) and fp32-exact
modes P_l is exact (a pooled base-family target needs at most 10 bits, a pooled fine2 target 13: hi + lo);
in the bf16 mode P_l is rounded to bf16 first, and everything after that is exact again (otf_levels()).
Pooled base-family targets of up to three levels are bf16 values already, so that rounding would go
unseen: the fine2 cases (fmap2 integers in [-127, 127] / 128) make it real from level 1 on.

The lookup bound K
------------------
rmd_corr_lookup (corr_lookup.hip: rows_body_buf / the tiles bodies, emit_row / emit_row_buf) and
rmd_corr_otf_lookup (corr_otf.hip, both the MFMA and the per-query patch path) evaluate one output as

    h_j = fma(fx, v[j][a+1] - v[j][a], v[j][a])       j = the two patch rows, each: 1 subtraction, 1 fma
    out = fma(fy, h_1 - h_0, h_0)                     1 subtraction, 1 fma

on exactly known values v (|v| <= M, the largest |stored value| of that query's level map) with exactly
known weights: fx = x/2^l - floor(x/2^l) in fp32 is exact (a power-of-two division, then a difference of
two floats with the same exponent or smaller).  The fp16 paths' fma(v1, 1, -v0) (diff_f32<MIX>) is the
same single rounding of the exact difference.  With u = 2^-24, |b - a| <= 2M and 0 <= f < 1:

    |h - h*|     <= f * 2M * u (the difference's rounding) + M * u (the fma's)            <= 3 u M
    |out - out*| <= 3 u M (the h errors, a convex combination)
                    + fy * 2M(1 + 3u) * u (difference) + M(1 + 3u)(1 + 2u) * u (fma)      <= 6 u M + 13 u^2 M

and the float64 reference's own error is below 2^-50 M.  So K = 6 to first order; K_LOOKUP = 8 is the next
power of two and covers the second-order terms ten million times over.  (Charging each h error twice, once
per use, gives 12 and would suggest 16; the h errors enter through a convex combination, so 8 holds.)  The record
kernel of the on-the-fly BACKWARD (otf_record_kernel) uses the (1 - f) a + f b form; it is not on any
forward path and is not covered here.

Reference semantics of the lookup (lookup_reference(), pinned to the reference's golden outputs on the CPU):
a masked level is 0 whatever the coordinate; a 1-pixel level is NaN; a NaN or +-inf coordinate gives a NaN
window on every other level; a finite coordinate so far off that no level's window meets its map gives
zeros (it is moved to a nearby value with the same property before numpy sees it: floor() of 3e38 does
not fit an integer); weights come from the float32 coordinate over 2^l, which is exact in float64 too.
One hand-placed query, (2, 3e38), is finite only in pixel coordinates: the reference's fp32 normalisation
to [-1, 1] (raft.py:73-74) overflows on it at level 0 and grid_sample returns NaN there.  The HIP kernels
work in pixel coordinates, where it is an ordinary far-off query, and give zeros (corr_lookup.hip
level_setup, the same lines in otf_lookup_kernel); the contract here is the kernels' documented one.
"""
from functools import lru_cache

import numpy as np

import lookup_digest_cases as lc
import oracle
from oracle.corr import _avg_pool2

U = 2.0 ** -24
K_LOOKUP = 8
LEVELS = 4

# precision -> (compute, storage asked for); storage "s24" falls back to "f32" off the x3 GEMM
MODES = {"bf16": ("bf16", "f16"), "bf16-f32": ("bf16", "f32"), "fp32": ("x3", "s24"), "fp32-f32": ("x3", "f32"),
         "fp32-exact": ("f32", "f32"), "fp32-f16": ("f32", "f16")}

# ---- restated rounding rules ------------------------------------------------------------------------


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even) as float32, on the bit pattern; NaN -> a quiet NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    r = np.where(nan, (u | np.uint32(0x00400000)) & np.uint32(0xffff0000), r)
    return r.astype(np.uint32).view(np.float32)


def s24_round(x):
    """float32 -> RMD_S24 as float32 (low mantissa byte zero): include/rmd.h, word + 0x80, top three bytes;
    NaN stays a quiet NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = np.where(nan, u | np.uint32(0x00400000), u + np.uint32(0x80)) & np.uint32(0xffffff00)
    return r.astype(np.uint32).view(np.float32)


def s24_bytes(x):
    """The three stored bytes (n, 3) of s24_round(x): bytes 1..3 of the little-endian word."""
    w = s24_round(x).reshape(-1).view(np.uint32)
    return np.stack([(w >> np.uint32(8 * k)) & np.uint32(0xff) for k in (1, 2, 3)], axis=1).astype(np.uint8)


def as_f32_exact(x64):
    """x as float32, after asserting that nothing is lost."""
    x32 = x64.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x64), "value is not a float32"
    return x32


def round_storage(x64, storage):
    """The exact float64 value rounded once by the storage rule, as float32."""
    x32 = as_f32_exact(x64)
    if storage == "f32":
        return x32
    if storage == "f16":
        return x32.astype(np.float16).astype(np.float32)
    assert storage == "s24", storage
    return s24_round(x32)


def storage_ulp_up(x32, storage):
    """The next stored value above |x| (one storage ulp away from zero), as float32."""
    if storage == "f16":
        h = np.float16(x32)
        return np.float32(np.nextafter(h, np.float16(np.inf) if h >= 0 else np.float16(-np.inf)))
    step = np.uint32(0x100 if storage == "s24" else 1)
    return (np.float32(x32).reshape(1).view(np.uint32) + step).view(np.float32)[0]


# ---- feature families (integer numerators over a power of two) -----------------------------------------

class Features:
    """fmap = n / den per map; `channels` real channels, zero-padded to `padded` for the GEMM call."""

    def __init__(self, n1, den1, n2, den2, padded=None):
        self.n1, self.n2, self.den1, self.den2 = n1.astype(np.int64), n2.astype(np.int64), den1, den2
        self.channels = n1.shape[1]
        self.padded = padded or self.channels

    def _map(self, n, den):
        f = (n / float(den)).astype(np.float32)
        if self.padded != self.channels:
            f = np.pad(f, ((0, 0), (0, self.padded - self.channels), (0, 0), (0, 0)))
        return np.ascontiguousarray(f)

    @property
    def fmap1(self):
        return self._map(self.n1, self.den1)

    @property
    def fmap2(self):
        return self._map(self.n2, self.den2)


def _draw(rng, lim, shape):
    return rng.integers(-lim, lim + 1, shape)


@lru_cache(maxsize=None)
def features(family, b, c, h, w, padded=None):
    """base:    both maps integers in [-8, 8] / 8 (bf16-exact)
    digest:  lookup_digest_cases.features(shape): integers in [-64, 64] / 32, b = 2, c = 16 (bf16-exact)
    cross12: fmap1 integers in [-512, 512] / 512 (a non-zero low part in the split), fmap2 base: hi.hi + lo.hi
    cross21: the other assignment: hi.hi + hi.lo
    mid:     both maps integers in [-64, 64] / 32 like the digest family, any shape: with 16 channels the
             level-0 sums pass 2^11, so the fp16 rounding is real at every level (base-family sums of 256
             channels are fp16 values up to level 1 or 2)
    bias:    fmap1 integers in [256, 512] / 512, fmap2 integers in [4, 8] / 8: all products positive, so with
             64 channels the level-0 sums pass 2^17 and the S24 rounding (16 significant bits) is real at
             every level, ties included (random-sign sums of the other families stay below 2^16 at level 0)
    fine2:   fmap1 base, fmap2 integers in [-127, 127] / 128 (bf16-exact; its 2x2 averages are not: the on-the-fly
             bf16 mode's target rounding is real from level 1 on, ties included)"""
    if family == "digest":
        assert (b, c) == (lc.BATCH, lc.CHANNELS)
        f1, f2 = lc.features((h, w))
        n1, n2 = np.rint(f1 * 32.0), np.rint(f2 * 32.0)
        assert np.array_equal(n1 / 32.0, f1) and np.array_equal(n2 / 32.0, f2)
        return Features(n1, 32, n2, 32, padded)
    rng = np.random.default_rng([b, c, h, w, {"base": 0, "cross12": 1, "cross21": 2, "fine2": 3, "mid": 4, "bias": 5}[family]])
    shape = (b, c, h, w)
    if family == "base":
        return Features(_draw(rng, 8, shape), 8, _draw(rng, 8, shape), 8, padded)
    if family == "mid":
        return Features(_draw(rng, 64, shape), 32, _draw(rng, 64, shape), 32, padded)
    if family == "bias":
        return Features(rng.integers(256, 513, shape), 512, rng.integers(4, 9, shape), 8, padded)
    if family == "fine2":
        return Features(_draw(rng, 8, shape), 8, _draw(rng, 127, shape), 128, padded)
    wide, narrow = _draw(rng, 512, shape), _draw(rng, 8, shape)
    wide.reshape(-1)[:2] = (512, -511)                      # the extremes are always present
    if family == "cross12":
        return Features(wide, 512, narrow, 8, padded)
    assert family == "cross21", family
    return Features(narrow, 8, wide, 512, padded)


# ---- the exactness precondition -----------------------------------------------------------------------

def _split(f32):
    hi = bf16_round(f32)
    lo = bf16_round(f32 - hi)
    return hi, lo


def check_exact(ft, levels, compute, scale):
    """Assert the precondition of the module docstring for features `ft` at `levels` levels in compute
    mode `compute` ("bf16", "x3", "f32") with `scale`; a violation is an error in the case table."""
    m, e = np.frexp(scale)
    assert m == 0.5 and -60 < e < 60, f"scale {scale} is not a power of two"
    pmax = int(np.abs(ft.n1).max()) * int(np.abs(ft.n2).max())
    assert ft.channels * pmax * 4 ** (levels - 1) <= 2 ** 24, (ft.channels, pmax, levels)
    f1, f2 = ft.fmap1, ft.fmap2
    if compute == "bf16":
        assert np.array_equal(bf16_round(f1), f1) and np.array_equal(bf16_round(f2 * np.float32(scale)), f2 * np.float32(scale))
    elif compute == "x3":
        los = []
        for f in (f1, f2):
            hi, lo = _split(f)
            assert np.array_equal(hi.astype(np.float64) + lo, f), "hi + lo is not the value"
            assert np.abs(hi).max() <= np.abs(f).max(), "hi exceeds the largest numerator"
            los.append(bool(lo.any()))
        assert not all(los), "both maps have a low part: the dropped lo.lo term is not zero"
    else:
        assert compute == "f32", compute


def level_sums(ft, levels):
    """Unscaled integer sums: level l (B, N, H_l, W_l) int64 = sum over C channels and the 4^l level-0
    targets of n1 * n2.  The matmul runs in float64 on integers below 2^53 and is checked to be integral."""
    b, c, h, w = ft.n1.shape
    a = ft.n1.reshape(b, c, h * w).astype(np.float64)
    s = np.matmul(a.transpose(0, 2, 1), ft.n2.reshape(b, c, h * w).astype(np.float64))
    s0 = np.rint(s).astype(np.int64)
    assert np.array_equal(s0, s)
    out = [s0.reshape(b, h * w, h, w)]
    for _ in range(1, levels):
        x = out[-1]
        h2, w2 = x.shape[-2] // 2, x.shape[-1] // 2
        x = x[..., : 2 * h2, : 2 * w2]
        out.append(x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2])
    assert max(int(np.abs(x).max()) for x in out if x.size) <= 2 ** 24
    return out


def exact_pyramid(ft, levels, scale):
    """The float64 pyramid times `scale`: list of (B, N, H_l, W_l), exact."""
    unit = scale / (ft.den1 * ft.den2)
    return [s.astype(np.float64) * (unit / 4.0 ** l) for l, s in enumerate(level_sums(ft, levels))]


def stored_pyramid(ft, levels, scale, storage):
    """What a GEMM must store: exact_pyramid rounded once by `storage`; list of float32 (B, N, H_l, W_l)."""
    return [round_storage(x, storage) for x in exact_pyramid(ft, levels, scale)]


def pyramid_mismatches(got32, want32):
    """Number of elements whose float32 bit patterns differ."""
    got32, want32 = np.ascontiguousarray(got32, np.float32), np.ascontiguousarray(want32, np.float32)
    assert got32.shape == want32.shape, (got32.shape, want32.shape)
    return int((got32.view(np.int32) != want32.view(np.int32)).sum())


# ---- the pyramid case table -----------------------------------------------------------------------------

class PyramidCase:
    def __init__(self, name, precision, family, b, c, h, w, scale, route, storage, padded=None):
        self.name, self.precision, self.family, self.route, self.storage = name, precision, family, route, storage
        self.b, self.c, self.h, self.w, self.scale, self.padded = b, c, h, w, scale, padded
        self.compute = MODES[precision][0]

    @property
    def gemm_channels(self):
        return self.padded or self.c

    def features(self):
        return features(self.family, self.b, self.c, self.h, self.w, self.padded)

    def stored(self):
        return _stored(self)


@lru_cache(maxsize=None)
def _stored(case):
    check_exact(case.features(), LEVELS, case.compute, case.scale)
    return tuple(stored_pyramid(case.features(), LEVELS, case.scale, case.storage))


def _pc(name, precision, family, b, c, h, w, scale, route, storage, padded=None):
    return PyramidCase(f"{route}-{precision}-{name}", precision, family, b, c, h, w, scale, route, storage, padded)


PYRAMID_CASES = [
    # w8 (bf16 operands, fp16 tiles layout, channels padding to 256)
    _pc("b2c256-16x24", "bf16", "base", 2, 256, 16, 24, 1 / 16, "w8", "f16"),
    _pc("b1c193-17x33", "bf16", "base", 1, 193, 17, 33, 1 / 16, "w8", "f16"),          # zero-padded channels, ragged
    _pc("b2c256-40x64", "bf16", "base", 2, 256, 40, 64, 1 / 16, "w8", "f16"),          # last block row of 8, query tiles split 4 ways: not paired
    # paired last block row (w8_balance: fewer than 32 query tiles, so no query split; W % 32 == 0; last row <= 8)
    _pc("b1c256-24x32", "bf16", "base", 1, 256, 24, 32, 1 / 16, "w8", "f16"),          # second half stores rows on every level
    _pc("b1c256-18x32", "bf16", "base", 1, 256, 18, 32, 1 / 16, "w8", "f16"),          # second half mostly past the map
    _pc("b1c256-23x96", "bf16", "base", 1, 256, 23, 96, 1 / 16, "w8", "f16"),          # odd column blocks
    _pc("b2c16p256-16x24", "bf16", "digest", 2, 16, 16, 24, 1 / 4, "w8", "f16", 256),  # digest kind bf16-tiles
    _pc("b2c16p256-15x20", "bf16", "digest", 2, 16, 15, 20, 1 / 4, "w8", "f16", 256),  # 1-pixel level 3
    _pc("b2c16p256-40x64-mid", "bf16", "mid", 2, 16, 40, 64, 1 / 4, "w8", "f16", 256),   # fp16 rounding at level 0 too
    _pc("b1c16p256-17x33-mid", "bf16", "mid", 1, 16, 17, 33, 1 / 4, "w8", "f16", 256),
    # tiled, bf16 operands (fp16 rows)
    _pc("b2c16-16x24", "bf16", "digest", 2, 16, 16, 24, 1 / 4, "tiled", "f16"),        # digest kind bf16-rows
    _pc("b2c16-15x20", "bf16", "digest", 2, 16, 15, 20, 1 / 4, "tiled", "f16"),
    _pc("b1c128-17x23", "bf16", "base", 1, 128, 17, 23, 1 / 8, "tiled", "f16"),
    _pc("b2c256-16x24", "bf16-f32", "base", 2, 256, 16, 24, 1 / 16, "tiled", "f32"),
    _pc("b1c40-17x23", "bf16-f32", "base", 1, 40, 17, 23, 1 / 4, "tiled", "f32"),
    # x3 (split bf16), S24 and f32 rows
    _pc("b1c256-8x8", "fp32", "base", 1, 256, 8, 8, 1 / 16, "x3", "s24"),
    _pc("b3c96-9x70", "fp32", "base", 3, 96, 9, 70, 1 / 8, "x3", "s24"),
    _pc("b2c200-23x40", "fp32", "base", 2, 200, 23, 40, 1 / 16, "x3", "s24"),
    _pc("b2c64-16x24-hilo", "fp32", "cross21", 2, 64, 16, 24, 1 / 8, "x3", "s24"),
    _pc("b2c64-16x24-lohi", "fp32", "cross12", 2, 64, 16, 24, 1 / 8, "x3", "s24"),
    _pc("b2c64-16x24-bias", "fp32", "bias", 2, 64, 16, 24, 1 / 8, "x3", "s24"),         # S24 rounding at level 0 too
    _pc("b2c16-16x24", "fp32", "digest", 2, 16, 16, 24, 1 / 4, "x3", "s24"),           # digest kind fp32
    _pc("b2c16-15x20", "fp32", "digest", 2, 16, 15, 20, 1 / 4, "x3", "s24"),
    _pc("b1c256-8x8", "fp32-f32", "base", 1, 256, 8, 8, 1 / 16, "x3", "f32"),
    _pc("b3c96-9x70", "fp32-f32", "base", 3, 96, 9, 70, 1 / 8, "x3", "f32"),
    _pc("b2c200-23x40", "fp32-f32", "base", 2, 200, 23, 40, 1 / 16, "x3", "f32"),
    _pc("b2c64-16x24-hilo", "fp32-f32", "cross21", 2, 64, 16, 24, 1 / 8, "x3", "f32"),
    _pc("b2c64-16x24-lohi", "fp32-f32", "cross12", 2, 64, 16, 24, 1 / 8, "x3", "f32"),
    _pc("b2c16-16x24", "fp32-f32", "digest", 2, 16, 16, 24, 1 / 4, "x3", "f32"),       # digest kind fp32-f32
    _pc("b2c16-15x20", "fp32-f32", "digest", 2, 16, 15, 20, 1 / 4, "x3", "f32"),
    # tiled, f32 operands
    _pc("b2c32-16x24", "fp32-exact", "base", 2, 32, 16, 24, 1 / 4, "tiled", "f32"),
    _pc("b1c320-16x24", "fp32", "base", 1, 320, 16, 24, 1 / 16, "tiled", "f32"),        # C > 256: f32 storage
    _pc("b1c32-17x23-mid", "fp32-f16", "mid", 1, 32, 17, 23, 1 / 8, "tiled", "f16"),
]

# digest kind -> name of its pyramid case per shape
DIGEST_PYRAMID = {(kind, shape): next(c for c in PYRAMID_CASES
                                      if c.family == "digest" and (c.h, c.w) == shape and c.precision == lc._PRECISION[kind]
                                      and (c.route == "w8") == (kind == "bf16-tiles"))
                  for kind in lc.KINDS for shape in lc.SHAPES}
ALL_RADII = tuple(range(1, 9))


# ---- lookup reference and comparator --------------------------------------------------------------------

def lookup_reference(stored, coords, radius, mask_costs=()):
    """oracle.corr_lookup in float64 on the stored levels (list of (B, P, H_l, W_l)), for float32 `coords`
    (B, 2, h, w) with h * w = P, under the contract of the module docstring -> float64 (B, L d^2, h, w)."""
    coords = np.asarray(coords)
    assert coords.dtype == np.float32, coords.dtype
    levels = len(stored)
    b, _, h, w = coords.shape
    d2 = (2 * radius + 1) ** 2
    mh, mw = stored[0].shape[-2:]
    co = coords.astype(np.float64)
    bad = ~np.isfinite(co).all(axis=1)                                    # (B, h, w): NaN / +-inf queries
    # beyond `far` every level's (2r+2)^2 patch lies off its map: |c| / 2^l >= max(H, W) + r + 2 for all l
    far = float(2 ** (levels - 1) * (max(mh, mw) + radius + 2))
    with np.errstate(invalid="ignore"):
        off = np.isfinite(co) & (np.abs(co) > far)
    safe = np.where(np.isfinite(co), co, 0.0)
    safe = np.where(off, np.sign(co) * far, safe)
    out = oracle.corr_lookup([np.asarray(x, dtype=np.float64) for x in stored], safe, radius, tuple(mask_costs))
    gone = off.any(axis=1) & ~bad                                         # (B, h, w): finite, off every map
    for l in range(levels):
        hl, wl = stored[l].shape[-2:]
        if l + 3 in mask_costs or hl < 2 or wl < 2:
            continue                                                      # 0 / NaN whatever the coordinate
        win = out[:, l * d2:(l + 1) * d2]
        assert not win.transpose(0, 2, 3, 1)[gone].any(), "a far-off window is not zero"
        win[np.broadcast_to(bad[:, None], win.shape)] = np.nan
    return out


def lookup_bound(stored, radius, h, w):
    """K_LOOKUP * 2^-24 * M per output element (B, L d^2, h, w): M the largest |stored value| of the
    query's own level-l map."""
    d2 = (2 * radius + 1) ** 2
    out = []
    for lvl in stored:
        b, p = lvl.shape[:2]
        m = np.abs(np.asarray(lvl, dtype=np.float64)).reshape(b, p, -1).max(axis=2) if lvl[0, 0].size else np.zeros((b, p))
        out.append(np.broadcast_to((K_LOOKUP * U * m).reshape(b, 1, h, w), (b, d2, h, w)))
    return np.concatenate(out, axis=1)


def check_lookup(got, ref, bound):
    """Every element: NaN exactly where the reference has NaN, |got - ref| <= bound elsewhere.  Returns
    (worst err / bound, elements compared); raises AssertionError naming the worst element."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (f"NaN positions differ: {int((np.isnan(got) & ~nan).sum())} extra, "
                                                f"{int((~np.isnan(got) & nan).sum())} missing")
    assert np.isfinite(ref[~nan]).all()
    err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, ref)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)                    # err > 0 over a zero bound -> inf
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= 1.0:
        k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"lookup bound exceeded at {k}: got {got[k]!r} ref {ref[k]!r} err {err[k]:.3e} > "
                             f"{bound[k]:.3e} ({int((ratio > 1.0).sum())} of {ratio.size} elements)")
    return worst, int(ratio.size)


def lookup_masks():
    """The two lookups of a digest case: unmasked, and level 1 masked (cost level 4)."""
    return ((), (4,))


# ---- on-the-fly lookup ------------------------------------------------------------------------------------

class OtfCase:
    def __init__(self, name, b, c, h, w, levels, radius, scale, mask=(), coords="lattice", precisions=("fp32", "fp32-exact", "bf16"),
                 sample=None, spread=24, family="base"):
        self.name, self.b, self.c, self.h, self.w, self.levels, self.radius = name, b, c, h, w, levels, radius
        self.scale, self.mask, self.coords_kind, self.precisions, self.sample, self.spread = scale, mask, coords, precisions, sample, spread
        self.family = family

    def features(self):
        return features(self.family, self.b, self.c, self.h, self.w)

    def coords(self):
        return _otf_coords(self)

    def queries(self):
        """Flat query indices (per image) the reference is evaluated on: all, or `sample` seeded ones plus
        the four corners and the hand-placed queries."""
        n = self.h * self.w
        if self.sample is None:
            return np.arange(n)
        rng = np.random.default_rng(self.sample)
        fixed = [0, self.w - 1, n - self.w, n - 1] + [5 * i for i in range(len(lc.special_points(self.h, self.w)))]
        return np.unique(np.concatenate([rng.choice(n, self.sample, replace=False), fixed]))


OTF_CASES = [
    OtfCase("b2c32-16x24-l4r4", 2, 32, 16, 24, 4, 4, 1 / 4, family="fine2"),
    OtfCase("b1c40-17x23-l3r3-mask1", 1, 40, 17, 23, 3, 3, 1 / 4, mask=(4,)),            # ragged, Cp padding
    OtfCase("b1c40-17x23-l3r3-fine", 1, 40, 17, 23, 3, 3, 1 / 4, family="fine2"),        # the same, targets that round
    OtfCase("b1c320-14x20-l3r3", 1, 320, 14, 20, 3, 3, 1 / 16),                          # runtime-channel path
    OtfCase("b2c128-18x40-l3r5", 2, 128, 18, 40, 3, 5, 1 / 8),                           # f32 operands: runtime loop
    OtfCase("b1c48-20x36-l2r8", 1, 48, 20, 36, 2, 8, 1 / 4),
    OtfCase("b1c8-9x70-l1r1", 1, 8, 9, 70, 1, 1, 1 / 2),
    # flow scattered over the whole map: wide union boxes.  At 4 x 600 a box holds at most 4 x 38 segments and
    # stays on the MFMA path; at 96 x 256 the level-0 boxes pass 1024 segments: the per-query path
    OtfCase("b1c24-4x600-l2r3-scattered", 1, 24, 4, 600, 2, 3, 1 / 4, coords="scattered"),
    OtfCase("b1c24-96x256-l2r3-scattered", 1, 24, 96, 256, 2, 3, 1 / 4, coords="scattered", sample=256),
    OtfCase("b1c32-512x256-l1r1-wide", 1, 32, 512, 256, 1, 1, 1 / 4, precisions=("bf16",), sample=256, spread=16),
]


@lru_cache(maxsize=None)
def _otf_coords(case):
    """float32 coordinates on a 1/8 lattice: the pixel grid plus up to `spread`/8 pixels ("lattice"), or
    scattered over the whole map and 5 / 2 pixels beyond it ("scattered": union boxes of more than 1024
    segments); lookup_digest_cases.special_points spread over image 0 at stride 5."""
    b, h, w = case.b, case.h, case.w
    rng = np.random.default_rng([h, w, case.radius])
    if case.coords_kind == "scattered":
        co = np.stack([rng.integers(-40, 8 * (w + 5) + 1, (b, h, w)), rng.integers(-16, 8 * (h + 2) + 1, (b, h, w))], 1) / 8.0
    else:
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        co = np.stack([xs, ys])[None].repeat(b, 0) + rng.integers(-case.spread, case.spread + 1, (b, 2, h, w)) / 8.0
    flat = co.reshape(b, 2, h * w)
    for i, (x, y) in enumerate(lc.special_points(h, w)):
        if 5 * i < h * w:
            flat[0, 0, 5 * i], flat[0, 1, 5 * i] = x, y
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(co.astype(np.float32))


def otf_levels(case, precision, queries=None):
    """The virtual pyramid of the on-the-fly lookup: level l (B, P, H_l, W_l) float64 = (fmap1 * scale)^T P_l
    over the queries `queries` (flat indices, default all), P_l the successive 2x2 averages of fmap2 —
    rounded to bf16 in the bf16 mode, where rmd_corr_otf_prepare converts the unscaled targets.  Asserts
    the exactness precondition for the mode."""
    ft = case.features()
    compute = MODES[precision][0]
    check_exact(ft, case.levels, compute, case.scale)
    b, c, h, w = ft.n1.shape
    q = ft.fmap1.astype(np.float64).reshape(b, c, h * w) * case.scale
    if queries is not None:
        q = q[:, :, queries]
    assert np.array_equal(bf16_round(q.astype(np.float32)), q), "the scaled query operand is not a bf16"
    out, p = [], ft.fmap2.astype(np.float64)
    for l in range(case.levels):
        if l:
            p = _avg_pool2(p)
        p32 = as_f32_exact(p)
        if compute == "bf16":
            t = bf16_round(p32).astype(np.float64)
        else:
            hi, lo = _split(p32)
            assert np.array_equal(hi.astype(np.float64) + lo, p), "a pooled target needs more than hi + lo"
            t = p
        # units: q numerators over den1 / scale, targets over den2 * 4^l: every partial sum an integer below 2^24
        assert c * int(np.abs(ft.n1).max()) * int(np.abs(ft.n2).max()) * 4 ** l <= 2 ** 24
        hl, wl = p.shape[-2:]
        v = np.matmul(q.transpose(0, 2, 1), t.reshape(b, c, hl * wl))
        as_f32_exact(v)
        out.append(v.reshape(b, q.shape[2], hl, wl))
    return out


# ---- which kernel paths a case reaches (host-side restatements of the dispatch) ---------------------------

OTF_MAX_TASKS = 1024        # corr_otf.hip kMaxTasks: a block's box of more (row, segment) tasks goes per query
OTF_WIDE_BLOCKS = 4096      # corr_otf.hip kWideBlocks: bf16 takes 16 x 4 query blocks from this many 16 x 2 ones


def otf_block_shape(case, precision):
    """(width, height) in queries of rmd_corr_otf_lookup's query block for this case."""
    blocks = ((case.w + 15) // 16) * ((case.h + 1) // 2) * case.b
    return (16, 4) if precision == "bf16" and blocks >= OTF_WIDE_BLOCKS else (16, 2)


def otf_channel_path(case, precision):
    """"compiled" (query fragments of a compiled channel count) or "runtime" (the channel loop)."""
    cp = next((c for c in (32, 64, 128, 256) if case.c <= c), (case.c + 127) // 128 * 128)
    return "runtime" if (precision == "fp32-exact" and cp >= 128) or cp > 256 else "compiled"


def otf_box_paths(case, precision):
    """{(level, path)} over all query blocks, path in "mfma", "per-query", "empty": otf_lookup_kernel's box
    of a block (window origins from the clamped level coordinate, clipped to the map, whole 16-pixel
    segments) and its task count against OTF_MAX_TASKS."""
    bx, by = otf_block_shape(case, precision)
    co, k = case.coords(), 2 * case.radius + 2
    seen = set()
    for l in range(case.levels):
        lh, lw = case.h >> l, case.w >> l
        if l + 3 in case.mask or lh < 2 or lw < 2:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            r = co * np.float32(1.0 / 2 ** l)
            c = np.where(np.isnan(r), np.float32(-1.0e6), np.clip(r, np.float32(-1.0e6), np.float32(1.0e6)))
        org = np.floor(c).astype(np.int64) - case.radius                 # (B, 2, H, W)
        for y0 in range(0, case.h, by):
            for x0 in range(0, case.w, bx):
                o = org[:, :, y0:y0 + by, x0:x0 + bx].reshape(case.b, 2, -1)
                lo, hi = o.min(axis=2), o.max(axis=2) + k - 1
                for b in range(case.b):
                    bx0, bx1 = max(lo[b, 0], 0), min(hi[b, 0], lw - 1)
                    by0, by1 = max(lo[b, 1], 0), min(hi[b, 1], lh - 1)
                    ntask = max(by1 - by0 + 1, 0) * ((bx1 >> 4) - (bx0 >> 4) + 1 if bx1 >= bx0 else 0)
                    seen.add((l, "empty" if ntask == 0 else "mfma" if ntask <= OTF_MAX_TASKS else "per-query"))
    return seen


_COMPUTE = {"bf16": "RMD_BF16", "x3": "RMD_BF16X3", "f32": "RMD_F32"}
_STORAGE = {"f16": "RMD_F16", "f32": "RMD_F32", "s24": "RMD_S24"}


def library_route(case):
    """(GEMM kernel name, storage name, desc) the library reports for a pyramid case: host-only calls."""
    from rmd import _lib
    compute = getattr(_lib, _COMPUTE[case.compute])
    asked = getattr(_lib, _STORAGE[MODES[case.precision][1]])
    d = _lib.describe_for(case.b, case.h, case.w, LEVELS, asked, case.gemm_channels, compute)
    name = _lib.lib().rmd_corr_gemm_kernel(d, case.gemm_channels, compute).decode()
    return name, {getattr(_lib, v): k for k, v in _STORAGE.items()}[d.storage], d
