"""Shared case table of test_oracle_corr_backward.py / test_gpu_corr_backward_stages.py: seeded inputs of the
RAFT correlation backward's stages with their float64 oracle results (oracle/corr.py, the staged oracle),
built once per process (lru_cache) and never modified.

Tolerance rule, the same for G, P and the unpooled gradient: per case, e = max|oracle in float32 - oracle in
float64| / max|float64| (CPU only, computed here), and the kernel is gated at max(1e-6, 8 e), max-normalised
against float64.  1e-6 is the project's gate for short fp32 sums (test_dicl_stack_int_edges_vs_oracle); the
factor 8 covers the kernels' separable x-then-y order with fused multiply-adds against the oracle's direct
four-weight product, and the spread of a maximum.  Nothing here comes from a kernel.

Range of e over the table (float32 run of the oracle against its float64 run): G of one lookup
0.7e-7 .. 1.4e-7, G summed over the lookups of a case 0.8e-7 .. 1.7e-7 (17 lookups), P 0 .. 0.4e-7, unpooled
gradient 0 .. 0.9e-7 (0: one level at scale 1 is a copy) — so the gate is 1e-6 for P and the unpooling and
1.0e-6 .. 1.4e-6 for G.
"""

import functools
import zlib

import numpy as np

import oracle

FLOOR = 1e-6
FACTOR = 8.0

# ---- G: (B, h, w, levels, radius, lookups, per-lookup mask_costs, accumulate into a non-zero G) -----------
# One lookup per radius, B = 2, 4 levels, N no multiple of 64; (K = 2r + 2 patch rows over three parts of PR =
# ceil(K / 3) rows: r = 1 leaves the last part empty, r = 2, 5, 8 fill all three, r = 3, 4, 6, 7 leave it
# short).  19x26: widths 26 / 13 / 6 / 3 (a patch row spans 2 and 3 chunks and ends in a partial chunk), level 1
# masked; 9x70: level 3 is 1 x 8 (no gradient).
LOOKUP_CASES = [
    (2, 16, 21, 4, 1, 1, ((),), False),
    (2, 17, 22, 4, 2, 1, ((),), False),
    (2, 19, 26, 4, 3, 1, ((4,),), False),
    (2, 9, 70, 4, 4, 1, ((),), False),
    (2, 16, 25, 4, 5, 1, ((),), False),
    (2, 17, 29, 4, 6, 1, ((),), False),
    (2, 19, 37, 4, 7, 1, ((3, 6),), False),
    (2, 18, 33, 4, 8, 1, ((),), False),
]
# The build's tiling: 64-query blocks, segments of 16 target rows built 2 at a time, tiles of 4 chunk columns,
# lookups in groups of 4, 16 per launch.  Heights 16 (one whole segment), 17 (a 1-row segment), 33 (two and a
# row); widths 32 / 33 / 70 (4, 5, 9 chunks per row: one tile, a tile of one chunk, two tiles and one chunk);
# N = 64 and 65, 455 = 65 x 7, 2310; 1, 4, 5, 16 and 17 lookups (17: a second, accumulating launch).
BUILD_CASES = [
    (2, 16, 32, 3, 4, 4, ((), (4,), (3, 5), ()), False),
    (1, 17, 33, 4, 3, 5, ((), (), (6,), (), (3,)), False),
    (1, 33, 70, 4, 4, 1, ((),), False),
    (2, 17, 40, 3, 2, 17, tuple((4,) if i % 5 == 3 else () for i in range(17)), False),
    (1, 8, 8, 2, 1, 16, tuple(() for _ in range(16)), False),
    (1, 13, 35, 3, 5, 4, ((), (5,), (), ()), True),
    (1, 5, 13, 2, 8, 2, ((), ()), False),
]


def case_id(case):
    b, h, w, levels, r, n, _, acc = case
    return f"b{b}_{h}x{w}_l{levels}_r{r}_n{n}" + ("_acc" if acc else "")


def max_norm_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def tolerance(e):
    return max(FLOOR, FACTOR * e)


def coords_mix(rng, b, h, w, radius, wild=True):
    """(B, 2, h, w) float32: grid + N(0, 3^2) + a per-image shift; one block of queries pushed off each of the
    four borders by about r + 1 (their patches straddle or just miss the border); a few at exactly integer
    positions (fx = fy = 0 on every level: multiples of 8) and at plain integers; with ``wild`` a few NaN,
    +-inf and +-1e9."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    co = np.stack([xs, ys])[None] + rng.normal(0.0, 3.0, (b, 2, h, w)) + rng.normal(0.0, 2.0, (b, 2, 1, 1))
    by, bx = max(h // 5, 1), max(w // 5, 1)
    off = radius + 1
    jit = lambda shape: rng.uniform(-1.0, 1.0, shape)  # noqa: E731
    co[:, 0, :by, :bx] = -off + jit((b, by, bx))                               # off the left border
    co[:, 0, :by, -bx:] = w - 1 + off + jit((b, by, bx))                       # right
    co[:, 1, -by:, :bx] = -off + jit((b, by, bx))                              # top
    co[:, 1, -by:, -bx:] = h - 1 + off + jit((b, by, bx))                      # bottom
    flat = co.reshape(b, 2, h * w)
    n = h * w
    pick = rng.choice(n, size=14, replace=False)
    flat[:, :, pick[:4]] = 8.0 * np.round(flat[:, :, pick[:4]] / 8.0)
    flat[:, :, pick[4:8]] = np.round(flat[:, :, pick[4:8]])
    if wild:
        bad = [np.nan, np.inf, -np.inf, 1e9, -1e9, np.nan]
        for k, q in enumerate(pick[8:]):
            flat[k % b, k % 2, q] = bad[k % len(bad)]
            if k == 1:
                flat[0, :, q] = (1e9, -np.inf)
    return co.astype(np.float32)


def _sum_levels(dtype, init, lookups, levels, radius, masks):
    """The levels of G: init + lookup 0 + lookup 1 + ... in ``dtype``; also lookup 0's alone."""
    total = [x.astype(dtype) for x in init]
    first = None
    for (co, go), m in zip(lookups, masks):
        gl = oracle.corr_lookup_grad_levels(co, levels, radius, go, m, dtype=dtype)
        if first is None:
            first = gl
        total = [t + g for t, g in zip(total, gl)]
    return first, total


@functools.lru_cache(maxsize=None)
def grad_case(case):
    """Seeded lookups (coords, grad_out; float32) of one case with the float64 levels of G — of lookup 0 alone
    ("first") and of all lookups on top of the initial G ("total") — e and the tolerance of both.  The initial
    G (accumulate cases: a random half-empty G with zero pads, else zeros) is "init" (levels) / "init_packed"."""
    b, h, w, levels, radius, n, masks, acc = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    d = 2 * radius + 1
    lookups = []
    for _ in range(n):
        co = coords_mix(rng, b, h, w, radius)
        go = rng.standard_normal((b, levels * d * d, h, w)).astype(np.float32)
        lookups.append((co, go))
    shapes = oracle.pyramid_level_shapes(h, w, levels)
    if acc:
        init = [(rng.standard_normal((b, h * w, hl, wl)) * (rng.random((b, h * w, hl, wl)) < 0.5)).astype(np.float32)
                for hl, wl in shapes]
    else:
        init = [np.zeros((b, h * w, hl, wl), np.float32) for hl, wl in shapes]
    first64, total64 = _sum_levels(np.float64, init, lookups, levels, radius, masks)
    first32, total32 = _sum_levels(np.float32, init, lookups, levels, radius, masks)
    cat = lambda ls: np.concatenate([x.reshape(-1) for x in ls])  # noqa: E731
    e_first = max_norm_err(cat(first32), cat(first64))
    e_total = max_norm_err(cat(total32), cat(total64))
    out = {"lookups": lookups, "masks": masks, "init": init, "init_packed": oracle.corr_grad_pack(init),
           "first": first64, "total": total64, "e_first": e_first, "e_total": e_total,
           "tol_first": tolerance(e_first), "tol_total": tolerance(e_total)}
    for v in (init + first64 + total64 + [x for lk in lookups for x in lk] + [out["init_packed"]]):
        v.setflags(write=False)
    return out


# ---- P and the unpooling: (B, C, h, w, levels) ------------------------------------------------------------
# 19x37: odd at every level (the floor crop drops a row and a column); 9x70: a 1 x 8 level; 8x8: a 1 x 1
# level; 13x27: a single level; 6x300: 304 padded level-0 targets per row, more than one block of 256 in x.
POOL_CASES = [(2, 3, 19, 37, 4), (1, 5, 9, 70, 4), (1, 1, 8, 8, 4), (3, 7, 13, 27, 1), (1, 2, 6, 300, 3)]


@functools.lru_cache(maxsize=None)
def pool_case(case, unit_scale):
    """fmap2 and dP (float32, seeded; dP random in the pad slots too, which the unpooling never reads) with the
    float64 P and unpooled gradient, e and the tolerance of both.  scale: 1/sqrt(C) rounded to float32, or 1."""
    b, c, h, w, levels = case
    rng = np.random.default_rng(zlib.crc32(repr((case, unit_scale)).encode()))
    scale = 1.0 if unit_scale else float(np.float32(c ** -0.5))
    t = oracle.corr_grad_geometry(h, w, levels).targets
    f2 = rng.standard_normal((b, c, h, w)).astype(np.float32)
    dP = rng.standard_normal((b, c, t)).astype(np.float32)
    P64 = oracle.corr_pool_targets(f2.astype(np.float64), levels, scale)
    P32 = oracle.corr_pool_targets(f2, levels, np.float32(scale))
    u64 = oracle.corr_unpool_targets(dP.astype(np.float64), h, w, levels, scale)
    u32 = oracle.corr_unpool_targets(dP, h, w, levels, np.float32(scale))
    assert P32.dtype == np.float32 and u32.dtype == np.float32
    e_pool, e_unpool = max_norm_err(P32, P64), max_norm_err(u32, u64)
    out = {"scale": scale, "fmap2": f2, "dP": dP, "P": P64, "unpooled": u64, "e_pool": e_pool, "e_unpool": e_unpool,
           "tol_pool": tolerance(e_pool), "tol_unpool": tolerance(e_unpool)}
    for v in (f2, dP, P64, u64):
        v.setflags(write=False)
    return out


# ---- the chain through autograd: (label, B, C, h, w, levels, radii per lookup, mask_costs per lookup) ------
CHAIN_CASES = [
    ("9x70_l4_r4", 2, 32, 9, 70, 4, (4, 4), ((), (4,))),                      # level 3 is 1 x 8: skipped on both sides
    ("17x33_l3_r1", 1, 24, 17, 33, 3, (1, 1), ((), ())),
    ("17x33_l3_r2", 1, 24, 17, 33, 3, (2, 2), ((), (5,))),
    ("17x33_l3_r5", 1, 24, 17, 33, 3, (5,), ((),)),
    ("17x33_l3_r8", 1, 24, 17, 33, 3, (8,), ((),)),
    ("12x20_l4_r2_n21", 2, 16, 12, 20, 4, (2,) * 21, ((),) * 21),             # 16 + 5: an accumulating launch
    ("19x26_l4_r4-4-2-4", 2, 16, 19, 26, 4, (4, 4, 2, 4), ((), (3,), (), ())),   # groups of equal radii
]


@functools.lru_cache(maxsize=None)
def chain_case(label):
    """Feature maps and lookups (coords of coords_mix without the non-finite ones, finite grad_out) of a chain
    case with the float64 gradients: the sum of oracle.corr_lookup_backward over the lookups."""
    _, b, c, h, w, levels, radii, masks = next(x for x in CHAIN_CASES if x[0] == label)
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    f1 = rng.standard_normal((b, c, h, w)).astype(np.float32)
    f2 = rng.standard_normal((b, c, h, w)).astype(np.float32)
    g1, g2 = np.zeros((b, c, h, w)), np.zeros((b, c, h, w))
    lookups = []
    for r, m in zip(radii, masks):
        co = coords_mix(rng, b, h, w, r, wild=False)
        go = rng.standard_normal((b, levels * (2 * r + 1) ** 2, h, w)).astype(np.float32)
        a1, a2 = oracle.corr_lookup_backward(f1.astype(np.float64), f2.astype(np.float64), co.astype(np.float64),
                                             levels, r, go.astype(np.float64), m)
        g1 += a1
        g2 += a2
        lookups.append((co, go, r, m))
    for v in (f1, f2, g1, g2) + tuple(x for lk in lookups for x in lk[:2]):
        v.setflags(write=False)
    return {"fmap1": f1, "fmap2": f2, "levels": levels, "lookups": lookups, "grad_fmap1": g1, "grad_fmap2": g2}
