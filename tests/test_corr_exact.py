"""The exact-arithmetic correlation cases checked on the CPU (tests/corr_exact_cases.py): the exactness
preconditions hold for every case, the expected pyramids are float32 values whatever the summation order,
the restated S24 / bf16 rounding agrees with the package's and torch's, the lookup wrapper is the
reference's behaviour (golden vectors), the comparators fail every planted error, and the case table
reaches every GEMM route but `stationary` (which needs a 4K map: test_stationary_path_4k_sampled_vs_oracle)
and every lookup phase the digest cases require."""
import numpy as np
import pytest
import torch

import corr_exact_cases as ce
import lookup_digest_cases as lc
import oracle
from conftest import load_golden, rel_max_err

PYR_IDS = [c.name for c in ce.PYRAMID_CASES]


# ---- preconditions -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ce.PYRAMID_CASES, ids=PYR_IDS)
def test_pyramid_case_is_exact(case):
    """check_exact holds (case.stored() asserts it), the integer route to the pyramid is the oracle's
    pyramid, and rounding by the storage rule is idempotent."""
    ft = case.features()
    stored = case.stored()
    exact = ce.exact_pyramid(ft, ce.LEVELS, case.scale)
    f1, f2 = (f[:, :case.c].astype(np.float64) for f in (ft.fmap1, ft.fmap2))
    ref = oracle.corr_pyramid(f1, f2, ce.LEVELS)
    for l in range(ce.LEVELS):
        want = ref[l] * (np.sqrt(float(case.c)) * case.scale)
        assert exact[l].shape == want.shape == stored[l].shape
        if want.size:
            assert np.abs(exact[l] - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300)
        assert ce.pyramid_mismatches(ce.round_storage(stored[l].astype(np.float64), case.storage), stored[l]) == 0
        assert np.isfinite(stored[l]).all()


def test_storage_rounding_is_real_at_every_level():
    """For each (route, rounding storage) some case rounds a good share of the elements of every level: a
    conversion that truncates, or rounds ties the other way, cannot pass."""
    best = {}
    for case in ce.PYRAMID_CASES:
        if case.storage == "f32":
            continue
        exact = ce.exact_pyramid(case.features(), ce.LEVELS, case.scale)
        share = min(float((s.astype(np.float64) != e).mean()) for s, e in zip(case.stored(), exact) if e.size)
        key = (case.route, case.compute, case.storage)
        best[key] = max(best.get(key, 0.0), share)
    assert set(best) == {("w8", "bf16", "f16"), ("tiled", "bf16", "f16"), ("tiled", "f32", "f16"), ("x3", "x3", "s24")}
    assert min(best.values()) > 0.25, best


def test_precondition_rejects_bad_tables():
    big = ce.features("base", 1, 256, 40, 64)
    ce.check_exact(big, 4, "bf16", 1 / 16)
    with pytest.raises(AssertionError):
        ce.check_exact(big, 4, "bf16", 256 ** -0.5 * 1.5)                 # not a power of two
    a, b = ce.features("cross12", 1, 64, 16, 24), ce.features("cross21", 1, 64, 16, 24)
    with pytest.raises(AssertionError):
        ce.check_exact(ce.Features(a.n1, 512, b.n2, 512), 1, "x3", 1 / 8)   # both maps have a low part
    with pytest.raises(AssertionError):
        ce.check_exact(a, 4, "bf16", 1 / 8)                                # 10-bit numerators are no bf16
    with pytest.raises(AssertionError):
        ce.check_exact(ce.features("cross12", 1, 128, 16, 24), 4, "x3", 1 / 8)   # C * pmax * 4^3 = 2^25


@pytest.mark.parametrize("case", ce.OTF_CASES, ids=[c.name for c in ce.OTF_CASES])
def test_otf_case_is_exact(case):
    """otf_levels asserts its preconditions; the fp32 modes agree with each other, and with the pooled
    volume of the same features (pooling fmap2 commutes with the product)."""
    q = case.queries()
    lv = {p: ce.otf_levels(case, p, q) for p in case.precisions}
    if "fp32" in lv:
        assert all(np.array_equal(a, b) for a, b in zip(lv["fp32"], lv["fp32-exact"]))
        if case.sample is None:
            exact = ce.exact_pyramid(case.features(), case.levels, case.scale)
            assert all(np.array_equal(a, b) for a, b in zip(lv["fp32"], exact))
        # the bf16 mode's target rounding is absent at level 0 and, with fine2 targets, real at every other
        assert np.array_equal(lv["bf16"][0], lv["fp32"][0])
        if case.family == "fine2":
            assert all(not np.array_equal(a, b) for a, b in zip(lv["bf16"][1:], lv["fp32"][1:]))
    assert any(c.family == "fine2" and c.levels == 4 for c in ce.OTF_CASES)


# ---- representability: float32 evaluation in two summation orders ----------------------------------------

def _pool_successive(x):
    h2, w2 = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., : 2 * h2, : 2 * w2]
    return np.float32(0.25) * (((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + x[..., 1::2, 0::2]) + x[..., 1::2, 1::2])


def _block_sum(x):
    h2, w2 = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., : 2 * h2, : 2 * w2]
    return (x[..., 1::2, 1::2] + x[..., 1::2, 0::2]) + (x[..., 0::2, 1::2] + x[..., 0::2, 0::2])


@pytest.mark.parametrize("case", ce.PYRAMID_CASES, ids=PYR_IDS)
def test_float32_evaluation_equals_float64_in_two_orders(case):
    ft = case.features()
    b, c, h, w = case.b, case.c, case.h, case.w
    f1 = ft.fmap1[:, :c].reshape(b, c, h * w)
    f2 = (ft.fmap2[:, :c] * np.float32(case.scale)).reshape(b, c, h * w)
    assert f1.dtype == f2.dtype == np.float32
    exact = ce.exact_pyramid(ft, ce.LEVELS, case.scale)
    # order A: one float32 GEMM over all channels, successive 0.25f * (a + b + c + d)
    a = [np.matmul(f1.transpose(0, 2, 1), f2).reshape(b, h * w, h, w)]
    # order B: channel chunks of 7 from the last to the first, running unscaled block sums scaled by 4^-l
    acc = np.zeros((b, h * w, h * w), np.float32)
    for c0 in reversed(range(0, c, 7)):
        acc = acc + np.matmul(f1[:, c0:c0 + 7].transpose(0, 2, 1), f2[:, c0:c0 + 7])
    run = acc.reshape(b, h * w, h, w)
    bb = [run]
    for l in range(1, ce.LEVELS):
        a.append(_pool_successive(a[-1]))
        run = _block_sum(run)
        bb.append(run * np.float32(0.25 ** l))
    for l in range(ce.LEVELS):
        assert a[l].dtype == bb[l].dtype == np.float32
        assert np.array_equal(a[l].astype(np.float64), exact[l]), f"order A, level {l}"
        assert np.array_equal(bb[l].astype(np.float64), exact[l]), f"order B, level {l}"


# ---- the restated rounding rules -------------------------------------------------------------------------

def _bit_patterns():
    rng = np.random.default_rng(24)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    edge = []
    for base in (0x00000000, 0x00000001, 0x00007fff, 0x3f800000, 0x3f7fff80, 0x3f80007f, 0x3f800080, 0x3f800081,
                 0x3f80ff80, 0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x7f7fffff, 0x7f7fff7f, 0x7f7fff80,
                 0x7f7f7fff, 0x7f7f8000, 0x7f800000, 0x7f800001, 0x7fc00000, 0x7fffffff, 0x007fffff, 0x00800000,
                 0x38800000, 0x33800000, 0x477fe000, 0x477ff000):
        edge += [base, base | 0x80000000]
    return np.concatenate([u, np.array(edge, dtype=np.uint32)]).view(np.float32)


def test_s24_restatement_matches_the_package():
    from rmd import library
    x = _bit_patterns()
    enc = library.s24_encode(torch.from_numpy(x.copy()))
    assert np.array_equal(enc.numpy(), ce.s24_bytes(x))
    dec = library.s24_decode(enc).numpy()
    assert np.array_equal(dec.view(np.uint32), ce.s24_round(x).view(np.uint32))
    fin = np.isfinite(dec)
    # half away from zero on the magnitude: never more than half a 24-bit ulp off
    assert (np.abs(dec[fin].astype(np.float64) - x[fin]) <= np.abs(x[fin].astype(np.float64)) * 2.0 ** -16 + 1e-42).all()


def test_bf16_restatement_matches_torch():
    x = _bit_patterns()
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    got = ce.bf16_round(x)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    assert ((got.view(np.uint32) & 0xffff) == 0).all()


def test_fp16_rounding_is_nearest_even():
    x = _bit_patterns()
    x = x[np.isfinite(x)]
    want = torch.from_numpy(x.copy()).to(torch.float16).to(torch.float32).numpy()
    with np.errstate(over="ignore"):
        got = x.astype(np.float16).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the wrapper is the reference's behaviour ---------------------------------------------------------------

TOL64 = 2e-5      # float64 oracle vs the reference's fp32 grid_sample (tests/test_oracle_golden.py)


def _golden_lookup(name):
    g = load_golden(name)
    pyr = oracle.corr_pyramid(g["fmap1"].astype(np.float64), g["fmap2"].astype(np.float64), int(g["levels"]))
    co = np.ascontiguousarray(g["coords"], dtype=np.float32)
    assert np.array_equal(co, g["coords"], equal_nan=True)
    return g, pyr, co, int(g["radius"]), tuple(g["mask_costs"].tolist())


@pytest.mark.parametrize("name", ["corr_b2_c32_24x40", "corr_b2_c32_24x40_mask", "corr_b1_c16_12x20_nan",
                                  "corr_b1_c32_20x28_r7_l2", "corr_b2_c64_17x23_l1"])
def test_wrapper_matches_reference_on_finite_fixtures(name):
    g, pyr, co, radius, mask = _golden_lookup(name)
    got = ce.lookup_reference(pyr, co, radius, mask)
    assert rel_max_err(got, g["out"]) < TOL64
    plain = oracle.corr_lookup(pyr, co.astype(np.float64), radius, mask)      # nothing to make safe: same bits
    assert np.array_equal(got, plain, equal_nan=True)


def test_wrapper_reproduces_the_reference_nan_pattern():
    g, pyr, co, radius, mask = _golden_lookup("corr_b2_c16_16x24_nonfinite")
    got = ce.lookup_reference(pyr, co, radius, mask)
    assert np.isnan(g["out"]).any() and np.array_equal(np.isnan(got), np.isnan(g["out"]))
    assert rel_max_err(got, g["out"]) < TOL64
    huge = np.isfinite(co).all(axis=1) & (np.abs(co) > 1e5).any(axis=1)
    assert huge.any() and not got.transpose(0, 2, 3, 1)[huge].any()
    # a masked level is zero even for a NaN coordinate: the reference replaces it by zeros (raft.py:86-87)
    d2 = (2 * radius + 1) ** 2
    masked = ce.lookup_reference(pyr, co, radius, (4,))
    assert not masked[:, d2:2 * d2].any() and np.array_equal(masked[:, :d2], got[:, :d2], equal_nan=True)


# ---- the comparators are sharp --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in ce.PYRAMID_CASES if c.name in (
    "w8-bf16-b2c16p256-15x20", "x3-fp32-b2c16-16x24", "x3-fp32-f32-b2c16-16x24")], ids=lambda c: c.name)
def test_pyramid_comparator_sees_one_storage_ulp(case):
    stored = case.stored()
    for l in range(ce.LEVELS):
        assert ce.pyramid_mismatches(stored[l].copy(), stored[l]) == 0
        bad = stored[l].copy()
        k = (1, bad.shape[1] // 2, bad.shape[2] - 1, bad.shape[3] - 1)
        bad[k] = ce.storage_ulp_up(bad[k], case.storage)
        assert bad[k] != stored[l][k]
        assert ce.round_storage(np.float64(bad[k]).reshape(1), case.storage)[0] == bad[k]     # a stored value
        assert ce.pyramid_mismatches(bad, stored[l]) == 1
    flipped = stored[0].copy()
    z = np.argwhere(flipped == 0)
    if len(z):
        flipped[tuple(z[0])] = -0.0                                # bit equality: the sign of zero counts
        assert ce.pyramid_mismatches(flipped, stored[0]) == 1


def _one_level(stored_l, coords, radius, shift):
    """Level l's window sampled at coords / 2^shift (a single-level lookup)."""
    return ce.lookup_reference([stored_l], (coords.astype(np.float64) / 2.0 ** shift).astype(np.float32), radius)


@pytest.mark.parametrize("radius", [1, 4, 8])
@pytest.mark.parametrize("kind,shape", [("bf16-tiles", (16, 24)), ("fp32", (15, 20)), ("fp32-f32", (16, 24))])
def test_lookup_comparator_fails_every_planted_error(kind, shape, radius):
    stored = ce.DIGEST_PYRAMID[kind, shape].stored()
    co = lc.coords(shape)
    h, w = shape
    d2 = (2 * radius + 1) ** 2
    ref = ce.lookup_reference(stored, co, radius)
    bound = ce.lookup_bound(stored, radius, h, w)
    worst, n = ce.check_lookup(ref, ref, bound)
    assert worst == 0.0 and n == ref.size == lc.BATCH * lc.LEVELS * d2 * h * w
    worst, _ = ce.check_lookup(ref.astype(np.float32), ref, bound)       # the output's own rounding: half an ulp
    assert worst <= 1.0 / ce.K_LOOKUP

    # (1) one query's fx replaced by 1 - fx (the first hand-placed query: x = w/2 + 0.25, inside the map)
    x, y = co[0, :, 0, 0]
    assert (x, y) == lc.special_points(h, w)[0]
    swapped = co.copy()
    swapped[0, 0, 0, 0] = np.floor(x) + (1.0 - (x - np.floor(x)))
    bad = ref.copy()
    bad[0, :d2, 0, 0] = ce.lookup_reference(stored, swapped, radius)[0, :d2, 0, 0]
    with pytest.raises(AssertionError, match="bound exceeded"):
        ce.check_lookup(bad, ref, bound)

    # (2) the window origin one column off for the queries whose level-0 window crosses the right edge
    x0 = np.floor(co[:, 0].astype(np.float64))
    with np.errstate(invalid="ignore"):
        edge = np.isfinite(co).all(axis=1) & (x0 - radius < w) & (x0 + radius + 1 >= w) & (np.abs(co[:, 1]) < h)
    assert edge.sum() > 4
    moved = co.copy()
    moved[:, 0][edge] += 1.0
    bad = ref.copy()
    sel = np.broadcast_to(edge[:, None], (lc.BATCH, d2, h, w))
    bad[:, :d2][sel] = ce.lookup_reference(stored, moved, radius)[:, :d2][sel]
    with pytest.raises(AssertionError, match="bound exceeded"):
        ce.check_lookup(bad, ref, bound)
    for bi, yi, xi in np.argwhere(edge)[:8]:                              # each such query alone is caught too
        one = ref.copy()
        one[bi, :d2, yi, xi] = bad[bi, :d2, yi, xi]
        if np.array_equal(one, ref, equal_nan=True):
            continue                                                      # a window with nothing but zeros
        with pytest.raises(AssertionError, match="bound exceeded"):
            ce.check_lookup(one, ref, bound)

    # (3) level 1's window sampled at level 2's scale
    assert np.array_equal(_one_level(stored[1], co, radius, 1), ref[:, d2:2 * d2], equal_nan=True)
    bad = ref.copy()
    bad[:, d2:2 * d2] = _one_level(stored[1], co, radius, 2)
    with pytest.raises(AssertionError, match="bound exceeded"):
        ce.check_lookup(bad, ref, bound)

    # (4) a NaN that moves, and a NaN that vanishes
    bad = ref.copy()
    k = tuple(np.argwhere(np.isnan(ref))[0])
    bad[k] = 0.0
    with pytest.raises(AssertionError, match="NaN positions"):
        ce.check_lookup(bad, ref, bound)
    bad = ref.copy()
    bad[tuple(np.argwhere(~np.isnan(ref))[0])] = np.nan
    with pytest.raises(AssertionError, match="NaN positions"):
        ce.check_lookup(bad, ref, bound)

    # (5) one element off by two bounds
    bad = ref.copy()
    k = np.unravel_index(int(np.argmax(np.where(np.isnan(ref), 0, bound))), ref.shape)
    bad[k] += 2 * bound[k]
    with pytest.raises(AssertionError, match="bound exceeded"):
        ce.check_lookup(bad, ref, bound)


# ---- coverage of the case table -----------------------------------------------------------------------------

def test_case_table_reaches_every_route_but_stationary():
    from rmd import _lib
    seen = set()
    for case in ce.PYRAMID_CASES:
        name, storage, d = ce.library_route(case)
        assert (name, storage) == (case.route, case.storage), case.name
        assert (d.layout == _lib.RMD_LAYOUT_TILES) == (name == "w8")
        seen.add((name, case.compute, storage))
    assert {n for n, _, _ in seen} == {"w8", "x3", "tiled"}
    assert seen >= {("w8", "bf16", "f16"), ("tiled", "bf16", "f16"), ("tiled", "bf16", "f32"), ("x3", "x3", "s24"),
                    ("x3", "x3", "f32"), ("tiled", "f32", "f32"), ("tiled", "x3", "f32"), ("tiled", "f32", "f16")}
    # `stationary` is the one other name and needs a map this table does not hold
    d = _lib.describe(1, 270, 480, 4, _lib.RMD_F16)
    assert _lib.lib().rmd_corr_gemm_kernel(d, 256, _lib.RMD_BF16) == b"stationary"
    for (kind, shape), case in ce.DIGEST_PYRAMID.items():
        dtype, tiles = lc.EXPECT[kind]
        assert case.storage == {"float16": "f16", "uint8": "s24", "float32": "f32"}[dtype]
        assert (case.route == "w8") == tiles and (case.h, case.w) == shape


def test_digest_pyramids_are_the_digest_cases_inputs():
    for (kind, shape), case in ce.DIGEST_PYRAMID.items():
        ft = case.features()
        f1, f2 = lc.features(shape)
        assert np.array_equal(ft.fmap1[:, :lc.CHANNELS], f1) and np.array_equal(ft.fmap2[:, :lc.CHANNELS], f2)
        assert not ft.fmap1[:, lc.CHANNELS:].any() and ft.fmap1.shape[1] == (256 if kind == "bf16-tiles" else 16)
        assert case.scale == 1.0 / float(lc.CHANNELS) ** 0.5           # build_pyramid's scale, a power of two


def test_lookup_cases_cover_every_phase_at_every_radius():
    assert set(lc.RADII) <= set(ce.ALL_RADII) == set(range(1, 9))
    for shape in lc.SHAPES:
        for radius in ce.ALL_RADII:
            assert lc.phase_coverage(shape, radius) == {(lvl, sh, par) for lvl in (0, 1) for sh in range(4)
                                                        for par in range(2)}, (shape, radius)


def test_otf_coordinates_sit_on_the_lattice_and_hold_the_special_points():
    for case in ce.OTF_CASES:
        co = case.coords()
        assert co.dtype == np.float32 and co.shape == (case.b, 2, case.h, case.w)
        fin = np.isfinite(co) & (np.abs(co) < 1e6)
        assert np.array_equal(co[fin] * 8, np.rint(co[fin] * 8))
        pts = lc.special_points(case.h, case.w)
        flat = co.reshape(case.b, 2, -1)
        assert case.h * case.w >= 5 * len(pts)
        for i, (x, y) in enumerate(pts):
            assert np.array_equal(flat[0, :, 5 * i], np.array([x, y], np.float32), equal_nan=True)
        assert set(5 * i for i in range(len(pts))) <= set(case.queries().tolist())


def test_otf_cases_reach_every_lookup_path():
    """Host-side restatement of rmd_corr_otf_lookup's dispatch: compiled and runtime channel loops, the MFMA
    box path, the per-query path (boxes of more than 1024 segments) and the 16 x 4 query blocks of wide
    bf16 maps are all reached, each by the case named for it."""
    by_name = {c.name: c for c in ce.OTF_CASES}
    seen = set()
    for case in ce.OTF_CASES:
        for precision in case.precisions:
            paths = {p for _, p in ce.otf_box_paths(case, precision)}
            seen |= {(precision, ce.otf_channel_path(case, precision), ce.otf_block_shape(case, precision), p)
                     for p in paths}
    for precision in ("fp32", "fp32-exact", "bf16"):
        assert {("compiled", "mfma"), ("runtime", "mfma"), ("compiled", "per-query")} <= \
            {(c, p) for pr, c, _, p in seen if pr == precision}, precision
    assert ("bf16", "compiled", (16, 4), "mfma") in seen
    assert ce.otf_channel_path(by_name["b2c128-18x40-l3r5"], "fp32-exact") == "runtime"
    assert ce.otf_channel_path(by_name["b2c128-18x40-l3r5"], "fp32") == "compiled"
    assert ce.otf_channel_path(by_name["b1c320-14x20-l3r3"], "bf16") == "runtime"
    assert {p for _, p in ce.otf_box_paths(by_name["b1c24-4x600-l2r3-scattered"], "fp32")} == {"mfma"}
    assert (0, "per-query") in ce.otf_box_paths(by_name["b1c24-96x256-l2r3-scattered"], "fp32")
    assert ce.otf_block_shape(by_name["b1c32-512x256-l1r1-wide"], "bf16") == (16, 4)
