"""The staged float64 oracle of the RAFT correlation backward (oracle/corr.py: corr_lookup_grad_levels,
corr_grad_pack / unpack, corr_pool_targets, corr_unpool_targets and their composition corr_lookup_backward)
checked on the CPU against things it shares no code with: the forward oracle (adjoint identity; the forward is
pinned by the reference's golden vectors), the dense restatement it replaces (kept below as a helper), the
reference's autograd gradients (golden) and the library's own target count."""

import warnings

import numpy as np
import pytest

import oracle
from conftest import load_golden, rel_max_err
from corr_backward_cases import coords_mix


def _dense_backward(fmap1, fmap2, coords, levels, radius, grad_out, mask_costs=()):
    """The dense restatement oracle.corr_lookup_backward was before it became a composition of stages: bilinear
    scatter per tap, spread over 2^i x 2^i blocks, one GEMM pair on the level-0 gradient."""
    b, c, h, w = fmap1.shape
    d = 2 * radius + 1
    n = h * w
    shapes = oracle.pyramid_level_shapes(h, w, levels)
    g = grad_out.reshape(b, levels, d, d, n)
    cx = coords[:, 0].reshape(b, n)
    cy = coords[:, 1].reshape(b, n)
    one = np.asarray(1, dtype=fmap1.dtype)
    gcorr0 = np.zeros((b, n, h, w), dtype=fmap1.dtype)
    bi = np.arange(b)[:, None]
    pi = np.arange(n)[None, :]
    for i, (hl, wl) in enumerate(shapes):
        if i + 3 in mask_costs:
            continue
        s = np.asarray(2.0 ** i, dtype=fmap1.dtype)
        gl = np.zeros((b, n, hl, wl), dtype=fmap1.dtype)
        lx, ly = cx / s, cy / s
        x0 = np.floor(lx)
        y0 = np.floor(ly)
        fx, fy = lx - x0, ly - y0
        x0 = x0.astype(np.int64)
        y0 = y0.astype(np.int64)
        for a in range(d):
            for bb in range(d):
                gv = g[:, i, a, bb, :]
                for ddy, wy in ((0, one - fy), (1, fy)):
                    for ddx, wx in ((0, one - fx), (1, fx)):
                        xx = x0 + a - radius + ddx
                        yy = y0 + bb - radius + ddy
                        v = (xx >= 0) & (xx < wl) & (yy >= 0) & (yy < hl)
                        np.add.at(gl, (bi, pi, np.clip(yy, 0, hl - 1), np.clip(xx, 0, wl - 1)), gv * wx * wy * v)
        k = 2 ** i
        up = np.repeat(np.repeat(gl, k, axis=-2), k, axis=-1) / np.asarray(k * k, dtype=gl.dtype)
        gcorr0[..., : hl * k, : wl * k] += up
    gcorr0 = gcorr0.reshape(b, n, n) / np.sqrt(np.asarray(c, dtype=fmap1.dtype))
    gf1 = np.matmul(fmap2.reshape(b, c, n), gcorr0.transpose(0, 2, 1)).reshape(b, c, h, w)
    gf2 = np.matmul(fmap1.reshape(b, c, n), gcorr0).reshape(b, c, h, w)
    return gf1, gf2


def _far_mix(rng, b, h, w, radius):
    """coords_mix (off all four borders, integer positions) plus queries far outside; finite, float64."""
    co = coords_mix(rng, b, h, w, radius, wild=False).astype(np.float64)
    flat = co.reshape(b, 2, h * w)
    q = rng.choice(h * w, 6, replace=False)
    flat[:, 0, q[:3]] += (400.0, -2.5e4, 1.0e9)
    flat[:, 1, q[3:]] += (-77.0, 3.1e4, -1.0e9)
    return co


@pytest.mark.parametrize("b,h,w,levels,radius,mask", [
    (2, 13, 21, 3, 1, (4,)),
    (1, 19, 26, 4, 4, ()),
    (2, 9, 70, 4, 4, (3,)),         # level 3 is 1 x 8: NaN in the forward, excluded there, zero in G
    (1, 18, 33, 3, 8, (5,)),
])
def test_grad_levels_are_the_adjoint_of_the_forward_lookup(b, h, w, levels, radius, mask):
    """The lookup is linear in the pyramid, so for any pyramid (random here, not a product of feature maps)
    sum(corr_lookup(pyr) * go) == sum_l <G_l, pyr_l>, to 1e-12 of the sum of the terms' magnitudes."""
    rng = np.random.default_rng(h * w + radius)
    n, dd = h * w, (2 * radius + 1) ** 2
    shapes = oracle.pyramid_level_shapes(h, w, levels)
    pyr = [rng.standard_normal((b, n, hl, wl)) for hl, wl in shapes]
    co = _far_mix(rng, b, h, w, radius)
    go = rng.standard_normal((b, levels * dd, h, w))
    out = oracle.corr_lookup(pyr, co, radius, mask)
    one_pixel = [l for l, (hl, wl) in enumerate(shapes) if hl < 2 or wl < 2]
    gl = oracle.corr_lookup_grad_levels(co, levels, radius, go, mask)
    assert [g.shape for g in gl] == [p.shape for p in pyr] and all(g.dtype == np.float64 for g in gl)
    for l in one_pixel:
        assert np.isnan(out[:, l * dd:(l + 1) * dd]).all() and not gl[l].any()
        out[:, l * dd:(l + 1) * dd] = 0.0
    for m in mask:
        assert not gl[m - 3].any()
    assert np.isfinite(out).all()
    lhs = float((out * go).sum())
    rhs = float(sum((g * p).sum() for g, p in zip(gl, pyr)))
    size = float(np.abs(out * go).sum())
    assert abs(lhs - rhs) <= 1e-12 * size, (lhs, rhs, size)
    assert any(g.any() for g in gl)


@pytest.mark.parametrize("b,c,h,w,levels,radius,n", [(2, 8, 19, 37, 4, 3, 3), (1, 6, 18, 33, 3, 8, 2)])
def test_staged_oracle_equals_the_dense_restatement(b, c, h, w, levels, radius, n):
    rng = np.random.default_rng(h + w)
    f1 = rng.standard_normal((b, c, h, w))
    f2 = rng.standard_normal((b, c, h, w))
    for i in range(n):
        co = _far_mix(rng, b, h, w, radius)
        go = rng.standard_normal((b, levels * (2 * radius + 1) ** 2, h, w))
        mask = (4,) if i == 1 else ()
        s1, s2 = oracle.corr_lookup_backward(f1, f2, co, levels, radius, go, mask)
        d1, d2 = _dense_backward(f1, f2, co, levels, radius, go, mask)
        assert rel_max_err(s1, d1) < 1e-12 and rel_max_err(s2, d2) < 1e-12


def test_staged_oracle_matches_reference_golden():
    """Each stage on its own, composed by hand here, against the reference's autograd gradients, at the
    tolerance test_oracle_golden.py holds corr_lookup_backward to."""
    g = load_golden("corr_b2_c32_24x40")
    f1, f2, co, go = (np.asarray(g[k], np.float64) for k in ("fmap1", "fmap2", "coords", "grad_out"))
    b, c, h, w = f1.shape
    n = h * w
    gl = oracle.corr_lookup_grad_levels(co, 4, 4, go)
    G = oracle.corr_grad_pack(gl)                                              # (B, TC, N, 8)
    geo = oracle.corr_grad_geometry(h, w, 4)
    assert G.shape == (b, geo.TC, n, 8)
    Gm = G.transpose(0, 1, 3, 2).reshape(b, geo.targets, n)
    P = oracle.corr_pool_targets(f2, 4, c ** -0.5)
    g1 = (P @ Gm).reshape(b, c, h, w)
    g2 = oracle.corr_unpool_targets(f1.reshape(b, c, n) @ Gm.transpose(0, 2, 1), h, w, 4, c ** -0.5)
    assert rel_max_err(g1, g["grad_fmap1"]) < 2e-5
    assert rel_max_err(g2, g["grad_fmap2"]) < 2e-5


@pytest.mark.parametrize("h,w,levels", [(19, 26, 4), (9, 70, 4), (8, 8, 4), (13, 27, 1), (6, 300, 3), (17, 33, 3)])
def test_pack_unpack_geometry(h, w, levels):
    """pack and unpack are inverse to each other, every pad slot is zero, the element order is the header's
    formula, and T' is the library's rmd_corr_grad_targets (a host-only call)."""
    rng = np.random.default_rng(h * w)
    b, n = 2, h * w
    geo = oracle.corr_grad_geometry(h, w, levels)
    assert geo.lh == [h >> l for l in range(levels)] and geo.lw == [w >> l for l in range(levels)]
    assert geo.nch == [(x + 7) // 8 for x in geo.lw]
    assert geo.coff == [sum(geo.lh[k] * geo.nch[k] for k in range(l)) for l in range(levels)]
    assert geo.TC == geo.coff[-1] + geo.lh[-1] * geo.nch[-1] and geo.targets == 8 * geo.TC
    lv = [rng.standard_normal((b, n, hl, wl)) + 3.0 for hl, wl in oracle.pyramid_level_shapes(h, w, levels)]
    G = oracle.corr_grad_pack(lv)
    assert G.shape == (b, geo.TC, n, 8)
    back = oracle.corr_grad_unpack(G.reshape(-1), b, h, w, levels)
    assert all(np.array_equal(x, y) for x, y in zip(back, lv))
    pad = oracle.corr_grad_pad_slots(h, w, levels)
    assert pad.shape == (geo.TC, 8) and pad.sum() == sum(geo.lh[l] * (8 * geo.nch[l] - geo.lw[l]) for l in range(levels))
    assert (G.transpose(0, 2, 1, 3)[:, :, pad] == 0).all() and (G.transpose(0, 2, 1, 3)[:, :, ~pad] != 0).all()
    assert np.array_equal(oracle.corr_grad_pack(back), G)
    flat = G.reshape(-1)
    for _ in range(20):                                                        # the header's index formula
        l = int(rng.integers(levels))
        bi, p, y, x = int(rng.integers(b)), int(rng.integers(n)), int(rng.integers(geo.lh[l])), int(rng.integers(geo.lw[l]))
        at = ((bi * geo.TC + geo.coff[l] + y * geo.nch[l] + x // 8) * n + p) * 8 + x % 8
        assert flat[at] == lv[l][bi, p, y, x]
    from rmd import _lib
    assert _lib.lib().rmd_corr_grad_targets(h, w, levels) == geo.targets


def test_pool_and_unpool_targets_are_adjoint_and_match_the_pyramid_pooling():
    rng = np.random.default_rng(5)
    b, c, h, w, levels = 2, 3, 19, 37, 4
    geo = oracle.corr_grad_geometry(h, w, levels)
    f = rng.standard_normal((b, c, h, w))
    d = rng.standard_normal((b, c, geo.targets))
    P = oracle.corr_pool_targets(f, levels, 0.37)
    assert P.shape == (b, c, geo.targets)
    pad = oracle.corr_grad_pad_slots(h, w, levels).reshape(-1)
    assert (P[..., pad] == 0).all()
    # level l of P is the l-fold 2x2 average of the map (the pooling of oracle.corr_pyramid)
    lv = f
    for l in range(levels):
        rows = P[..., 8 * geo.coff[l]: 8 * (geo.coff[l] + geo.lh[l] * geo.nch[l])].reshape(b, c, geo.lh[l], -1)
        assert np.allclose(rows[..., : geo.lw[l]], 0.37 * lv, rtol=0, atol=1e-14)
        lv = oracle.corr._avg_pool2(lv)
    d0 = np.where(pad, 0.0, d)
    u = oracle.corr_unpool_targets(d, h, w, levels, 0.37)
    assert u.shape == (b, c, h, w)
    assert abs((P * d0).sum() - (f * u).sum()) < 1e-12 * np.abs(P * d0).sum()


def test_nonfinite_coordinates_add_nothing_and_warn_nothing():
    rng = np.random.default_rng(8)
    b, h, w, levels, radius = 1, 12, 17, 3, 2
    co = coords_mix(rng, b, h, w, radius, wild=False)
    clean = co.copy()
    flat = co.reshape(b, 2, h * w)
    bad = {3: (np.nan, 4.0), 20: (5.0, np.nan), 41: (np.inf, 2.0), 77: (3.0, -np.inf), 100: (1e9, 6.0),
           130: (7.0, -1e9), 150: (np.nan, np.inf), 151: (-1e9, 1e9)}
    for q, v in bad.items():
        flat[0, :, q] = v
    go = rng.standard_normal((b, levels * 25, h, w)).astype(np.float32)
    for dtype in (np.float64, np.float32):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            gl = oracle.corr_lookup_grad_levels(co, levels, radius, go, dtype=dtype)
            ref = oracle.corr_lookup_grad_levels(clean, levels, radius, go, dtype=dtype)
        keep = np.setdiff1d(np.arange(h * w), list(bad))
        for g, r in zip(gl, ref):
            assert g.dtype == dtype and np.isfinite(g).all()
            assert not g[:, list(bad)].any()
            assert np.array_equal(g[:, keep], r[:, keep]) and r[:, list(bad)].any()
