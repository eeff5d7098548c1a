"""Every stage of the RAFT correlation backward (corr_backward.hip) against the staged float64 oracle
(oracle/corr.py), stage by stage: (a) rmd_corr_lookup_backward and (b) rmd_corr_grad_build against the oracle's G
— values, support (no stray writes) and pad slots —, (c) rmd_corr_pool_targets / rmd_corr_unpool_targets against
the oracle's P and unpooled gradient, (d) the chain through autograd at shapes with a 1-pixel level, every
radius group, a second accumulating launch and mixed radii.  Cases, references and the tolerance rule
(max(1e-6, 8 e), e the oracle's own float32 error): corr_backward_cases.py.  Each test prints e, its tolerance
and the kernel's error."""

import ctypes

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_max_err
from corr_backward_cases import (BUILD_CASES, CHAIN_CASES, LOOKUP_CASES, POOL_CASES, case_id, chain_case, grad_case,
                                 max_norm_err, pool_case)

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = ctypes.c_void_p
CHAIN_TOL = {"fp32": 1e-4, "fp32-exact": 1e-4, "bf16": 1e-2}      # test_gpu_corr.py's backward gates


def _lib():
    from rmd import _lib as L
    return L


def _t(a):
    return torch.tensor(np.asarray(a), device=DEV)         # a copy: the cases' arrays are read-only


def _desc(b, h, w, levels):
    L = _lib()
    return L.describe(b, h, w, levels, L.RMD_F32)


def _mask_bits(mask_costs):
    return sum(1 << (m - 3) for m in mask_costs)


def _check_G(G, ref_levels, case, e, tol, what):
    """Values within tol (max-normalised over all levels), no non-zero outside the oracle's support, pads 0."""
    b, h, w, levels = case[:4]
    got = G.cpu().numpy()
    assert np.isfinite(got).all(), "non-finite G (a NaN of the pre-fill left, or produced)"
    geo = oracle.corr_grad_geometry(h, w, levels)
    pad = oracle.corr_grad_pad_slots(h, w, levels)
    assert (got.reshape(b, geo.TC, h * w, 8).transpose(0, 2, 1, 3)[:, :, pad] == 0).all(), "non-zero pad target"
    lv = oracle.corr_grad_unpack(got, b, h, w, levels)
    scale = max(float(np.abs(r).max()) for r in ref_levels)
    err = max(float(np.abs(g - r).max()) for g, r in zip(lv, ref_levels)) / scale
    stray = sum(int(((g != 0) & (r == 0)).sum()) for g, r in zip(lv, ref_levels))
    print(f"{what} {case_id(case)}: e {e:.2e} tol {tol:.2e} kernel error {err:.2e} stray writes {stray}")
    assert stray == 0, f"{stray} non-zero elements outside the oracle's support"
    assert err < tol, (err, tol)


@pytest.mark.parametrize("case", LOOKUP_CASES + BUILD_CASES, ids=case_id)
def test_lookup_backward_G_vs_oracle(case):
    """(a) one rmd_corr_lookup_backward (the case's first lookup) into a zeroed G."""
    L = _lib()
    b, h, w, levels, radius = case[:5]
    c = grad_case(case)
    d = _desc(b, h, w, levels)
    co, go = (_t(x) for x in c["lookups"][0])
    t = L.lib().rmd_corr_grad_targets(h, w, levels)
    G = torch.zeros(b * h * w * t, dtype=torch.float32, device=DEV)
    L.check(L.lib().rmd_corr_lookup_backward(P(go.data_ptr()), ctypes.byref(d), P(co.data_ptr()), radius,
                                             _mask_bits(c["masks"][0]), P(G.data_ptr()), None), "lookup_backward")
    _check_G(G, c["first"], case, c["e_first"], c["tol_first"], "lookup_backward")


@pytest.mark.parametrize("case", LOOKUP_CASES + BUILD_CASES, ids=case_id)
def test_grad_build_G_vs_oracle(case):
    """(b) rmd_corr_grad_build over all lookups of the case, into a NaN-filled G (accumulate = 0) or onto a
    non-zero G (accumulate = 1), against the oracle's float64 sum."""
    L = _lib()
    b, h, w, levels, radius, n, _, acc = case
    c = grad_case(case)
    d = _desc(b, h, w, levels)
    lk = [(_t(co), _t(go)) for co, go in c["lookups"]]
    t = L.lib().rmd_corr_grad_targets(h, w, levels)
    if acc:
        G = _t(c["init_packed"]).reshape(-1).clone()
    else:
        G = torch.full((b * h * w * t,), float("nan"), dtype=torch.float32, device=DEV)
    assert G.numel() == b * h * w * t
    gouts = (P * n)(*[go.data_ptr() for _, go in lk])
    cos = (P * n)(*[co.data_ptr() for co, _ in lk])
    ms = (ctypes.c_uint * n)(*[_mask_bits(m) for m in c["masks"]])
    L.check(L.lib().rmd_corr_grad_build(gouts, cos, ms, n, ctypes.byref(d), radius, 1 if acc else 0,
                                        P(G.data_ptr()), None), "grad_build")
    _check_G(G, c["total"], case, c["e_total"], c["tol_total"], "grad_build")


@pytest.mark.parametrize("unit_scale", [False, True], ids=["rsqrtC", "one"])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "b%d_c%d_%dx%d_l%d" % c)
def test_pool_and_unpool_targets_vs_oracle(case, unit_scale):
    """(c) P and the unpooled gradient against the oracle, into NaN-filled outputs; pads of P exactly 0; and the
    two GPU results adjoint to each other: <pool(f), d> == <f, unpool(d)> to 1e-5 of |pool(f)| |d| (float64 sums
    of fp32 results a few 1e-7 off each)."""
    L = _lib()
    b, c, h, w, levels = case
    k = pool_case(case, unit_scale)
    t = L.lib().rmd_corr_grad_targets(h, w, levels)
    f2, dP = _t(k["fmap2"]), _t(k["dP"])
    Pg = torch.full((b, c, t), float("nan"), dtype=torch.float32, device=DEV)
    U = torch.full((b, c, h, w), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.lib().rmd_corr_pool_targets(P(f2.data_ptr()), b, c, h, w, levels, k["scale"], P(Pg.data_ptr()), None),
            "pool_targets")
    L.check(L.lib().rmd_corr_unpool_targets(P(dP.data_ptr()), b, c, h, w, levels, k["scale"], P(U.data_ptr()), None),
            "unpool_targets")
    Pn, Un = Pg.cpu().numpy().astype(np.float64), U.cpu().numpy().astype(np.float64)
    assert np.isfinite(Pn).all() and np.isfinite(Un).all(), "a NaN of the pre-fill is left"
    pad = oracle.corr_grad_pad_slots(h, w, levels).reshape(-1)
    assert (Pn[..., pad] == 0).all(), "non-zero pad target in P"
    ep, eu = max_norm_err(Pn, k["P"]), max_norm_err(Un, k["unpooled"])
    print(f"pool {case} scale {k['scale']:.4f}: e {k['e_pool']:.2e} tol {k['tol_pool']:.2e} kernel error {ep:.2e}; "
          f"unpool: e {k['e_unpool']:.2e} tol {k['tol_unpool']:.2e} kernel error {eu:.2e}")
    assert ep < k["tol_pool"], (ep, k["tol_pool"])
    assert eu < k["tol_unpool"], (eu, k["tol_unpool"])
    d64, f64 = k["dP"].astype(np.float64), k["fmap2"].astype(np.float64)
    lhs, rhs = float((Pn * d64).sum()), float((f64 * Un).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(np.sqrt((Pn ** 2).sum() * (d64 ** 2).sum())), (lhs, rhs)


@pytest.mark.parametrize("precision", ["fp32", "fp32-exact", "bf16"])
@pytest.mark.parametrize("label", [c[0] for c in CHAIN_CASES])
def test_chain_through_autograd_vs_oracle(label, precision):
    """(d) grad_fmap1 / grad_fmap2 of the product path (G build, pooled targets, both grad GEMMs, unpooling)
    against oracle.corr_lookup_backward summed over the lookups."""
    import rmd
    from rmd import ops
    k = chain_case(label)
    t1, t2 = _t(k["fmap1"]).requires_grad_(True), _t(k["fmap2"]).requires_grad_(True)
    radii = {r for _, _, r, _ in k["lookups"]}
    if len(radii) == 1:
        cb = rmd.raft.CorrBlock(t1, t2, k["levels"], radii.pop(), precision=precision)
        outs = [cb(_t(co), list(m)) for co, _, _, m in k["lookups"]]
    else:
        _, st, token = ops.corr_block_autograd(t1, t2, k["levels"], precision)
        outs = [ops.corr_lookup_autograd(token, st, _t(co), r, m) for co, _, r, m in k["lookups"]]
    torch.autograd.backward(outs, [_t(go) for _, go, _, _ in k["lookups"]])
    e1 = rel_max_err(t1.grad.cpu().numpy(), k["grad_fmap1"])
    e2 = rel_max_err(t2.grad.cpu().numpy(), k["grad_fmap2"])
    print(f"chain {label} [{precision}]: tol {CHAIN_TOL[precision]:.0e} grad_fmap1 error {e1:.2e} grad_fmap2 error {e2:.2e}")
    assert e1 < CHAIN_TOL[precision] and e2 < CHAIN_TOL[precision], (e1, e2)
