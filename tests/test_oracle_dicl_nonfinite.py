"""The DICL stack oracle at non-finite sample positions, pinned against the ATen composite behind
torch.ops.rmd.dicl_stack on CPU tensors (rmd/cpu.py: grid_sample, the reference's own op):

  * a NaN or +-inf coordinate makes that pixel's whole f2 window NaN, a huge finite one gives zeros;
  * a non-finite grid scale ((wl-1)/(nw-1) with a 1-pixel normalisation map: inf, or NaN for 0/0)
    makes the whole f2 half NaN — the oracle divides as IEEE does instead of raising ZeroDivisionError;
  * in the backward a tap at a non-finite position contributes nothing: grad_fmap2 has no NaN, and is
    all zero under a non-finite scale.

Tolerance: the composite is fp32 through grid_sample's [-1, 1] round trip, 1e-4 max-normalised against
the float64 oracle; the NaN patterns and the zero grad_fmap2 are exact.
"""

import numpy as np
import pytest
import torch

import dicl_route_cases as cases
from conftest import rel_max_err

CPU_TOL = 1e-4


def _cpu(r, x):
    import rmd
    f1 = torch.from_numpy(x.f1.copy()).requires_grad_(True)
    f2 = torch.from_numpy(x.f2.copy()).requires_grad_(True)
    st = rmd.ops.dicl_stack(f1, f2, torch.from_numpy(x.coords.copy()), r.r, level=r.level, norm_hw=(r.nh, r.nw),
                            extra_delta=r.extra)
    g1, g2 = torch.autograd.grad(st, (f1, f2), torch.from_numpy(x.grad.copy()))
    return st.detach().numpy(), g1.numpy(), g2.numpy()


@pytest.mark.parametrize("row_id", cases.NONFINITE_COORD_IDS)
def test_nonfinite_coordinates_match_the_cpu_composite(row_id):
    r, x, ref = cases.row(row_id), cases.inputs(row_id, True), cases.reference(row_id, True)
    st, g1, g2 = _cpu(r, x)
    c = r.c
    assert rel_max_err(st[:, :, :, :2 * c], ref.stack) < CPU_TOL          # asserts the NaN pattern too
    for b, y, px, _, v in cases.NONFINITE_COORDS:
        win = ref.stack[b, :, :, c:, y, px]
        assert np.isnan(win).all() if not np.isfinite(v) else not win.any()
    assert np.isnan(ref.stack).sum() == c * (2 * r.r + 1) ** 2 * (len(cases.NONFINITE_COORDS) - len(cases.HUGE_FINITE))
    assert not np.isnan(ref.grad_f2).any() and not np.isnan(g2).any()
    assert rel_max_err(g1, ref.grad_f1) < CPU_TOL
    assert rel_max_err(g2, ref.grad_f2) < CPU_TOL


@pytest.mark.parametrize("r", cases.NONFINITE_SCALE, ids=lambda r: r.id)
def test_nonfinite_scale_matches_the_cpu_composite(r):
    x, ref = cases.inputs(r.id), cases.reference(r.id)
    st, g1, g2 = _cpu(r, x)
    c = r.c
    assert np.array_equal(ref.stack[:, :, :, :c], np.broadcast_to(x.f1[:, None, None], ref.stack[:, :, :, :c].shape))
    assert np.isnan(ref.stack[:, :, :, c:]).all() and np.isnan(st[:, :, :, c:2 * c]).all()
    assert np.array_equal(st[:, :, :, :c], ref.stack[:, :, :, :c].astype(np.float32))
    assert not ref.grad_f2.any() and not g2.any()
    assert rel_max_err(g1, ref.grad_f1) < CPU_TOL


def test_scale_division_is_ieee():
    from oracle.dicl import _grid_scale
    sx, sy = _grid_scale(4, 8, 4, 1)
    assert np.isposinf(sx) and sy == 1.0
    sx, sy = _grid_scale(4, 1, 1, 1)
    assert np.isnan(sx) and np.isposinf(sy)
    assert _grid_scale(6, 10, 12, 20) == (9 / 19, 5 / 11)
