"""GPU parity of rmd_dicl_stack / rmd_dicl_stack_backward on every kernel route: the rows of
dicl_route_cases.py (test_dicl_routes.py pins which kernel each one runs) through the C ABI, against
the float64 oracle.

Outputs are pre-filled with NaN, so an element no kernel wrote shows up.  Per row: the f1 half of the
stack is bit-equal to fmap1, the delta channels are exact, the f2 half is within 1e-5 max-normalised
with an equal NaN pattern, grad_fmap1 within 1e-5 and grad_fmap2 within 1e-4 (test_gpu_dicl.py's
tolerances: fp32 bilinear in pixel coordinates; float atomics in the scatter).  The wide rows keep those
tolerances meaningful by putting the coordinates on a 2^-6 lattice under dyadic grid scales: their
sample positions are exact in fp32.
"""

import ctypes

import numpy as np
import pytest
import torch

import dicl_route_cases as cases
from conftest import rel_max_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _run(r, x):
    """rmd_dicl_stack and rmd_dicl_stack_backward on NaN-filled outputs -> (stack, grad_fmap1, grad_fmap2)."""
    from rmd import _lib
    lib = _lib.lib()
    d = 2 * r.r + 1
    f1, f2, co, g = (torch.from_numpy(a).to(DEV) for a in (x.f1, x.f2, x.coords, x.grad))
    nan = float("nan")
    out = torch.full((r.b, d, d, 2 * r.c + (2 if r.extra else 0), r.h, r.w), nan, device=DEV)
    g1 = torch.full((r.b, r.c, r.h, r.w), nan, device=DEV)
    g2 = torch.full((r.b, r.c, r.hl, r.wl), nan, device=DEV)
    assert lib.rmd_dicl_stack(_ptr(f1), _ptr(f2), _ptr(co), *r.args, _ptr(out), None) == 0
    assert lib.rmd_dicl_stack_backward(_ptr(g), _ptr(co), *r.args, _ptr(g1), _ptr(g2), None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy()


def _check_copies(r, x, st):
    c, d = r.c, 2 * r.r + 1
    assert np.array_equal(st[:, :, :, :c], np.broadcast_to(x.f1[:, None, None], st[:, :, :, :c].shape))
    if r.extra:
        a = (np.arange(d) - r.r).astype(np.float32)
        assert np.array_equal(st[:, :, :, 2 * c], np.broadcast_to(a[None, :, None, None, None], st[:, :, :, 0].shape))
        assert np.array_equal(st[:, :, :, 2 * c + 1],
                              np.broadcast_to(a[None, None, :, None, None], st[:, :, :, 0].shape))


def _errors(tag, st, g1, g2, ref, c):
    e = (rel_max_err(st[:, :, :, c:2 * c], ref.stack[:, :, :, c:]), rel_max_err(g1, ref.grad_f1),
         rel_max_err(g2, ref.grad_f2))
    print(f"{tag}: f2 half {e[0]:.3e}  grad_fmap1 {e[1]:.3e}  grad_fmap2 {e[2]:.3e}")
    return e


@pytest.mark.parametrize("r", cases.ROWS, ids=lambda r: r.id)
def test_stack_route_vs_oracle(r):
    from rmd import _lib
    lib = _lib.lib()
    x, ref = cases.inputs(r.id), cases.reference(r.id)
    st, g1, g2 = _run(r, x)
    _check_copies(r, x, st)
    # the route is reported, not asserted: parity holds on whatever kernel serves the shape
    e = _errors(f"{r.id} [{cases.query(lib, r, False)} | {cases.query(lib, r, True)}]", st, g1, g2, ref, r.c)
    if r in cases.NONFINITE_SCALE:
        assert np.isnan(st[:, :, :, r.c:2 * r.c]).all()
        assert not g2.any()
    else:
        assert not np.isnan(ref.stack).any()
    assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 1e-4


@pytest.mark.parametrize("row_id", cases.NONFINITE_COORD_IDS)
def test_stack_nonfinite_coordinates_vs_oracle(row_id):
    """NaN, +inf, -inf, 3e9 and -1e30 in single coordinates, one shape per forward family: a non-finite
    coordinate makes that pixel's f2 window NaN (and nothing else), a huge finite one gives exact zeros;
    neither reaches grad_fmap2."""
    r, x, ref = cases.row(row_id), cases.inputs(row_id, True), cases.reference(row_id, True)
    st, g1, g2 = _run(r, x)
    _check_copies(r, x, st)
    c = r.c
    for b, y, px, _, v in cases.NONFINITE_COORDS:
        win = st[b, :, :, c:2 * c, y, px]
        print(f"{row_id} [{r.fwd}] coordinate {v!r}: {int(np.isnan(win).sum())} NaN, "
              f"{int((win == 0).sum())} zeros of {win.size}")
    e = _errors(f"{row_id} [{r.fwd} | {r.bwd}]", st, g1, g2, ref, c)   # asserts equal NaN patterns
    for b, y, px, _, v in cases.HUGE_FINITE:
        assert not st[b, :, :, c:2 * c, y, px].any()
    assert not np.isnan(g2).any()
    assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 1e-4
