"""Which kernel rmd_dicl_stack / rmd_dicl_stack_backward run for the shapes of dicl_route_cases.py:
the launchers dispatch on the decision rmd_dicl_stack_kernel reports (host only, no GPU), so these
run on a CPU-only machine against the built library.  test_gpu_dicl_routes.py runs the same rows on
the GPU against the oracle; together they say that every reachable kernel is compared with something,
and a retuned threshold that moves a row onto another route fails here instead of silently dropping
the coverage."""

import pytest

import dicl_route_cases as cases


def _lib():
    from rmd import _lib
    return _lib.lib()


@pytest.mark.parametrize("r", cases.ROWS, ids=lambda r: r.id)
def test_route_of_every_row(r):
    lib = _lib()
    got = (cases.query(lib, r, False), cases.query(lib, r, True))
    print(f"{r.id}: forward {got[0]}, backward {got[1]}")
    assert got == (r.fwd, r.bwd)


@pytest.mark.parametrize("backward", [0, 1])
def test_rows_cover_every_route(backward):
    """The rows' routes are exactly the library's list, less the exemption written out in
    dicl_route_cases.py (patch1/R/*: stacks of >= 4 GiB per image, untested).  A route added without a
    row, or a route that no longer exists, fails here."""
    listed = _lib().rmd_dicl_stack_kernel_list(backward).decode().split(",")
    assert len(listed) == len(set(listed)) and "invalid" not in listed
    covered = {r.bwd if backward else r.fwd for r in cases.ROWS}
    exempt = cases.EXEMPT_BACKWARD if backward else cases.EXEMPT_FORWARD
    assert exempt == ({f"patch1/{r}/{win}" for r in (1, 2, 3, 4) for win in ("small", "large")} if backward else set())
    assert exempt <= set(listed) and not (exempt & covered)
    assert covered | exempt == set(listed), (sorted(set(listed) - covered - exempt), sorted(covered - set(listed)))


def test_patch1_route_is_the_4gib_stack():
    """The exempt route exists: a unit-step stack of 4 GiB per image (C = 1036, 81 displacements,
    80 x 80: 81 * 2072 * 6400 * 4 B = 2^32 + 1.5 MB) leaves the 32-bit lane offsets of patch / patch2."""
    lib = _lib()
    args = (1, 1036, 80, 80, 80, 80, 4, 0, 80, 80, 0)
    assert lib.rmd_dicl_stack_kernel(*args, 0) == b"general"
    assert lib.rmd_dicl_stack_kernel(*args, 1) == b"patch1/4/small"
    assert lib.rmd_dicl_stack_kernel(1, 1035, 80, 80, 80, 80, 4, 0, 80, 80, 0, 1) == b"patch2/4/small"


@pytest.mark.parametrize("args", [(0, 3, 4, 8, 4, 8, 2, 0, 4, 8, 0), (2, 3, 3, 7, 3, 7, 2, 0, 3, 7, 0),
                                  (2, 3, 4, 8, 4, 8, 33, 0, 4, 8, 0), (2, 3, 4, 8, 4, 8, 2, 16, 4, 8, 0)])
def test_rejected_arguments_are_invalid(args):
    """Arguments the stack calls reject (empty batch, h*w not a multiple of 4, radius > 32, level > 15)."""
    lib = _lib()
    assert lib.rmd_dicl_stack_kernel(*args, 0) == b"invalid"
    assert lib.rmd_dicl_stack_kernel(*args, 1) == b"invalid"
