"""The hidden-state upsamplers on the GPU: csrc/hsup.hip through torch.ops.rmd.local_cross_attn and
rmd.hsup against the fixtures the reference wrote (tests/golden/gen_golden_hsup.py) and against the
float64 restatement of hsup_cases.py over the shape sweep (both routes, every window size), gradient
selection, views, determinism, opcheck, the no-host-synchronisation rule and argument checks.

Gate: conftest.rel_max_err <= 1e-5 for out, grad_q, grad_k and grad_v (hsup_cases.GATE, reasoned
there: the reference's own fp32 composition stays within a quarter of it on these inputs)."""

import numpy as np
import pytest
import torch

import hsup_cases as cases
from conftest import rel_max_err
from hsup_cases import GATE, MODULE_FIXTURES, RESULTS, SWEEP, fixture

pytestmark = pytest.mark.gpu

DEV = "cuda"
FAST_SHAPE, GENERIC_SHAPE = (2, 8, 6, 3, 5, 2, 2, 3, 3), (1, 4, 3, 2, 3, 3, 1, 3, 3)


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _check(label, got, ref):
    err = rel_max_err(got.detach().cpu().numpy(), ref)
    print(f"{label}: {err:.3e}")
    assert err <= GATE, (label, err)


def _run(c, label):
    """Forward and backward of a case through rmd.ops on the GPU against its float64 results."""
    from rmd import ops
    q, k, v = (_t(c[n], True) for n in ("q", "k", "v"))
    out = ops.local_cross_attn(q, k, v, window=c["window"])
    assert out.shape == c["out"].shape and out.dtype == torch.float32
    _check(f"{label} out", out, c["out"])
    for name, got in zip(RESULTS[1:], torch.autograd.grad(out, (q, k, v), _t(c["grad"]))):
        assert got.shape == c[name].shape
        _check(f"{label} {name}", got, c[name])


@pytest.mark.parametrize("name", MODULE_FIXTURES + [cases.BILINEAR_FIXTURE])
def test_fixtures_through_the_modules(name):
    """HUpCrossAttn / HUpBilinear on the reference's inputs: output, input gradients and every weight gradient."""
    g = fixture(name)
    got, keys = cases.run_module(name, DEV)
    assert keys == sorted(g["keys"].tolist())
    names = [n for n in g if n == "out" or n.startswith("grad_")]
    assert len(names) == 3 + len(keys)
    for n in names:
        assert got[n].shape == g[n].shape
        err = rel_max_err(got[n], g[n])
        print(f"{name} {n}: {err:.3e}")
        assert err <= GATE, (n, err)


def test_core_fixture_through_the_operator():
    """Non-finite q, k and v: values and NaN positions of the reference, forward and backward."""
    import rmd  # noqa: F401
    g = fixture(cases.CORE_FIXTURE)
    q, k, v = _t(g["q"]), _t(g["k"]), _t(g["v"])
    _check("core out", torch.ops.rmd.local_cross_attn(q, k, v, 3, 3), g["out"])
    grads = torch.ops.rmd.local_cross_attn_backward(_t(g["grad"]), q, k, v, 3, 3)
    for name, got in zip(RESULTS[1:], grads):
        _check(f"core {name}", got, g[name])


@pytest.mark.parametrize("shape", SWEEP, ids=["x".join(map(str, s)) for s in SWEEP])
def test_shape_sweep_against_float64(shape):
    _run(cases.sweep_case(shape), f"{cases.route(shape)} {shape}")


def test_peaked_softmax_against_float64():
    _run(cases.peaked_case(), "peaked")


@pytest.mark.parametrize("shape", [FAST_SHAPE, GENERIC_SHAPE], ids=["fast", "generic"])
def test_gradient_selection(shape):
    """Only q requires a gradient, then only k and v."""
    from rmd import ops
    c = cases.sweep_case(shape)
    grad = _t(c["grad"])
    q, k, v = _t(c["q"], True), _t(c["k"]), _t(c["v"])
    (dq,) = torch.autograd.grad(ops.local_cross_attn(q, k, v, c["window"]), q, grad)
    _check(f"{shape} q only", dq, c["grad_q"])
    q, k, v = _t(c["q"]), _t(c["k"], True), _t(c["v"], True)
    dk, dv = torch.autograd.grad(ops.local_cross_attn(q, k, v, c["window"]), (k, v), grad)
    _check(f"{shape} k of k, v", dk, c["grad_k"])
    _check(f"{shape} v of k, v", dv, c["grad_v"])


@pytest.mark.parametrize("shape", [FAST_SHAPE, GENERIC_SHAPE], ids=["fast", "generic"])
def test_views_give_the_results_of_their_contiguous_copies(shape):
    """Permuted (non-contiguous) tensors and views at a storage offset, bitwise."""
    import rmd  # noqa: F401
    c = cases.sweep_case(shape)
    wy, wx = c["window"]
    q, k, v, grad = (_t(c[n]) for n in ("q", "k", "v", "grad"))
    ref = torch.ops.rmd.local_cross_attn(q, k, v, wy, wx)
    ref_back = torch.ops.rmd.local_cross_attn_backward(grad, q, k, v, wy, wx)

    def permuted(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

    def offset(t):
        return torch.zeros(t.numel() + 3, device=DEV)[3:].view_as(t).copy_(t)

    for view in (permuted, offset):
        qv, kv, vv, gv = view(q), view(k), view(v), view(grad)
        assert not qv.is_contiguous() or qv.storage_offset() == 3
        assert torch.equal(torch.ops.rmd.local_cross_attn(qv, kv, vv, wy, wx), ref)
        for a, b in zip(torch.ops.rmd.local_cross_attn_backward(gv, qv, kv, vv, wy, wx), ref_back):
            assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(1, 19, 21, 5, 35, 2, 2, 3, 3), (1, 3, 9, 6, 67, 1, 1, 5, 5)], ids=["fast", "generic"])
def test_two_runs_are_bitwise_equal(shape):
    import rmd  # noqa: F401
    c = cases.sweep_case(shape)
    wy, wx = c["window"]
    q, k, v, grad = (_t(c[n]) for n in ("q", "k", "v", "grad"))
    a, b = (torch.ops.rmd.local_cross_attn(q, k, v, wy, wx) for _ in range(2))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a, b = (torch.ops.rmd.local_cross_attn_backward(grad, q, k, v, wy, wx) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_opcheck():
    import rmd  # noqa: F401
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    for shape in (FAST_SHAPE, GENERIC_SHAPE):
        c = cases.sweep_case(shape)
        wy, wx = c["window"]
        torch.library.opcheck(torch.ops.rmd.local_cross_attn, (_t(c["q"], True), _t(c["k"], True), _t(c["v"], True), wy, wx),
                              test_utils=utils)
        torch.library.opcheck(torch.ops.rmd.local_cross_attn_backward,
                              (_t(c["grad"]), _t(c["q"]), _t(c["k"]), _t(c["v"]), wy, wx), test_utils=utils)


def test_forward_and_backward_never_wait_for_the_host():
    from rmd import ops
    c = cases.sweep_case(FAST_SHAPE)
    q, k, v, grad = _t(c["q"], True), _t(c["k"], True), _t(c["v"], True), _t(c["grad"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.autograd.grad(ops.local_cross_attn(q, k, v), (q, k, v), grad)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd
    from rmd import _lib

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
    with pytest.raises(RuntimeError, match=r"\(2, 4, 7, 6\).*\(2, 4, 3, 3\)"):                         # 7 / 3
        torch.ops.rmd.local_cross_attn(z(2, 4, 7, 6), z(2, 4, 3, 3), z(2, 5, 3, 3), 3, 3)
    with pytest.raises(RuntimeError, match=r"\(1, 12, 6, 7\).*\(1, 12, 3, 3\)"):
        rmd.HUpCrossAttn(12).to(DEV)(z(1, 12, 3, 3), z(1, 12, 6, 7))
    bad = [
        lambda: torch.ops.rmd.local_cross_attn(z(2, 4, 6, 6), z(2, 3, 3, 3), z(2, 5, 3, 3), 3, 3),
        lambda: torch.ops.rmd.local_cross_attn(z(2, 4, 6, 6), z(2, 4, 3, 3), z(2, 5, 3, 3), 2, 3),
        lambda: torch.ops.rmd.local_cross_attn(z(2, 4, 6, 6, dtype=torch.int64), z(2, 4, 3, 3), z(2, 5, 3, 3), 3, 3),
        lambda: torch.ops.rmd.local_cross_attn(z(2, 4, 6, 6), torch.zeros(2, 4, 3, 3), z(2, 5, 3, 3), 3, 3),   # mixed devices
        lambda: rmd.ops.local_cross_attn(z(2, 4, 6, 6), z(2, 4, 3, 3), torch.zeros(2, 5, 3, 3)),
        lambda: torch.ops.rmd.local_cross_attn_backward(z(2, 5, 6, 5), z(2, 4, 6, 6), z(2, 4, 3, 3), z(2, 5, 3, 3), 3, 3),
        lambda: torch.ops.rmd.local_cross_attn_backward(torch.zeros(2, 5, 6, 6), z(2, 4, 6, 6), z(2, 4, 3, 3),
                                                        z(2, 5, 3, 3), 3, 3),
    ]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
