"""The DICL flow head on the GPU: csrc/dicl_head.hip through torch.ops.rmd.dicl_flow_head against the
fixtures the reference wrote (tests/golden/gen_golden_dicl_head.py) and against the float64
restatement of dicl_head_cases.py over a shape sweep (register and generic paths, with and without
the coarse flow), gradient selection, views, the level fixture through FlowLevelMixin, determinism,
opcheck, the no-host-synchronisation rule and argument checks.

Gate: conftest.rel_max_err <= 1e-5 for flow, entropy and grad_cost (dicl_head_cases.GATE, reasoned
there); the level fixture within 1e-4 (the DAP runs in split-bf16)."""

import numpy as np
import pytest
import torch

import dicl_head_cases as cases
from conftest import rel_max_err
from dicl_head_cases import GATE, HEAD_FIXTURES, SWEEP, fixture

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _check(label, got, ref):
    err = rel_max_err(got.detach().cpu().numpy(), ref)
    print(f"{label}: {err:.3e}")
    assert err <= GATE, (label, err)


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_fixtures_through_the_modules(name):
    """FlowRegression / FlowEntropy on the reference's inputs: values, NaN positions, one backward through both."""
    import rmd
    g = fixture(name)
    cost = _t(g["cost"], True)
    flow, entropy = rmd.dicl.FlowRegression()(cost), rmd.dicl.FlowEntropy()(cost)
    assert flow.shape == g["flow"].shape and entropy.shape == g["entropy"].shape
    _check(f"{name} flow", flow, g["flow"])
    _check(f"{name} entropy", entropy, g["entropy"])
    (dc,) = torch.autograd.grad((flow, entropy), cost, (_t(g["grad_flow"]), _t(g["grad_entropy"])))
    _check(f"{name} grad_cost", dc, g["grad_cost"])


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_fixtures_through_the_operator(name):
    """One forward and one backward launch for both outputs."""
    import rmd  # noqa: F401
    g = fixture(name)
    cost = _t(g["cost"])
    out = torch.ops.rmd.dicl_flow_head(cost, None, cases.EPS)
    _check(f"{name} flow", out[:, :2], g["flow"])
    _check(f"{name} entropy", out[:, 2], g["entropy"])
    grad = _t(np.concatenate([g["grad_flow"], g["grad_entropy"][:, None]], axis=1))
    _check(f"{name} grad_cost", torch.ops.rmd.dicl_flow_head_backward(grad, cost, cases.EPS), g["grad_cost"])


@pytest.mark.parametrize("with_coarse", [False, True], ids=["plain", "coarse"])
@pytest.mark.parametrize("shape", SWEEP)
def test_shape_sweep_against_float64(shape, with_coarse):
    """Forward and backward against the float64 restatement on mixed-scale costs."""
    from rmd import ops
    c = cases.sweep_case(shape)
    cost = _t(c["cost"], True)
    coarse = _t(c["coarse"], True) if with_coarse else None
    flow, entropy = ops.dicl_flow_head(cost, coarse)
    assert flow.shape == c["flow"].shape and entropy.shape == (shape[0], 1) + shape[3:]
    _check(f"{shape} flow", flow, c["flow_coarse"] if with_coarse else c["flow"])
    _check(f"{shape} entropy", entropy[:, 0], c["entropy"])
    if shape[1] == 0 and shape[2] == 0:                          # D = 1
        assert torch.equal(flow.detach(), coarse.detach() if with_coarse else torch.zeros_like(flow))
        assert torch.isnan(entropy).all()
    grad = _t(c["grad"])
    grads = torch.autograd.grad((flow, entropy), (cost, coarse) if with_coarse else (cost,), (grad[:, :2], grad[:, 2:]))
    _check(f"{shape} grad_cost", grads[0], c["grad_cost"])
    if with_coarse:
        assert torch.equal(grads[1], grad[:, :2])


@pytest.mark.parametrize("shape", [(2, 3, 3, 5, 13), (3, 2, 5, 7, 9)], ids=["register", "generic"])
def test_gradient_selection(shape):
    """Only the flow or only the entropy carries an upstream gradient."""
    from rmd import ops
    c = cases.sweep_case(shape)
    grad = _t(c["grad"])
    cost = _t(c["cost"], True)
    flow, entropy = ops.dicl_flow_head(cost)
    (d_flow,) = torch.autograd.grad(flow, cost, grad[:, :2], retain_graph=True)
    _check(f"{shape} flow only", d_flow, c["grad_cost_flow_only"])
    (d_ent,) = torch.autograd.grad(entropy, cost, grad[:, 2:])
    _check(f"{shape} entropy only", d_ent, c["grad_cost_entropy_only"])


def test_views_give_the_results_of_their_contiguous_copies():
    """A permuted (non-contiguous) cost and a view at a storage offset."""
    import rmd  # noqa: F401
    c = cases.sweep_case((2, 3, 3, 5, 13))
    cost, grad = _t(c["cost"]), _t(c["grad"])
    ref = torch.ops.rmd.dicl_flow_head(cost, None, cases.EPS)
    ref_back = torch.ops.rmd.dicl_flow_head_backward(grad, cost, cases.EPS)
    permuted = cost.permute(0, 3, 4, 1, 2).contiguous().permute(0, 3, 4, 1, 2)
    buf = torch.zeros(cost.numel() + 3, device=DEV)
    offset = buf[3:].view_as(cost).copy_(cost)
    grad_view = grad.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not permuted.is_contiguous() and offset.storage_offset() == 3 and not grad_view.is_contiguous()
    for view in (permuted, offset):
        assert torch.equal(torch.ops.rmd.dicl_flow_head(view, None, cases.EPS), ref)
        assert torch.equal(torch.ops.rmd.dicl_flow_head_backward(grad_view, view, cases.EPS), ref_back)


def test_level_fixture_through_the_mixin():
    """cost -> DAP -> one head launch -> context network, forward and four gradients, against the reference's level."""
    g = fixture(cases.LEVEL_FIXTURE)
    got, keys = cases.run_level(DEV)
    assert keys == sorted(g["keys"].tolist())
    for name in ("flow", "flow_raw", "grad_feat1", "grad_feat2", "grad_dap_conv1", "grad_ctxnet_conv0"):
        err = rel_max_err(got[name], g[name])
        print(f"level {name}: {err:.3e}")
        assert err <= cases.LEVEL_GATE, (name, err)


@pytest.mark.parametrize("shape", [(1, 4, 4, 3, 67), (3, 2, 5, 7, 9)], ids=["register", "generic"])
def test_two_runs_are_bitwise_equal(shape):
    import rmd  # noqa: F401
    c = cases.sweep_case(shape)
    cost, coarse, grad = _t(c["cost"]), _t(c["coarse"]), _t(c["grad"])
    a, b = (torch.ops.rmd.dicl_flow_head(cost, coarse, cases.EPS) for _ in range(2))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a, b = (torch.ops.rmd.dicl_flow_head_backward(grad, cost, cases.EPS) for _ in range(2))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_opcheck():
    import rmd  # noqa: F401
    c = cases.sweep_case((2, 3, 3, 5, 13))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.rmd.dicl_flow_head, (_t(c["cost"], True), _t(c["coarse"], True), 1e-9), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.dicl_flow_head, (_t(c["cost"], True), None, 1e-9), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.dicl_flow_head_backward, (_t(c["grad"]), _t(c["cost"]), 1e-9), test_utils=utils)


def test_forward_and_backward_never_wait_for_the_host():
    from rmd import ops
    c = cases.sweep_case((2, 3, 3, 5, 13))
    cost, coarse, grad = _t(c["cost"], True), _t(c["coarse"], True), _t(c["grad"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        flow, entropy = ops.dicl_flow_head(cost, coarse)
        torch.autograd.grad((flow, entropy), (cost, coarse), (grad[:, :2], grad[:, 2:]))
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_bad_shapes_and_dtypes_are_rejected_before_any_launch(monkeypatch):
    import rmd  # noqa: F401
    from rmd import _lib

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
    bad = [
        lambda: torch.ops.rmd.dicl_flow_head(z(2, 49, 4, 5), None, 1e-9),
        lambda: torch.ops.rmd.dicl_flow_head(z(2, 6, 7, 4, 5), None, 1e-9),
        lambda: torch.ops.rmd.dicl_flow_head(z(2, 7, 19, 4, 5), None, 1e-9),
        lambda: torch.ops.rmd.dicl_flow_head(z(2, 7, 7, 4, 5), z(2, 3, 4, 5), 1e-9),
        lambda: torch.ops.rmd.dicl_flow_head(z(2, 7, 7, 4, 5), None, 0.5),
        lambda: torch.ops.rmd.dicl_flow_head(z(2, 7, 7, 4, 5, dtype=torch.int64), None, 1e-9),
        lambda: torch.ops.rmd.dicl_flow_head(z(2, 7, 7, 4, 5), torch.zeros(2, 2, 4, 5), 1e-9),          # mixed devices
        lambda: torch.ops.rmd.dicl_flow_head_backward(z(2, 3, 4, 6), z(2, 7, 7, 4, 5), 1e-9),
        lambda: torch.ops.rmd.dicl_flow_head_backward(z(2, 3, 4, 5, dtype=torch.int32), z(2, 7, 7, 4, 5), 1e-9),
    ]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
