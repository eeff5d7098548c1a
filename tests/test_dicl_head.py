"""The DICL flow head without a GPU: the float64 restatement of dicl_head_cases.py against the fixtures
the reference wrote (tests/golden/gen_golden_dicl_head.py), the CPU kernels of the two operators and
the drop-in modules against the same fixtures (the reference's own ATen expressions: error 0.0), the
operator table, schemas, fake shapes, the C ABI's argument checks and FlowLevelMixin on the level
fixture."""

import ctypes

import numpy as np
import pytest
import torch

import dicl_head_cases as cases
from conftest import rel_max_err
from dicl_head_cases import HEAD_FIXTURES, fixture


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_restatement_reproduces_the_reference(name):
    """forward64 / backward64 against the reference's fp32 outputs, NaN positions included."""
    g = fixture(name)
    flow, entropy = cases.forward64(g["cost"])
    grad = cases.backward64(g["cost"], g["grad_flow"], g["grad_entropy"])
    for key, ours in (("flow", flow), ("entropy", entropy), ("grad_cost", grad)):
        err = rel_max_err(g[key], ours)
        print(f"{name} {key}: reference fp32 vs float64 restatement {err:.3e}")
        assert err <= cases.GATE, (name, key, err)


def test_restatement_coarse_flow_and_single_displacement():
    """The coarse flow is added to the flow only; D = 1 gives flow 0 and entropy 0 / 0 = NaN."""
    c = cases.sweep_case((2, 3, 3, 5, 13))
    assert np.array_equal(c["flow_coarse"], c["flow"] + c["coarse"].astype(np.float64))
    one = cases.sweep_case((1, 0, 0, 2, 3))
    assert np.array_equal(one["flow"], np.zeros((1, 2, 2, 3))) and np.isnan(one["entropy"]).all()
    assert np.isnan(one["grad_cost"]).all()


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_cpu_operators_reproduce_the_fixtures(name):
    """CPU dispatch: the same ATen operations as the reference, so the error is 0.0."""
    import rmd  # noqa: F401
    g = fixture(name)
    cost = torch.from_numpy(g["cost"]).requires_grad_(True)
    out = torch.ops.rmd.dicl_flow_head(cost, None, cases.EPS)
    assert out.shape == (cost.shape[0], 3) + tuple(cost.shape[3:]) and out.dtype == torch.float32
    assert rel_max_err(out[:, :2].detach().numpy(), g["flow"]) == 0.0
    assert rel_max_err(out[:, 2].detach().numpy(), g["entropy"]) == 0.0
    grad = torch.from_numpy(np.concatenate([g["grad_flow"], g["grad_entropy"][:, None]], axis=1))
    (dc,) = torch.autograd.grad(out, cost, grad)
    assert rel_max_err(dc.numpy(), g["grad_cost"]) == 0.0
    back = torch.ops.rmd.dicl_flow_head_backward(grad, cost.detach(), cases.EPS)
    assert rel_max_err(back.numpy(), g["grad_cost"]) == 0.0


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_cpu_modules_are_drop_ins(name):
    """FlowRegression / FlowEntropy: constructor, shapes, dtypes, values and gradients of the reference."""
    import rmd
    g = fixture(name)
    cost = torch.from_numpy(g["cost"]).requires_grad_(True)
    regression, entropy = rmd.dicl.FlowRegression(), rmd.dicl.FlowEntropy()
    assert entropy.eps == 1e-9 and rmd.dicl.FlowEntropy(eps=1e-6).eps == 1e-6
    assert not list(regression.parameters()) and not list(entropy.state_dict())
    flow, ent = regression(cost), entropy(cost)
    assert flow.shape == g["flow"].shape and ent.shape == g["entropy"].shape
    assert flow.dtype == ent.dtype == torch.float32
    assert rel_max_err(flow.detach().numpy(), g["flow"]) == 0.0
    assert rel_max_err(ent.detach().numpy(), g["entropy"]) == 0.0
    (dc,) = torch.autograd.grad((flow, ent), cost, (torch.from_numpy(g["grad_flow"]), torch.from_numpy(g["grad_entropy"])))
    assert rel_max_err(dc.numpy(), g["grad_cost"]) == 0.0


def test_ops_entry_returns_views_and_the_coarse_gradient():
    from rmd import ops
    c = cases.sweep_case((2, 3, 3, 5, 13))
    cost = torch.from_numpy(c["cost"]).requires_grad_(True)
    coarse = torch.from_numpy(c["coarse"]).requires_grad_(True)
    flow, entropy = ops.dicl_flow_head(cost, coarse)
    assert flow.shape == (2, 2, 5, 13) and entropy.shape == (2, 1, 5, 13)
    assert flow._base is not None and flow._base is entropy._base           # two views of the one output
    assert rel_max_err(flow.detach().numpy(), c["flow_coarse"]) <= cases.GATE
    assert rel_max_err(entropy[:, 0].detach().numpy(), c["entropy"]) <= cases.GATE
    grad = torch.from_numpy(c["grad"])
    dc, df = torch.autograd.grad((flow, entropy), (cost, coarse), (grad[:, :2], grad[:, 2:]))
    assert torch.equal(df, grad[:, :2])
    assert rel_max_err(dc.numpy(), c["grad_cost"]) <= cases.GATE
    with pytest.raises(ValueError, match="different devices"):
        ops.dicl_flow_head(cost, coarse.detach().to("meta"))


def test_head_operator_table():
    from rmd import library
    assert library.head_operators() == ["dicl_flow_head", "dicl_flow_head_backward"]
    for name in library.head_operators():
        assert hasattr(torch.ops.rmd, name)
        assert name not in library.operators() + library.loss_operators() + library.metric_operators()


def test_schemas():
    import rmd  # noqa: F401
    fwd = torch.ops.rmd.dicl_flow_head.default._schema
    assert [(a.name, str(a.type)) for a in fwd.arguments] == [("cost", "Tensor"), ("flow_coarse", "Optional[Tensor]"),
                                                              ("eps", "float")]
    assert [str(r.type) for r in fwd.returns] == ["Tensor"]
    bwd = torch.ops.rmd.dicl_flow_head_backward.default._schema
    assert [(a.name, str(a.type)) for a in bwd.arguments] == [("grad", "Tensor"), ("cost", "Tensor"), ("eps", "float")]
    assert [str(r.type) for r in bwd.returns] == ["Tensor"]


def test_fake_kernels_propagate_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import rmd  # noqa: F401
    with FakeTensorMode():
        cost = torch.empty(2, 7, 5, 12, 16, device="cuda")
        coarse = torch.empty(2, 2, 12, 16, device="cuda")
        for fc in (None, coarse):
            out = torch.ops.rmd.dicl_flow_head(cost, fc, 1e-9)
            assert out.shape == (2, 3, 12, 16) and out.dtype == torch.float32 and out.device.type == "cuda"
        one = torch.empty(1, 1, 1, 2, 3, device="cuda")                         # D = 1
        assert torch.ops.rmd.dicl_flow_head(one, None, 1e-9).shape == (1, 3, 2, 3)
        grad = torch.empty(2, 3, 12, 16, device="cuda")
        back = torch.ops.rmd.dicl_flow_head_backward(grad, cost.half(), 1e-9)
        assert back.shape == cost.shape and back.dtype == torch.float32
        assert torch.ops.rmd.dicl_flow_head_backward(torch.empty(1, 3, 2, 3, device="cuda"), one, 1e-9).shape == one.shape
        with pytest.raises(ValueError, match="odd"):
            torch.ops.rmd.dicl_flow_head(torch.empty(2, 4, 5, 12, 16, device="cuda"), None, 1e-9)


@pytest.mark.parametrize("bad", [
    lambda: torch.ops.rmd.dicl_flow_head(torch.zeros(2, 49, 4, 5), None, 1e-9),                      # not 5-D
    lambda: torch.ops.rmd.dicl_flow_head(torch.zeros(2, 6, 7, 4, 5), None, 1e-9),                    # even du
    lambda: torch.ops.rmd.dicl_flow_head(torch.zeros(2, 7, 19, 4, 5), None, 1e-9),                   # rv = 9
    lambda: torch.ops.rmd.dicl_flow_head(torch.zeros(2, 7, 7, 4, 5), torch.zeros(2, 2, 5, 4), 1e-9),  # coarse shape
    lambda: torch.ops.rmd.dicl_flow_head(torch.zeros(2, 7, 7, 4, 5), None, 0.5),                     # eps
    lambda: torch.ops.rmd.dicl_flow_head(torch.zeros(2, 7, 7, 4, 5), None, -1e-9),
    lambda: torch.ops.rmd.dicl_flow_head(torch.zeros(2, 7, 7, 4, 5, dtype=torch.int32), None, 1e-9),  # dtype
    lambda: torch.ops.rmd.dicl_flow_head_backward(torch.zeros(2, 2, 4, 5), torch.zeros(2, 7, 7, 4, 5), 1e-9),
])
def test_bad_arguments_raise_on_the_cpu(bad):
    import rmd  # noqa: F401
    with pytest.raises(ValueError, match="dicl_flow_head"):
        bad()


def test_abi_argument_checks_need_no_gpu():
    """Every check runs on the host before any launch: negative codes and a message, no GPU touched.  The
    pointers are never dereferenced (host buffers stand in for device memory)."""
    from rmd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(cost=p, aux=p, batch=1, du=3, dv=3, pixels=1, eps=1e-9, out=p)
    bad = [dict(cost=None), dict(out=None), dict(du=4), dict(dv=2), dict(du=19), dict(dv=-1), dict(du=0),
           dict(batch=0), dict(batch=65536), dict(pixels=0), dict(pixels=-3), dict(eps=0.5), dict(eps=-1e-3),
           dict(eps=float("nan"))]
    for fn, needs_aux in ((lib.rmd_dicl_flow_head, False), (lib.rmd_dicl_flow_head_backward, True)):
        for change in bad + ([dict(aux=None)] if needs_aux else []):
            a = {**good, **change}
            rc = fn(a["cost"], a["aux"], a["batch"], a["du"], a["dv"], a["pixels"], a["eps"], a["out"], None)
            assert rc in (-1, -2), (fn.__name__, change, rc)
            assert b"rmd_dicl_flow_head" in lib.rmd_last_error(), (fn.__name__, change)


def test_flow_level_mixin_on_the_cpu_matches_the_reference_level():
    """FlowLevelMixin.forward -> compute_flow with one head call: flow, flow_raw, the four gradients and the
    state-dict keys of the reference's FlowLevel."""
    g = fixture(cases.LEVEL_FIXTURE)
    got, keys = cases.run_level("cpu")
    assert keys == sorted(g["keys"].tolist())
    for name in ("flow", "flow_raw", "grad_feat1", "grad_feat2", "grad_dap_conv1", "grad_ctxnet_conv0"):
        err = rel_max_err(got[name], g[name])
        print(f"level {name}: {err:.3e}")
        assert got[name].shape == g[name].shape
        assert err == 0.0, (name, err)


def test_flow_level_mixin_launches_one_head_per_level(monkeypatch):
    """compute_flow calls the head operator once (coarse flow passed in), never the two modules."""
    import rmd
    g = fixture(cases.LEVEL_FIXTURE)
    lvl = cases.make_level(int(g["channels"]), 3, (3, 3)).eval()
    calls = []
    real = rmd.cpu.dicl_flow_head_eager
    monkeypatch.setattr(rmd.cpu, "dicl_flow_head_eager", lambda *a: calls.append(a[1] is not None) or real(*a))
    lvl.flow.register_forward_hook(lambda *a: calls.append("flow module"))
    lvl.entropy.register_forward_hook(lambda *a: calls.append("entropy module"))
    t = torch.from_numpy
    with torch.no_grad():
        flow, raw = lvl(t(g["img1"]), t(g["feat1"]), t(g["feat2"]), t(g["flow_coarse"]), raw=False)
    assert calls == [True] and raw is None and flow.shape == g["flow"].shape
