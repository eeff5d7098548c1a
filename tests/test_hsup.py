"""The hidden-state upsamplers without a GPU: the float64 restatement of hsup_cases.py against the
fixtures the reference wrote (tests/golden/gen_golden_hsup.py), the reference's fp32 composition
against the restatement on every sweep case (a quarter of the gate at the most), the CPU kernels of the
two operators and the drop-in modules against the fixtures (the reference's own ATen expressions: error
0.0), the operator table, schemas, fake shapes, the factory, the C ABI's argument checks and the
route query."""

import ctypes

import numpy as np
import pytest
import torch

import hsup_cases as cases
from conftest import rel_max_err
from hsup_cases import GATE, MODULE_FIXTURES, fixture


def test_restatement_reproduces_the_reference_core():
    """forward64 / backward64 against the reference's fp32 results on non-finite inputs, NaN positions included."""
    g = fixture(cases.CORE_FIXTURE)
    assert np.isnan(g["q"]).any() and np.isnan(g["k"]).any() and np.isnan(g["v"]).any() and np.isinf(g["v"]).any()
    assert np.isfinite(g["out"]).any() and np.isnan(g["out"]).any()
    out, _ = cases.forward64(g["q"], g["k"], g["v"])
    grads = cases.backward64(g["grad"], g["q"], g["k"], g["v"])
    for key, ours in zip(cases.RESULTS, (out,) + grads):
        err = rel_max_err(g[key], ours)
        print(f"core {key}: reference fp32 vs float64 restatement {err:.3e}")
        assert err <= GATE, (key, err)


@pytest.mark.parametrize("name", MODULE_FIXTURES)
def test_restatement_reproduces_the_reference_module(name):
    """The 1x1 convolutions in float64 around forward64 against the reference module's output."""
    from detinit import det_init
    import rmd
    g = fixture(name)
    m = det_init(rmd.hsup.HUpCrossAttn(int(g["channels"]))).double()
    with torch.no_grad():
        hp, hi = torch.from_numpy(g["h_prev"]).double(), torch.from_numpy(g["h_init"]).double()
        x, _ = cases.forward64(m.conv_q(hi).numpy(), m.conv_k(hp).numpy(), m.conv_v_prev(hp).numpy())
        out = m.conv_out(m.conv_v_init(hi) + torch.from_numpy(x)).numpy()
    err = rel_max_err(g["out"], out)
    print(f"{name} out: reference fp32 vs float64 restatement {err:.3e}")
    assert err <= GATE


def test_restatement_weights_are_a_softmax_over_the_window():
    c = cases.sweep_case((1, 5, 7, 1, 1, 1, 1, 3, 3))
    _, a = cases.forward64(c["q"], c["k"], c["v"], c["window"])
    assert a.shape == (1, 9, 1, 1) and abs(a.sum() - 1.0) < 1e-12
    # eight padded neighbours: logit 0 each, part of the softmax
    s = float((c["q"].astype(np.float64) * c["k"]).sum())
    assert np.allclose(a[0, 4, 0, 0], np.exp(s) / (np.exp(s) + 8.0), rtol=1e-12)
    assert np.allclose(c["out"][0, :, 0, 0], a[0, 4, 0, 0] * c["v"][0, :, 0, 0].astype(np.float64), rtol=1e-12)


def test_reference_fp32_error_is_within_a_quarter_of_the_gate():
    """The gate as a condition on the inputs: what fp32 itself loses on the sweep and the peaked case."""
    errors = cases.reference_fp32_errors()
    assert len(errors) == len(cases.SWEEP) + 1
    for label, per in errors.items():
        for name, err in per.items():
            assert err <= cases.REFERENCE_SHARE * GATE, (label, name, err)


def test_peaked_case_is_peaked():
    c = cases.peaked_case()
    _, a = cases.forward64(c["q"], c["k"], c["v"], c["window"])
    assert np.median(a.max(axis=1)) > 0.99


def test_cpu_operators_reproduce_the_core_fixture():
    """CPU dispatch: the same ATen operations as the reference, so the error is 0.0."""
    import rmd  # noqa: F401
    g = fixture(cases.CORE_FIXTURE)
    q, k, v = (torch.from_numpy(g[n]).requires_grad_(True) for n in ("q", "k", "v"))
    out = torch.ops.rmd.local_cross_attn(q, k, v, 3, 3)
    assert out.shape == g["out"].shape and out.dtype == torch.float32
    assert rel_max_err(out.detach().numpy(), g["out"]) == 0.0
    grad = torch.from_numpy(g["grad"])
    for name, got in zip(cases.RESULTS[1:], torch.autograd.grad(out, (q, k, v), grad)):
        assert rel_max_err(got.numpy(), g[name]) == 0.0, name
    back = torch.ops.rmd.local_cross_attn_backward(grad, q.detach(), k.detach(), v.detach(), 3, 3)
    for name, got in zip(cases.RESULTS[1:], back):
        assert rel_max_err(got.numpy(), g[name]) == 0.0, name


@pytest.mark.parametrize("name", MODULE_FIXTURES + [cases.BILINEAR_FIXTURE])
def test_cpu_modules_are_drop_ins(name):
    """Values, input and weight gradients and state-dict keys of the reference's modules."""
    g = fixture(name)
    got, keys = cases.run_module(name, "cpu")
    assert keys == sorted(g["keys"].tolist())
    names = [n for n in g if n == "out" or n.startswith("grad_")]
    assert len(names) == 3 + len(keys)
    for n in names:
        assert got[n].shape == g[n].shape
        assert rel_max_err(got[n], g[n]) == 0.0, n


def test_modules_keep_the_reference_interface():
    import rmd
    m = rmd.HUpCrossAttn(12)
    assert sorted({k.split(".")[0] for k in m.state_dict()}) == cases.CROSSATTN_KEYS
    assert m.window_size == (3, 3) and m.window_padding == (1, 1)
    assert m.conv_q.out_channels == m.conv_k.out_channels == 64 and m.conv_v_prev.out_channels == 12
    bil = rmd.HUpBilinear(5)
    assert sorted(bil.state_dict()) == ["conv1.bias", "conv1.weight"]
    assert torch.equal(bil.conv1.weight[:, :, 0, 0], torch.eye(5))                # initialised as the identity
    h_prev, h_init = torch.randn(1, 5, 2, 3), torch.randn(1, 5, 4, 6)
    assert rmd.HUpNone(5)(h_prev, h_init) is h_init and not list(rmd.HUpNone(5).state_dict())
    with pytest.raises(RuntimeError, match=r"\(1, 12, 5, 6\).*\(1, 12, 2, 3\)"):
        m(torch.zeros(1, 12, 2, 3), torch.zeros(1, 12, 5, 6))


def test_factory_names_and_error():
    import rmd
    for name, cls in (("none", rmd.HUpNone), ("bilinear", rmd.HUpBilinear), ("crossattn", rmd.HUpCrossAttn)):
        assert type(rmd.make_hidden_state_upsampler(name, 8)) is cls
        assert type(rmd.hsup.make_hidden_state_upsampler(name, 8)) is cls
    with pytest.raises(ValueError, match="unknown hidden state upsampler type 'nearest'"):
        rmd.make_hidden_state_upsampler("nearest", 8)


def test_ops_entry_on_the_cpu():
    from rmd import ops
    c = cases.sweep_case((1, 4, 3, 3, 4, 2, 2, 5, 3))
    q, k, v = (torch.from_numpy(c[n]).requires_grad_(True) for n in ("q", "k", "v"))
    out = ops.local_cross_attn(q, k, v, window=c["window"])
    assert rel_max_err(out.detach().numpy(), c["out"]) <= GATE
    for name, got in zip(cases.RESULTS[1:], torch.autograd.grad(out, (q, k, v), torch.from_numpy(c["grad"]))):
        assert rel_max_err(got.numpy(), c[name]) <= GATE, name
    with pytest.raises(ValueError, match="different devices"):
        ops.local_cross_attn(q, k.detach().to("meta"), v)


def test_attn_operator_table():
    from rmd import library
    assert library.attn_operators() == ["local_cross_attn", "local_cross_attn_backward"]
    others = (library.operators() + library.loss_operators() + library.metric_operators()
              + library.head_operators())
    for name in library.attn_operators():
        assert hasattr(torch.ops.rmd, name) and name not in others


def test_schemas():
    import rmd  # noqa: F401
    fwd = torch.ops.rmd.local_cross_attn.default._schema
    assert [(a.name, str(a.type)) for a in fwd.arguments] == [("q", "Tensor"), ("k", "Tensor"), ("v", "Tensor"),
                                                              ("win_y", "int"), ("win_x", "int")]
    assert [str(r.type) for r in fwd.returns] == ["Tensor"]
    bwd = torch.ops.rmd.local_cross_attn_backward.default._schema
    assert [(a.name, str(a.type)) for a in bwd.arguments] == [("grad", "Tensor"), ("q", "Tensor"), ("k", "Tensor"),
                                                              ("v", "Tensor"), ("win_y", "int"), ("win_x", "int")]
    assert [str(r.type) for r in bwd.returns] == ["Tensor"] * 3


def test_fake_kernels_propagate_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import rmd  # noqa: F401
    with FakeTensorMode():
        q = torch.empty(2, 64, 12, 16, device="cuda")
        k = torch.empty(2, 64, 6, 4, device="cuda")
        v = torch.empty(2, 128, 6, 4, device="cuda", dtype=torch.float16)
        out = torch.ops.rmd.local_cross_attn(q, k, v, 3, 5)
        assert out.shape == (2, 128, 12, 16) and out.dtype == torch.float32 and out.device.type == "cuda"
        grads = torch.ops.rmd.local_cross_attn_backward(torch.empty(2, 128, 12, 16, device="cuda"), q, k, v, 3, 5)
        assert [g.shape for g in grads] == [q.shape, k.shape, v.shape]
        assert all(g.dtype == torch.float32 for g in grads)
        with pytest.raises(RuntimeError, match="integer multiple"):
            torch.ops.rmd.local_cross_attn(torch.empty(2, 64, 13, 16, device="cuda"), k, v, 3, 3)


@pytest.mark.parametrize("bad, kind", [
    (lambda: torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 6), torch.zeros(2, 4, 3, 3), torch.zeros(2, 5, 3, 3), 3, 3),
     ValueError),                                                                                    # not 4-D
    (lambda: torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 6, 6), torch.zeros(2, 3, 3, 3), torch.zeros(2, 5, 3, 3), 3, 3),
     ValueError),                                                                                    # ck differs
    (lambda: torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 6, 6), torch.zeros(2, 4, 3, 3), torch.zeros(2, 5, 3, 2), 3, 3),
     ValueError),                                                                                    # k / v cells
    (lambda: torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 6, 6), torch.zeros(2, 4, 3, 3), torch.zeros(2, 5, 3, 3), 2, 3),
     ValueError),                                                                                    # even window
    (lambda: torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 6, 6), torch.zeros(2, 4, 3, 3), torch.zeros(2, 5, 3, 3), 3, 7),
     ValueError),                                                                                    # window 7
    (lambda: torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 7, 6), torch.zeros(2, 4, 3, 3), torch.zeros(2, 5, 3, 3), 3, 3),
     RuntimeError),                                                                                  # 7 / 3
    (lambda: torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 6, 6, dtype=torch.int32), torch.zeros(2, 4, 3, 3),
                                            torch.zeros(2, 5, 3, 3), 3, 3), ValueError),             # dtype
    (lambda: torch.ops.rmd.local_cross_attn_backward(torch.zeros(2, 4, 6, 6), torch.zeros(2, 4, 6, 6),
                                                     torch.zeros(2, 4, 3, 3), torch.zeros(2, 5, 3, 3), 3, 3),
     ValueError),                                                                                    # grad channels
])
def test_bad_arguments_raise_on_the_cpu(bad, kind):
    import rmd  # noqa: F401
    with pytest.raises(kind, match="local_cross_attn"):
        bad()


def test_non_dividing_message_names_both_shapes():
    import rmd  # noqa: F401
    with pytest.raises(RuntimeError, match=r"\(2, 4, 7, 6\).*\(2, 4, 3, 3\)"):
        torch.ops.rmd.local_cross_attn(torch.zeros(2, 4, 7, 6), torch.zeros(2, 4, 3, 3), torch.zeros(2, 5, 3, 3), 3, 3)


def test_abi_argument_checks_need_no_gpu():
    """Every check runs on the host before any launch: negative codes and a message, no GPU touched.  The
    pointers are never dereferenced (host buffers stand in for device memory)."""
    from rmd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(q=p, k=p, v=p, batch=1, ck=2, cv=2, h=2, w=2, h2=1, w2=1, wy=3, wx=3, out=p, grad=p, gk=p, gv=p, ws=p)
    sizes = ("batch", "ck", "cv", "h", "w", "h2", "w2", "wy", "wx")
    bad = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(wy=2), dict(wx=4), dict(wy=0), dict(wx=7),
           dict(wy=-3), dict(h2=0), dict(w2=0), dict(h=1, h2=2), dict(w=1, w2=2), dict(h=3, h2=2),     # factor 0, 3 / 2 dict(w=5, w2=3), dict(batch=0), dict(ck=0), dict(cv=-1),
           dict(h=0), dict(h=130, h2=2), dict(batch=70000)]
    for change in bad:
        a = {**good, **change}
        rc = lib.rmd_local_cross_attn(a["q"], a["k"], a["v"], *(a[s] for s in sizes), a["out"], None)
        assert rc in (-1, -2), (change, rc)
        assert b"rmd_local_cross_attn" in lib.rmd_last_error(), change
    for change in bad + [dict(grad=None), dict(gk=None), dict(gv=None), dict(ws=None)]:
        a = {**good, **change}
        rc = lib.rmd_local_cross_attn_backward(a["grad"], a["q"], a["k"], a["v"], *(a[s] for s in sizes), a["out"],
                                               a["gk"], a["gv"], a["ws"], None)
        assert rc in (-1, -2), (change, rc)
        assert b"rmd_local_cross_attn_backward" in lib.rmd_last_error(), change
        if not any(n in change for n in ("q", "k", "v", "out", "grad", "gk", "gv", "ws")):
            assert lib.rmd_local_cross_attn_kernel(*(a[s] for s in sizes)) == b"invalid", change


def test_workspace_bytes():
    from rmd import _lib
    lib = _lib.lib()
    assert lib.rmd_local_cross_attn_workspace_bytes(8, 56, 128, 3, 3) == 8 * 2 * 9 * 56 * 128 * 4
    assert lib.rmd_local_cross_attn_workspace_bytes(1, 3, 5, 5, 1) == 2 * 5 * 15 * 4
    assert lib.rmd_local_cross_attn_workspace_bytes(0, 3, 5, 3, 3) == 0


def test_route_query():
    """The 3x3 window at factor 2x2 takes the specialised route, everything else the generic one, and every
    route has a sweep shape."""
    from rmd import _lib
    lib = _lib.lib()
    assert lib.rmd_local_cross_attn_kernel(8, 64, 128, 56, 128, 28, 64, 3, 3) == cases.FAST.encode()
    for args in ((8, 64, 128, 56, 128, 28, 64, 5, 5), (8, 64, 128, 56, 128, 28, 64, 1, 3), (1, 4, 4, 6, 6, 2, 3, 3, 3),
                 (1, 4, 4, 6, 6, 3, 2, 3, 3), (1, 4, 4, 6, 6, 6, 6, 3, 3), (1, 4, 4, 12, 12, 3, 3, 3, 3)):
        assert lib.rmd_local_cross_attn_kernel(*args) == cases.GENERIC.encode(), args
    routes = {cases.route(s) for s in cases.SWEEP}
    assert routes == {cases.FAST, cases.GENERIC}
    assert cases.route(cases.PEAKED) == cases.FAST
    generic_windows = {s[7:] for s in cases.SWEEP if cases.route(s) == cases.GENERIC}
    assert {(3, 3), (1, 1), (5, 3), (1, 5), (5, 5)} <= generic_windows
