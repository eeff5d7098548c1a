"""The differentiable fused dicl-1x1 cost without a GPU: the float64 oracle of dicl_match_grad_cases.py against
the reference's gradient fixtures, the ReLU guard's cap and the emulation-error bound that the GPU tests'
tolerance rests on, the CPU operators against the module path's autograd, module routing with
fused_backward on and off, hooks, state-dict keys, the operator table, schemas, fake shapes and the C
entry points' argument checks."""

import ctypes

import numpy as np
import pytest
import torch

import dicl_match_cases as fwd
import dicl_match_grad_cases as cases

CASES = cases.all_cases()
ORACLE_VS_FP32 = 1e-5        # the reference's fp32 composite is 1e-7 .. 1.1e-6 from float64 on the fixtures


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_oracle_matches_the_reference_fixture(name):
    """dap=False: the oracle's gradients of the folded parameters, taken through the fold by hand (conv
    weight s gW', batch-norm beta gt, last layer gw4 / gb4), and of both feature maps."""
    g, c = cases.fixture(name), cases.fixture_case(name)
    mod = cases.build_module(name)
    want = {k[len("nodap.grad."):]: g[k] for k in g if k.startswith("nodap.grad.")}
    got = {"fmap1": c["ref"]["grad_fmap1"], "fmap2": c["ref"]["grad_fmap2"],
           "mnet.3.weight": c["ref"]["gw4"], "mnet.3.bias": c["ref"]["gb4"]}
    for l in range(3):
        norm = mod.mnet[l][1]
        gw, gt = c["ref"][f"gW{l + 1}"], c["ref"][f"gt{l + 1}"]
        if isinstance(norm, torch.nn.BatchNorm2d):
            s = (norm.weight / torch.sqrt(norm.running_var + norm.eps)).detach().numpy().astype(np.float64)
            got[f"mnet.{l}.1.bias"] = gt
            with np.errstate(invalid="ignore"):
                gw = s[:, None] * gw
        got[f"mnet.{l}.0.weight"] = gw
    assert set(got) <= set(want)
    for k, v in got.items():
        if name == cases.NAN_FIXTURE:
            # positions only: ATen's threshold_backward lets the gradient through a NaN unit (NaN <= 0 is
            # false) where the mask z > 0 blocks it, so the finite values at the two poisoned pixels differ
            assert np.array_equal(np.isnan(v.reshape(want[k].shape)), np.isnan(want[k])), k
            continue
        err = cases.max_norm_err(want[k], v.reshape(want[k].shape))
        print(f"{name} {k}: fixture against float64 {err:.3e}")
        assert err <= ORACLE_VS_FP32, (k, err)


def test_nan_fixture_pins_the_positions_the_reference_has():
    g = cases.fixture(cases.NAN_FIXTURE)
    for tag in ("dap", "nodap"):
        assert np.isfinite(g[f"{tag}.grad.fmap1"]).all() and np.isfinite(g[f"{tag}.grad.fmap2"]).all()
        w1 = g[f"{tag}.grad.mnet.0.0.weight"][:, :, 0, 0]
        c = w1.shape[1] // 2
        assert np.isfinite(w1[:, :c]).all() and np.isnan(w1[:, c:]).all()          # the f2-half columns
        for k in ("mnet.1.0.weight", "mnet.2.0.weight", "mnet.3.weight"):
            assert np.isnan(g[f"{tag}.grad.{k}"]).all(), k
        for k in ("mnet.0.1.bias", "mnet.1.1.bias", "mnet.2.1.bias", "mnet.3.bias"):
            assert np.isfinite(g[f"{tag}.grad.{k}"]).all(), k


@pytest.mark.parametrize("label,get", CASES, ids=[c[0] for c in CASES])
def test_guard_cap_and_emulation_error(label, get):
    """At most GUARD_CAP of the columns guarded; e <= E_MAX on every output, so that a wrong emulation
    cannot widen the GPU gate max(1e-5, 3 e); with the guard the emulation's masks are float64's."""
    c = get()
    print(f"{label}: guarded {c['guarded']:.4f}  e " + "  ".join(f"{k} {v:.2e}" for k, v in c["e"].items()))
    assert c["guarded"] <= cases.GUARD_CAP
    assert not c["grad"][cases.guard(c["args"])].any() and np.count_nonzero(c["grad"]) > 0.85 * c["grad"].size
    for k, e in c["e"].items():
        assert e <= cases.E_MAX, (k, e)
        assert c["tol"][k] == max(1e-5, 3 * e)
    x, _ = fwd._columns(*c["args"][:4])
    z64, _ = cases.forward64(x, *c["args"][4:])
    zem, _ = cases.forward_emulated(x, *c["args"][4:])
    live = c["grad"].reshape(-1) != 0
    for a, e in zip(z64, zem):
        assert np.array_equal((a > 0)[:, live], (e > 0)[:, live])


@pytest.mark.parametrize("dap", [True, False], ids=["dap", "nodap"])
@pytest.mark.parametrize("name", cases.FIXTURES)
def test_cpu_operators_equal_the_module_path(name, dap):
    """fused="on", fused_backward=True on CPU tensors (the CPU kernels of both operators) against the same
    module with fused="off" and against the fixture; the forward hook fires once with the cost."""
    g = cases.fixture(name)
    off = cases.build_module(name, fused="off")
    on = cases.build_module(name, fused="on", fused_backward=True)
    seen = []
    handle = on.mnet.register_forward_hook(lambda m, i, o: seen.append((type(i[0]).__name__, tuple(o.shape))))
    want, _ = cases.module_gradients(off, g, dap)
    got, calls = cases.module_gradients(on, g, dap)
    handle.remove()
    b, _, h, w = g["fmap1"].shape
    d = 2 * int(g["radius"]) + 1
    assert seen == [("StackSpec", (b, d, d, h, w))] and calls == [(b, d, d, h, w)]
    tag = "dap" if dap else "nodap"
    assert set(got) == set(want) == {k[len(tag) + 6:] for k in g if k.startswith(tag + ".grad.")}
    for k in want:
        if name == cases.NAN_FIXTURE:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
            assert np.array_equal(np.isnan(got[k]), np.isnan(g[f"{tag}.grad.{k}"])), k
            continue
        assert cases.max_norm_err(got[k], want[k]) <= 1e-5, k
        assert cases.max_norm_err(got[k], g[f"{tag}.grad.{k}"]) <= 1e-5, k


def test_backward_operator_on_cpu_and_needs_grad():
    import rmd  # noqa: F401
    c = cases.sweep_case(fwd.SWEEP[1])
    f1, f2, co, r, weights, biases = c["args"]
    a = (_t(c["grad"]), _t(f1), _t(f2), _t(co), r, [_t(w) for w in weights], [_t(t) for t in biases])
    full = torch.ops.rmd.dicl_match_1x1_backward(*a, [True, True, True])
    for k, got in zip(cases.OUTPUTS, full):
        assert cases.max_norm_err(got.numpy().reshape(c["ref"][k].shape), c["ref"][k]) <= 1e-5, k
    part = torch.ops.rmd.dicl_match_1x1_backward(*a, [False, True, False])
    assert [t.numel() for t in part] == [0, full[1].numel()] + [0] * 8 and torch.equal(part[1], full[1])
    out = torch.ops.rmd.dicl_match_1x1_train(*a[1:])
    assert torch.equal(out, torch.ops.rmd.dicl_match_1x1(*a[1:], 3))


@pytest.mark.parametrize("name", cases.FIXTURES[:2])
def test_module_routing_with_fused_backward(name):
    g = cases.fixture(name)
    f1, f2, co = _t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"])
    assert cases.build_module(name).fused_backward is False              # the default: nothing changes
    default_auto, default_on = cases.build_module(name, fused="auto"), cases.build_module(name, fused="on")
    auto, on = (cases.build_module(name, fused=f, fused_backward=True) for f in ("auto", "on"))
    on_bf16 = cases.build_module(name, fused="on", fused_backward=True, precision="bf16")
    auto_bf16 = cases.build_module(name, fused="auto", fused_backward=True, precision="bf16")
    seen = []
    for m in (default_auto, default_on, auto, on, on_bf16, auto_bf16):
        m.mnet.register_forward_hook(lambda mod, i, o: seen.append(type(i[0]).__name__))
    # the default reproduces today's fallback and error text
    out = default_auto(f1, f2, co)
    assert seen == ["Tensor"] and out.requires_grad
    with pytest.raises(RuntimeError, match=r"fused='on'\): a gradient is needed \(the fused operator is not differentiable\)"):
        default_on(f1, f2, co)
    # opt-in: a needed gradient is no fallback reason any more
    for m in (auto, on):
        seen.clear()
        out = m(f1, f2, co)
        assert seen == ["StackSpec"] and out.requires_grad
        assert torch.allclose(out, default_auto(f1, f2, co), rtol=0, atol=1e-5 * float(out.detach().abs().max()))
    # the one-product mode has no backward: auto falls back, on raises, and says which condition failed
    seen.clear()
    assert auto_bf16(f1, f2, co).requires_grad and seen == ["Tensor"]
    with pytest.raises(RuntimeError, match="one-product mode has no backward"):
        on_bf16(f1, f2, co)
    with torch.no_grad():                                                  # no gradient needed: as before
        seen.clear()
        on_bf16(f1, f2, co)
        on(f1, f2, co)
        assert seen == ["StackSpec", "StackSpec"]
    if str(fwd.fixture(cases.FORWARD_FIXTURE[name])["norm_type"]) == "batch":      # not foldable: train-mode batch norm
        on.train()
        with pytest.raises(RuntimeError, match="per-call statistics"):
            on(f1, f2, co)
        on.eval()
        for p in on.mnet.parameters():                                     # frozen parameters, a feature gradient
            p.requires_grad_(False)
        seen.clear()
        x = f1.clone().requires_grad_(True)
        on(x, f2, co).sum().backward()
        assert seen == ["StackSpec"] and x.grad is not None and on.mnet[0][0].weight.grad is None


@pytest.mark.parametrize("name", cases.FIXTURES[:2])
def test_state_dict_keys_unchanged(name):
    g = fwd.fixture(cases.FORWARD_FIXTURE[name])
    mod = cases.build_module(name, fused="on", fused_backward=True)
    assert sorted(mod.state_dict().keys()) == sorted(g["sd.keys"].tolist())
    assert mod.output_dim == (2 * int(g["radius"]) + 1) ** 2 and "delta" in dict(mod.named_buffers())


def test_operator_table_schema_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from rmd import library
    assert library.match_train_operators() == ["dicl_match_1x1_backward", "dicl_match_1x1_train"]
    assert library.match_operators() == ["dicl_match_1x1"]
    others = (library.operators() + library.loss_operators() + library.metric_operators() + library.head_operators()
              + library.attn_operators() + library.match_operators())
    assert not set(library.match_train_operators()) & set(others)
    assert str(torch.ops.rmd.dicl_match_1x1_train.default._schema) == (
        "rmd::dicl_match_1x1_train(Tensor fmap1, Tensor fmap2, Tensor coords, int radius, Tensor[] weights, "
        "Tensor[] biases) -> Tensor")
    assert str(torch.ops.rmd.dicl_match_1x1_backward.default._schema) == (
        "rmd::dicl_match_1x1_backward(Tensor grad, Tensor fmap1, Tensor fmap2, Tensor coords, int radius, "
        "Tensor[] weights, Tensor[] biases, bool[] needs_grad) -> Tensor[]")
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for op in library.match_train_operators():
        for key in ("CUDA", "CPU", "Meta", "AutogradCPU"):
            assert has(f"rmd::{op}", key), (op, key)
    assert has("rmd::dicl_match_1x1_train", "Autograd")
    with FakeTensorMode():
        f = torch.empty(2, 32, 12, 16, device="cuda")
        co = torch.empty(2, 2, 12, 16, device="cuda")
        ws = [torch.empty(s, device="cuda") for s in ((96, 64), (128, 96), (64, 128), (64,))]
        ts = [torch.empty(s, device="cuda") for s in (96, 128, 64, 1)]
        out = torch.ops.rmd.dicl_match_1x1_train(f, f, co, 4, ws, ts)
        assert out.shape == (2, 9, 9, 12, 16) and out.dtype == torch.float32 and out.device.type == "cuda"
        grads = torch.ops.rmd.dicl_match_1x1_backward(out, f, f, co, 4, ws, ts, [True, False, True])
        assert [tuple(t.shape) for t in grads] == [(2, 32, 12, 16), (0,), (96, 64), (128, 96), (64, 128), (64,), (96,),
                                                   (128,), (64,), (1,)]
        with pytest.raises(ValueError, match="grad must be"):
            torch.ops.rmd.dicl_match_1x1_backward(out[:, :8], f, f, co, 4, ws, ts, [True, True, True])
        with pytest.raises(ValueError, match="needs_grad"):
            torch.ops.rmd.dicl_match_1x1_backward(out, f, f, co, 4, ws, ts, [True])
        with pytest.raises(ValueError, match="weights\\[1\\]"):
            torch.ops.rmd.dicl_match_1x1_train(f, f, co, 4, [ws[0], ws[2], ws[2], ws[3]], ts)
    c = fwd.sweep_case(fwd.SWEEP[0])
    x = torch.randn(1, 16, 3, 4, requires_grad=True)
    a = (x, x.detach().clone().requires_grad_(True), torch.zeros(1, 2, 3, 4), 1,
         [_t(w).requires_grad_(True) for w in c["args"][4]], [_t(t).requires_grad_(True) for t in c["args"][5]])
    assert torch.ops.rmd.dicl_match_1x1_train(*a).requires_grad
    torch.library.opcheck(torch.ops.rmd.dicl_match_1x1_train, a,
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_abi_argument_checks_supported_and_workspace():
    """Host-side only: every check fails before a launch, so no GPU is touched."""
    from rmd import _lib
    L = _lib.lib()
    sup = L.rmd_dicl_match_1x1_backward_supported
    assert sup(32, 96, 128, 64, 4) == 1 and sup(16, 32, 32, 32, 1) == 1 and sup(64, 128, 128, 128, 3) == 1
    for bad in ((24, 96, 128, 64, 4), (80, 96, 128, 64, 4), (32, 48, 128, 64, 4), (32, 96, 160, 64, 4),
                (32, 96, 128, 64, 0), (32, 96, 128, 64, 5)):
        assert sup(*bad) == 0 and L.rmd_dicl_match_1x1_supported(*bad) == 0, bad
    ws = L.rmd_dicl_match_1x1_backward_workspace_bytes
    nfrag = 3 * 4 + 4 * 6 + 2 * 8
    nw, nv = 96 * 64 + 128 * 96 + 64 * 128, 2 * 64 + 96 + 128 + 1
    small = ws(1, 32, 4, 8, 4, 96, 128, 64)           # one strip: one workgroup's partials
    assert 4 * nfrag * 1024 + 4 * (nw + 4 * nv) <= small <= 4 * nfrag * 1024 + 4 * (nw + 4 * nv) + 3 * 256
    big = ws(6, 32, 48, 64, 4, 96, 128, 64)           # the training shape: one partial per CU, far below the stack
    assert small < big <= 4 * nfrag * 1024 + 256 * 4 * (nw + 4 * nv) + 3 * 256 < 6 * 81 * 64 * 48 * 64 * 4 // 8
    assert ws(1, 24, 4, 8, 4, 96, 128, 64) == 0 and ws(0, 32, 4, 8, 4, 96, 128, 64) == 0 and ws(1, 32, 4, 8, 5, 96, 128, 64) == 0
    p = ctypes.c_void_p(256)       # never dereferenced: each call below is refused before any launch

    def call(ptr=p, b=1, c=32, h=4, w=4, r=4, widths=(96, 128, 64), compute=_lib.RMD_BF16X3, pg=(p,) * 8, work=p):
        return L.rmd_dicl_match_1x1_backward(ptr, p, p, p, b, c, h, w, r, p, p, p, p, p, p, p, *widths, compute, p, p,
                                             *pg, work, None)

    assert call(ptr=None) == -1 and b"null" in L.rmd_last_error()
    assert call(work=None) == -1
    assert call(compute=_lib.RMD_BF16) == -1 and b"RMD_BF16X3" in L.rmd_last_error()
    assert call(compute=_lib.RMD_F32) == -1
    assert call(pg=(p,) * 5 + (None,) + (p,) * 2) == -1 and b"all given or all NULL" in L.rmd_last_error()
    assert call(b=0) == -2 and call(h=0) == -2
    assert call(c=24) == -2 and b"unsupported" in L.rmd_last_error()
    assert call(widths=(48, 128, 64)) == -2 and call(r=5) == -2 and call(r=0) == -2
    assert call(c=64, h=1 << 12, w=1 << 12) == -2 and b"pixels" in L.rmd_last_error()
