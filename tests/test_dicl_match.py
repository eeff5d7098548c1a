"""Fused dicl-1x1 cost without a GPU: the tests' float64 restatement against the reference's fixtures, the
operator's CPU kernel, MatchingNet1x1.folded() / foldable(), the module's routing, the operator table and
the C ABI's argument checks (dicl_match_cases.py states the restatement and the tolerance rule)."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dicl_match_cases as cases
from conftest import rel_max_err


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_restatement_matches_the_reference_fixture(name):
    """float64 restatement (folded parameters) vs the reference module's mnet output: 1e-5 max-normalised
    (the reference's own fp32 composite sits about 4e-7 from float64 on such data)."""
    g, c = cases.fixture(name), cases.fixture_case(name)
    for tag in ("dap", "nodap"):
        err = cases.max_norm_err(g[f"{tag}.cost"], c["ref"])
        print(f"{name} {tag}: reference fp32 cost vs float64 restatement {err:.2e}; emulation e {c['e']}")
        assert err <= 1e-5


def test_nan_positions_are_the_poisoned_pixels_only():
    g, c = cases.fixture(cases.NAN_FIXTURE), cases.fixture_case(cases.NAN_FIXTURE)
    want = np.zeros(c["ref"].shape, dtype=bool)
    for b, y, x in cases.NAN_PIXELS:
        want[b, :, :, y, x] = True
    d = 2 * int(g["radius"]) + 1
    assert want.sum() == len(cases.NAN_PIXELS) * d * d
    assert np.array_equal(np.isnan(c["ref"]), want)
    assert np.array_equal(np.isnan(g["nodap.cost"]), want)
    for products in (1, 3):
        assert np.array_equal(np.isnan(cases.emulate(*c["args"], products)), want)


def test_emulation_errors_are_of_the_expected_size():
    """The tolerance rule's input, printed for the record: three products stay near fp32, one near bf16."""
    for label, get in cases.all_cases():
        c = get()
        print(f"{label}: e fp32 {c['e']['fp32']:.2e} bf16 {c['e']['bf16']:.2e}")
        assert c["e"]["fp32"] < 1e-4 and c["e"]["bf16"] < 5e-2
        assert c["tol"]["fp32"] == max(1e-5, 3 * c["e"]["fp32"])


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_cpu_operator_equals_the_module_path(name):
    """torch.ops.rmd.dicl_match_1x1 on CPU tensors vs today's module path (stack, convolutions, norms)."""
    from rmd import ops
    g = cases.fixture(name)
    mod = cases.build_module(name)
    cap = {}
    mod.mnet.register_forward_hook(lambda m, i, o: cap.update(cost=o))
    with torch.no_grad():
        mod(_t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"]), dap=False)
        weights, biases = mod.mnet.folded()
        for precision in ("fp32", "bf16"):          # the CPU kernel is fp32 whatever the mode
            got = ops.dicl_match_1x1(_t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"]), int(g["radius"]), weights, biases,
                                     precision=precision)
            assert got.shape == cap["cost"].shape and got.dtype == torch.float32
            assert rel_max_err(got.numpy(), cap["cost"].numpy()) <= 1e-6
    assert rel_max_err(cap["cost"].numpy(), g["nodap.cost"]) <= 1e-6


@pytest.mark.parametrize("norm", ["batch", "none"])
def test_folded_against_explicit_conv_norm_relu(norm):
    from rmd.blocks.dicl import MatchingNet1x1
    from detinit import det_init
    torch.manual_seed(3)
    net = det_init(MatchingNet1x1(32, norm_type=norm, scale=0.5)).eval()
    if norm == "batch":
        with torch.no_grad():
            for block in list(net)[:3]:
                block[1].running_var.uniform_(0.5, 2.0)
                block[1].running_mean.normal_(0.0, 0.3)
    assert net.foldable()
    x = torch.randn(5, 32, 3, 4)
    with torch.no_grad():
        weights, biases = net.folded()
        assert [tuple(w.shape) for w in weights] == [(48, 32), (64, 48), (32, 64), (32,)]
        assert [tuple(t.shape) for t in biases] == [(48,), (64,), (32,), (1,)]
        y = x
        for block, w, t in zip(list(net)[:3], weights, biases):
            want = block[2](block[1](block[0](y)))
            got = F.relu(F.conv2d(y, w[:, :, None, None], t))
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
            y = want
        assert torch.allclose(F.conv2d(y, weights[3].reshape(1, -1, 1, 1), biases[3]), net[3](y), rtol=1e-5, atol=1e-6)
    affine_less = MatchingNet1x1(8)
    for block in list(affine_less)[:3]:
        block[1] = torch.nn.BatchNorm2d(block[0].out_channels, affine=False)
    affine_less.eval()
    w0, t0 = affine_less.folded()[0][0], affine_less.folded()[1][0]
    bn = affine_less[0][1]
    s = torch.rsqrt(bn.running_var + bn.eps)
    assert torch.equal(w0, s[:, None] * affine_less[0][0].weight[:, :, 0, 0]) and torch.equal(t0, -bn.running_mean * s)


def test_foldable_is_false_where_statistics_are_per_call():
    from rmd.blocks.dicl import MatchingNet, MatchingNet1x1
    assert not any(hasattr(MatchingNet, n) for n in ("foldable", "folded"))     # the 3x3 network has no fused path
    assert not MatchingNet1x1(32, norm_type="batch").train().foldable()
    assert MatchingNet1x1(32, norm_type="batch").eval().foldable()
    assert MatchingNet1x1(32, norm_type="none").train().foldable()
    for norm in ("group", "instance"):
        net = MatchingNet1x1(32, norm_type=norm).eval()
        assert not net.foldable()
        with pytest.raises(RuntimeError, match="cannot be folded"):
            net.folded()


def _today(mod, f1, f2, co, dap):
    """The module's forward as it was before the fused path existed."""
    from rmd import ops
    cost = mod.mnet(ops.dicl_stack(f1, f2, co, mod.radius))
    if dap:
        cost = mod.dap(cost)
    return cost.reshape(f1.shape[0], -1, *f1.shape[-2:])


@pytest.mark.parametrize("name", cases.FIXTURES[:2])
def test_module_routing(name):
    g = cases.fixture(name)
    f1, f2, co = _t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"])
    off, auto, on = (cases.build_module(name, fused=f) for f in ("off", "auto", "on"))
    assert cases.build_module(name).fused == "off"                       # the default
    with pytest.raises(ValueError, match="fused"):
        cases.build_module(name, fused="yes")
    with pytest.raises(ValueError, match="precision"):
        cases.build_module(name, precision="fp16")
    seen = []
    for m in (off, auto, on):
        m.mnet.register_forward_hook(lambda mod, i, o: seen.append((type(i[0]).__name__, tuple(o.shape))))
    with torch.no_grad():
        for dap in (True, False):
            want = _today(off, f1, f2, co, dap)
            seen.clear()
            assert torch.equal(off(f1, f2, co, dap=dap), want)           # off: bitwise today's output
            assert [s[0] for s in seen] == ["Tensor"]
            for m in (auto, on):
                seen.clear()
                got = m(f1, f2, co, dap=dap)
                d = 2 * m.radius + 1
                assert seen == [("StackSpec", (f1.shape[0], d, d) + tuple(f1.shape[-2:]))]   # hook: once, the cost
                assert rel_max_err(got.numpy(), g["dap.out" if dap else "nodap.out"]) <= 1e-6
    # a gradient is needed (the parameters require it and grad mode is on): auto falls back, on raises
    seen.clear()
    out = auto(f1, f2, co)
    assert [s[0] for s in seen] == ["Tensor"] and out.requires_grad
    assert torch.equal(out.detach(), _today(off, f1, f2, co, True).detach())
    with pytest.raises(RuntimeError, match="gradient is needed"):
        on(f1, f2, co)
    for p in auto.parameters():
        p.requires_grad_(False)
    seen.clear()
    auto(f1.clone().requires_grad_(True), f2, co)                         # an input requires it
    assert [s[0] for s in seen] == ["Tensor"]
    seen.clear()
    auto(f1, f2, co)                                                      # nothing requires it: fused
    assert [s[0] for s in seen] == ["StackSpec"]
    # not foldable: train-mode batch norm
    if str(g["norm_type"]) == "batch":
        on.train()
        with torch.no_grad(), pytest.raises(RuntimeError, match="per-call statistics"):
            on(f1, f2, co)


@pytest.mark.parametrize("name", cases.FIXTURES[:2])
def test_state_dict_keys_unchanged(name):
    g = cases.fixture(name)
    for fused in ("off", "auto", "on"):
        mod = cases.build_module(name, fused=fused)
        assert sorted(mod.state_dict().keys()) == sorted(g["sd.keys"].tolist())
        assert mod.output_dim == (2 * int(g["radius"]) + 1) ** 2 and "delta" in dict(mod.named_buffers())


def test_operator_table_schema_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from rmd import _lib, library
    assert library.match_operators() == ["dicl_match_1x1"]
    assert "dicl_match_1x1" not in library.operators()
    schema = str(torch.ops.rmd.dicl_match_1x1.default._schema)
    assert schema == ("rmd::dicl_match_1x1(Tensor fmap1, Tensor fmap2, Tensor coords, int radius, Tensor[] weights, "
                      "Tensor[] biases, int compute) -> Tensor")
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for key in ("CUDA", "CPU", "Meta", "Autograd"):
        assert has("rmd::dicl_match_1x1", key), key
    with FakeTensorMode():
        f = torch.empty(2, 32, 12, 16, device="cuda")
        co = torch.empty(2, 2, 12, 16, device="cuda")
        ws = [torch.empty(s, device="cuda") for s in ((96, 64), (128, 96), (64, 128), (64,))]
        ts = [torch.empty(s, device="cuda") for s in (96, 128, 64, 1)]
        out = torch.ops.rmd.dicl_match_1x1(f, f, co, 4, ws, ts, _lib.RMD_BF16X3)
        assert out.shape == (2, 9, 9, 12, 16) and out.dtype == torch.float32 and out.device.type == "cuda"
        with pytest.raises(ValueError, match="weights\\[1\\]"):
            torch.ops.rmd.dicl_match_1x1(f, f, co, 4, [ws[0], ws[2], ws[2], ws[3]], ts, _lib.RMD_BF16X3)
        with pytest.raises(ValueError, match="compute"):
            torch.ops.rmd.dicl_match_1x1(f, f, co, 4, ws, ts, _lib.RMD_F32)
        with pytest.raises(ValueError, match="coords"):
            torch.ops.rmd.dicl_match_1x1(f, f, co[:, :1], 4, ws, ts, _lib.RMD_BF16)
    x = torch.randn(1, 16, 3, 4, requires_grad=True)       # not differentiable: the result carries no graph
    c = cases.sweep_case(cases.SWEEP[0])
    out = torch.ops.rmd.dicl_match_1x1(x, x, torch.zeros(1, 2, 3, 4), 1, [_t(w) for w in c["args"][4]],
                                       [_t(t) for t in c["args"][5]], _lib.RMD_BF16X3)
    assert not out.requires_grad
    torch.library.opcheck(torch.ops.rmd.dicl_match_1x1,
                          (x.detach(), x.detach(), torch.zeros(1, 2, 3, 4), 1, [_t(w) for w in c["args"][4]],
                           [_t(t) for t in c["args"][5]], _lib.RMD_BF16),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_wrapper_pads_hidden_widths():
    from rmd import ops
    c = cases.sweep_case(cases.SWEEP[4])
    weights, biases = [_t(w) for w in c["args"][4]], [_t(t) for t in c["args"][5]]
    assert ops.match_padded_widths(weights) == (64, 64, 32)
    pw, pt = ops._pad_match(weights, biases)
    assert [tuple(w.shape) for w in pw] == [(64, 64), (64, 64), (32, 64), (32,)] and [t.numel() for t in pt] == [64, 64, 32, 1]
    assert torch.equal(pw[0][:48], weights[0]) and not pw[0][48:].any() and not pw[1][:, 48:].any() and not pt[0][48:].any()
    padded = cases.reference64(*c["args"][:4], [w.numpy() for w in pw], [t.numpy() for t in pt])
    assert np.array_equal(padded, c["ref"])                 # zero rows and columns change nothing
    with pytest.raises(ValueError, match="precision"):
        ops.dicl_match_1x1(*[_t(a) for a in c["args"][:3]], 4, weights, biases, precision="fp16")


def test_abi_argument_checks_and_supported():
    """Host-side only: every check fails before a launch, so no GPU is touched."""
    from rmd import _lib
    L = _lib.lib()
    sup = L.rmd_dicl_match_1x1_supported
    assert sup(32, 96, 128, 64, 4) == 1 and sup(16, 32, 32, 32, 1) == 1 and sup(64, 128, 128, 128, 3) == 1
    assert sup(48, 64, 96, 32, 1) == 1
    for bad in ((24, 96, 128, 64, 4), (80, 96, 128, 64, 4), (0, 96, 128, 64, 4),        # channels
                (32, 48, 128, 64, 4), (32, 96, 160, 64, 4), (32, 96, 128, 0, 4),        # widths
                (32, 96, 128, 64, 0), (32, 96, 128, 64, 5)):                            # radius
        assert sup(*bad) == 0, bad
    ws = L.rmd_dicl_match_1x1_workspace_bytes
    nfrag = 3 * 4 + 4 * 6 + 2 * 8
    assert ws(32, 96, 128, 64, _lib.RMD_BF16) == nfrag * 1024 and ws(32, 96, 128, 64, _lib.RMD_BF16X3) == 2 * nfrag * 1024
    assert ws(32, 96, 128, 64, _lib.RMD_F32) == 0 and ws(24, 96, 128, 64, _lib.RMD_BF16) == 0
    p = ctypes.c_void_p(256)       # never dereferenced: each call below is refused before any launch

    def call(ptr=p, b=1, c=32, h=4, w=4, r=4, widths=(96, 128, 64), compute=_lib.RMD_BF16X3, out=p):
        return L.rmd_dicl_match_1x1(ptr, p, p, b, c, h, w, r, p, p, p, p, p, p, p, p, *widths, compute, out, p, None)

    assert call(ptr=None) == -1 and b"null" in L.rmd_last_error()
    assert call(out=None) == -1
    assert call(compute=_lib.RMD_F32) == -1 and b"compute" in L.rmd_last_error()
    assert call(b=0) == -2 and call(h=0) == -2
    assert call(c=24) == -2 and b"unsupported" in L.rmd_last_error()
    assert call(widths=(48, 128, 64)) == -2 and call(r=5) == -2 and call(r=0) == -2
    assert call(c=64, h=1 << 12, w=1 << 12) == -2 and b"pixels" in L.rmd_last_error()      # 32-bit lane offsets
