"""The fused SepConvGRU without a GPU: the tests' float64 restatement against the reference's fixtures, the
CPU operator and the drop-in modules (fused "off" / "auto" / "on" on CPU tensors) against the fixtures, state-dict
keys, routing, the operator table, schema and fake shapes, the supported widths, the workspace bound, the ABI's
argument checks and the forward hook on the update block.

The fixtures are the reference's fp32 results; its composition is 3.0e-7 (max-normalised) from float64 on
them, so the restatement is held to 1e-5 and the CPU paths, which run the same ATen composition, to 1e-6."""

import ctypes

import numpy as np
import pytest
import torch

import gru_cases as cases

REFERENCE_FP32 = 1e-6


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _gru(name, **kwargs):
    import rmd.raft
    from detinit import det_init_fanin
    g = cases.fixture(name)
    return det_init_fanin(rmd.raft.SepConvGru(g["h"].shape[1], g["x"].shape[1], **kwargs)).eval()


def _block(**kwargs):
    import rmd.raft
    from detinit import det_init_fanin
    return det_init_fanin(rmd.raft.BasicUpdateBlock(324, **kwargs)).eval()


def test_restatement_matches_the_fixtures():
    for name in (cases.FIXTURE,) + cases.NAN_FIXTURES:
        g = cases.fixture(name)
        ws, bs = cases.fixture_params(g["h"].shape[1], g["x"].shape[1])
        err = cases.max_norm_err(g["out"], cases.gru64(g["h"], g["x"], ws, bs))
        print(f"{name}: reference fp32 vs float64 {err:.3e}")
        assert err <= 1e-5, (name, err)
    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = _block()
    with torch.no_grad():
        x = torch.cat((_t(g["x"]), blk.enc(_t(g["flow"]), _t(g["corr"]))), dim=1).numpy()
    ws, bs = cases.module_params(blk.gru)
    err = cases.max_norm_err(g["h_out"], cases.gru64(g["h"], x, ws, bs))
    assert err <= 1e-5, err


def test_emulation_errors_are_what_the_modes_promise():
    """The gate's e on shape 1: the split mode holds fp32 accuracy, the one-product mode bf16's."""
    c = cases.shape_case(cases.SHAPES[0])
    print("e:", c["e"])
    assert c["e"]["fp32"] < 1e-4 and 1e-4 < c["e"]["bf16"] < 5e-2


def test_nan_fixtures_poison_the_receptive_field_only():
    ws, bs = cases.fixture_params(32, 16)
    for name in cases.NAN_FIXTURES:
        g = cases.fixture(name)
        nan = np.isnan(g["out"])
        assert np.array_equal(nan, np.broadcast_to(cases.nan_squares(g), nan.shape))     # every channel, +-4 each way
        for products in (None, 3, 1):
            assert np.array_equal(np.isnan(cases.gru64(g["h"], g["x"], ws, bs, products)), nan)
    assert np.isnan(cases.fixture(cases.NAN_FIXTURES[0])["out"]).all()
    assert not np.isnan(cases.fixture(cases.NAN_FIXTURES[1])["out"]).all()


@pytest.mark.parametrize("fused", ["off", "auto", "on"])
def test_modules_on_cpu_match_the_fixtures(fused):
    for name in (cases.FIXTURE,) + cases.NAN_FIXTURES:
        g = cases.fixture(name)
        mod = _gru(name, fused=fused)
        with torch.no_grad():
            out = mod(_t(g["h"]), _t(g["x"]))
        assert cases.max_norm_err(out.numpy(), g["out"]) <= REFERENCE_FP32
        if fused == "off":
            assert np.array_equal(out.numpy(), g["out"], equal_nan=True)        # the reference's lines: bitwise
        assert sorted(mod.state_dict().keys()) == sorted(g["keys"].tolist())
    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = _block(gru_fused=fused)
    with torch.no_grad():
        h_out, d = blk(_t(g["h"]), _t(g["x"]), _t(g["corr"]), _t(g["flow"]))
    assert cases.max_norm_err(h_out.numpy(), g["h_out"]) <= REFERENCE_FP32
    assert cases.max_norm_err(d.numpy(), g["d"]) <= REFERENCE_FP32
    assert sorted(blk.state_dict().keys()) == sorted(g["keys"].tolist())


def test_cpu_operator_matches_the_fixture_and_ignores_compute():
    from rmd import _lib, ops
    g = cases.fixture(cases.FIXTURE)
    ws, bs = cases.fixture_params(128, 256)
    args = (_t(g["h"]), _t(g["x"]), [_t(w) for w in ws], [_t(b) for b in bs])
    a = torch.ops.rmd.sepconv_gru(*args, _lib.RMD_BF16X3)
    b = ops.sepconv_gru(*args, precision="bf16")
    assert torch.equal(a, b) and cases.max_norm_err(a.numpy(), g["out"]) <= REFERENCE_FP32
    with pytest.raises(ValueError, match="precision"):
        ops.sepconv_gru(*args, precision="fp16")


def test_routing_falls_back_or_raises_with_the_reason(monkeypatch):
    from rmd import ops
    g = cases.fixture(cases.NAN_FIXTURES[1])
    h, x = _t(g["h"]), _t(g["x"])
    calls = []
    real = ops.sepconv_gru
    monkeypatch.setattr(ops, "sepconv_gru", lambda *a, **k: calls.append(1) or real(*a, **k))
    auto, on = _gru(cases.NAN_FIXTURES[1], fused="auto"), _gru(cases.NAN_FIXTURES[1], fused="on")

    with torch.no_grad():
        auto(h, x)
    assert len(calls) == 1                              # grad mode off: the operator
    for p in auto.parameters():
        p.requires_grad_(False)
    auto(h, x)
    assert len(calls) == 2                              # nothing requires grad: the operator
    out = auto(h.clone().requires_grad_(True), x)
    assert len(calls) == 2 and out.requires_grad        # a gradient: the composition, which trains
    with pytest.raises(RuntimeError, match="gradient"):
        on(h, x)                                        # its parameters require grad
    with torch.no_grad():
        with torch.autocast("cpu", dtype=torch.bfloat16):
            auto(h, x)
            assert len(calls) == 2
            with pytest.raises(RuntimeError, match="autocast"):
                on(h, x)
        with pytest.raises(RuntimeError, match="float32"):
            on(h.half(), x.half())
    with pytest.raises(ValueError, match="fused"):
        _gru(cases.NAN_FIXTURES[1], fused="yes")
    with pytest.raises(ValueError, match="precision"):
        _gru(cases.NAN_FIXTURES[1], precision="fp16")


def test_unsupported_widths_are_a_named_reason():
    """The width check is the GPU kernel's: ask it the way the module does, without a GPU."""
    import rmd.raft
    from rmd import library
    mod = rmd.raft.SepConvGru(24, 16, fused="on")
    assert not library.gru_supported(24, 16) and library.gru_supported(128, 256)

    class OnGpu:
        """h / x stand-ins that claim to be fp32 GPU tensors of the module's widths."""
        def __init__(self, c):
            self.shape, self.dtype, self.is_cuda, self.requires_grad = (1, c, 4, 4), torch.float32, True, False
            self.device = next(mod.parameters()).device

        def dim(self):
            return 4

    with torch.no_grad():
        assert "unsupported widths" in mod.fallback_reason(OnGpu(24), OnGpu(16))


def test_operator_table_schema_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from rmd import _lib, library
    assert library.update_operators() == ["sepconv_gru"]
    assert "sepconv_gru" not in library.operators()
    assert library.match_operators() == ["dicl_match_1x1"]
    assert library.match_train_operators() == ["dicl_match_1x1_backward", "dicl_match_1x1_train"]
    assert library.attn_operators() == ["local_cross_attn", "local_cross_attn_backward"]
    assert library.head_operators() == ["dicl_flow_head", "dicl_flow_head_backward"]
    assert library.loss_operators() == ["sequence_loss", "sequence_loss_backward"]
    assert library.metric_operators() == ["flow_metrics"]
    schema = str(torch.ops.rmd.sepconv_gru.default._schema)
    assert schema == "rmd::sepconv_gru(Tensor h, Tensor x, Tensor[] weights, Tensor[] biases, int compute) -> Tensor"
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for key in ("CUDA", "CPU", "Meta", "Autograd"):
        assert has("rmd::sepconv_gru", key), key
    with FakeTensorMode():
        h, x = torch.empty(2, 128, 12, 16, device="cuda"), torch.empty(2, 256, 12, 16, device="cuda")
        ws = [torch.empty((128, 384, 1, 5) if i < 3 else (128, 384, 5, 1), device="cuda") for i in range(6)]
        bs = [torch.empty(128, device="cuda") for _ in range(6)]
        out = torch.ops.rmd.sepconv_gru(h, x, ws, bs, _lib.RMD_BF16X3)
        assert out.shape == (2, 128, 12, 16) and out.dtype == torch.float32 and out.device.type == "cuda"
        with pytest.raises(ValueError, match="weights\\[3\\]"):
            torch.ops.rmd.sepconv_gru(h, x, ws[:3] + ws[:3], bs, _lib.RMD_BF16X3)
        with pytest.raises(ValueError, match="compute"):
            torch.ops.rmd.sepconv_gru(h, x, ws, bs, _lib.RMD_F32)
        with pytest.raises(ValueError, match="6 weights"):
            torch.ops.rmd.sepconv_gru(h, x, ws[:5], bs, _lib.RMD_BF16)
        with pytest.raises(ValueError, match="expected"):
            torch.ops.rmd.sepconv_gru(h, x[:, :, :-1], ws, bs, _lib.RMD_BF16)
    h, x, ws, bs = cases.shape_case(cases.SHAPES[2])["args"]
    args = (_t(h), _t(x), [_t(w) for w in ws], [_t(b) for b in bs])
    out = torch.ops.rmd.sepconv_gru(args[0].clone().requires_grad_(True), *args[1:], _lib.RMD_BF16X3)
    assert not out.requires_grad                         # not differentiable: the result carries no graph
    torch.library.opcheck(torch.ops.rmd.sepconv_gru, args + (_lib.RMD_BF16,),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_abi_supported_workspace_and_argument_checks():
    """Host-side only: every check fails before a launch, so no GPU is touched."""
    from rmd import _lib
    L = _lib.lib()
    sup = L.rmd_sepconv_gru_supported
    for hd in range(0, 200, 8):
        for xd in range(0, 560, 8):
            want = hd % 32 == 0 and 32 <= hd <= 128 and xd % 16 == 0 and xd >= 16 and hd + xd <= 512
            assert sup(hd, xd) == int(want), (hd, xd)
    ws = L.rmd_sepconv_gru_workspace_bytes
    for b, hd, xd, h, w in cases.SHAPES + [(8, 128, 256, 55, 128)]:
        bound = 6 * hd * 5 * (hd + xd) * 2 * 2 + 3 * b * hd * h * w * 4
        assert bound <= ws(b, hd, xd, h, w) <= bound + 4096, (b, hd, xd, h, w)
    assert ws(1, 24, 16, 4, 4) == 0 and ws(0, 32, 16, 4, 4) == 0 and ws(1, 32, 16, 0, 4) == 0

    p = ctypes.c_void_p(1 << 20)       # never dereferenced: each call below is refused before any launch
    six = (ctypes.c_void_p * 6)(*([1 << 30] * 6))

    def call(h=p, x=ctypes.c_void_p(1 << 24), weights=six, biases=six, out=ctypes.c_void_p(1 << 26),
             work=ctypes.c_void_p(1 << 28), b=1, hd=32, xd=16, ht=4, wd=4, compute=_lib.RMD_BF16X3, axis=None):
        if axis is None:
            return L.rmd_sepconv_gru(h, x, weights, biases, out, work, b, hd, xd, ht, wd, compute, None)
        return L.rmd_sepconv_gru_half(h, x, weights, biases, out, work, b, hd, xd, ht, wd, axis, compute, None)

    assert call(h=None) == -1 and b"null" in L.rmd_last_error()
    assert call(out=None) == -1 and call(work=None) == -1 and call(weights=None) == -1
    holes = (ctypes.c_void_p * 6)(1 << 30, 1 << 30, 1 << 30, 1 << 30, None, 1 << 30)
    assert call(biases=holes) == -1 and b"null" in L.rmd_last_error()
    assert call(compute=_lib.RMD_F32) == -1 and b"compute" in L.rmd_last_error()
    assert call(axis=2) == -1 and b"axis" in L.rmd_last_error()
    assert call(b=0) == -2 and call(ht=0) == -2 and call(wd=0) == -2
    assert call(hd=24) == -2 and b"unsupported" in L.rmd_last_error()
    assert call(hd=160) == -2 and call(xd=8) == -2 and call(hd=128, xd=400) == -2
    assert call(hd=128, xd=384, ht=1 << 11, wd=1 << 10) == -2 and b"pixels" in L.rmd_last_error()
    assert call(out=p) == -1 and b"overlaps" in L.rmd_last_error()                     # out is h
    assert call(out=ctypes.c_void_p((1 << 24) + 64)) == -1 and b"overlaps" in L.rmd_last_error()   # out inside x
    assert call(work=ctypes.c_void_p((1 << 26) - 256)) == -1 and b"workspace" in L.rmd_last_error()


def test_forward_hook_on_the_block_sees_the_lookup():
    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = _block(gru_fused="on")
    seen, gru_calls, conv_calls = [], [], []
    blk.register_forward_hook(lambda m, inputs, output: seen.append(inputs[2]))
    blk.gru.register_forward_hook(lambda m, inputs, output: gru_calls.append(1))
    blk.gru.convz1.register_forward_hook(lambda m, inputs, output: conv_calls.append(1))
    corr = _t(g["corr"])
    with torch.no_grad():
        blk(_t(g["h"]), _t(g["x"]), corr, _t(g["flow"]))
    assert len(seen) == 1 and seen[0] is corr and gru_calls == [1]
    assert conv_calls == []                              # the inner convolutions are not called on the fused path
