"""The fused k x k convolutions without a GPU: the CPU operators against the tests' float64 restatement
(conv_cases.py) on the ten shapes, the drop-in modules with fused "off" / "auto" / "on" on CPU tensors against
each other and the reference's fixtures, state-dict keys, routing, the operator table, schemas and fake shapes,
the supported range, the workspace sizes and the ABI's argument checks.

The CPU operators are plain fp32 ATen: 1e-5 max-normalised against float64.  The fixtures are the reference's
fp32 results and the CPU paths run the same ATen composition: 1e-6, as test_gru.py."""

import ctypes

import numpy as np
import pytest
import torch

import conv_cases as cases

REFERENCE_FP32 = 1e-6
CPU_FP32 = 1e-5


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _block(**kwargs):
    import rmd.raft
    from detinit import det_init_fanin
    return det_init_fanin(rmd.raft.BasicUpdateBlock(324, **kwargs)).eval()


def _up8(**kwargs):
    import rmd.raft
    from detinit import det_init_fanin
    g = cases.fixture(cases.UP8_FIXTURE)
    return det_init_fanin(rmd.raft.Up8Network(g["hidden"].shape[1], **kwargs)).eval()


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_cpu_operator_against_float64(shape, act):
    from rmd import ops
    c = cases.shape_case(shape)
    x0, x1, weight, bias = c["args"]
    out = ops.conv2d_act(_t(x0), _t(x1), _t(weight), _t(bias), act=act)
    assert out.shape == c["ref"][act].shape and out.dtype == torch.float32
    err = cases.max_norm_err(out.numpy(), c["ref"][act])
    print(f"{shape} [{act}]: cpu {err:.3e}  e {c['e'][act, 'fp32']:.3e} / {c['e'][act, 'bf16']:.3e}")
    assert err <= CPU_FP32, (shape, act, err)
    assert torch.equal(out, ops.conv2d_act(_t(x0), _t(x1), _t(weight), _t(bias), act=act, precision="bf16"))


def test_emulation_errors_are_what_the_modes_promise():
    c = cases.shape_case(cases.SHAPES[2])
    print("e:", c["e"])
    assert c["e"]["none", "fp32"] < 1e-4 and 1e-4 < c["e"]["none", "bf16"] < 5e-2


def test_cpu_motion_encoder_against_float64_and_the_module():
    from rmd import ops
    g = cases.fixture(cases.BLOCK_FIXTURE)
    ws, bs = cases.encoder_params()
    out = ops.motion_encoder(_t(g["flow"]), _t(g["corr"]), [_t(w) for w in ws], [_t(b) for b in bs])
    assert out.shape == (1, 128, 6, 10)
    assert cases.max_norm_err(out.numpy(), cases.encoder_ref(g["flow"], g["corr"], ws, bs)) <= CPU_FP32
    assert np.array_equal(out.numpy()[:, 126:], g["flow"])
    with torch.no_grad():
        assert cases.max_norm_err(out.numpy(), _block().enc(_t(g["flow"]), _t(g["corr"])).numpy()) <= REFERENCE_FP32


@pytest.mark.parametrize("fused", ["off", "auto", "on"])
def test_modules_on_cpu_match_the_off_modules_and_the_fixtures(fused):
    g = cases.fixture(cases.BLOCK_FIXTURE)
    args = [_t(g[k]) for k in ("h", "x", "corr", "flow")]
    blk = _block(gru_fused=fused, fused=fused)
    assert blk.enc.fused == blk.flow.fused == blk.gru.fused == fused
    with torch.no_grad():
        h_out, d = blk(*args)
        h_off, d_off = _block()(*args)
    assert cases.max_norm_err(h_out.numpy(), g["h_out"]) <= REFERENCE_FP32
    assert cases.max_norm_err(d.numpy(), g["d"]) <= REFERENCE_FP32
    assert cases.max_norm_err(h_out.numpy(), h_off.numpy()) <= REFERENCE_FP32
    assert cases.max_norm_err(d.numpy(), d_off.numpy()) <= REFERENCE_FP32
    if fused == "off":
        assert np.array_equal(h_out.numpy(), g["h_out"]) and np.array_equal(d.numpy(), g["d"])
    assert sorted(blk.state_dict().keys()) == sorted(g["keys"].tolist())

    g = cases.fixture(cases.UP8_FIXTURE)
    up = _up8(fused=fused)
    with torch.no_grad():
        out = up(_t(g["hidden"]), _t(g["flow"]))
        off = _up8()(_t(g["hidden"]), _t(g["flow"]))
    assert cases.max_norm_err(out.numpy(), g["out"]) <= 1e-5       # the fixture's own fp32 softmax
    assert cases.max_norm_err(out.numpy(), off.numpy()) <= REFERENCE_FP32
    assert sorted(up.state_dict().keys()) == sorted(g["keys"].tolist())


def test_defaults_build_the_modules_of_before():
    import rmd.raft
    blk = rmd.raft.BasicUpdateBlock(324)
    assert blk.enc.fused == blk.flow.fused == blk.gru.fused == "off"
    assert blk.enc.precision == blk.flow.precision == "fp32"
    assert [n for n, _ in blk.enc.named_children()] == ["convc1", "convc2", "convf1", "convf2", "conv"]
    assert [n for n, _ in blk.flow.named_children()] == ["conv1", "conv2", "relu"]
    up = rmd.raft.Up8Network(128)
    assert up.fused == "off" and [n for n, _ in up.named_children()] == ["conv1", "relu1", "conv2"]
    only_gru = rmd.raft.BasicUpdateBlock(324, gru_fused="on", gru_precision="bf16")
    assert only_gru.gru.fused == "on" and only_gru.gru.precision == "bf16" and only_gru.enc.fused == "off"
    both = rmd.raft.BasicUpdateBlock(324, fused="auto", precision="bf16")
    assert both.enc.fused == both.flow.fused == "auto" and both.enc.precision == both.flow.precision == "bf16"
    assert both.gru.fused == "off" and both.gru.precision == "fp32"


def test_unknown_modes_raise():
    import rmd.raft
    for make in (lambda **k: rmd.raft.BasicMotionEncoder(324, **k), lambda **k: rmd.raft.FlowHead(**k),
                 lambda **k: rmd.raft.Up8Network(**k), lambda **k: rmd.raft.BasicUpdateBlock(324, **k)):
        with pytest.raises(ValueError, match="fused"):
            make(fused="yes")
        with pytest.raises(ValueError, match="precision"):
            make(precision="fp16")
    from rmd import ops
    x, w, b = torch.zeros(1, 2, 3, 3), torch.zeros(4, 2, 3, 3), torch.zeros(4)
    with pytest.raises(ValueError, match="precision"):
        ops.conv2d_act(x, None, w, b, precision="fp16")
    with pytest.raises(ValueError, match="activation"):
        ops.conv2d_act(x, None, w, b, act="tanh")


def test_routing_falls_back_or_raises_with_the_reason(monkeypatch):
    import rmd.raft
    from rmd import ops
    g = cases.fixture(cases.BLOCK_FIXTURE)
    flow, corr, h = _t(g["flow"]), _t(g["corr"]), _t(g["h"])
    calls = []
    real_enc, real_conv = ops.motion_encoder, ops.conv2d_act
    monkeypatch.setattr(ops, "motion_encoder", lambda *a, **k: calls.append("enc") or real_enc(*a, **k))
    monkeypatch.setattr(ops, "conv2d_act", lambda *a, **k: calls.append("conv") or real_conv(*a, **k))
    auto, on = _block(fused="auto"), _block(fused="on")
    with torch.no_grad():
        auto.enc(flow, corr)
        auto.flow(h)
    assert calls == ["enc", "conv", "conv"]
    out = auto.enc(flow, corr)                          # the parameters require grad: the composition, which trains
    assert len(calls) == 3 and out.requires_grad
    assert auto.flow(h).requires_grad and len(calls) == 3
    with pytest.raises(RuntimeError, match="gradient"):
        on.enc(flow, corr)
    with pytest.raises(RuntimeError, match="gradient"):
        on.flow(h)
    with torch.no_grad():
        with torch.autocast("cpu", dtype=torch.bfloat16):
            auto.enc(flow, corr)
            assert len(calls) == 3
            with pytest.raises(RuntimeError, match="autocast"):
                on.enc(flow, corr)
        with pytest.raises(RuntimeError, match="float32"):
            on.flow(h.double())
        g8 = cases.fixture(cases.UP8_FIXTURE)
        mixed = rmd.raft.Up8Network(32, mixed_precision=True, fused="on")
        with pytest.raises(RuntimeError, match="mixed_precision"):
            mixed(_t(g8["hidden"]), _t(g8["flow"]))
        assert rmd.raft.Up8Network(32, mixed_precision=True, fused="auto").fallback_reason(_t(g8["hidden"]))
        assert _up8(fused="on").fallback_reason(_t(g8["hidden"])) is None


def test_forward_hooks_on_the_modules_fire_and_the_inner_ones_do_not():
    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = _block(gru_fused="on", fused="on")
    outer, inner = [], []
    for m in (blk, blk.enc, blk.flow):
        m.register_forward_hook(lambda m, inputs, output: outer.append(1))
    for m in (blk.enc.convc1, blk.enc.conv, blk.flow.conv1, blk.flow.relu, blk.flow.conv2):
        m.register_forward_hook(lambda m, inputs, output: inner.append(1))
    with torch.no_grad():
        blk(*[_t(g[k]) for k in ("h", "x", "corr", "flow")])
    assert outer == [1, 1, 1] and inner == []


def test_operator_table_schema_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from rmd import _lib, library
    assert library.conv_operators() == ["conv2d_act", "motion_encoder"]
    assert library.update_operators() == ["sepconv_gru"]
    assert not set(library.conv_operators()) & set(library.operators())
    assert str(torch.ops.rmd.conv2d_act.default._schema) == \
        "rmd::conv2d_act(Tensor x0, Tensor? x1, Tensor weight, Tensor bias, int act, int compute) -> Tensor"
    assert str(torch.ops.rmd.motion_encoder.default._schema) == \
        "rmd::motion_encoder(Tensor flow, Tensor corr, Tensor[] weights, Tensor[] biases, int compute) -> Tensor"
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for name in library.conv_operators():
        for key in ("CUDA", "CPU", "Meta", "Autograd"):
            assert has(f"rmd::{name}", key), (name, key)
    X3 = _lib.RMD_BF16X3
    with FakeTensorMode():
        def e(*s):
            return torch.empty(*s, device="cuda")
        out = torch.ops.rmd.conv2d_act(e(2, 192, 12, 16), e(2, 64, 12, 16), e(126, 256, 3, 3), e(126), 1, X3)
        assert out.shape == (2, 126, 12, 16) and out.dtype == torch.float32 and out.device.type == "cuda"
        assert torch.ops.rmd.conv2d_act(e(1, 2, 5, 7), None, e(128, 2, 7, 5), e(128), 0, _lib.RMD_BF16).shape == (1, 128, 5, 7)
        ws = [e(256, 324, 1, 1), e(192, 256, 3, 3), e(128, 2, 7, 7), e(64, 128, 3, 3), e(126, 256, 3, 3)]
        bs = [e(w.shape[0]) for w in ws]
        out = torch.ops.rmd.motion_encoder(e(2, 2, 12, 16), e(2, 324, 12, 16), ws, bs, X3)
        assert out.shape == (2, 128, 12, 16) and out.dtype == torch.float32
        with pytest.raises(ValueError, match="odd"):
            torch.ops.rmd.conv2d_act(e(1, 2, 5, 7), None, e(8, 2, 2, 3), e(8), 0, X3)
        with pytest.raises(ValueError, match="weight must be"):
            torch.ops.rmd.conv2d_act(e(1, 2, 5, 7), e(1, 3, 5, 7), e(8, 2, 3, 3), e(8), 0, X3)
        with pytest.raises(ValueError, match="x1 must be"):
            torch.ops.rmd.conv2d_act(e(1, 2, 5, 7), e(1, 3, 5, 6), e(8, 5, 3, 3), e(8), 0, X3)
        with pytest.raises(ValueError, match="bias"):
            torch.ops.rmd.conv2d_act(e(1, 2, 5, 7), None, e(8, 2, 3, 3), e(7), 0, X3)
        with pytest.raises(ValueError, match="compute"):
            torch.ops.rmd.conv2d_act(e(1, 2, 5, 7), None, e(8, 2, 3, 3), e(8), 0, _lib.RMD_F32)
        with pytest.raises(ValueError, match="act"):
            torch.ops.rmd.conv2d_act(e(1, 2, 5, 7), None, e(8, 2, 3, 3), e(8), 2, X3)
        with pytest.raises(ValueError, match="weights\\[2\\]"):
            torch.ops.rmd.motion_encoder(e(2, 2, 12, 16), e(2, 324, 12, 16), ws[:2] + [ws[3]] + ws[3:], bs, X3)
        with pytest.raises(ValueError, match="5 weights"):
            torch.ops.rmd.motion_encoder(e(2, 2, 12, 16), e(2, 324, 12, 16), ws[:4], bs, X3)
        with pytest.raises(ValueError, match="expected"):
            torch.ops.rmd.motion_encoder(e(2, 3, 12, 16), e(2, 324, 12, 16), ws, bs, X3)
    x0, x1, weight, bias = cases.shape_case(cases.SHAPES[5])["args"]
    args = (_t(x0), _t(x1), _t(weight), _t(bias), 1)
    assert not torch.ops.rmd.conv2d_act(args[0].clone().requires_grad_(True), *args[1:], X3).requires_grad
    torch.library.opcheck(torch.ops.rmd.conv2d_act, args + (_lib.RMD_BF16,),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    g = cases.fixture(cases.BLOCK_FIXTURE)
    ws, bs = cases.encoder_params()
    torch.library.opcheck(torch.ops.rmd.motion_encoder,
                          (_t(g["flow"]), _t(g["corr"]), [_t(w) for w in ws], [_t(b) for b in bs], X3),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_abi_supported_workspace_and_argument_checks():
    """Host-side only: every check fails before a launch, so no GPU is touched."""
    from rmd import _lib, library
    L = _lib.lib()
    for kh, kw, c0, c1, cout in [(k, l, a, b, o) for k in range(0, 10) for l in (1, 2, 3, 7, 9) for a in (0, 1, 324, 512, 513)
                                 for b in (-1, 0, 13, 200) for o in (0, 1, 2, 576, 1024, 1025)]:
        want = kh % 2 == 1 and kw % 2 == 1 and 1 <= kh <= 7 and 1 <= kw <= 7 and c0 >= 1 and c1 >= 0 \
            and c0 + c1 <= 512 and 1 <= cout <= 1024
        assert L.rmd_conv2d_supported(kh, kw, c0, c1, cout) == int(want), (kh, kw, c0, c1, cout)
        assert (L.rmd_conv2d_workspace_bytes(c0, c1, cout, kh, kw) > 0) == want
    for _, c0, c1, cout, kh, kw, _, _ in cases.SHAPES:
        packed = -(-cout // 32) * 32 * kh * kw * -(-(c0 + c1) // 16) * 16 * 2 * 2
        assert L.rmd_conv2d_workspace_bytes(c0, c1, cout, kh, kw) == packed + 256
    for b, planes, ht, wd in [(1, 324, 6, 10), (8, 324, 55, 128), (2, 81, 7, 9)]:
        packed = sum(L.rmd_conv2d_workspace_bytes(planes if cin is None else cin, 0, cout, k, k) - 256
                     for cout, cin, k in library.ENCODER_CONVS)
        bound = packed + (256 + 128 + 256) * b * ht * wd * 4
        assert bound <= L.rmd_motion_encoder_workspace_bytes(b, planes, ht, wd) <= bound + 4096
    assert L.rmd_motion_encoder_workspace_bytes(0, 324, 6, 10) == 0
    assert L.rmd_motion_encoder_workspace_bytes(1, 513, 6, 10) == 0

    def p(at):
        return ctypes.c_void_p(at)          # never dereferenced: each call below is refused before any launch

    def conv(in0=p(1 << 20), in1=None, weight=p(1 << 22), bias=p(1 << 23), out=p(1 << 24), work=p(1 << 26), b=1, c0=16,
             c1=0, cout=8, kh=3, kw=3, ht=4, wd=4, total=8, off=0, act=0, compute=_lib.RMD_BF16X3):
        return L.rmd_conv2d(in0, in1, weight, bias, out, work, b, c0, c1, cout, kh, kw, ht, wd, total, off, act,
                            compute, None)

    assert conv(in0=None) == -1 and b"null" in L.rmd_last_error()
    assert conv(out=None) == -1 and conv(work=None) == -1 and conv(weight=None) == -1 and conv(bias=None) == -1
    assert conv(c1=4) == -1 and b"in1" in L.rmd_last_error()                # C1 > 0 without in1
    assert conv(in1=p(1 << 21)) == -1 and b"in1" in L.rmd_last_error()      # in1 without C1
    assert conv(compute=_lib.RMD_F32) == -1 and b"compute" in L.rmd_last_error()
    assert conv(act=2) == -1 and b"act" in L.rmd_last_error()
    assert conv(b=0) == -2 and conv(ht=0) == -2 and conv(wd=0) == -2
    assert conv(kh=2) == -2 and b"unsupported" in L.rmd_last_error()
    assert conv(kw=9) == -2 and conv(c0=513) == -2 and conv(cout=1025, total=1025) == -2
    assert conv(c0=500, c1=13, in1=p(1 << 21)) == -2
    assert conv(total=7) == -2 and b"slice" in L.rmd_last_error()
    assert conv(total=10, off=3) == -2 and conv(off=-1) == -2
    assert conv(c0=512, ht=1 << 11, wd=1 << 10) == -2 and b"pixels" in L.rmd_last_error()
    assert conv(out=p(1 << 20)) == -1 and b"overlaps" in L.rmd_last_error()                 # out is in0
    assert conv(out=p((1 << 22) + 64)) == -1 and b"overlaps" in L.rmd_last_error()          # out inside the weight
    assert conv(work=p((1 << 24) - 256)) == -1 and b"workspace" in L.rmd_last_error()

    five = (ctypes.c_void_p * 5)(*([1 << 30] * 5))

    def enc(flow=p(1 << 20), corr=p(1 << 22), weights=five, biases=five, out=p(1 << 24), work=p(1 << 26), b=1,
            planes=324, ht=4, wd=4, compute=_lib.RMD_BF16X3):
        return L.rmd_motion_encoder(flow, corr, weights, biases, out, work, b, planes, ht, wd, compute, None)

    assert enc(flow=None) == -1 and enc(corr=None) == -1 and enc(out=None) == -1 and enc(work=None) == -1
    holes = (ctypes.c_void_p * 5)(1 << 30, 1 << 30, None, 1 << 30, 1 << 30)
    assert enc(weights=holes) == -1 and b"null" in L.rmd_last_error()
    assert enc(compute=_lib.RMD_F16) == -1 and b"compute" in L.rmd_last_error()
    assert enc(b=0) == -2 and enc(planes=0) == -2 and enc(planes=513) == -2
    assert enc(out=p(1 << 22)) == -1 and b"overlaps" in L.rmd_last_error()
    assert enc(work=p((1 << 24) - 256)) == -1 and b"workspace" in L.rmd_last_error()
