"""The backward of the fused k x k convolutions without a GPU: the tests' float64 restatement
(conv_backward_cases.py) against torch.autograd.grad of the float64 composite, the CPU operators against the
restatement, the emulation's error cap, the operator table, schemas, fake shapes and needs_grad empties, module
routing with fused_backward on and off, CPU training through the modules, state-dict keys and hooks, the
supported range, the workspace formula and the ABI's argument checks.

The CPU operators are plain fp32 ATen: 1e-5 max-normalised against float64."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_backward_cases as cases
import conv_cases

CPU_FP32 = 1e-5
RESTATEMENT = 1e-12
ACT_CODE = {"none": 0, "relu": 1}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _composite_grads(x, weight, bias, g, act, dtype):
    """torch.autograd.grad of F.conv2d + relu in `dtype` -> gx, gW, gb as numpy."""
    kh, kw = weight.shape[2:]
    ins = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (x, weight, bias)]
    out = F.conv2d(ins[0], ins[1], ins[2], padding=(kh // 2, kw // 2))
    if act == "relu":
        out = F.relu(out)
    return [t.numpy() for t in torch.autograd.grad(out, ins, torch.from_numpy(g).to(dtype))]


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_restatement_against_autograd_of_the_float64_composite(shape, act):
    c = cases.shape_case(shape)
    _, _, weight, bias = c["args"]
    got = _composite_grads(c["x"], weight, bias, c["g"], act, torch.float64)
    # the composite masks with its own float64 pre-activation; the oracle's y is that rounded to fp32: same sign
    for name, a, r in zip(("gx", "gw", "gb"), c["ref"][act], got):
        err = cases.max_norm_err(a, r)
        print(f"{shape} [{act}] {name}: restatement vs autograd {err:.3e}")
        assert err <= RESTATEMENT, (shape, act, name, err)


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_cpu_operators_against_the_restatement(shape, act):
    import rmd  # noqa: F401
    c = cases.shape_case(shape)
    x0, x1, weight, bias = c["args"]
    out = torch.ops.rmd.conv2d_act_train(_t(x0), _t(x1), _t(weight), _t(bias), ACT_CODE[act])
    ref_out = conv_cases.conv64([(weight, c["x"])], bias, act)
    assert cases.max_norm_err(out.numpy(), ref_out) <= CPU_FP32
    grads = torch.ops.rmd.conv2d_act_backward(_t(c["g"]), _t(c["y"][act]), _t(x0), _t(x1), _t(weight), ACT_CODE[act],
                                              [True, True, True, True])
    gx, gw, gb = c["ref"][act]
    gx0, gx1 = cases.split_sources(gx, x0.shape[1])
    assert grads[1].shape == ((0,) if x1 is None else x1.shape)
    for name, got, ref in (("gx0", grads[0], gx0), ("gx1", grads[1], gx1), ("gw", grads[2], gw), ("gb", grads[3], gb)):
        if ref is None:
            continue
        assert got.dtype == torch.float32 and got.shape == ref.shape
        err = cases.max_norm_err(got.numpy(), ref)
        print(f"{shape} [{act}] {name}: cpu {err:.3e}")
        assert err <= CPU_FP32, (shape, act, name, err)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_emulation_error_stays_under_its_cap(shape):
    c = cases.shape_case(shape)
    print(f"{shape}: e {c['e']}")
    for key, e in c["e"].items():
        assert e <= cases.E_MAX, (shape, key, e)
        assert c["tol"][key] == max(cases.FLOOR, cases.FACTOR * e)


def test_operator_table_schema_fake_shapes_and_empties():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from rmd import library
    assert library.conv_train_operators() == ["conv2d_act_backward", "conv2d_act_train"]
    # every other family returns what it returned before
    assert library.conv_operators() == ["conv2d_act", "motion_encoder"]
    assert library.update_operators() == ["sepconv_gru"]
    assert library.match_train_operators() == ["dicl_match_1x1_backward", "dicl_match_1x1_train"]
    others = [library.operators(), library.loss_operators(), library.metric_operators(), library.head_operators(),
              library.attn_operators(), library.match_operators(), library.match_train_operators(),
              library.update_operators(), library.conv_operators(), library.encoder_operators(),
              library.mnet_operators()]
    for names in others:
        assert names and not set(names) & set(library.conv_train_operators())
    assert sum(len(n) for n in others) + 2 == len(library._OPS)
    assert str(torch.ops.rmd.conv2d_act_train.default._schema) == \
        "rmd::conv2d_act_train(Tensor x0, Tensor? x1, Tensor weight, Tensor bias, int act) -> Tensor"
    assert str(torch.ops.rmd.conv2d_act_backward.default._schema) == \
        "rmd::conv2d_act_backward(Tensor grad, Tensor? y, Tensor x0, Tensor? x1, Tensor weight, int act, " \
        "bool[] needs_grad) -> Tensor[]"
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for name in library.conv_train_operators():
        for key in ("CUDA", "CPU", "Meta", "AutogradCPU"):
            assert has(f"rmd::{name}", key), (name, key)
    assert has("rmd::conv2d_act_train", "Autograd")
    with FakeTensorMode():
        def e(*s):
            return torch.empty(*s, device="cuda")
        out = torch.ops.rmd.conv2d_act_train(e(2, 192, 12, 16), e(2, 64, 12, 16), e(126, 256, 3, 3), e(126), 1)
        assert out.shape == (2, 126, 12, 16) and out.dtype == torch.float32 and out.device.type == "cuda"
        g = e(2, 126, 12, 16)
        grads = torch.ops.rmd.conv2d_act_backward(g, g, e(2, 192, 12, 16), e(2, 64, 12, 16), e(126, 256, 3, 3), 1,
                                                  [True, True, True, True])
        assert [tuple(t.shape) for t in grads] == [(2, 192, 12, 16), (2, 64, 12, 16), (126, 256, 3, 3), (126,)]
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in grads)
        grads = torch.ops.rmd.conv2d_act_backward(g, None, e(2, 256, 12, 16), None, e(126, 256, 3, 3), 0,
                                                  [False, True, True, False])
        assert [tuple(t.shape) for t in grads] == [(0,), (0,), (126, 256, 3, 3), (0,)]
        with pytest.raises(ValueError, match="grad must be"):
            torch.ops.rmd.conv2d_act_backward(e(2, 125, 12, 16), None, e(2, 256, 12, 16), None, e(126, 256, 3, 3), 0,
                                              [True] * 4)
        with pytest.raises(ValueError, match="y must be"):
            torch.ops.rmd.conv2d_act_backward(g, e(2, 126, 12, 15), e(2, 256, 12, 16), None, e(126, 256, 3, 3), 1,
                                              [True] * 4)
        with pytest.raises(ValueError, match="exactly when act"):
            torch.ops.rmd.conv2d_act_backward(g, None, e(2, 256, 12, 16), None, e(126, 256, 3, 3), 1, [True] * 4)
        with pytest.raises(ValueError, match="exactly when act"):
            torch.ops.rmd.conv2d_act_backward(g, g, e(2, 256, 12, 16), None, e(126, 256, 3, 3), 0, [True] * 4)
        with pytest.raises(ValueError, match="needs_grad"):
            torch.ops.rmd.conv2d_act_backward(g, None, e(2, 256, 12, 16), None, e(126, 256, 3, 3), 0, [True] * 3)
        with pytest.raises(ValueError, match="odd"):
            torch.ops.rmd.conv2d_act_train(e(1, 2, 5, 7), None, e(8, 2, 2, 3), e(8), 0)
        with pytest.raises(ValueError, match="weight must be"):
            torch.ops.rmd.conv2d_act_backward(g, None, e(2, 255, 12, 16), None, e(126, 256, 3, 3), 0, [True] * 4)
        with pytest.raises(ValueError, match="act"):
            torch.ops.rmd.conv2d_act_train(e(1, 2, 5, 7), None, e(8, 2, 3, 3), e(8), 2)
    # the CPU kernels' empties and the non-differentiable operators, which stay as they are
    c = cases.shape_case(cases.SHAPES[4])
    x0, x1, weight, bias = (_t(a) for a in c["args"])
    for needs in ([True, False, False, True], [False, True, True, False], [False] * 4):
        grads = torch.ops.rmd.conv2d_act_backward(_t(c["g"]), None, x0, x1, weight, 0, needs)
        full = torch.ops.rmd.conv2d_act_backward(_t(c["g"]), None, x0, x1, weight, 0, [True] * 4)
        for got, ref, need in zip(grads, full, needs):
            assert tuple(got.shape) == (tuple(ref.shape) if need else (0,))
            assert not need or torch.equal(got, ref)
    from rmd import _lib, ops
    assert not torch.ops.rmd.conv2d_act(x0.clone().requires_grad_(True), x1, weight, bias, 1, _lib.RMD_BF16X3).requires_grad
    assert torch.ops.rmd.conv2d_act_train(x0.clone().requires_grad_(True), x1, weight, bias, 1).requires_grad
    assert ops.conv2d_act(x0, x1, weight.clone().requires_grad_(True), bias, "relu", differentiable=True).requires_grad
    assert not ops.conv2d_act(x0, x1, weight.clone().requires_grad_(True), bias, "relu").requires_grad
    with pytest.raises(ValueError, match="no backward"):
        ops.conv2d_act(x0, x1, weight, bias, precision="bf16", differentiable=True)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.rmd.conv2d_act_train, (x0, x1, weight, bias, 1), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.conv2d_act_backward,
                          (_t(c["g"]), _t(c["y"]["relu"]), x0, x1, weight, 1, [True, False, True, True]), test_utils=utils)


def _modules(**kwargs):
    import rmd.raft
    return {"flow": cases.int_init(rmd.raft.FlowHead(**kwargs), 1),
            "enc": cases.int_init(rmd.raft.BasicMotionEncoder(324, **kwargs), 2),
            "up8": cases.saturate_up8(cases.int_init(rmd.raft.Up8Network(128, **kwargs), 3)),
            "block": cases.int_init(rmd.raft.BasicUpdateBlock(324, **kwargs), 4)}


def _inputs(name, ht=6, wd=10, seed=0):
    rng = np.random.default_rng(seed)
    h = _t(4 * cases.exact_ints(rng, (1, 128, ht, wd), 2))
    x = _t(cases.exact_ints(rng, (1, 128, ht, wd), 2))
    corr = _t(cases.exact_ints(rng, (1, 324, ht, wd), 2))
    flow = _t(cases.exact_ints(rng, (1, 2, ht, wd), 2))
    return {"flow": [h], "enc": [flow, corr], "up8": [h, flow], "block": [h, x, corr, flow]}[name]


def _train(module, inputs):
    """Integer-weighted sum of the outputs -> (outputs, input gradients, parameter gradients)."""
    inputs = [t.clone().requires_grad_(True) for t in inputs]
    module.zero_grad()
    outs = module(*inputs)
    outs = list(outs) if isinstance(outs, tuple) else [outs]
    rng = np.random.default_rng(99)
    loss = sum((o * torch.from_numpy(cases.exact_ints(rng, tuple(o.shape), 2)).to(o.device)).sum() for o in outs)
    loss.backward()
    return ([o.detach() for o in outs], [t.grad for t in inputs],
            {n: p.grad for n, p in module.named_parameters()})


@pytest.mark.parametrize("fused", ["off", "auto", "on"])
@pytest.mark.parametrize("name", ["flow", "enc", "up8", "block"])
def test_modules_train_on_cpu_to_the_gradients_of_off(name, fused):
    ref = _train(_modules()[name], _inputs(name))
    mod = _modules(fused=fused, fused_backward=True)[name]
    got = _train(mod, _inputs(name))
    assert sorted(mod.state_dict().keys()) == sorted(_modules()[name].state_dict().keys())
    for a, b in zip(got[0] + got[1], ref[0] + ref[1]):
        assert float((a - b).abs().max()) == 0.0
    for n in ref[2]:
        assert float((got[2][n] - ref[2][n]).abs().max()) == 0.0, n
    assert any(float(g.abs().max()) > 0 for g in list(ref[2].values()) + ref[1])


def test_routing_with_the_flag_on_and_off(monkeypatch):
    import rmd.raft
    from rmd import ops
    g = conv_cases.fixture(conv_cases.BLOCK_FIXTURE)
    flow, corr, h = _t(g["flow"]), _t(g["corr"]), _t(g["h"])
    calls = []
    real_enc, real_conv = ops.motion_encoder, ops.conv2d_act

    def conv(*a, **k):
        calls.append("train" if (k.get("differentiable") or (len(a) > 6 and a[6])) else "conv")
        return real_conv(*a, **k)

    monkeypatch.setattr(ops, "motion_encoder", lambda *a, **k: calls.append("enc") or real_enc(*a, **k))
    monkeypatch.setattr(ops, "conv2d_act", conv)
    for make, args in ((lambda **k: rmd.raft.BasicMotionEncoder(324, **k), (flow, corr)),
                       (lambda **k: rmd.raft.FlowHead(**k), (h,)),
                       (lambda **k: rmd.raft.Up8Network(128, **k), (h, flow))):
        n_train = 5 if len(args) == 2 and args[0] is flow and args[1] is corr else 2
        assert make().fused_backward is False
        # flag off: today's strings and routes
        with pytest.raises(RuntimeError, match="a gradient is needed \\(the fused convolutions are inference only\\)"):
            make(fused="on")(*args)
        calls.clear()
        assert make(fused="auto")(*args).requires_grad and calls == []
        # flag on: the train operators when a gradient is needed, the inference path otherwise
        for fused in ("auto", "on"):
            calls.clear()
            assert make(fused=fused, fused_backward=True)(*args).requires_grad
            assert calls == ["train"] * n_train, (fused, calls)
            calls.clear()
            with torch.no_grad():
                make(fused=fused, fused_backward=True)(*args)
            assert calls == (["enc"] if n_train == 5 else ["conv", "conv"])
        calls.clear()
        assert make(fused="off", fused_backward=True)(*args).requires_grad and calls == []
        # every fall-back reason with the flag on
        bf = make(fused="on", fused_backward=True, precision="bf16")
        with pytest.raises(RuntimeError, match="fp32 only"):
            bf(*args)
        calls.clear()
        assert make(fused="auto", fused_backward=True, precision="bf16")(*args).requires_grad and calls == []
        with torch.autocast("cpu", dtype=torch.bfloat16):
            with pytest.raises(RuntimeError, match="autocast"):
                make(fused="on", fused_backward=True)(*args)
            make(fused="auto", fused_backward=True)(*args)
            assert calls == []
        with pytest.raises(RuntimeError, match="float32"):
            make(fused="on", fused_backward=True).double()(*[a.double() for a in args])
        with pytest.raises(RuntimeError, match="4-D"):
            make(fused="on", fused_backward=True)(*[a[0] for a in args])
    mixed = rmd.raft.Up8Network(128, mixed_precision=True, fused="on", fused_backward=True)
    with pytest.raises(RuntimeError, match="mixed_precision"):
        mixed(h, flow)
    assert rmd.raft.Up8Network(128, mixed_precision=True, fused="auto", fused_backward=True).fallback_reason(h)
    blk = rmd.raft.BasicUpdateBlock(324, fused="on", fused_backward=True)
    assert blk.enc.fused_backward and blk.flow.fused_backward and blk.gru.fused == "off"
    assert not rmd.raft.BasicUpdateBlock(324, fused="on").enc.fused_backward


def test_hooks_on_the_modules_fire_and_the_inner_ones_do_not():
    import rmd.raft
    blk = cases.int_init(rmd.raft.BasicUpdateBlock(324, fused="on", fused_backward=True), 4)
    outer, inner = [], []
    for m in (blk, blk.enc, blk.flow):
        m.register_forward_hook(lambda m, inputs, output: outer.append(1))
    for m in (blk.enc.convc1, blk.enc.conv, blk.flow.conv1, blk.flow.relu, blk.flow.conv2):
        m.register_forward_hook(lambda m, inputs, output: inner.append(1))
    out = blk(*_inputs("block"))
    assert out[1].requires_grad and outer == [1, 1, 1] and inner == []


def test_abi_supported_workspace_and_argument_checks():
    """Host-side only: every check fails before a launch, so no GPU is touched."""
    from rmd import _lib
    L = _lib.lib()
    for kh, kw, c0, c1, cout in [(k, l, a, b, o) for k in range(0, 10) for l in (1, 2, 3, 7, 9) for a in (0, 1, 324, 512, 513)
                                 for b in (-1, 0, 13, 200) for o in (0, 1, 2, 576, 1024, 1025)]:
        want = L.rmd_conv2d_supported(kh, kw, c0, c1, cout)
        assert L.rmd_conv2d_backward_supported(kh, kw, c0, c1, cout) == want, (kh, kw, c0, c1, cout)
        assert (L.rmd_conv2d_backward_workspace_bytes(2, c0, c1, cout, kh, kw, 5, 7) > 0) == bool(want)
    for kh, kw, c0, c1, cout in cases.NINE:
        assert L.rmd_conv2d_backward_supported(kh, kw, c0, c1, cout) == 1
    assert L.rmd_conv2d_supported(1, 1, 576, 0, 256) == 0          # the public forward answer has not moved
    for shape in cases.SHAPES + [(6, 192, 64, 126, 3, 3, 48, 64), (8, 324, 0, 256, 1, 1, 55, 128)]:
        b, c0, c1, cout, kh, kw, ht, wd = shape
        assert L.rmd_conv2d_backward_workspace_bytes(b, c0, c1, cout, kh, kw, ht, wd) == cases.workspace_bytes(*shape), shape
    assert L.rmd_conv2d_backward_workspace_bytes(0, 16, 0, 8, 3, 3, 4, 4) == 0
    assert L.rmd_conv2d_backward_workspace_bytes(1, 16, 0, 8, 3, 3, 0, 4) == 0

    def p(at):
        return ctypes.c_void_p(at)          # never dereferenced: each call below is refused before any launch

    def bwd(grad=p(1 << 20), y=None, in0=p(1 << 22), in1=None, weight=p(1 << 24), gx0=p(1 << 26), gx1=None,
            gw=p(1 << 27), gb=p(1 << 28), work=p(1 << 30), b=1, c0=16, c1=0, cout=8, kh=3, kw=3, ht=4, wd=4, act=0):
        return L.rmd_conv2d_backward(grad, y, in0, in1, weight, gx0, gx1, gw, gb, work, b, c0, c1, cout, kh, kw, ht,
                                     wd, act, None)

    assert bwd(grad=None) == -1 and b"null" in L.rmd_last_error()
    assert bwd(in0=None) == -1 and bwd(weight=None) == -1 and bwd(work=None) == -1
    assert bwd(act=2) == -1 and b"act" in L.rmd_last_error()
    assert bwd(act=1) == -1 and b"y must" in L.rmd_last_error()                 # ReLU without y
    assert bwd(y=p(1 << 21)) == -1 and b"y must" in L.rmd_last_error()          # y without ReLU
    assert bwd(c1=4) == -1 and b"in1" in L.rmd_last_error()
    assert bwd(in1=p(1 << 23)) == -1 and b"in1" in L.rmd_last_error()
    assert bwd(gx1=p(1 << 29)) == -1 and b"grad_in1" in L.rmd_last_error()      # a second gradient without a source
    assert bwd(b=0) == -2 and bwd(ht=0) == -2 and bwd(wd=0) == -2
    assert bwd(kh=2) == -2 and b"unsupported" in L.rmd_last_error()
    assert bwd(kw=9) == -2 and bwd(c0=513) == -2 and bwd(cout=1025) == -2
    assert bwd(c0=512, ht=1 << 11, wd=1 << 10) == -2 and b"pixels" in L.rmd_last_error()
    assert bwd(gx0=p(1 << 22)) == -1 and b"overlaps" in L.rmd_last_error()      # a gradient is its input
    assert bwd(gw=p((1 << 24) + 64)) == -1 and b"overlaps" in L.rmd_last_error()
    assert bwd(gb=p(1 << 27)) == -1 and b"overlaps" in L.rmd_last_error()       # two gradients in one place
    assert bwd(work=p((1 << 26) - 256)) == -1 and b"workspace" in L.rmd_last_error()
    assert bwd(work=p((1 << 20) - 256)) == -1 and b"workspace" in L.rmd_last_error()
    # nothing asked for: accepted, nothing launched
    assert bwd(gx0=None, gw=None, gb=None) == 0
