"""The backward of the fused k x k convolutions on the GPU: csrc/conv_backward.hip through
torch.ops.rmd.conv2d_act_backward, torch.ops.rmd.conv2d_act_train and the drop-in modules with fused="on",
fused_backward=True, against the tests' float64 restatement (conv_backward_cases.py) on the ten shapes with both
activations, one-hot output gradients and weights against their closed forms, exact integer data bitwise against
the CPU composite, needs_grad selection, views, repeatability, sample independence, NaN positions, opcheck, the
no-host-synchronisation rule, the allocation bound and the argument checks.

Tolerance (conv_backward_cases.py): gx and gW per case at max(1e-5, 3 e), e the error of the CPU float64 emulation
of the three-product arithmetic against float64 — never a figure of the kernel's; gb at 1e-5.  The operator-level
tests pass the oracle's own y, so both sides use the same mask.

Every test here calls the new operators: none can pass without the kernels."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_backward_cases as cases
import conv_cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
ACT_CODE = {"none": 0, "relu": 1}
ALL = [True, True, True, True]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _backward(g, y, x0, x1, weight, act, needs=ALL):
    import rmd  # noqa: F401
    return torch.ops.rmd.conv2d_act_backward(_t(g), _t(y), _t(x0), _t(x1), _t(weight), ACT_CODE[act], list(needs))


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_against_float64(shape, act):
    c = cases.shape_case(shape)
    x0, x1, weight, _ = c["args"]
    grads = _backward(c["g"], c["y"][act], x0, x1, weight, act)
    gx, gw, gb = c["ref"][act]
    got_gx = torch.cat([g for g in grads[:2] if g.numel()], dim=1).cpu().numpy()
    assert grads[0].shape == x0.shape and grads[1].shape == ((0,) if x1 is None else x1.shape)
    assert all(g.dtype == torch.float32 and g.is_contiguous() for g in grads)
    errs = {"gx": cases.max_norm_err(got_gx, gx), "gw": cases.max_norm_err(grads[2].cpu().numpy(), gw),
            "gb": cases.max_norm_err(grads[3].cpu().numpy(), gb)}
    tols = {"gx": c["tol"][act, "gx"], "gw": c["tol"][act, "gw"], "gb": cases.BIAS_TOL}
    print(f"{shape} [{act}]: kernel {errs}  emulation e {c['e'][act, 'gx']:.3e} / {c['e'][act, 'gw']:.3e}  "
          f"tolerances {tols}")
    for name in errs:
        assert errs[name] <= tols[name], (shape, act, name, errs[name], tols[name])


def test_one_hot_output_gradient_gives_the_shifted_input():
    """g a single 1 at (b, o, y, x), small-integer x: gW[o, :, i, j] = x[b, :, y + i - k/2, x + j - k/2] exactly
    (zero outside the map) and every other row of gW zero, for every tap of a 3 x 3 and of a 7 x 7 kernel at once."""
    b, c0, c1, cout, ht, wd = cases.ONEHOT_SHAPE
    rng = np.random.default_rng(12)
    x = cases.exact_ints(rng, (b, c0 + c1, ht, wd), 9)
    assert set(cases.ONEHOT_CIN) <= set(range(c0 + c1)) and max(cases.ONEHOT_COUT) < cout
    n = 0
    for k in (3, 7):
        p = k // 2
        padded = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
        weight = np.zeros((cout, c0 + c1, k, k), np.float32)
        for y0, xx0 in cases.ONEHOT_PIXELS:
            o = cases.ONEHOT_COUT[n % len(cases.ONEHOT_COUT)]
            n += 1
            g = np.zeros((b, cout, ht, wd), np.float32)
            g[0, o, y0, xx0] = 1.0
            grads = _backward(g, None, x[:, :c0], x[:, c0:], weight, "none", [False, False, True, True])
            want = np.zeros_like(weight)
            want[o] = padded[0, :, y0:y0 + k, xx0:xx0 + k]
            assert np.array_equal(grads[2].cpu().numpy().view(np.uint32), want.view(np.uint32)), (k, o, y0, xx0)
            gb = np.zeros(cout, np.float32)
            gb[o] = 1.0
            assert np.array_equal(grads[3].cpu().numpy(), gb)
    print(f"one-hot g: {n} cases, every tap and input channel of each, bitwise")


def test_one_hot_weight_gives_the_shifted_output_gradient():
    """A single W[o, c, i, j] = 1, small-integer g: gx[:, c] is g[:, o] read at (y - i + k/2, x - j + k/2), every
    other channel zero; conv_cases.onehot_cases() covers every tap and the channel boundaries."""
    b, c0, c1, cout, ht, wd = conv_cases.ONEHOT_SHAPE
    rng = np.random.default_rng(13)
    g = cases.exact_ints(rng, (b, cout, ht, wd), 9)
    x0, x1 = np.zeros((b, c0, ht, wd), np.float32), np.zeros((b, c1, ht, wd), np.float32)
    for k, o, c, i, j in conv_cases.onehot_cases():
        weight = np.zeros((cout, c0 + c1, k, k), np.float32)
        weight[o, c, i, j] = 1.0
        grads = _backward(g, None, x0, x1, weight, "none", [True, True, False, False])
        got = torch.cat(grads[:2], dim=1).cpu().numpy()
        want = np.zeros((b, c0 + c1, ht, wd), np.float32)
        # the forward reads (y + i - k/2, x + j - k/2): the gradient comes back through the mirrored tap
        want[:, c] = conv_cases.onehot_expected(g, k, o, k - 1 - i, k - 1 - j)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, o, c, i, j)
    print(f"one-hot W: {len(conv_cases.onehot_cases())} cases, bitwise")


def _cpu_composite(x0, x1, weight, bias, g, act):
    """y and the four gradients of F.conv2d + relu on CPU tensors."""
    kh, kw = weight.shape[2:]
    ins = [None if a is None else torch.from_numpy(a).requires_grad_(True) for a in (x0, x1, weight, bias)]
    x = ins[0] if x1 is None else torch.cat([ins[0], ins[1]], dim=1)
    y = F.conv2d(x, ins[2], ins[3], padding=(kh // 2, kw // 2))
    y = F.relu(y) if act == "relu" else y
    grads = torch.autograd.grad(y, [t for t in ins if t is not None], torch.from_numpy(g))
    grads = list(grads) if x1 is not None else [grads[0], torch.empty(0), grads[1], grads[2]]
    return y.detach(), grads


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("shape", cases.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integer_data_is_bitwise_the_cpu_composite(shape, act):
    x0, x1, weight, bias, g = cases.exact_case(shape)
    y, want = _cpu_composite(x0, x1, weight, bias, g, act)
    import rmd  # noqa: F401
    out = torch.ops.rmd.conv2d_act_train(_t(x0), _t(x1), _t(weight), _t(bias), ACT_CODE[act])
    assert _same_bits(out, y)
    grads = _backward(g, y.numpy() if act == "relu" else None, x0, x1, weight, act)
    for name, a, b in zip(("gx0", "gx1", "gw", "gb"), grads, want):
        assert float((a.cpu() - b).abs().max()) == 0.0 if b.numel() else a.numel() == 0, (shape, act, name)
        assert _same_bits(a + 0.0, b + 0.0), (shape, act, name)        # + 0.0: -0.0 and 0.0 are the same result


def _modules(**kwargs):
    import rmd.raft
    return {"flow": cases.int_init(rmd.raft.FlowHead(**kwargs), 1),
            "enc": cases.int_init(rmd.raft.BasicMotionEncoder(324, **kwargs), 2),
            "up8": cases.saturate_up8(cases.int_init(rmd.raft.Up8Network(128, **kwargs), 3)),
            "block": cases.int_init(rmd.raft.BasicUpdateBlock(324, **kwargs), 4)}


def _inputs(name, ht, wd):
    rng = np.random.default_rng(ht * 1000 + wd)
    h = torch.from_numpy(4 * cases.exact_ints(rng, (1, 128, ht, wd), 2))
    x = torch.from_numpy(cases.exact_ints(rng, (1, 128, ht, wd), 2))
    corr = torch.from_numpy(cases.exact_ints(rng, (1, 324, ht, wd), 2))
    flow = torch.from_numpy(cases.exact_ints(rng, (1, 2, ht, wd), 2))
    return {"flow": [h], "enc": [flow, corr], "up8": [h, flow], "block": [h, x, corr, flow]}[name]


def _train(module, inputs):
    """A fixed integer-weighted sum of the outputs -> (outputs, input gradients, parameter gradients), on the CPU."""
    inputs = [t.clone().requires_grad_(True) for t in inputs]
    module.zero_grad()
    outs = module(*inputs)
    outs = list(outs) if isinstance(outs, tuple) else [outs]
    rng = np.random.default_rng(99)
    loss = sum((o * torch.from_numpy(cases.exact_ints(rng, tuple(o.shape), 2)).to(o.device)).sum() for o in outs)
    loss.backward()
    return ([o.detach().cpu() for o in outs], [t.grad.cpu() for t in inputs],
            {n: p.grad.cpu() for n, p in module.named_parameters()})


@pytest.mark.parametrize("size", [(6, 10), (9, 70)], ids=["6x10", "9x70"])
@pytest.mark.parametrize("name", ["flow", "enc", "up8", "block"])
def test_modules_train_to_the_gradients_of_the_off_module_on_the_cpu(name, size):
    """Exact integer parameters and inputs (conv_backward_cases.int_init): every activation and gradient is a small
    integer (a multiple of 1/16 behind the recurrent unit, whose parameters are zero), so every path computes the
    same numbers and the fused and eager ReLU masks agree by construction.  Up8Network's softmax is made exactly
    one-hot (saturate_up8), which is what makes its convex combination comparable across devices at all; the
    gradient reaching its mask head is then exactly zero, and the head's own arithmetic is covered by the operator
    tests on its two shapes."""
    ref = _train(_modules()[name], _inputs(name, *size))
    mod = _modules(fused="on", fused_backward=True)[name].to(DEV)
    got = _train(mod, [t.to(DEV) for t in _inputs(name, *size)])
    for k, (a, b) in enumerate(zip(got[0] + got[1], ref[0] + ref[1])):
        assert float((a - b).abs().max()) == 0.0, (name, size, k)
    for n in ref[2]:
        assert float((got[2][n] - ref[2][n]).abs().max()) == 0.0, (name, size, n)
    assert any(float(g.abs().max()) > 0 for g in list(ref[2].values()) + ref[1])
    # the forward is bitwise that of fused="on" without the flag
    plain = _modules(fused="on")[name].to(DEV)
    with torch.no_grad():
        outs = plain(*[t.to(DEV) for t in _inputs(name, *size)])
    outs = list(outs) if isinstance(outs, tuple) else [outs]
    for a, b in zip(got[0], outs):
        assert _same_bits(a, b), (name, size)


def test_needs_grad_selects_the_kernels():
    from rmd import library
    shape = cases.SHAPES[4]
    c = cases.shape_case(shape)
    x0, x1, weight, _ = c["args"]
    full = {act: _backward(c["g"], c["y"][act], x0, x1, weight, act) for act in cases.ACTS}
    for needs in ([True, False, False, False], [False, True, False, False], [False, False, True, False],
                  [False, False, False, True], [True, False, True, True], [False] * 4):
        for act in cases.ACTS:
            grads = _backward(c["g"], c["y"][act], x0, x1, weight, act, needs)
            for got, ref, need in zip(grads, full[act], needs):
                assert tuple(got.shape) == (tuple(ref.shape) if need else (0,))
                assert not need or _same_bits(got, ref), (needs, act)
    kernels = library.conv_backward_kernels
    assert kernels([False] * 4, 1) == []
    assert kernels([False, False, False, True], 0) == kernels([False, False, False, True], 1) == ["mask_bias"]
    assert kernels([True, False, False, False], 0) == ["pack0", "conv0"]
    assert kernels([True, False, False, False], 1) == ["mask_bias+gm", "pack0", "conv0"]
    assert kernels([False, True, False, False], 0) == ["pack1", "conv1"]
    assert kernels([False, True, False, False], 0, has_x1=False) == []
    assert kernels([False, False, True, False], 0) == ["wgrad", "reduce"]
    assert kernels(ALL, 0) == ["mask_bias", "pack0", "conv0", "pack1", "conv1", "wgrad", "reduce"]
    assert kernels(ALL, 1) == ["mask_bias+gm", "pack0", "conv0", "pack1", "conv1", "wgrad", "reduce"]
    # through autograd: only what requires a gradient is computed
    t0, t1, tw = _t(x0), _t(x1), _t(weight).requires_grad_(True)
    tb = _t(c["args"][3])
    out = torch.ops.rmd.conv2d_act_train(t0, t1, tw, tb, 1)
    out.backward(_t(c["g"]))
    assert t0.grad is None and tb.grad is None and tw.grad is not None


def test_views_give_the_results_of_their_contiguous_copies():
    import rmd  # noqa: F401

    def permuted(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

    def offset(t):
        return torch.zeros(t.numel() + 3, device=DEV)[3:].view_as(t).copy_(t)

    c = cases.shape_case(cases.SHAPES[5])
    x0, x1, weight, _ = (_t(a) for a in c["args"])
    g, y = _t(c["g"]), _t(c["y"]["relu"])
    ref = torch.ops.rmd.conv2d_act_backward(g, y, x0, x1, weight, 1, ALL)
    for view in (permuted, offset):
        assert not view(x0).is_contiguous() or view(x0).storage_offset() == 3
        got = torch.ops.rmd.conv2d_act_backward(view(g), view(y), view(x0), view(x1), view(weight), 1, ALL)
        for a, b in zip(got, ref):
            assert _same_bits(a, b)


def test_runs_repeat_and_samples_do_not_depend_on_the_batch():
    for shape in (cases.BATCH_SHAPE, cases.SHAPES[5], cases.SHAPES[7]):
        c = cases.shape_case(shape)
        x0, x1, weight, _ = c["args"]
        a, b = (_backward(c["g"], c["y"]["relu"], x0, x1, weight, "relu") for _ in range(2))
        for s, t in zip(a, b):
            assert _same_bits(s, t), shape
    c = cases.shape_case(cases.BATCH_SHAPE)
    x0, _, weight, _ = c["args"]
    full = _backward(c["g"], c["y"]["relu"], x0, None, weight, "relu")[0]
    for i in range(x0.shape[0]):
        alone = _backward(c["g"][i:i + 1], c["y"]["relu"][i:i + 1], x0[i:i + 1], None, weight, "relu",
                          [True, False, False, False])[0]
        assert _same_bits(alone, full[i:i + 1]), i


def test_nan_positions():
    """A NaN in g reaches exactly the gx positions whose transposed receptive field holds it; a NaN in y keeps the
    gradient (!(y <= 0)), a masked NaN in g is dropped."""
    shape = (1, 20, 13, 40, 3, 3, 8, 40)
    b, c0, c1, cout, kh, kw, ht, wd = shape
    rng = np.random.default_rng(21)
    x = rng.standard_normal((b, c0 + c1, ht, wd)).astype(np.float32)
    weight = rng.standard_normal((cout, c0 + c1, kh, kw)).astype(np.float32)
    g = rng.standard_normal((b, cout, ht, wd)).astype(np.float32)
    g[0, 7, 3, 33] = np.nan
    grads = _backward(g, None, x[:, :c0], x[:, c0:], weight, "none")
    want = np.zeros((b, c0 + c1, ht, wd), bool)
    want[:, :, 2:5, 32:35] = True
    assert np.array_equal(np.isnan(torch.cat(grads[:2], dim=1).cpu().numpy()), want)
    gw = np.isnan(grads[2].cpu().numpy())
    assert gw[7].all() and not np.delete(gw, 7, axis=0).any()
    gb = np.isnan(grads[3].cpu().numpy())
    assert gb[7] and gb.sum() == 1
    # the mask: y <= 0 drops the NaN of g, a NaN in y keeps the gradient at its position
    y = np.ones_like(g)
    y[0, 7, 3, 33] = 0.0
    y[0, 9, 5, 5] = np.nan
    y[0, 11] = -1.0
    grads = _backward(g, y, x[:, :c0], x[:, c0:], weight, "relu")
    ref = cases.backward_ref(g, y, x, weight, "relu")
    assert not any(torch.isnan(t).any() for t in grads)
    emulated = cases.backward_ref(g, y, x, weight, "relu", 3)
    for k in (0, 1):
        got = torch.cat(grads[:2], dim=1) if k == 0 else grads[2]
        assert cases.max_norm_err(got.cpu().numpy(), ref[k]) <= cases.tolerance(emulated[k], ref[k])[1], k
    assert cases.max_norm_err(grads[3].cpu().numpy(), ref[2]) <= cases.BIAS_TOL
    assert float(grads[3][11]) == 0.0 and float(grads[2][11].abs().max()) == 0.0
    # the oracle keeps every position of channel 9, the one under the NaN of y too
    assert abs(ref[2][9] - g[0, 9].astype(np.float64).sum()) <= 1e-9


def test_opcheck():
    import rmd  # noqa: F401
    c = cases.shape_case(cases.SHAPES[4])
    x0, x1, weight, bias = (_t(a) for a in c["args"])
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.rmd.conv2d_act_train, (x0, x1, weight, bias, 1), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.conv2d_act_train,
                          (x0.clone().requires_grad_(True), None, weight[:, :20].contiguous().requires_grad_(True), bias, 0),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.conv2d_act_backward,
                          (_t(c["g"]), _t(c["y"]["relu"]), x0, x1, weight, 1, [True, False, True, True]), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.conv2d_act_backward,
                          (_t(c["g"]), None, x0, x1, weight, 0, ALL), test_utils=utils)


def test_training_never_waits_for_the_host_and_stays_in_its_workspace():
    """Sync-debug mode over one training step of the fused modules, then the peak allocation of a backward call:
    its outputs and the workspace of rmd_conv2d_backward_workspace_bytes, nothing else."""
    import rmd.raft
    from rmd import _lib
    blk = cases.int_init(rmd.raft.BasicUpdateBlock(324, fused="on", fused_backward=True), 4).to(DEV)
    args = [t.to(DEV) for t in _inputs("block", 6, 10)]

    def step():
        blk.zero_grad(set_to_none=False)
        h, d = blk(*args)
        (h.sum() + d.sum()).backward()

    step()                                              # the warm-up call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")

    shape = cases.SHAPES[5]
    c = cases.shape_case(shape)
    x0, x1, weight, _ = (_t(a) for a in c["args"])
    g, y = _t(c["g"]), _t(c["y"]["relu"])
    torch.ops.rmd.conv2d_act_backward(g, y, x0, x1, weight, 1, ALL)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    grads = torch.ops.rmd.conv2d_act_backward(g, y, x0, x1, weight, 1, ALL)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bound = sum(t.numel() * 4 for t in grads) + _lib.lib().rmd_conv2d_backward_workspace_bytes(*shape)
    assert peak <= bound + 5 * 512, (peak, bound)       # the allocator rounds each of the five blocks up to 512 bytes


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd.raft
    from rmd import _lib, ops
    c = cases.shape_case(cases.SHAPES[4])
    x0, x1, weight, bias = c["args"]
    t0, t1, tw, tb, g = _t(x0), _t(x1), _t(weight), _t(bias), _t(c["g"])
    gfix = conv_cases.fixture(conv_cases.BLOCK_FIXTURE)
    h, flow, corr = _t(gfix["h"]), _t(gfix["flow"]), _t(gfix["corr"])
    makes = ((lambda **k: rmd.raft.BasicMotionEncoder(324, **k).to(DEV), (flow, corr)),
             (lambda **k: rmd.raft.FlowHead(**k).to(DEV), (h,)),
             (lambda **k: rmd.raft.Up8Network(128, **k).to(DEV), (h, flow)))

    class NoLaunch:
        def __getattr__(self, name):
            if name in ("rmd_conv2d_supported", "rmd_conv2d_backward_supported"):
                return lambda *a: 1
            raise AssertionError(f"reached {name}")

    real = _lib._lib
    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    for make, args in makes:
        with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(RuntimeError, match="autocast"):
            make(fused="on", fused_backward=True)(*args)
        with pytest.raises(RuntimeError, match="inference only"):
            make(fused="on")(*args)
        with pytest.raises(RuntimeError, match="fp32 only"):
            make(fused="on", fused_backward=True, precision="bf16")(*args)
    with pytest.raises(RuntimeError, match="mixed_precision"):
        rmd.raft.Up8Network(128, mixed_precision=True, fused="on", fused_backward=True).to(DEV)(h, flow)
    cpu = torch.from_numpy
    for fn in (lambda: torch.ops.rmd.conv2d_act_train(t0, cpu(x1), tw, tb, 0),
               lambda: torch.ops.rmd.conv2d_act_backward(g, None, t0, t1, cpu(weight), 0, ALL),
               lambda: torch.ops.rmd.conv2d_act_backward(cpu(c["g"]), None, t0, t1, tw, 0, ALL)):
        with pytest.raises(ValueError, match="must be on the GPU"):
            fn()
    with pytest.raises(ValueError, match="different devices"):
        ops.conv2d_act(t0, cpu(x1), tw, tb, differentiable=True)
    with pytest.raises(ValueError, match="grad must be"):
        torch.ops.rmd.conv2d_act_backward(g[:, :-1].contiguous(), None, t0, t1, tw, 0, ALL)
    with pytest.raises(ValueError, match="y must be"):
        torch.ops.rmd.conv2d_act_backward(g, g[:, :, :-1].contiguous(), t0, t1, tw, 1, ALL)
    with pytest.raises(ValueError, match="exactly when act"):
        torch.ops.rmd.conv2d_act_backward(g, None, t0, t1, tw, 1, ALL)
    with pytest.raises(ValueError, match="needs_grad"):
        torch.ops.rmd.conv2d_act_backward(g, None, t0, t1, tw, 0, [True, True])
    with pytest.raises(ValueError, match="odd"):
        torch.ops.rmd.conv2d_act_backward(g, None, t0, t1, tw[:, :, :2].contiguous(), 0, ALL)
    with pytest.raises(ValueError, match="weight must be"):
        torch.ops.rmd.conv2d_act_backward(g, None, t0, None, tw, 0, ALL)
    with pytest.raises(ValueError, match="unsupported on the GPU"):                             # C0 + C1 > 512
        torch.ops.rmd.conv2d_act_backward(torch.zeros(1, 8, 4, 4, device=DEV), None, torch.zeros(1, 500, 4, 4, device=DEV),
                                          torch.zeros(1, 13, 4, 4, device=DEV), torch.zeros(8, 513, 3, 3, device=DEV),
                                          0, ALL)
    monkeypatch.setattr(_lib, "_lib", real)
    # the C ABI refuses an overlap of two gradients before it launches anything: the buffers stay as they were
    b, c0, c1, cout, kh, kw, ht, wd = cases.SHAPES[4]
    work = _lib.workspace("conv2d_backward", t0, b, c0, c1, cout, kh, kw, ht, wd)
    gx0 = torch.full_like(t0, 7.0)
    with pytest.raises(_lib.RmdError, match="overlaps"):
        _lib.launch("rmd_conv2d_backward", t0, g, None, t0, t1, tw, gx0, torch.empty_like(t1), tw, None, work, b, c0, c1,
                    cout, kh, kw, ht, wd, 0)
    torch.cuda.synchronize()
    assert float((gx0 - 7.0).abs().max()) == 0.0
