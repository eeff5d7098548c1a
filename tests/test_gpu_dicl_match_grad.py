"""The differentiable fused dicl-1x1 cost on the GPU: csrc/dicl_match_grad.hip through
torch.ops.rmd.dicl_match_1x1_train / dicl_match_1x1_backward, rmd.ops.dicl_match_1x1(differentiable=True) and
the dicl-1x1 module with fused="on", fused_backward=True, against the tests' float64 oracle
(dicl_match_grad_cases.py) on the gradient fixtures and the shape sweep.

Tolerance (dicl_match_grad_cases.py): per case and output max(1e-5, 3 e), e the error of the CPU float64
emulation of the kernel's roundings against float64, on a grad_cost that is zero on the ReLU-guarded columns
— never a figure of the kernel's.  The module tests compare with the reference's fp32 autograd gradients
under the largest of the case's ten tolerances plus 1e-6 for the reference's own fp32 composite: a raw
parameter's gradient mixes gW_l and gt_l through the batch-norm fold.

Every test here needs the operators: none can pass without the kernel."""

import ctypes

import numpy as np
import pytest
import torch

import dicl_match_cases as fwd
import dicl_match_grad_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
REFERENCE_FP32 = 1e-6
CASES = cases.all_cases()
MODELS_SHAPE = fwd.SWEEP[2]
GENERIC_SHAPE = fwd.SWEEP[1]
TRAIN_SHAPE = (6, 32, 48, 64, 4, (96, 128, 64))       # the 1/8 level of the models' training shape


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gradients(args, grad, needs=(True, True, True)):
    """The ten gradients (None for a skipped group) through rmd.ops and autograd: padding included."""
    from rmd import ops
    f1, f2, co, r, weights, biases = args
    tf1, tf2 = _t(f1).requires_grad_(needs[0]), _t(f2).requires_grad_(needs[1])
    ws, ts = [_t(w).requires_grad_(needs[2]) for w in weights], [_t(t).requires_grad_(needs[2]) for t in biases]
    out = ops.dicl_match_1x1(tf1, tf2, _t(co), r, ws, ts, differentiable=True)
    ins = [t for t in (tf1, tf2, *ws, *ts) if t.requires_grad]
    got = iter(torch.autograd.grad(out, ins, _t(grad)))
    flat = [next(got) if t.requires_grad else None for t in (tf1, tf2, *ws, *ts)]
    return dict(zip(cases.OUTPUTS, flat))


def _random_case(shape, seed=5):
    """Unguarded random inputs for the tests that compare the kernel with itself."""
    args = fwd.sweep_case(shape)["args"]
    b, _, h, w, r, _ = shape
    d = 2 * r + 1
    return args, np.random.default_rng(seed).standard_normal((b, d, d, h, w)).astype(np.float32)


@pytest.mark.parametrize("label,get", CASES, ids=[c[0] for c in CASES])
def test_against_float64(label, get):
    """Fixtures, sweep, the widest network and a shape with more work items than the grid: all ten
    outputs, NaN positions identical (max_norm_err asserts it), finite values within max(1e-5, 3 e)."""
    c = get()
    got = _gradients(c["args"], c["grad"])
    bad = []
    for k in cases.OUTPUTS:
        err = cases.max_norm_err(got[k].cpu().numpy().reshape(c["ref"][k].shape), c["ref"][k])
        print(f"{label} {k}: kernel {err:.3e}  emulation e {c['e'][k]:.3e}  tolerance {c['tol'][k]:.3e}")
        if not err <= c["tol"][k]:
            bad.append((k, err, c["tol"][k]))
    assert not bad, (label, bad)


def test_train_forward_is_bitwise_the_inference_operator():
    import rmd  # noqa: F401
    from rmd import _lib
    for shape in (MODELS_SHAPE, GENERIC_SHAPE):
        f1, f2, co, r, weights, biases = fwd.sweep_case(shape)["args"]
        a = (_t(f1), _t(f2), _t(co), r, [_t(w) for w in weights], [_t(t) for t in biases])
        want = torch.ops.rmd.dicl_match_1x1(*a, _lib.RMD_BF16X3)
        got = torch.ops.rmd.dicl_match_1x1_train(*a)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("shape", [MODELS_SHAPE, GENERIC_SHAPE, fwd.WIDEST], ids=["models", "generic", "widest"])
def test_fragment_order_on_exact_integer_data(shape):
    """Small-integer features, weights, biases and grad_cost with coordinates on the grid: every product
    and sum is exact, so every gradient must equal float64 bit for bit — a transposed fragment in the wrong
    k order, or a swapped row, changes almost every value."""
    b, c, h, w, r, widths = shape
    rng = np.random.default_rng(11)
    f1 = rng.integers(-1, 2, (b, c, h, w)).astype(np.float32)
    f2 = rng.integers(-1, 2, (b, c, h, w)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    co = (np.stack([xs, ys])[None] + rng.integers(-2, 3, (b, 2, h, w))).astype(np.float32)
    weights, biases, cin = [], [], 2 * c
    for cout in widths + (1,):
        wt = rng.integers(-1, 2, (cout, cin)) * (rng.random((cout, cin)) < 0.12)
        weights.append((wt + np.eye(cout, cin, k=3)).astype(np.float32))
        biases.append(rng.integers(-2, 3, cout).astype(np.float32))
        cin = cout
    weights[3] = weights[3].reshape(-1)
    d = 2 * r + 1
    grad = rng.integers(-2, 3, (b, d, d, h, w)).astype(np.float32)
    args = (f1, f2, co, r, weights, biases)
    ref = cases._outputs(args, grad, False)
    emu = cases._outputs(args, grad, True)
    got = _gradients(args, grad)
    for k in cases.OUTPUTS:
        assert np.array_equal(emu[k], ref[k]), k                        # exact data: the emulation is float64
        assert np.abs(ref[k]).max() > 2, k                              # not a degenerate network
        assert np.array_equal(got[k].cpu().numpy().astype(np.float64).reshape(ref[k].shape), ref[k]), k


def test_one_hot_grad_cost_localises_the_gradients():
    shape = MODELS_SHAPE
    args, _ = _random_case(shape)
    b, c, h, w, r, _ = shape
    f1, f2, co = args[:3]
    co = co.copy()
    y, x, a, bb = 4, 7, 5, 3
    co[0, :, y, x] = (6.25, 3.5)                      # the sample (6.25 + a - r, 3.5 + bb - r) lies inside the map
    grad = np.zeros((b, 2 * r + 1, 2 * r + 1, h, w), np.float32)
    grad[0, a, bb, y, x] = 1.5
    got = _gradients((f1, f2, co) + args[3:], grad)
    g1, g2 = got["grad_fmap1"].cpu().numpy(), got["grad_fmap2"].cpu().numpy()
    assert np.abs(g1[0, :, y, x]).max() > 0
    g1[0, :, y, x] = 0
    assert not g1.any()
    px, py = 6.25 + a - r, 3.5 + bb - r
    taps = {(int(np.floor(py)) + dy, int(np.floor(px)) + dx) for dy in (0, 1) for dx in (0, 1)}
    hit = {(int(yy), int(xx)) for yy, xx in zip(*np.nonzero(np.abs(g2[0]).max(axis=0)))}
    assert hit and hit <= taps and not g2[1:].any()


@pytest.mark.parametrize("dap", [True, False], ids=["dap", "nodap"])
@pytest.mark.parametrize("name", cases.FIXTURES)
def test_fused_module_against_the_gradient_fixture(name, dap):
    """fused="on", fused_backward=True: the gradients of fmap1, fmap2 and every raw parameter (the DAP
    weight too) against the reference's autograd; the forward hook fires once, on the fused path."""
    g, c = cases.fixture(name), cases.fixture_case(name)
    mod = cases.build_module(name, DEV, fused="on", fused_backward=True)
    seen = []
    handle = mod.mnet.register_forward_hook(lambda m, i, o: seen.append(type(i[0]).__name__))
    got, calls = cases.module_gradients(mod, g, dap, DEV)
    handle.remove()
    assert seen == ["StackSpec"] and len(calls) == 1
    tag = "dap" if dap else "nodap"
    tol = max(c["tol"].values()) + REFERENCE_FP32
    keys = [k[len(tag) + 6:] for k in g if k.startswith(tag + ".grad.")]
    assert "fmap1" in keys and "fmap2" in keys and len(keys) >= 7 and (not dap or "dap.conv1.weight" in keys)
    bad = []
    for k in keys:
        want = g[f"{tag}.grad.{k}"]
        if name == cases.NAN_FIXTURE:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want)), k
            continue
        err = cases.max_norm_err(got[k], want)
        print(f"{name} {tag} {k}: module {err:.3e}  tolerance {tol:.3e}")
        if not err <= tol:
            bad.append((k, err))
    assert not bad, (tol, bad)


def test_nan_fixture_positions():
    """NaN positions identical to the float64 oracle's on every output (the fixture's are compared in
    test_fused_module_against_the_gradient_fixture)."""
    c = cases.fixture_case(cases.NAN_FIXTURE)
    got = _gradients(c["args"], c["grad"])
    for k in cases.OUTPUTS:
        assert np.array_equal(np.isnan(got[k].cpu().numpy().reshape(c["ref"][k].shape)), np.isnan(c["ref"][k])), k
    assert np.isnan(c["ref"]["gW2"]).all() and np.isfinite(c["ref"]["grad_fmap1"]).all()


def test_needs_grad_selection():
    """A skipped group comes back as None and leaves the others bitwise unchanged (grad_fmap2: float
    atomics, compared by the tolerance of two runs of itself)."""
    args, grad = _random_case(GENERIC_SHAPE)
    full = _gradients(args, grad)
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = _gradients(args, grad, needs)
        groups = [needs[0], needs[1]] + [needs[2]] * 8
        for k, need in zip(cases.OUTPUTS, groups):
            if not need:
                assert got[k] is None, (needs, k)
            elif k in cases.DETERMINISTIC:
                assert torch.equal(got[k].view(torch.int32), full[k].view(torch.int32)), (needs, k)
            else:
                assert torch.allclose(got[k], full[k], rtol=0, atol=1e-5 * float(full[k].abs().max())), (needs, k)


def test_views_give_the_results_of_their_contiguous_copies():
    import rmd  # noqa: F401
    args, grad = _random_case(MODELS_SHAPE)
    f1, f2, co, r, weights, biases = args
    tg, tf1, tf2, tco = _t(grad), _t(f1), _t(f2), _t(co)
    ws, ts = [_t(w) for w in weights], [_t(t) for t in biases]
    ref = torch.ops.rmd.dicl_match_1x1_backward(tg, tf1, tf2, tco, r, ws, ts, [True, True, True])

    def permuted(t):
        if t.dim() == 5:
            return t.permute(0, 3, 4, 1, 2).contiguous().permute(0, 3, 4, 1, 2)
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if t.dim() == 4 else t.t().contiguous().t() if t.dim() == 2 else t

    def offset(t):
        return torch.zeros(t.numel() + 3, device=DEV)[3:].view_as(t).copy_(t)

    for view in (permuted, offset):
        got = torch.ops.rmd.dicl_match_1x1_backward(view(tg), view(tf1), view(tf2), view(tco), r, [view(w) for w in ws],
                                                    [view(t) for t in ts], [True, True, True])
        assert not view(tg).is_contiguous() or view(tg).storage_offset() == 3
        for k, a, b in zip(cases.OUTPUTS, got, ref):
            if k in cases.DETERMINISTIC:
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
            else:
                assert torch.allclose(a, b, rtol=0, atol=1e-5 * float(b.abs().max())), k


def test_two_runs_are_bitwise_equal():
    """Every output declared deterministic (include/rmd.h): all but grad_fmap2."""
    for shape in (MODELS_SHAPE, fwd.SWEEP[3], cases.MORE_THAN_GRID):
        args, grad = _random_case(shape)
        a, b = (_gradients(args, grad) for _ in range(2))
        for k in cases.DETERMINISTIC:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (shape, k)


def test_opcheck():
    import rmd  # noqa: F401
    f1, f2, co, r, weights, biases = fwd.sweep_case(GENERIC_SHAPE)["args"]
    _, grad = _random_case(GENERIC_SHAPE)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    a = (_t(f1).requires_grad_(True), _t(f2).requires_grad_(True), _t(co), r,
         [_t(w).requires_grad_(True) for w in weights], [_t(t).requires_grad_(True) for t in biases])
    torch.library.opcheck(torch.ops.rmd.dicl_match_1x1_train, a, test_utils=utils)
    b = (_t(grad), _t(f1), _t(f2), _t(co), r, [_t(w) for w in weights], [_t(t) for t in biases])
    for needs in ([True, True, True], [False, True, False]):
        torch.library.opcheck(torch.ops.rmd.dicl_match_1x1_backward, b + (needs,), test_utils=utils)
    assert torch.ops.rmd.dicl_match_1x1_train(*a).requires_grad


def test_forward_and_backward_never_wait_for_the_host():
    name = cases.FIXTURES[1]            # mnet scale 0.5: the padding runs too
    g = cases.fixture(name)
    mod = cases.build_module(name, DEV, fused="on", fused_backward=True)
    f1, f2, co = _t(g["fmap1"]).requires_grad_(True), _t(g["fmap2"]).requires_grad_(True), _t(g["coords"])
    go = _t(g["dap.grad_out"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mod(f1, f2, co).backward(go)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert f1.grad is not None and mod.mnet[0][0].weight.grad is not None


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd  # noqa: F401
    from rmd import _lib, ops
    args, grad = _random_case(GENERIC_SHAPE)
    f1, f2, co, r, weights, biases = args
    tg, tf1, tf2, tco = _t(grad), _t(f1), _t(f2), _t(co)
    ws, ts = [_t(w) for w in weights], [_t(t) for t in biases]
    all3 = [True, True, True]
    with pytest.raises(ValueError, match="unsupported on the GPU"):        # asks the library, launches nothing
        torch.ops.rmd.dicl_match_1x1_backward(torch.zeros(2, 11, 11, 5, 7, device=DEV), tf1, tf2, tco, 5, ws, ts, all3)
    # the C entry point: the one-product mode, a partial set of parameter gradients and a bad shape are
    # refused with their codes and nothing is written
    lib = _lib.lib()
    c1, c2, c3 = (w.shape[0] for w in weights[:3])
    work = _lib.workspace("dicl_match_1x1_backward", tf1, 2, 16, 5, 7, r, c1, c2, c3)
    outs = [torch.full_like(t, 7.0) for t in (tf1, tf2, ws[0], ts[0], ws[1], ts[1], ws[2], ts[2], ws[3], ts[3])]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(compute=_lib.RMD_BF16X3, radius=r, drop=None, ch=16):
        o = [None if i == drop else t for i, t in enumerate(outs)]
        return lib.rmd_dicl_match_1x1_backward(p(tg), p(tf1), p(tf2), p(tco), 2, ch, 5, 7, radius, p(ws[0]), p(ts[0]),
                                               p(ws[1]), p(ts[1]), p(ws[2]), p(ts[2]), p(ws[3]), c1, c2, c3, compute,
                                               *[p(t) for t in o], p(work), _lib.stream_ptr(tf1.device))

    assert call(compute=_lib.RMD_BF16) == -1 and b"RMD_BF16X3" in lib.rmd_last_error()
    assert call(drop=5) == -1 and b"all given or all NULL" in lib.rmd_last_error()
    assert call(radius=5) != 0 and call(ch=24) != 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    cpu = torch.from_numpy
    with pytest.raises(ValueError, match="must be on the GPU"):
        torch.ops.rmd.dicl_match_1x1_backward(tg, tf1, cpu(f2), tco, r, ws, ts, all3)
    with pytest.raises(ValueError, match="must be on the GPU"):
        torch.ops.rmd.dicl_match_1x1_train(tf1, tf2, tco, r, ws[:2] + [cpu(weights[2])] + ws[3:], ts)
    with pytest.raises(ValueError, match="grad must be"):
        torch.ops.rmd.dicl_match_1x1_backward(tg[:, :-1], tf1, tf2, tco, r, ws, ts, all3)
    with pytest.raises(ValueError, match="needs_grad"):
        torch.ops.rmd.dicl_match_1x1_backward(tg, tf1, tf2, tco, r, ws, ts, [True, True])
    with pytest.raises(ValueError, match="coords"):
        torch.ops.rmd.dicl_match_1x1_train(tf1, tf2, tco[:, :, :-1], r, ws, ts)
    with pytest.raises(ValueError, match="no backward"):
        ops.dicl_match_1x1(tf1, tf2, tco, r, ws, ts, precision="bf16", differentiable=True)


def test_backward_at_the_models_shape_holds_nothing_as_large_as_the_stack():
    """Forward kept for backward, then the backward, at the 1/8 level of the training shape: the peak
    above what is live before the call stays below the stack's bytes (B, 9, 9, 2C, h, w) fp32."""
    import rmd
    b, c, h, w, r, _ = TRAIN_SHAPE
    mod = rmd.corr.make_cmod("dicl-1x1", c, r, fused="on", fused_backward=True).to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(3)
    f1 = torch.randn(b, c, h, w, device=DEV, generator=gen).requires_grad_(True)
    f2 = torch.randn(b, c, h, w, device=DEV, generator=gen).requires_grad_(True)
    ys, xs = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
    co = (torch.stack([xs, ys]).float()[None] + torch.randn(b, 2, h, w, device=DEV, generator=gen)).contiguous()
    stack_bytes = b * (2 * r + 1) ** 2 * 2 * c * h * w * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = mod(f1, f2, co, dap=False)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    print(f"peak above the inputs {delta / 1e6:.1f} MB, stack {stack_bytes / 1e6:.1f} MB")
    assert delta < stack_bytes and bool(torch.isfinite(f1.grad).all()) and bool(torch.isfinite(f2.grad).all())
