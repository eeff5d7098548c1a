"""The fused dicl-1x1 cost on the GPU: csrc/dicl_match.hip through torch.ops.rmd.dicl_match_1x1, rmd.ops and
the dicl-1x1 module with fused="on", against the tests' float64 restatement (dicl_match_cases.py) on the
reference's three fixtures and the shape sweep in both compute modes, the fragment order on exact integer
data, column independence, views, determinism, opcheck, the no-host-synchronisation rule and argument checks.

Tolerance (dicl_match_cases.py): per case and mode max(1e-5, 3 e), e the error of the CPU float64 emulation
of the mode against float64 — never a figure of the kernel's.  The module tests compare with the fixture's
fp32 output by the same rule, plus 1e-6 for the reference's own fp32 composite (5.7e-7 from float64 on
these fixtures, test_dicl_match.py).  With dap=True, e is that of the whole chain against the float64 cost
through a float64 DAP: the emulated cost rounded to fp32, then an emulation of rmd_dap's own arithmetic
(a split-bf16 GEMM, hi.hi + hi.lo + lo.hi of the fp32 weight and input, dicl_match_cases.dap_emulate).

Every test here needs the operator: none can pass without the kernel."""

import numpy as np
import pytest
import torch

import dicl_match_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECISIONS = ("fp32", "bf16")
REFERENCE_FP32 = 1e-6
CASES = cases.all_cases()
MODELS_SHAPE = cases.SWEEP[2]       # C = 32, widths 96, 128, 64, r = 4: its own loops, several workgroups
GENERIC_SHAPE = cases.SWEEP[1]      # the guarded loops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(args, precision):
    from rmd import ops
    f1, f2, co, r, weights, biases = args
    out = ops.dicl_match_1x1(_t(f1), _t(f2), _t(co), r, [_t(w) for w in weights], [_t(t) for t in biases],
                             precision=precision)
    d = 2 * r + 1
    assert out.shape == (f1.shape[0], d, d) + f1.shape[-2:] and out.dtype == torch.float32 and out.is_contiguous()
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("label,get", CASES, ids=[c[0] for c in CASES])
def test_against_float64(label, get, precision):
    """The three fixtures, the sweep and the widest network: NaN positions identical (max_norm_err asserts
    it), finite values within max(1e-5, 3 e)."""
    c = get()
    err = cases.max_norm_err(_run(c["args"], precision).cpu().numpy(), c["ref"])
    print(f"{label} [{precision}]: kernel {err:.3e}  emulation e {c['e'][precision]:.3e}  tolerance {c['tol'][precision]:.3e}")
    assert err <= c["tol"][precision], (label, precision, err, c["tol"][precision])


def test_nan_fixture_poisons_exactly_two_pixels():
    c = cases.fixture_case(cases.NAN_FIXTURE)
    for precision in PRECISIONS:
        nan = np.isnan(_run(c["args"], precision).cpu().numpy())
        want = np.zeros_like(nan)
        for b, y, x in cases.NAN_PIXELS:
            want[b, :, :, y, x] = True
        assert np.array_equal(nan, want)


@pytest.mark.parametrize("shape", [MODELS_SHAPE, GENERIC_SHAPE, cases.WIDEST], ids=["models", "generic", "widest"])
def test_fragment_order_on_exact_integer_data(shape):
    """Small-integer features, weights and biases with coordinates on the grid: every product and sum is
    exact in bfloat16 operands and fp32 accumulators, so the kernel must equal the emulation bit for bit in
    both modes — a weight fragment in the wrong k order, or a swapped row, changes almost every output.
    The weights are sparse and asymmetric (activations stay below 2^8 for the one-product mode)."""
    b, c, h, w, r, widths = shape
    rng = np.random.default_rng(11)
    f1 = rng.integers(-1, 2, (b, c, h, w)).astype(np.float32)
    f2 = rng.integers(-1, 2, (b, c, h, w)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    co = (np.stack([xs, ys])[None] + rng.integers(-2, 3, (b, 2, h, w))).astype(np.float32)
    weights, biases, cin = [], [], 2 * c
    for cout in widths + (1,):
        wt = rng.integers(-1, 2, (cout, cin)) * (rng.random((cout, cin)) < 0.12)
        weights.append((wt + np.eye(cout, cin, k=3)).astype(np.float32))       # asymmetric
        biases.append(rng.integers(-2, 3, cout).astype(np.float32))
        cin = cout
    weights[3] = weights[3].reshape(-1)
    args = (f1, f2, co, r, weights, biases)
    ref = cases.reference64(*args)
    assert np.abs(ref).max() > 4 and len(np.unique(ref)) > 8          # not a degenerate network
    for precision, products in cases.PRODUCTS.items():
        want = cases.emulate(*args, products)
        if products == 3:
            assert np.array_equal(want, ref)                           # hi + lo holds every integer here
        assert np.array_equal(_run(args, precision).cpu().numpy().astype(np.float64), want), precision


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("dap", [True, False], ids=["dap", "nodap"])
@pytest.mark.parametrize("name", cases.FIXTURES)
def test_fused_module_against_the_fixture(name, dap, precision):
    from oracle.dicl import dap as dap64
    g, c = cases.fixture(name), cases.fixture_case(name)
    mod = cases.build_module(name, DEV, fused="on", precision=precision)
    seen = []
    mod.mnet.register_forward_hook(lambda m, i, o: seen.append((type(i[0]).__name__, o)))
    with torch.no_grad():
        out = mod(_t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"]), dap=dap)
    assert [s[0] for s in seen] == ["StackSpec"]                       # the hook fires once, on the fused path
    cost = seen[0][1].cpu().numpy()
    assert cases.max_norm_err(cost, c["ref"]) <= c["tol"][precision]
    tag = "dap" if dap else "nodap"
    ref, emu = c["ref"], cases.emulate(*c["args"], cases.PRODUCTS[precision])
    if dap:
        wt = mod.dap.conv1.weight.detach().cpu().numpy()
        with np.errstate(all="ignore"):
            ref, emu = dap64(ref, wt.astype(np.float64)), cases.dap_emulate(emu, wt)
    nan = np.isnan(ref)
    e = float(np.abs(emu[~nan] - ref[~nan]).max() / np.abs(ref[~nan]).max())
    tol = max(cases.FLOOR, cases.FACTOR * e) + REFERENCE_FP32
    err = cases.max_norm_err(out.cpu().numpy(), g[f"{tag}.out"])
    print(f"{name} {tag} [{precision}]: module {err:.3e}  e {e:.3e}  tolerance {tol:.3e}")
    assert out.shape == g[f"{tag}.out"].shape and err <= tol


def test_auto_takes_the_fused_path_without_grad_and_falls_back_with_it():
    name = cases.FIXTURES[0]
    g = cases.fixture(name)
    mod = cases.build_module(name, DEV, fused="auto")
    seen = []
    mod.mnet.register_forward_hook(lambda m, i, o: seen.append(type(i[0]).__name__))
    f1, f2, co = _t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"])
    with torch.no_grad():
        mod(f1, f2, co)
    out = mod(f1, f2, co)
    assert seen == ["StackSpec", "Tensor"] and out.requires_grad


@pytest.mark.parametrize("precision", PRECISIONS)
def test_column_independence(precision):
    """Poisoning one pixel's coordinate changes that pixel's outputs only; the rest is bitwise the same."""
    c = cases.sweep_case(MODELS_SHAPE)
    f1, f2, co, r, weights, biases = c["args"]
    base = _run(c["args"], precision)
    for b, y, x, v in ((0, 4, 7, np.nan), (0, 8, 18, np.inf), (0, 0, 0, 1e30)):
        co2 = co.copy()
        co2[b, 1, y, x] = v
        out = _run((f1, f2, co2, r, weights, biases), precision)
        same = torch.ones_like(out, dtype=torch.bool)
        same[b, :, :, y, x] = False
        assert torch.equal(out[same].view(torch.int32), base[same].view(torch.int32))
        if not np.isfinite(v):
            assert torch.isnan(out[b, :, :, y, x]).all()
        else:
            assert torch.equal(out[b, :, :, y, x], torch.full_like(out[b, :, :, y, x], float(out[b, 0, 0, y, x])))


@pytest.mark.parametrize("shape", [MODELS_SHAPE, GENERIC_SHAPE], ids=["models", "generic"])
def test_views_give_the_results_of_their_contiguous_copies(shape):
    """Permuted (non-contiguous) tensors and views at a storage offset, bitwise."""
    import rmd  # noqa: F401
    from rmd import _lib
    f1, f2, co, r, weights, biases = cases.sweep_case(shape)["args"]
    tf1, tf2, tco = _t(f1), _t(f2), _t(co)
    ws, ts = [_t(w) for w in weights], [_t(t) for t in biases]
    ref = torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco, r, ws, ts, _lib.RMD_BF16X3)

    def permuted(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if t.dim() == 4 else t.t().contiguous().t() if t.dim() == 2 else t

    def offset(t):
        return torch.zeros(t.numel() + 3, device=DEV)[3:].view_as(t).copy_(t)

    for view in (permuted, offset):
        got = torch.ops.rmd.dicl_match_1x1(view(tf1), view(tf2), view(tco), r, [view(w) for w in ws],
                                           [view(t) for t in ts], _lib.RMD_BF16X3)
        assert not view(tf1).is_contiguous() or view(tf1).storage_offset() == 3
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_runs_are_bitwise_equal(precision):
    for shape in (MODELS_SHAPE, cases.SWEEP[3]):
        a, b = (_run(cases.sweep_case(shape)["args"], precision) for _ in range(2))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_opcheck():
    import rmd  # noqa: F401
    from rmd import _lib
    f1, f2, co, r, weights, biases = cases.sweep_case(GENERIC_SHAPE)["args"]
    for compute in (_lib.RMD_BF16X3, _lib.RMD_BF16):
        torch.library.opcheck(torch.ops.rmd.dicl_match_1x1,
                              (_t(f1), _t(f2), _t(co), r, [_t(w) for w in weights], [_t(t) for t in biases], compute),
                              test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    out = torch.ops.rmd.dicl_match_1x1(_t(f1).requires_grad_(True), _t(f2), _t(co), r, [_t(w) for w in weights],
                                       [_t(t) for t in biases], _lib.RMD_BF16X3)
    assert not out.requires_grad


def test_the_fused_module_never_waits_for_the_host():
    name = cases.FIXTURES[1]            # mnet scale 0.5: the padding runs too
    g = cases.fixture(name)
    mod = cases.build_module(name, DEV, fused="on")
    f1, f2, co = _t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            mod(f1, f2, co)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd  # noqa: F401
    from rmd import _lib, ops
    f1, f2, co, r, weights, biases = cases.sweep_case(GENERIC_SHAPE)["args"]
    tf1, tf2, tco = _t(f1), _t(f2), _t(co)
    ws, ts = [_t(w) for w in weights], [_t(t) for t in biases]
    with pytest.raises(ValueError, match="unsupported on the GPU"):        # asks the library, launches nothing
        torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco, 5, ws, ts, _lib.RMD_BF16X3)
    with pytest.raises(ValueError, match="unsupported on the GPU"):
        torch.ops.rmd.dicl_match_1x1(tf1[:, :8], tf2[:, :8], tco, r, [ws[0][:, :16]] + ws[1:], ts, _lib.RMD_BF16X3)
    mod = rmd.corr.make_cmod("dicl-1x1", 24, 3, fused="on").to(DEV).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="unsupported shape"):
        mod(torch.zeros(1, 24, 4, 4, device=DEV), torch.zeros(1, 24, 4, 4, device=DEV), torch.zeros(1, 2, 4, 4, device=DEV))

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    cpu = torch.from_numpy
    bad = [
        lambda: torch.ops.rmd.dicl_match_1x1(tf1, cpu(f2), tco, r, ws, ts, _lib.RMD_BF16X3),           # a CPU fmap
        lambda: torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco, r, ws[:2] + [cpu(weights[2])] + ws[3:], ts,
                                             _lib.RMD_BF16X3),                                         # a list member
        lambda: torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco, r, ws, ts[:3] + [cpu(biases[3])], _lib.RMD_BF16),
    ]
    for fn in bad:
        with pytest.raises(ValueError, match="must be on the GPU"):
            fn()
    with pytest.raises(ValueError, match="different devices"):
        ops.dicl_match_1x1(tf1, tf2, cpu(co), r, ws, ts)
    with pytest.raises(ValueError, match="coords"):
        torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco[:, :, :-1], r, ws, ts, _lib.RMD_BF16X3)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco, r, ws, ts, _lib.RMD_F32)
