"""The fused SepConvGRU on the GPU: csrc/gru.hip through torch.ops.rmd.sepconv_gru, rmd_sepconv_gru_half and the
drop-in modules with fused="on", against the tests' float64 restatement (gru_cases.py) on the seven shapes in
both compute modes, the reference's fixtures, NaN positions, one-hot weights against their closed form, sample
independence, repeatability, views, opcheck, the no-host-synchronisation rule, argument checks and the
allocation bound.

Tolerance (gru_cases.py): per case and mode max(1e-5, 3 e), e the error of the CPU float64 emulation of the
mode against float64 — never a figure of the kernel's.  The module tests compare with the fixture's fp32
output by the same rule, plus 1e-6 for the reference's own fp32 composition (3.0e-7 from float64 on these
fixtures, test_gru.py).

Every test here needs the operator: none can pass without the kernel."""

import copy

import numpy as np
import pytest
import torch

import gru_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECISIONS = ("fp32", "bf16")
REFERENCE_FP32 = 1e-6
MODELS_SHAPE, TILES_SHAPE = cases.SHAPES[0], cases.SHAPES[5]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(args, precision):
    from rmd import ops
    h, x, ws, bs = args
    out = ops.sepconv_gru(_t(h), _t(x), [_t(w) for w in ws], [_t(b) for b in bs], precision=precision)
    assert out.shape == h.shape and out.dtype == torch.float32 and out.is_contiguous()
    return out


def _run_half(args, axis, precision):
    """rmd_sepconv_gru_half through the package's launch path: gates 3 axis .. 3 axis + 2."""
    import rmd  # noqa: F401
    from rmd import _lib, library, ops
    h, x, ws, bs = args
    th, tx = _t(h), _t(x)
    tw, tb = [_t(w) for w in ws[3 * axis:3 * axis + 3]], [_t(b) for b in bs[3 * axis:3 * axis + 3]]
    b, hd, ht, wd = h.shape
    work = _lib.workspace("sepconv_gru", th, b, hd, x.shape[1], ht, wd)
    out = torch.empty_like(th)
    _lib.launch("rmd_sepconv_gru_half", th, th, tx, library._pointers(tw), library._pointers(tb), out, work, b, hd,
                x.shape[1], ht, wd, axis, ops.GRU_PRECISIONS[precision])
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=[repr(s) for s in cases.SHAPES])
def test_against_float64(shape, precision):
    """Both halves together, and each axis alone through rmd_sepconv_gru_half."""
    c = cases.shape_case(shape)
    err = cases.max_norm_err(_run(c["args"], precision).cpu().numpy(), c["ref"])
    print(f"{shape} [{precision}]: kernel {err:.3e}  emulation e {c['e'][precision]:.3e}  tolerance {c['tol'][precision]:.3e}")
    assert err <= c["tol"][precision], (shape, precision, err, c["tol"][precision])
    for axis in (0, 1):
        err = cases.max_norm_err(_run_half(c["args"], axis, precision).cpu().numpy(), c["ref_half"][axis])
        print(f"{shape} [{precision}] axis {axis}: kernel {err:.3e}  tolerance {c['tol_half'][precision][axis]:.3e}")
        assert err <= c["tol_half"][precision][axis], (shape, precision, axis, err)


def _module_tolerance(h, x, ws, bs, precision):
    ref = cases.gru64(h, x, ws, bs)
    e = cases.max_norm_err(cases.gru64(h, x, ws, bs, cases.PRODUCTS[precision]), ref)
    return max(cases.FLOOR, cases.FACTOR * e) + REFERENCE_FP32


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_modules_match_the_fixtures(precision):
    import rmd.raft
    from detinit import det_init_fanin
    for name in (cases.FIXTURE,) + cases.NAN_FIXTURES:
        g = cases.fixture(name)
        mod = det_init_fanin(rmd.raft.SepConvGru(g["h"].shape[1], g["x"].shape[1], fused="on", precision=precision))
        ws, bs = cases.module_params(mod)
        with torch.no_grad():
            out = mod.eval().to(DEV)(_t(g["h"]), _t(g["x"])).cpu().numpy()
        err = cases.max_norm_err(out, g["out"])             # asserts identical NaN positions
        assert err <= _module_tolerance(g["h"], g["x"], ws, bs, precision), (name, precision, err)
    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = det_init_fanin(rmd.raft.BasicUpdateBlock(324, gru_fused="on", gru_precision=precision)).eval()
    with torch.no_grad():
        x = torch.cat((torch.from_numpy(g["x"]), blk.enc(torch.from_numpy(g["flow"]), torch.from_numpy(g["corr"]))), 1)
        ws, bs = cases.module_params(blk.gru)
        tol = _module_tolerance(g["h"], x.numpy(), ws, bs, precision)
        # the flow delta's e: the float64 flow head on the emulated hidden state against it on the exact one
        head = copy.deepcopy(blk.flow).double()
        d_ref, d_emu = (head(torch.from_numpy(cases.gru64(g["h"], x.numpy(), ws, bs, p))).numpy()
                        for p in (None, cases.PRODUCTS[precision]))
        tol_d = max(cases.FLOOR, cases.FACTOR * cases.max_norm_err(d_emu, d_ref)) + REFERENCE_FP32
        h_out, d = blk.to(DEV)(_t(g["h"]), _t(g["x"]), _t(g["corr"]), _t(g["flow"]))
    assert cases.max_norm_err(h_out.cpu().numpy(), g["h_out"]) <= tol
    assert cases.max_norm_err(d.cpu().numpy(), g["d"]) <= tol_d


def test_nan_positions_are_the_fixtures():
    ws, bs = cases.fixture_params(32, 16)
    for name in cases.NAN_FIXTURES:
        g = cases.fixture(name)
        for precision in PRECISIONS:
            nan = np.isnan(_run((g["h"], g["x"], ws, bs), precision).cpu().numpy())
            assert np.array_equal(nan, np.isnan(g["out"])), (name, precision)


def test_infinity_gives_nan_in_the_split_mode():
    """The one documented deviation: inf - inf in the residual."""
    g = cases.fixture(cases.NAN_FIXTURES[1])
    ws, bs = cases.fixture_params(32, 16)
    h = np.where(np.isnan(g["h"]), np.float32(np.inf), g["h"])
    x = np.where(np.isnan(g["x"]), np.float32(np.inf), g["x"])
    out = _run((h, x, ws, bs), "fp32").cpu().numpy()
    assert np.array_equal(np.isnan(out), np.isnan(g["out"]))


def test_one_hot_weights_give_the_closed_form():
    """A single (gate, output channel, input channel, tap) set to 1, everything else 0: a reversed tap, a wrong
    fragment order, a missed k-step or seam, or a q that reads h instead of r.h moves the output by O(0.1).
    The inputs equal their bf16 hi + lo split exactly, so the split mode carries them without rounding and the
    closed form holds to the fp32 epilogue's rounding: 1e-6."""
    from rmd import ops
    b, hd, xd, ht, wd = cases.ONEHOT_SHAPE
    rng = np.random.default_rng(7)
    h = cases.exact_split(np.tanh(rng.standard_normal((b, hd, ht, wd))))
    x = cases.exact_split(np.maximum(rng.standard_normal((b, xd, ht, wd)), 0))
    th, tx = _t(h), _t(x)
    ws = [torch.zeros((hd, hd + xd, 1, 5) if g < 3 else (hd, hd + xd, 5, 1), device=DEV) for g in range(6)]
    bs = [torch.zeros(hd, device=DEV) for _ in range(6)]
    worst = 0.0
    for gate, cout, cin, tap in cases.onehot_cases():
        ws[gate].view(hd, hd + xd, 5)[cout, cin, tap] = 1.0
        out = ops.sepconv_gru(th, tx, ws, bs).cpu().numpy()
        ws[gate].view(hd, hd + xd, 5)[cout, cin, tap] = 0.0
        err = float(np.abs(out - cases.onehot_expected(h, x, gate, cout, cin, tap)).max())
        worst = max(worst, err)
        assert err <= 1e-6, (gate, cout, cin, tap, err)
    print(f"one-hot: worst {worst:.3e} over {len(cases.onehot_cases())} cases")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_samples_do_not_depend_on_the_batch(precision):
    h, x, ws, bs = cases.shape_case(TILES_SHAPE)["args"]
    full = _run((h, x, ws, bs), precision)
    for i in range(h.shape[0]):
        alone = _run((h[i:i + 1], x[i:i + 1], ws, bs), precision)
        assert torch.equal(alone.view(torch.int32), full[i:i + 1].view(torch.int32)), i


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_runs_are_bitwise_equal(precision):
    for shape in (MODELS_SHAPE, TILES_SHAPE):
        a, b = (_run(cases.shape_case(shape)["args"], precision) for _ in range(2))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_views_give_the_results_of_their_contiguous_copies():
    """Permuted (non-contiguous) tensors and views at a storage offset, bitwise."""
    import rmd  # noqa: F401
    from rmd import _lib
    h, x, ws, bs = cases.shape_case(cases.SHAPES[3])["args"]
    th, tx, tw, tb = _t(h), _t(x), [_t(w) for w in ws], [_t(b) for b in bs]
    ref = torch.ops.rmd.sepconv_gru(th, tx, tw, tb, _lib.RMD_BF16X3)

    def permuted(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if t.dim() == 4 else t

    def offset(t):
        return torch.zeros(t.numel() + 3, device=DEV)[3:].view_as(t).copy_(t)

    for view in (permuted, offset):
        got = torch.ops.rmd.sepconv_gru(view(th), view(tx), [view(w) for w in tw], [view(b) for b in tb],
                                        _lib.RMD_BF16X3)
        assert not view(th).is_contiguous() or view(th).storage_offset() == 3
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_opcheck():
    import rmd  # noqa: F401
    from rmd import _lib
    h, x, ws, bs = cases.shape_case(cases.SHAPES[2])["args"]
    args = (_t(h), _t(x), [_t(w) for w in ws], [_t(b) for b in bs])
    for compute in (_lib.RMD_BF16X3, _lib.RMD_BF16):
        torch.library.opcheck(torch.ops.rmd.sepconv_gru, args + (compute,),
                              test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    out = torch.ops.rmd.sepconv_gru(args[0].clone().requires_grad_(True), *args[1:], _lib.RMD_BF16X3)
    assert not out.requires_grad


def test_the_fused_block_never_waits_for_the_host_and_stays_in_its_workspace():
    """Sync-debug mode over one call of the update block, then the operator's peak allocation: the output and the
    workspace of rmd_sepconv_gru_workspace_bytes, nothing else."""
    import rmd.raft
    from rmd import _lib
    from detinit import det_init_fanin
    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = det_init_fanin(rmd.raft.BasicUpdateBlock(324, gru_fused="on")).eval().to(DEV)
    args = [_t(g[k]) for k in ("h", "x", "corr", "flow")]
    with torch.no_grad():
        blk(*args)                                      # MIOpen picks its algorithms outside the checked call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            blk(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")

    h, x, ws, bs = cases.shape_case(TILES_SHAPE)["args"]
    th, tx, tw, tb = _t(h), _t(x), [_t(w) for w in ws], [_t(b) for b in bs]
    b, hd, ht, wd = h.shape
    bound = th.numel() * 4 + _lib.lib().rmd_sepconv_gru_workspace_bytes(b, hd, x.shape[1], ht, wd)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = torch.ops.rmd.sepconv_gru(th, tx, tw, tb, _lib.RMD_BF16X3)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    assert peak <= bound + 2 * 512, (peak, bound)       # the allocator rounds each of the two blocks up to 512 bytes


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd.raft
    from rmd import _lib, ops
    h, x, ws, bs = cases.shape_case(cases.SHAPES[2])["args"]
    th, tx, tw, tb = _t(h), _t(x), [_t(w) for w in ws], [_t(b) for b in bs]
    with pytest.raises(ValueError, match="unsupported on the GPU"):        # asks the library, launches nothing
        torch.ops.rmd.sepconv_gru(th[:, :24], tx[:, :16], [w[:24, :40] for w in tw], [b[:24] for b in tb], _lib.RMD_BF16X3)
    mod = rmd.raft.SepConvGru(24, 16, fused="on").to(DEV).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="unsupported widths"):
        mod(torch.zeros(1, 24, 4, 4, device=DEV), torch.zeros(1, 16, 4, 4, device=DEV))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(RuntimeError, match="autocast"):
        rmd.raft.SepConvGru(32, 48, fused="on").to(DEV)(th, tx)
    with pytest.raises(RuntimeError, match="gradient"):
        rmd.raft.SepConvGru(32, 48, fused="on").to(DEV)(th, tx)
    auto = rmd.raft.SepConvGru(32, 48, fused="auto").to(DEV)
    assert auto(th, tx).requires_grad                     # falls back to the composition, which trains

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    cpu = torch.from_numpy
    bad = [
        lambda: torch.ops.rmd.sepconv_gru(th, cpu(x), tw, tb, _lib.RMD_BF16X3),                     # a CPU map
        lambda: torch.ops.rmd.sepconv_gru(th, tx, tw[:2] + [cpu(ws[2])] + tw[3:], tb, _lib.RMD_BF16X3),
        lambda: torch.ops.rmd.sepconv_gru(th, tx, tw, tb[:5] + [cpu(bs[5])], _lib.RMD_BF16),
    ]
    for fn in bad:
        with pytest.raises(ValueError, match="must be on the GPU"):
            fn()
    with pytest.raises(ValueError, match="different devices"):
        ops.sepconv_gru(th, cpu(x), tw, tb)
    with pytest.raises(ValueError, match="weights\\[4\\]"):
        torch.ops.rmd.sepconv_gru(th, tx, tw[:4] + [tw[0]] + tw[5:], tb, _lib.RMD_BF16X3)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.sepconv_gru(th, tx, tw, tb, _lib.RMD_F32)
