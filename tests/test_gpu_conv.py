"""The fused k x k convolutions on the GPU: csrc/conv.hip through torch.ops.rmd.conv2d_act, torch.ops.rmd.motion_encoder,
rmd_conv2d's slice writes and the drop-in modules with fused="on", against the tests' float64 restatement
(conv_cases.py) on the ten shapes in both compute modes and with both activations, one-hot weights against their
closed form, NaN and inf positions, the reference's fixtures, sample independence, repeatability, views, opcheck,
the no-host-synchronisation rule, the allocation bound and the argument checks.

Tolerance (conv_cases.py): per case and mode max(1e-5, 3 e), e the error of the CPU float64 emulation of the mode
(of the emulated chain for the modules) against float64 — never a figure of the kernel's.  Comparisons with a
fixture's fp32 output add 1e-6 for the reference's own fp32 composition, as test_gpu_gru.py.

Every test here calls the new operators: none can pass without the kernel."""

import numpy as np
import pytest
import torch

import conv_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECISIONS = ("fp32", "bf16")
REFERENCE_FP32 = 1e-6


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(args, act, precision):
    from rmd import ops
    x0, x1, weight, bias = args
    out = ops.conv2d_act(_t(x0), _t(x1), _t(weight), _t(bias), act=act, precision=precision)
    assert out.shape == (x0.shape[0], weight.shape[0]) + x0.shape[2:]
    assert out.dtype == torch.float32 and out.is_contiguous()
    return out


def _launch(args, act, precision, total, off, fill):
    """rmd_conv2d through the package's launch path into channels off .. off + Cout of a `total`-channel
    destination prefilled with `fill`."""
    import rmd  # noqa: F401
    from rmd import _lib, ops
    x0, x1, weight, bias = args
    b, c0, ht, wd = x0.shape
    cout, _, kh, kw = weight.shape
    c1 = 0 if x1 is None else x1.shape[1]
    t0, t1, tw, tb = _t(x0), _t(x1), _t(weight), _t(bias)
    out = torch.full((b, total, ht, wd), fill, device=DEV)
    work = _lib.workspace("conv2d", t0, c0, c1, cout, kh, kw)
    _lib.launch("rmd_conv2d", t0, t0, t1, tw, tb, out, work, b, c0, c1, cout, kh, kw, ht, wd, total, off,
                ops.CONV_ACTS[act], ops.CONV_PRECISIONS[precision])
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_against_float64(shape, act, precision):
    c = cases.shape_case(shape)
    err = cases.max_norm_err(_run(c["args"], act, precision).cpu().numpy(), c["ref"][act])
    print(f"{shape} [{act}, {precision}]: kernel {err:.3e}  emulation e {c['e'][act, precision]:.3e}  "
          f"tolerance {c['tol'][act, precision]:.3e}")
    assert err <= c["tol"][act, precision], (shape, act, precision, err, c["tol"][act, precision])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [cases.SHAPES[4], cases.SHAPES[5], cases.SHAPES[7]], ids=lambda s: "x".join(map(str, s)))
def test_a_slice_is_written_and_nothing_else(shape, precision):
    args = cases.shape_case(shape)["args"]
    cout = args[2].shape[0]
    sentinel = -12345.678
    whole = _launch(args, "relu", precision, cout, 0, sentinel)
    assert torch.equal(_bits(whole), _bits(_run(args, "relu", precision)))
    part = _launch(args, "relu", precision, cout + 5, 3, sentinel)
    assert torch.equal(_bits(part[:, 3:3 + cout]), _bits(whole))
    rest = torch.cat([part[:, :3], part[:, 3 + cout:]], dim=1)
    assert torch.equal(_bits(rest), _bits(torch.full_like(rest, sentinel)))


def test_one_hot_weights_give_the_shifted_channel():
    """A single W[o, c, i, j] = 1, no bias, no activation: output channel o is input channel c shifted by the tap,
    every other channel zero.  The inputs equal their bf16 hi + lo split exactly, so the split mode gives them back
    bitwise (hi . 1 + lo . 1 is exact) and the one-product mode their bf16 rounding.  A reversed tap, a wrong
    fragment order, a missed k-step, seam, padded tail or output tile moves the output by O(1)."""
    from dicl_match_cases import bf16_round
    from rmd import ops
    b, c0, c1, cout, ht, wd = cases.ONEHOT_SHAPE
    rng = np.random.default_rng(11)
    x = cases.exact_split(rng.standard_normal((b, c0 + c1, ht, wd)))
    t0, t1 = _t(x[:, :c0]), _t(x[:, c0:])
    bias = torch.zeros(cout, device=DEV)
    weights = {k: torch.zeros(cout, c0 + c1, k, k, device=DEV) for k in (3, 7)}
    want = {"fp32": x, "bf16": bf16_round(x)}
    for k, o, c, i, j in cases.onehot_cases():
        weights[k][o, c, i, j] = 1.0
        got = {p: ops.conv2d_act(t0, t1, weights[k], bias, precision=p).cpu().numpy() for p in PRECISIONS}
        weights[k][o, c, i, j] = 0.0
        for p in PRECISIONS:
            expected = np.zeros((b, cout, ht, wd), np.float32)
            expected[:, o] = cases.onehot_expected(want[p], k, c, i, j)
            assert np.array_equal(got[p].view(np.uint32), expected.view(np.uint32)), (k, o, c, i, j, p)
    print(f"one-hot: {len(cases.onehot_cases())} cases, both modes, bitwise")


def _poisoned(value):
    """flow and corr of a 14 x 16 map with one `value` each, away from the border."""
    rng = np.random.default_rng(5)
    flow = rng.standard_normal((1, 2, 14, 16)).astype(np.float32)
    corr = rng.standard_normal((1, 324, 14, 16)).astype(np.float32)
    flow[0, 1, 4, 5] = value
    corr[0, 200, 9, 10] = value
    return flow, corr


def test_nan_and_inf_positions():
    import rmd.raft
    from detinit import det_init_fanin
    from rmd import ops
    enc = det_init_fanin(rmd.raft.BasicUpdateBlock(324)).enc.eval()
    assert enc.fused == "off"
    ws, bs = cases.encoder_params()
    tw, tb = [_t(w) for w in ws], [_t(b) for b in bs]
    flow, corr = _poisoned(np.nan)
    with torch.no_grad():
        ref = np.isnan(enc(torch.from_numpy(flow), torch.from_numpy(corr)).numpy())
        ref1 = np.isnan(torch.relu(enc.convc2(torch.from_numpy(corr[:, :256]))).numpy())
    assert ref.any() and not ref.all() and ref1.any() and not ref1.all()
    for precision in PRECISIONS:
        out = ops.motion_encoder(_t(flow), _t(corr), tw, tb, precision=precision).cpu().numpy()
        assert np.array_equal(np.isnan(out), ref), precision
        # ReLU after a single convolution: fmaxf(NaN, 0) would be 0
        one = ops.conv2d_act(_t(corr[:, :256]), None, tw[1], tb[1], act="relu", precision=precision).cpu().numpy()
        assert np.array_equal(np.isnan(one), ref1), precision
    for value in (np.inf, -np.inf):
        flow, corr = _poisoned(value)
        out = ops.motion_encoder(_t(flow), _t(corr), tw, tb, precision="fp32").cpu().numpy()
        ref_inf = ref.copy()
        ref_inf[:, 126:] = False                         # the copied flow holds the inf itself
        assert np.array_equal(np.isnan(out), ref_inf), value
        one = ops.conv2d_act(_t(corr[:, :256]), None, tw[1], tb[1], act="relu", precision="fp32").cpu().numpy()
        assert np.array_equal(np.isnan(one), ref1), value


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_modules_match_the_fixtures(precision):
    import rmd.raft
    from detinit import det_init_fanin
    from oracle.heads import up8
    from rmd import ops
    products = cases.PRODUCTS[precision]

    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = det_init_fanin(rmd.raft.BasicUpdateBlock(324, gru_fused="on", gru_precision=precision, fused="on",
                                                   precision=precision)).eval()
    assert sorted(blk.state_dict().keys()) == sorted(g["keys"].tolist())
    enc_w, enc_b = cases.encoder_params()
    gru_w, gru_b = cases.module_params(blk.gru)
    head_w, head_b = cases.conv_params(blk.flow, ("conv1", "conv2"))

    def chain(p):
        m = cases.encoder_ref(g["flow"], g["corr"], enc_w, enc_b, p)
        h = cases.gru64(g["h"], np.concatenate([g["x"].astype(np.float64), m], axis=1), gru_w, gru_b, p)
        return m, h, cases.two_conv_ref(h, head_w, head_b, p)

    exact, emulated = chain(None), chain(products)
    # the motion features are compared with float64 itself, h_out and d with the fixture's fp32 results
    tols = [cases.tolerance(e, r)[1] + extra for e, r, extra in zip(emulated, exact, (0.0, REFERENCE_FP32, REFERENCE_FP32))]
    blk = blk.to(DEV)
    with torch.no_grad():
        m = blk.enc(_t(g["flow"]), _t(g["corr"]))
        h_out, d = blk(_t(g["h"]), _t(g["x"]), _t(g["corr"]), _t(g["flow"]))
    errs = [cases.max_norm_err(m.cpu().numpy(), exact[0]), cases.max_norm_err(h_out.cpu().numpy(), g["h_out"]),
            cases.max_norm_err(d.cpu().numpy(), g["d"])]
    print(f"block [{precision}]: motion / h_out / d errors {errs}  tolerances {tols}")
    assert all(e <= t for e, t in zip(errs, tols)), (errs, tols)

    g = cases.fixture(cases.UP8_FIXTURE)
    up = det_init_fanin(rmd.raft.Up8Network(g["hidden"].shape[1], fused="on", precision=precision)).eval()
    assert sorted(up.state_dict().keys()) == sorted(g["keys"].tolist())
    assert up.temperature == float(g["temperature"])
    ws, bs = cases.conv_params(up, ("conv1", "conv2"))
    mask_exact, mask_emulated = (cases.two_conv_ref(g["hidden"], ws, bs, p) for p in (None, products))
    tol_mask = cases.tolerance(mask_emulated, mask_exact)[1] + REFERENCE_FP32
    flow64 = g["flow"].astype(np.float64)
    tol_out = cases.tolerance(up8(mask_emulated, flow64, up.temperature), up8(mask_exact, flow64, up.temperature))[1] \
        + REFERENCE_FP32
    up = up.to(DEV)
    with torch.no_grad():
        mask = ops.conv2d_act(_t(g["hidden"]), None, up.conv1.weight, up.conv1.bias, "relu", precision)
        mask = ops.conv2d_act(mask, None, up.conv2.weight, up.conv2.bias, "none", precision)
        out = up(_t(g["hidden"]), _t(g["flow"]))
    errs = [cases.max_norm_err(mask.cpu().numpy(), g["mask"]), cases.max_norm_err(out.cpu().numpy(), g["out"])]
    print(f"up8 [{precision}]: mask / out errors {errs}  tolerances {[tol_mask, tol_out]}")
    assert errs[0] <= tol_mask and errs[1] <= tol_out, (errs, tol_mask, tol_out)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_samples_do_not_depend_on_the_batch_and_runs_repeat(precision):
    x0, x1, weight, bias = cases.shape_case(cases.BATCH_SHAPE)["args"]
    full = _run((x0, x1, weight, bias), "relu", precision)
    for i in range(x0.shape[0]):
        alone = _run((x0[i:i + 1], None, weight, bias), "relu", precision)
        assert torch.equal(_bits(alone), _bits(full[i:i + 1])), i
    for shape in (cases.BATCH_SHAPE, cases.SHAPES[4], cases.SHAPES[7]):
        a, b = (_run(cases.shape_case(shape)["args"], "none", precision) for _ in range(2))
        assert torch.equal(_bits(a), _bits(b)), shape


def test_views_give_the_results_of_their_contiguous_copies():
    """Permuted (non-contiguous) tensors and views at a storage offset, bitwise."""
    import rmd  # noqa: F401
    from rmd import _lib
    X3 = _lib.RMD_BF16X3

    def permuted(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if t.dim() == 4 else t

    def offset(t):
        return torch.zeros(t.numel() + 3, device=DEV)[3:].view_as(t).copy_(t)

    x0, x1, weight, bias = (_t(a) for a in cases.shape_case(cases.SHAPES[4])["args"])
    ref = torch.ops.rmd.conv2d_act(x0, x1, weight, bias, 1, X3)
    g = cases.fixture(cases.BLOCK_FIXTURE)
    ws, bs = cases.encoder_params()
    flow, corr, tw, tb = _t(g["flow"]), _t(g["corr"]), [_t(w) for w in ws], [_t(b) for b in bs]
    ref_enc = torch.ops.rmd.motion_encoder(flow, corr, tw, tb, X3)
    for view in (permuted, offset):
        assert not view(x0).is_contiguous() or view(x0).storage_offset() == 3
        got = torch.ops.rmd.conv2d_act(view(x0), view(x1), view(weight), view(bias), 1, X3)
        assert torch.equal(_bits(got), _bits(ref))
        got = torch.ops.rmd.motion_encoder(view(flow), view(corr), [view(w) for w in tw], [view(b) for b in tb], X3)
        assert torch.equal(_bits(got), _bits(ref_enc))


def test_opcheck():
    import rmd  # noqa: F401
    from rmd import _lib
    x0, x1, weight, bias = (_t(a) for a in cases.shape_case(cases.SHAPES[5])["args"])
    g = cases.fixture(cases.BLOCK_FIXTURE)
    ws, bs = cases.encoder_params()
    enc_args = (_t(g["flow"]), _t(g["corr"]), [_t(w) for w in ws], [_t(b) for b in bs])
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    for compute in (_lib.RMD_BF16X3, _lib.RMD_BF16):
        torch.library.opcheck(torch.ops.rmd.conv2d_act, (x0, x1, weight, bias, 1, compute), test_utils=utils)
        torch.library.opcheck(torch.ops.rmd.conv2d_act, (x0, None, weight[:, :20].contiguous(), bias, 0, compute),
                              test_utils=utils)
        torch.library.opcheck(torch.ops.rmd.motion_encoder, enc_args + (compute,), test_utils=utils)
    out = torch.ops.rmd.conv2d_act(x0.clone().requires_grad_(True), x1, weight, bias, 1, _lib.RMD_BF16X3)
    assert not out.requires_grad
    out = torch.ops.rmd.motion_encoder(enc_args[0], enc_args[1].clone().requires_grad_(True), *enc_args[2:],
                                       _lib.RMD_BF16X3)
    assert not out.requires_grad


def test_the_fused_modules_never_wait_for_the_host_and_stay_in_their_workspaces():
    """Sync-debug mode over one call of the fully fused update block and of Up8Network, then the operators' peak
    allocation: the output and the workspace of rmd_*_workspace_bytes, nothing else."""
    import rmd.raft
    from detinit import det_init_fanin
    from rmd import _lib
    g = cases.fixture(cases.BLOCK_FIXTURE)
    blk = det_init_fanin(rmd.raft.BasicUpdateBlock(324, gru_fused="on", fused="on")).eval().to(DEV)
    up = det_init_fanin(rmd.raft.Up8Network(128, fused="on")).eval().to(DEV)
    args = [_t(g[k]) for k in ("h", "x", "corr", "flow")]
    with torch.no_grad():
        h, d = blk(*args)                               # the warm-up call
        up(h, d)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            h, d = blk(*args)
            up(h, d)
    finally:
        torch.cuda.set_sync_debug_mode("default")

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        return peak, out.numel() * 4

    L = _lib.lib()
    x0, x1, weight, bias = (_t(a) for a in cases.shape_case(cases.SHAPES[4])["args"])
    _, c0, c1, cout, kh, kw, _, _ = cases.SHAPES[4]
    peak, out_bytes = peak_of(lambda: torch.ops.rmd.conv2d_act(x0, x1, weight, bias, 1, _lib.RMD_BF16X3))
    bound = out_bytes + L.rmd_conv2d_workspace_bytes(c0, c1, cout, kh, kw)
    assert peak <= bound + 2 * 512, (peak, bound)       # the allocator rounds each of the two blocks up to 512 bytes
    ws, bs = cases.encoder_params()
    tw, tb = [_t(w) for w in ws], [_t(b) for b in bs]
    peak, out_bytes = peak_of(lambda: torch.ops.rmd.motion_encoder(args[3], args[2], tw, tb, _lib.RMD_BF16X3))
    bound = out_bytes + L.rmd_motion_encoder_workspace_bytes(1, 324, 6, 10)
    assert peak <= bound + 2 * 512, (peak, bound)


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd.raft
    from rmd import _lib, ops
    X3 = _lib.RMD_BF16X3
    x0, x1, weight, bias = cases.shape_case(cases.SHAPES[5])["args"]
    t0, t1, tw, tb = _t(x0), _t(x1), _t(weight), _t(bias)
    g = cases.fixture(cases.BLOCK_FIXTURE)
    h, flow, corr = _t(g["h"]), _t(g["flow"]), _t(g["corr"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="autocast"):
            rmd.raft.BasicMotionEncoder(324, fused="on").to(DEV)(flow, corr)
        with pytest.raises(RuntimeError, match="autocast"):
            rmd.raft.FlowHead(fused="on").to(DEV)(h)
        with pytest.raises(RuntimeError, match="autocast"):
            rmd.raft.Up8Network(fused="on").to(DEV)(h, flow)
    with pytest.raises(RuntimeError, match="gradient"):
        rmd.raft.BasicMotionEncoder(324, fused="on").to(DEV)(flow, corr)
    with pytest.raises(RuntimeError, match="gradient"):
        rmd.raft.FlowHead(fused="on").to(DEV)(h)
    with pytest.raises(RuntimeError, match="gradient"):
        rmd.raft.Up8Network(fused="on").to(DEV)(h, flow)
    assert rmd.raft.BasicMotionEncoder(324, fused="auto").to(DEV)(flow, corr).requires_grad
    assert rmd.raft.FlowHead(fused="auto").to(DEV)(h).requires_grad     # the composition, which trains
    assert rmd.raft.Up8Network(fused="auto").to(DEV)(h, flow).requires_grad
    with torch.no_grad(), pytest.raises(RuntimeError, match="mixed_precision"):
        rmd.raft.Up8Network(mixed_precision=True, fused="on").to(DEV)(h, flow)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    cpu = torch.from_numpy
    ws, bs = cases.encoder_params()
    ew, eb = [_t(w) for w in ws], [_t(b) for b in bs]
    for fn in (lambda: torch.ops.rmd.conv2d_act(t0, cpu(x1), tw, tb, 0, X3),                    # a CPU map
               lambda: torch.ops.rmd.conv2d_act(t0, t1, cpu(weight), tb, 0, X3),
               lambda: torch.ops.rmd.conv2d_act(t0, t1, tw, cpu(bias), 1, _lib.RMD_BF16),
               lambda: torch.ops.rmd.motion_encoder(flow, cpu(g["corr"]), ew, eb, X3),
               lambda: torch.ops.rmd.motion_encoder(flow, corr, ew[:2] + [cpu(ws[2])] + ew[3:], eb, X3)):
        with pytest.raises(ValueError, match="must be on the GPU"):
            fn()
    with pytest.raises(ValueError, match="different devices"):
        ops.conv2d_act(t0, cpu(x1), tw, tb)
    with pytest.raises(ValueError, match="different devices"):
        ops.motion_encoder(flow, corr, ew, eb[:4] + [cpu(bs[4])])
    with pytest.raises(ValueError, match="odd"):                                                # an even kernel size
        torch.ops.rmd.conv2d_act(t0, t1, tw[:, :, :2].contiguous(), tb, 0, X3)
    with pytest.raises(ValueError, match="unsupported on the GPU"):                             # C0 + C1 > 512
        torch.ops.rmd.conv2d_act(torch.zeros(1, 500, 4, 4, device=DEV), torch.zeros(1, 13, 4, 4, device=DEV),
                                 torch.zeros(8, 513, 3, 3, device=DEV), torch.zeros(8, device=DEV), 0, X3)
    with pytest.raises(ValueError, match="weight must be"):                                     # not the inputs' channels
        torch.ops.rmd.conv2d_act(t0, None, tw, tb, 0, X3)
    with pytest.raises(ValueError, match="weights\\[3\\]"):
        torch.ops.rmd.motion_encoder(flow, corr, ew[:3] + [ew[1]] + ew[4:], eb, X3)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.conv2d_act(t0, t1, tw, tb, 0, _lib.RMD_F32)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.motion_encoder(flow, corr, ew, eb, _lib.RMD_F32)
