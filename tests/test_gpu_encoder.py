"""The fused feature / context encoder on the GPU: csrc/encoder.hip through torch.ops.rmd.conv2d_norm_act,
instance_norm_stats, residual_join and feature_encoder and the drop-in modules with fused="on", against the tests'
float64 restatement (encoder_cases.py) and the float64 output of the reference's fixtures: the strided convolution
on ten shapes (the issue's six and four for the kernel's other paths) in both compute modes and with both
activations, one-hot weights at stride 2 and the load transform
against their closed forms, the statistics' accuracy, the join, the whole encoder and a residual block alone,
sample independence, repeatability, NaN, views, opcheck, the no-host-synchronisation rule, the allocation bound and
the argument checks.

Tolerance (encoder_cases.py): per case and mode max(1e-5, 3 e), e the error of the CPU float64 emulation of the mode
(of the emulated chain for the modules) against float64 — never a figure of the kernel's.  The encoder is compared
with the fixtures' float64 output, not their fp32 one: the reference's own fp32 run is 0.6 - 1.1e-6 from float64
there.  The statistics are held to 1e-5 on relu(x a + d) against the float64 instance norm; on the N(100, 1) input
exact statistics rounded to fp32 are at 2.8e-6 and a one-pass fp32 sum of squares is at 4.2e-4.

Every test here calls the new operators: none can pass without the kernels."""

import numpy as np
import pytest
import torch

import encoder_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECISIONS = ("fp32", "bf16")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(c, act, precision):
    from rmd import ops
    x, scale, shift, weight, bias, residual = c["args"]
    out = ops.conv2d_norm_act(_t(x), _t(weight), _t(bias), scale=_t(scale), shift=_t(shift), residual=_t(residual),
                              stride=c["stride"], act=act, precision=precision)
    assert out.shape == c["ref"][act].shape and out.dtype == torch.float32 and out.is_contiguous()
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("shape,transformed", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_strided_convolution_against_float64(shape, transformed, act, precision):
    c = cases.shape_case(shape, transformed)
    err = cases.max_norm_err(_run(c, act, precision).cpu().numpy(), c["ref"][act])
    print(f"{shape} [{act}, {precision}]: kernel {err:.3e}  emulation e {c['e'][act, precision]:.3e}  "
          f"tolerance {c['tol'][act, precision]:.3e}")
    assert err <= c["tol"][act, precision], (shape, act, precision, err, c["tol"][act, precision])


def test_one_hot_weights_at_stride_2_give_the_subsampled_channel():
    """A single W[o, c, i, j] = 1, no bias, no activation: output channel o is input channel c read at
    (2 y + i - k/2, 2 x + j - k/2), every other channel zero.  The inputs equal their bf16 hi + lo split exactly, so
    the split mode gives them back bitwise and the one-product mode their bf16 rounding.  A wrong column plane, a
    reversed tap, a missed k-step or output tile moves the output by O(1)."""
    from rmd import ops
    b, c, cout, ht, wd = cases.ONEHOT_SHAPE
    rng = np.random.default_rng(12)
    x = cases.exact_split(rng.standard_normal((b, c, ht, wd)))
    tx = _t(x)
    bias = torch.zeros(cout, device=DEV)
    weights = {k: torch.zeros(cout, c, k, k, device=DEV) for k in (3, 7)}
    want = {"fp32": x, "bf16": cases.bf16_round(x)}
    for k, o, cin, i, j in cases.onehot_cases():
        weights[k][o, cin, i, j] = 1.0
        got = {p: ops.conv2d_norm_act(tx, weights[k], bias, stride=2, precision=p).cpu().numpy() for p in PRECISIONS}
        weights[k][o, cin, i, j] = 0.0
        for p in PRECISIONS:
            expected = np.zeros((b, cout, cases.out_side(ht, 2), cases.out_side(wd, 2)), np.float32)
            expected[:, o] = cases.onehot_expected(want[p], k, cin, i, j)
            assert np.array_equal(got[p].view(np.uint32), expected.view(np.uint32)), (k, o, cin, i, j, p)
    print(f"one-hot at stride 2: {len(cases.onehot_cases())} cases, both modes, bitwise")


@pytest.mark.parametrize("stride", (1, 2))
def test_load_transform_leaves_the_padding_zero(stride):
    """relu(x a + d) with every d > 0 and a one-hot weight: a padding position that went through the transform
    would read relu(d) > 0 where the closed form has the zero of the normalised map's padding.  Every a is a power of
    two, so x a is exact and x a + d rounds once with or without a fused multiply-add; the expected plane is that
    fp32 value's bf16 hi + lo (its bf16 rounding in the one-product mode), bitwise."""
    from rmd import ops
    b, c, cout, ht, wd = 2, 20, 40, 5, 35
    rng = np.random.default_rng(13 + stride)
    x = rng.standard_normal((b, c, ht, wd)).astype(np.float32)
    scale = (2.0 ** rng.integers(-1, 2, (b, c))).astype(np.float32)
    shift = rng.uniform(0.5, 2.0, (b, c)).astype(np.float32)
    v = np.maximum(x * scale[:, :, None, None] + shift[:, :, None, None], np.float32(0)).astype(np.float32)
    want = {"fp32": cases.exact_split(v), "bf16": cases.bf16_round(v)}
    tx, ta, td, bias = _t(x), _t(scale), _t(shift), torch.zeros(cout, device=DEV)
    weight = torch.zeros(cout, c, 3, 3, device=DEV)
    n = 0
    for i in range(3):
        for j in range(3):
            o, cin = (7 * n + 3) % cout, (5 * n + 16) % c
            n += 1
            weight[o, cin, i, j] = 1.0
            got = {p: ops.conv2d_norm_act(tx, weight, bias, scale=ta, shift=td, stride=stride, precision=p).cpu().numpy()
                   for p in PRECISIONS}
            weight[o, cin, i, j] = 0.0
            for p in PRECISIONS:
                plane = cases.onehot_expected(want[p], 3, cin, i, j, stride)
                if (i, j) != (1, 1):
                    assert (plane == 0).any()            # this tap reads padding somewhere: relu(d) would show there
                expected = np.zeros_like(got[p])
                expected[:, o] = plane
                assert np.array_equal(got[p].view(np.uint32), expected.view(np.uint32)), (stride, i, j, p)


def test_statistics_accuracy():
    from rmd import ops
    rng = np.random.default_rng(14)
    inputs = {"N(0,1) b2 c5 18x70": rng.standard_normal((2, 5, 18, 70)).astype(np.float32),
              "N(0,1) b1 c3 2x1": rng.standard_normal((1, 3, 2, 1)).astype(np.float32),
              "N(100,1) b1 c4 9x67": (100.0 + rng.standard_normal((1, 4, 9, 67))).astype(np.float32)}
    for name, x in inputs.items():
        tx = _t(x)
        scale, shift = ops.instance_norm_stats(tx)
        assert scale.shape == shift.shape == x.shape[:2] and scale.dtype == torch.float32
        got = torch.relu(tx * scale[:, :, None, None] + shift[:, :, None, None]).cpu().numpy()
        err = cases.max_norm_err(got, cases.relu64(cases.instance_norm64(x)))
        a64, d64 = cases.stats_ref(x)
        print(f"statistics {name}: relu(x a + d) vs float64 {err:.3e}; a {np.abs(scale.cpu().numpy() / a64 - 1).max():.2e}"
              f" d {np.abs(shift.cpu().numpy() - d64).max():.2e}")
        assert err <= 1e-5, (name, err)
        again = ops.instance_norm_stats(tx)
        assert torch.equal(_bits(again[0]), _bits(scale)) and torch.equal(_bits(again[1]), _bits(shift))


def test_join_against_float64():
    from rmd import ops
    rng = np.random.default_rng(15)
    y = rng.standard_normal((2, 7, 9, 35)).astype(np.float32)
    x = rng.standard_normal((2, 7, 9, 35)).astype(np.float32)
    ys = tuple(s.astype(np.float32) for s in cases.stats_ref(y))
    xs = tuple(s.astype(np.float32) for s in cases.stats_ref(x))
    for y_stats, x_stats in ((ys, None), (ys, xs), (None, None)):
        out = ops.residual_join(_t(y), _t(x), None if y_stats is None else tuple(map(_t, y_stats)),
                                None if x_stats is None else tuple(map(_t, x_stats))).cpu().numpy()
        err = cases.max_norm_err(out, cases.join_ref(y, y_stats, x, x_stats))
        # two fp32 multiply-adds, an add and the store: a few 2^-24 of an O(1) value
        assert err <= 1e-6, (y_stats is not None, x_stats is not None, err)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("norm", cases.NORMS)
def test_whole_encoder_against_the_fixtures_float64(norm, precision):
    c = cases.encoder_case(norm)
    m = cases.build_encoder(norm, fused="on", precision=precision).to(DEV)
    assert sorted(m.state_dict().keys()) == sorted(c["keys"].tolist())
    with torch.no_grad():
        out = m(_t(c["x"]))
    assert out.shape == c["ref"].shape and out.dtype == torch.float32
    err = cases.max_norm_err(out.cpu().numpy(), c["ref"])
    print(f"encoder {norm} [{precision}]: kernel {err:.3e}  emulation e {c['e'][precision]:.3e}  tolerance "
          f"{c['tol'][precision]:.3e}  (the reference's own fp32 run: {c['ref_err']:.3e})")
    assert err <= c["tol"][precision], (norm, precision, err, c["tol"][precision])


@pytest.mark.parametrize("norm", ("none", "batch"))
def test_images_whose_sides_stop_halving(norm):
    """Images of 1 to 5 pixels a side: a side of 1 stays 1 through the stride-2 convolutions while the channels grow,
    so layer2's and layer3's maps are larger than layer1's and the 128-channel projection larger than the 96-channel
    one.  A batch of 8, so that a map sized for an earlier layer would be overrun by more than the workspace's
    alignment slack.  (The instance norm refuses a one-pixel plane: its case is 1 x 16.)"""
    from rmd import ops
    c = cases.encoder_case(norm)
    ws, bs = [_t(w) for w in c["weights"]], [_t(b) for b in c["biases"]]
    rng = np.random.default_rng(17)
    for ht, wd in ((1, 1), (2, 2), (4, 4), (3, 5), (1, 9)):
        x = rng.standard_normal((8, 3, ht, wd)).astype(np.float32)
        ref = cases.encoder_ref(x, c["weights"], c["biases"], False)
        _, tol = cases.tolerance(cases.encoder_ref(x, c["weights"], c["biases"], False, 3), ref)
        out = ops.feature_encoder(_t(x), ws, bs, norm="none")
        again = ops.feature_encoder(_t(x), ws, bs, norm="none")
        err = cases.max_norm_err(out.cpu().numpy(), ref)
        print(f"encoder {norm} on 8 images of {ht} x {wd}: kernel {err:.3e}  tolerance {tol:.3e}")
        assert err <= tol, (ht, wd, err, tol)
        assert torch.equal(_bits(out), _bits(again))
    # the instance norm on 1 x 16 images (planes of 1 x 8, 1 x 4 and 1 x 2): two-pixel planes are too ill-conditioned
    # for an accuracy bound, so each sample of the batch against its own run, bitwise — maps that overlapped or
    # overran their region would not give that
    ci = cases.encoder_case("instance")
    wi, bi = [_t(w) for w in ci["weights"]], [_t(b) for b in ci["biases"]]
    x = _t(rng.standard_normal((8, 3, 1, 16)).astype(np.float32))
    out = ops.feature_encoder(x, wi, bi, norm="instance")
    assert out.shape == (8, 256, 1, 2) and torch.isfinite(out).all()
    for i in range(8):
        assert torch.equal(_bits(ops.feature_encoder(x[i:i + 1], wi, bi, norm="instance")), _bits(out[i:i + 1])), i


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("norm", cases.NORMS)
def test_residual_block_alone(norm, stride):
    from detinit import det_init_fanin
    from rmd.blocks.raft import ResidualBlock
    rng = np.random.default_rng(16)
    x = np.maximum(rng.standard_normal((2, 64, 9, 35)), 0).astype(np.float32)
    for precision, products in cases.PRODUCTS.items():
        blk = det_init_fanin(ResidualBlock(64, 96 if stride == 2 else 64, norm, stride=stride, fused="on",
                                           precision=precision)).eval()
        ws, bs = cases.folded_params(blk, cases.block_names(stride))
        ref = cases.block_ref(x, ws, bs, stride, norm == "instance")
        e, tol = cases.tolerance(cases.block_ref(x, ws, bs, stride, norm == "instance", products), ref)
        with torch.no_grad():
            out = blk.to(DEV)(_t(x))
        err = cases.max_norm_err(out.cpu().numpy(), ref)
        print(f"block {norm} stride {stride} [{precision}]: kernel {err:.3e}  emulation e {e:.3e}  tolerance {tol:.3e}")
        assert err <= tol, (norm, stride, precision, err, tol)


@pytest.mark.parametrize("norm", cases.NORMS)
def test_samples_do_not_depend_on_the_batch_and_runs_repeat(norm):
    c = cases.encoder_case(norm)
    x = _t(c["x"])
    for precision in PRECISIONS if norm == "instance" else ("fp32",):
        m = cases.build_encoder(norm, fused="on", precision=precision).to(DEV)
        with torch.no_grad():
            full, again = m(x), m(x)
            pair = m((x[:1], x[1:]))
            alone = [m(x[i:i + 1]) for i in range(2)]
        assert torch.equal(_bits(full), _bits(again))
        assert isinstance(pair, tuple) and torch.equal(_bits(torch.cat(pair)), _bits(full))
        for i in range(2):
            assert torch.equal(_bits(alone[i]), _bits(full[i:i + 1])), (precision, i)


@pytest.mark.parametrize("norm", ("instance", "none"))
def test_nan_stays_in_its_sample_and_follows_the_eager_pattern(norm):
    c = cases.encoder_case(norm)
    x = c["x"].copy()
    x[0, 1, 20, 20] = np.nan
    eager = cases.build_encoder(norm)
    with torch.no_grad():
        ref = np.isnan(eager(torch.from_numpy(x)).numpy())
    assert ref[0].any() and not ref[1].any()
    assert ref[0].all() if norm == "instance" else not ref[0].all()
    for precision in PRECISIONS:
        m = cases.build_encoder(norm, fused="on", precision=precision).to(DEV)
        with torch.no_grad():
            clean, out = m(_t(c["x"])), m(_t(x))
        assert torch.equal(_bits(out[1]), _bits(clean[1])), precision
        assert np.array_equal(np.isnan(out.cpu().numpy()), ref), precision


def test_hooks_on_the_encoder_fire_and_inner_hooks_do_not():
    x = _t(cases.encoder_case("instance")["x"])
    m = cases.build_encoder("instance", fused="on").to(DEV)
    outer, inner = [], []
    m.register_forward_hook(lambda mod, inp, out: outer.append(tuple(out.shape)))
    m.conv1.register_forward_hook(lambda mod, inp, out: inner.append("conv1"))
    m.layer2[0].norm3.register_forward_hook(lambda mod, inp, out: inner.append("norm3"))
    with torch.no_grad():
        m(x)
    assert outer == [(2, 256, 5, 18)] and inner == []
    m.fused = "off"
    with torch.no_grad():
        m(x)
    assert len(outer) == 2 and inner == ["conv1", "norm3"]


def _views():
    def permuted(t):
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if t.dim() == 4 else t

    def offset(t):
        return torch.zeros(t.numel() + 3, device=DEV)[3:].view_as(t).copy_(t)

    return permuted, offset


def test_views_give_the_results_of_their_contiguous_copies():
    import rmd  # noqa: F401
    from rmd import _lib
    X3 = _lib.RMD_BF16X3
    x, scale, shift, weight, bias, residual = (_t(a) for a in cases.shape_case(*cases.SHAPES[5])["args"])
    ref = torch.ops.rmd.conv2d_norm_act(x, scale, shift, weight, bias, residual, 1, 1, X3)
    ref_stats = torch.ops.rmd.instance_norm_stats(x, 1e-5)
    ref_join = torch.ops.rmd.residual_join(ref, None, None, residual, None, None)
    c = cases.encoder_case("instance")
    img, ws, bs = _t(c["x"]), [_t(w) for w in c["weights"]], [_t(b) for b in c["biases"]]
    ref_enc = torch.ops.rmd.feature_encoder(img, ws, bs, 1, X3)
    for view in _views():
        assert not view(x).is_contiguous() or view(x).storage_offset() == 3
        got = torch.ops.rmd.conv2d_norm_act(view(x), view(scale), view(shift), view(weight), view(bias), view(residual),
                                            1, 1, X3)
        assert torch.equal(_bits(got), _bits(ref))
        got = torch.ops.rmd.instance_norm_stats(view(x), 1e-5)
        assert torch.equal(_bits(got[0]), _bits(ref_stats[0])) and torch.equal(_bits(got[1]), _bits(ref_stats[1]))
        got = torch.ops.rmd.residual_join(view(ref), None, None, view(residual), None, None)
        assert torch.equal(_bits(got), _bits(ref_join))
        got = torch.ops.rmd.feature_encoder(view(img), [view(w) for w in ws], [view(b) for b in bs], 1, X3)
        assert torch.equal(_bits(got), _bits(ref_enc))


def test_opcheck():
    import rmd  # noqa: F401
    from rmd import _lib
    x, scale, shift, weight, bias, residual = (_t(a) for a in cases.shape_case(*cases.SHAPES[5])["args"])
    c = cases.encoder_case("instance")
    enc_args = (_t(c["x"]), [_t(w) for w in c["weights"]], [_t(b) for b in c["biases"]])
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    strided = torch.zeros(40, 20, 3, 3, device=DEV)
    for compute in (_lib.RMD_BF16X3, _lib.RMD_BF16):
        torch.library.opcheck(torch.ops.rmd.conv2d_norm_act, (x, scale, shift, weight, bias, residual, 1, 1, compute),
                              test_utils=utils)
        torch.library.opcheck(torch.ops.rmd.conv2d_norm_act, (x, None, None, strided, bias, None, 2, 0, compute),
                              test_utils=utils)
        for norm in (0, 1):
            torch.library.opcheck(torch.ops.rmd.feature_encoder, enc_args + (norm, compute), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.instance_norm_stats, (x, 1e-5), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.residual_join, (x, scale, shift, x.flip(0), None, None), test_utils=utils)
    torch.library.opcheck(torch.ops.rmd.residual_join, (x, scale, shift, x.flip(0), shift, scale), test_utils=utils)
    grad = x.clone().requires_grad_(True)
    assert not torch.ops.rmd.conv2d_norm_act(grad, scale, shift, weight, bias, residual, 1, 1, _lib.RMD_BF16X3).requires_grad
    assert not torch.ops.rmd.instance_norm_stats(grad, 1e-5)[0].requires_grad
    assert not torch.ops.rmd.residual_join(grad, None, None, x, None, None).requires_grad
    assert not torch.ops.rmd.feature_encoder(enc_args[0].clone().requires_grad_(True), *enc_args[1:], 1,
                                             _lib.RMD_BF16X3).requires_grad


def test_the_fused_encoder_never_waits_for_the_host_and_stays_in_its_workspace():
    """Sync-debug mode over one fused call of each norm type (the batch norm is folded on the device), then the
    operator's peak allocation: the output and the workspace of rmd_feature_encoder_workspace_bytes, nothing else."""
    import rmd  # noqa: F401
    from rmd import _lib
    x = _t(cases.encoder_case("none")["x"])
    mods = [cases.build_encoder(norm, fused="on").to(DEV) for norm in cases.NORMS]
    with torch.no_grad():
        for m in mods:
            m(x)                                            # the warm-up call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            for m in mods:
                m(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")

    c = cases.encoder_case("instance")
    ws, bs = [_t(w) for w in c["weights"]], [_t(b) for b in c["biases"]]
    for norm in (0, 1):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = torch.ops.rmd.feature_encoder(x, ws, bs, norm, _lib.RMD_BF16X3)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        bound = out.numel() * 4 + _lib.lib().rmd_feature_encoder_workspace_bytes(2, 36, 140, 256)
        assert peak <= bound + 2 * 512, (norm, peak, bound)     # the allocator rounds each of the two blocks up to 512 bytes


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd.encoders  # noqa: F401
    from rmd import _lib, ops
    from rmd.blocks.raft import ResidualBlock
    X3 = _lib.RMD_BF16X3
    x, scale, shift, weight, bias, residual = cases.shape_case(*cases.SHAPES[5])["args"]
    tx, ta, td, tw, tb, tr = (_t(a) for a in (x, scale, shift, weight, bias, residual))
    c = cases.encoder_case("none")
    img, ws, bs = _t(c["x"]), [_t(w) for w in c["weights"]], [_t(b) for b in c["biases"]]
    assert cases.build_encoder("none", fused="auto").to(DEV)(img).requires_grad     # the composition, which trains
    on = {norm: cases.build_encoder(norm, fused="on").to(DEV) for norm in ("instance", "batch")}
    block = ResidualBlock(20, 40, "none", stride=2, fused="on").to(DEV)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="autocast"):
            on["instance"](img)
        with pytest.raises(RuntimeError, match="autocast"):
            block(tx)
    with pytest.raises(RuntimeError, match="gradient"):
        on["instance"](img)
    with pytest.raises(RuntimeError, match="gradient"):
        block(tx)
    with torch.no_grad(), pytest.raises(RuntimeError, match="training mode"):
        on["batch"].train()(img)
    cpu = torch.from_numpy
    for fn in (lambda: torch.ops.rmd.conv2d_norm_act(tx, ta, td, cpu(weight), tb, tr, 1, 1, X3),      # a CPU tensor
               lambda: torch.ops.rmd.conv2d_norm_act(tx, cpu(scale), td, tw, tb, tr, 1, 1, X3),
               lambda: torch.ops.rmd.residual_join(tx, ta, td, cpu(x), None, None),
               lambda: torch.ops.rmd.feature_encoder(img, ws[:3] + [cpu(c["weights"][3])] + ws[4:], bs, 0, X3)):
        with pytest.raises(ValueError, match="must be on the GPU"):
            fn()
    with pytest.raises(ValueError, match="different devices"):
        ops.conv2d_norm_act(tx, tw, cpu(bias))
    with pytest.raises(ValueError, match="different devices"):
        ops.feature_encoder(img, ws, bs[:15] + [cpu(c["biases"][15])])
    with pytest.raises(ValueError, match="stride 3"):
        torch.ops.rmd.conv2d_norm_act(tx, None, None, tw, tb, None, 3, 0, X3)
    with pytest.raises(ValueError, match="odd"):                                                # an even kernel
        torch.ops.rmd.conv2d_norm_act(tx, None, None, tw[:, :, :2].contiguous(), tb, None, 1, 0, X3)
    with pytest.raises(ValueError, match="need 16 weights"):
        torch.ops.rmd.feature_encoder(img, ws[:15], bs, 0, X3)
    with pytest.raises(ValueError, match="weights\\[4\\]"):
        torch.ops.rmd.feature_encoder(img, ws[:4] + [ws[6]] + ws[5:], bs, 0, X3)
    with pytest.raises(ValueError, match="residual must be"):
        torch.ops.rmd.conv2d_norm_act(tx, None, None, tw, tb, tr, 2, 0, X3)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.conv2d_norm_act(tx, None, None, tw, tb, None, 1, 0, _lib.RMD_F32)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.feature_encoder(img, ws, bs, 0, _lib.RMD_F32)
    with pytest.raises(ValueError, match="one pixel"):
        torch.ops.rmd.instance_norm_stats(torch.zeros(2, 3, 1, 1, device=DEV), 1e-5)
    with pytest.raises(ValueError, match="more than one pixel"):
        torch.ops.rmd.feature_encoder(torch.zeros(1, 3, 8, 8, device=DEV), ws, bs, 1, X3)


def test_the_c_abi_checks_run_before_any_launch():
    """rmd_instance_stats refuses a one-pixel plane with RMD_ERR_SHAPE; null pointers and an output that overlaps an
    input are RMD_ERR_ARG.  The launchers return before their first launch, so the buffers are never touched."""
    import ctypes
    import rmd  # noqa: F401
    from rmd import _lib
    x = torch.zeros(1, 2, 4, 4, device=DEV)
    a, d = torch.full((1, 2), 7.0, device=DEV), torch.full((1, 2), 7.0, device=DEV)
    eps = ctypes.c_float(1e-5)
    with pytest.raises(_lib.RmdError, match=r"code -2\).*one pixel"):
        _lib.launch("rmd_instance_stats", x, x, a, d, 1, 2, 1, 1, eps)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*null pointer"):
        _lib.launch("rmd_instance_stats", x, x, None, d, 1, 2, 4, 4, eps)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*overlap"):
        _lib.launch("rmd_instance_stats", x, x, a, a, 1, 2, 4, 4, eps)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*overlaps"):
        _lib.launch("rmd_residual_join", x, x, None, None, x, None, None, x, 1, 2, 4, 4)
    w, b = torch.zeros(2, 2, 3, 3, device=DEV), torch.zeros(2, device=DEV)
    work = _lib.workspace("conv2d_strided", x, 2, 2, 3, 3)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*out overlaps"):
        _lib.launch("rmd_conv2d_strided", x, x, None, None, w, b, None, x, work, 1, 2, 2, 3, 3, 4, 4, 1, 0, _lib.RMD_BF16X3)
    with pytest.raises(_lib.RmdError, match=r"code -2\).*unsupported"):
        _lib.launch("rmd_conv2d_strided", x, x, None, None, w, b, None, torch.empty_like(x), work, 1, 2, 2, 3, 3, 4, 4, 3,
                    0, _lib.RMD_BF16X3)
    assert _lib.lib().rmd_feature_encoder_workspace_bytes(1, 16, 16, 2000) == 0
    assert _lib.lib().rmd_feature_encoder_supported(256, 2) == 0 and _lib.lib().rmd_feature_encoder_supported(256, 1) == 1
    assert _lib.lib().rmd_conv2d_strided_supported(3, 3, 3, 8, 8) == 0
    assert torch.equal(a, torch.full((1, 2), 7.0, device=DEV)) and not x.any()
