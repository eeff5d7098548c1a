"""The feature / context encoder without a GPU: the drop-in modules' state-dict keys and reference composition against
the fixtures of tests/golden/gen_golden_encoder.py, the tests' float64 restatement (encoder_cases.py) against the
reference's own float64 run, the operators' CPU composites against the restatement, the fake kernels' shapes, the
operator family, the fall-back reasons of fused="auto" / "on" and the folded batch norm.

Bounds.  The reference composition in fp32 is compared with the fixture's float64 output at max(1e-5, 3 ref_err),
ref_err the reference's own fp32 error stored in the fixture (another CPU may order its fp32 sums differently, so
bitwise equality with the fixture's fp32 output is printed, not asserted).  The CPU composites are fp32 ATen
compositions and are held to the project's floor, 1e-5 max-normalised against float64.  The float64 restatement
and the reference's float64 run differ by rounding in float64 only: 1e-12.
"""

import numpy as np
import pytest
import torch

import encoder_cases as cases

FP32 = 1e-5
FP64 = 1e-12


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("norm", cases.NORMS)
def test_state_dict_keys_and_reference_composition(norm):
    c = cases.encoder_case(norm)
    m = cases.build_encoder(norm)
    assert m.fused == "off"
    assert sorted(m.state_dict().keys()) == sorted(c["keys"].tolist())
    with torch.no_grad():
        out = m(_t(c["x"])).numpy()
        auto = cases.build_encoder(norm, fused="auto")(_t(c["x"])).numpy()       # CPU tensors: the composition
        pair = cases.build_encoder(norm)((_t(c["x"][:1]), _t(c["x"][1:])))
    err = cases.max_norm_err(out, c["ref"])
    print(f"{norm}: off vs float64 {err:.3e} (reference's own {c['ref_err']:.3e}); bitwise the fixture's fp32: "
          f"{np.array_equal(out, c['out'])}")
    assert err <= max(FP32, 3 * c["ref_err"])
    assert np.array_equal(out, auto)
    assert isinstance(pair, tuple) and len(pair) == 2 and pair[0].shape == (1, 256, 5, 18)
    if norm != "batch":     # eval batch norm is per element; instance statistics are per sample either way
        assert cases.max_norm_err(torch.cat(pair).numpy(), c["ref"]) <= max(FP32, 3 * c["ref_err"])


@pytest.mark.parametrize("norm", cases.NORMS)
def test_restatement_matches_the_reference_in_float64(norm):
    c = cases.encoder_case(norm)
    err = cases.max_norm_err(cases.encoder_ref(c["x"], c["weights"], c["biases"], norm == "instance"), c["ref"])
    print(f"{norm}: restatement vs the reference's float64 run {err:.3e}; emulation e {c['e']}, tolerances {c['tol']}")
    # the batch norm's fold is rounded to fp32 (the operator's input): its rounding, 2^-24 per weight
    assert err <= (FP64 if norm != "batch" else 1e-6)
    assert all(c["e"][p] < 0.1 for p in c["e"])


@pytest.mark.parametrize("shape,transformed", cases.SHAPES, ids=cases.SHAPE_IDS)
def test_cpu_convolution_matches_the_restatement(shape, transformed):
    from rmd import ops
    c = cases.shape_case(shape, transformed)
    x, scale, shift, weight, bias, residual = (_t(a) for a in c["args"])
    for act in cases.ACTS:
        out = ops.conv2d_norm_act(x, weight, bias, scale=scale, shift=shift, residual=residual, stride=c["stride"],
                                  act=act)
        assert out.shape == c["ref"][act].shape and out.dtype == torch.float32
        assert cases.max_norm_err(out.numpy(), c["ref"][act]) <= FP32


def test_cpu_statistics_join_and_encoder_match_the_restatement():
    from rmd import ops
    rng = np.random.default_rng(3)
    x = (100.0 + rng.standard_normal((1, 4, 9, 67))).astype(np.float32)
    y = rng.standard_normal((1, 4, 9, 67)).astype(np.float32)
    scale, shift = ops.instance_norm_stats(_t(x))
    want = cases.stats_ref(x)
    assert scale.shape == (1, 4) and np.abs(scale.numpy() / want[0] - 1).max() <= 1e-6
    assert np.abs(shift.numpy() / want[1] - 1).max() <= 1e-6
    normed = torch.relu(_t(x) * scale[:, :, None, None] + shift[:, :, None, None]).numpy()
    assert cases.max_norm_err(normed, cases.relu64(cases.instance_norm64(x))) <= FP32
    ys, xs = cases.stats_ref(y), want
    for y_stats, x_stats in ((ys, None), (ys, xs), (None, None)):
        out = ops.residual_join(_t(y), _t(x), None if y_stats is None else tuple(_t(cases.f32(s).astype(np.float32)) for s in y_stats),
                                None if x_stats is None else tuple(_t(cases.f32(s).astype(np.float32)) for s in x_stats))
        assert cases.max_norm_err(out.numpy(), cases.join_ref(y, y_stats, x, x_stats)) <= FP32
    with pytest.raises(ValueError, match="one pixel"):
        ops.instance_norm_stats(torch.zeros(1, 2, 1, 1))
    for norm in cases.NORMS:
        c = cases.encoder_case(norm)
        out = ops.feature_encoder(_t(c["x"]), [_t(w) for w in c["weights"]], [_t(b) for b in c["biases"]],
                                  norm="instance" if norm == "instance" else "none")
        assert cases.max_norm_err(out.numpy(), c["ref"]) <= FP32, norm


def test_fake_kernels_give_the_strided_sizes():
    import rmd  # noqa: F401
    from rmd import _lib

    def meta(*shape):
        return torch.empty(shape, device="meta")

    X3 = _lib.RMD_BF16X3
    for (b, c, cout, k, ht, wd, stride), _ in cases.SHAPES:
        out = torch.ops.rmd.conv2d_norm_act(meta(b, c, ht, wd), None, None, meta(cout, c, *cases.kernel_sides(k)),
                                            meta(cout), None, stride, 1, X3)
        assert out.shape == (b, cout, (ht - 1) // stride + 1, (wd - 1) // stride + 1) and out.dtype == torch.float32
    assert torch.ops.rmd.conv2d_norm_act(meta(1, 3, 13, 70), None, None, meta(64, 3, 7, 7), meta(64), None, 2, 0,
                                         X3).shape == (1, 64, 7, 35)
    scale, shift = torch.ops.rmd.instance_norm_stats(meta(2, 5, 3, 4), 1e-5)
    assert scale.shape == shift.shape == (2, 5)
    assert torch.ops.rmd.residual_join(meta(2, 5, 3, 4), scale, shift, meta(2, 5, 3, 4), None, None).shape == (2, 5, 3, 4)
    c = cases.encoder_case("none")
    ws, bs = [meta(*w.shape) for w in c["weights"]], [meta(*b.shape) for b in c["biases"]]
    assert torch.ops.rmd.feature_encoder(meta(2, 3, 36, 140), ws, bs, 1, X3).shape == (2, 256, 5, 18)
    assert torch.ops.rmd.feature_encoder(meta(1, 3, 440, 1024), ws, bs, 0, X3).shape == (1, 256, 55, 128)
    with pytest.raises(ValueError, match="stride 3"):
        torch.ops.rmd.conv2d_norm_act(meta(1, 3, 8, 8), None, None, meta(4, 3, 3, 3), meta(4), None, 3, 0, X3)


def test_encoder_operators_are_a_family_of_their_own():
    from rmd import library
    assert library.encoder_operators() == cases.OPERATORS
    others = (library.operators, library.loss_operators, library.metric_operators, library.head_operators,
              library.attn_operators, library.match_operators, library.match_train_operators,
              library.update_operators, library.conv_operators)
    for family in others:
        assert not set(family()) & set(cases.OPERATORS), family.__name__
    for name in cases.OPERATORS:
        assert hasattr(torch.ops.rmd, name)


def test_fallback_reasons_and_on_errors():
    import rmd.encoders
    from rmd.blocks.raft import ResidualBlock
    x = torch.randn(1, 3, 16, 24)

    def reason(m, inp=x):
        return m.fallback_reason(inp)

    def enc(norm, **kwargs):
        return rmd.encoders.FeatureEncoder(64, norm, fused="on", **kwargs).eval()

    with torch.no_grad():
        assert "group norm" in reason(enc("group"))
        assert "training mode" in reason(enc("batch").train())
        m = enc("instance")
        m.layer2[0].norm2 = torch.nn.InstanceNorm2d(96, affine=True)
        assert "affine parameters or running statistics" in reason(m)
        m = enc("instance")
        m.norm1 = torch.nn.InstanceNorm2d(64, track_running_stats=True).eval()
        assert "affine parameters or running statistics" in reason(m)
        assert "dropout is active" in reason(enc("none", dropout=0.5).train())
        assert "not on the GPU" in reason(enc("none", dropout=0.5))        # eval: dropout is off
        assert "float32" in reason(enc("none"), x.double())
        m = enc("batch")
        m.layer3[0].norm3.running_var = m.layer3[0].norm3.running_var.double()     # folded() reads the buffers too
        assert "float32" in reason(m)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert "autocast" in reason(enc("instance"))
        for norm in ("instance", "batch", "none"):
            assert "not on the GPU" in reason(enc(norm))
            with pytest.raises(RuntimeError, match="FeatureEncoder\\(fused='on'\\): the tensors are not on the GPU"):
                enc(norm)(x)
            blk = ResidualBlock(8, 16, norm, stride=2, fused="on").eval()
            with pytest.raises(RuntimeError, match="ResidualBlock\\(fused='on'\\): the tensors are not on the GPU"):
                blk(torch.randn(1, 8, 6, 6))
        assert "group norm" in ResidualBlock(8, 16, fused="auto").fallback_reason(torch.randn(1, 8, 6, 6))
    assert "gradient" in reason(enc("none"))                    # grad mode on, parameters require grad
    with pytest.raises(RuntimeError, match="gradient"):
        enc("instance")(x)
    auto = rmd.encoders.FeatureEncoder(64, "instance", fused="auto")
    assert auto(x).requires_grad                                # the composition, which trains
    with pytest.raises(ValueError, match="fused mode"):
        rmd.encoders.FeatureEncoder(64, "none", fused="yes")
    with pytest.raises(ValueError, match="precision"):
        ResidualBlock(8, 8, "none", precision="fp16")
    assert isinstance(rmd.encoders.make_encoder_s3("raft", 32, "none", 0.0, fused="auto"), rmd.encoders.FeatureEncoder)
    for ty in ("dicl", "rfpm-raft", "nope"):
        with pytest.raises(ValueError, match="encoder type"):
            rmd.encoders.make_encoder_s3(ty, 32, "none", 0.0)


def test_forward_hooks_on_the_encoder_fire():
    m = cases.build_encoder("none", fused="auto")
    seen = []
    m.register_forward_hook(lambda mod, inp, out: seen.append(tuple(out.shape)))
    with torch.no_grad():
        m(torch.randn(1, 3, 16, 24))
    assert seen == [(1, 256, 2, 3)]


def test_folded_batch_norm_matches_float64():
    from rmd.blocks.raft import folded
    m = cases.build_encoder("batch")
    weights, biases = cases.folded_params(m)
    pairs = m.conv_norms()
    assert len(pairs) == 16 and pairs[15][1] is None
    folds = 0
    with torch.no_grad():
        for (conv, norm), w64, b64 in zip(pairs, weights, biases):
            w, b = folded(conv, norm)
            folds += w is not conv.weight
            assert np.abs(w.numpy() - w64).max() <= 1e-6 * np.abs(w64).max()
            assert np.abs(b.numpy() - b64).max() <= 1e-6 * max(np.abs(b64).max(), 1.0)
    assert folds == 15                                          # every convolution but the last has a norm
    inst = cases.build_encoder("instance")
    assert all(folded(c, n)[0] is c.weight for c, n in inst.conv_norms())


def test_workspace_regions_hold_every_map_written():
    """The carve-up of rmd_feature_encoder's workspace against the schedule, for every image side from 1 to 9 (a side
    of 1 stays 1 through the stride-2 convolutions while the channels grow from 64 to 128, so the largest map is not
    always the first) and two real sizes: each of the three rotating maps holds the stem's result and every block's
    first and second result, the projection map holds both projections, and the regions add up to the workspace."""
    import ctypes
    from rmd import _lib, library
    L = _lib.lib()
    batch, output_dim = 3, 256
    sides = [(h, w) for h in range(1, 10) for w in range(1, 10)] + [(36, 140), (440, 1024)]
    for ht, wd in sides:
        regions = (ctypes.c_size_t * 4)()
        _lib.check(L.rmd_feature_encoder_workspace_regions(batch, ht, wd, output_dim, regions), "regions")
        packed, stat, one_map, proj = list(regions)
        h, w, maps, projections = ht, wd, [], []
        for cout, cin, k, stride in library.feature_encoder_convs(output_dim)[:-1]:
            ho, wo = library.out_side(h, stride), library.out_side(w, stride)
            if k == 1:                                          # the projection reads the block's input, as its conv1 did
                projections.append(batch * cout * h * w * 4)
                continue
            maps.append(batch * cout * ho * wo * 4)
            h, w = ho, wo
        assert len(maps) == 13 and len(projections) == 2
        assert one_map >= max(maps), (ht, wd, one_map, max(maps))
        assert proj >= max(projections), (ht, wd, proj, max(projections))
        assert stat >= batch * 128 * 4
        assert packed == sum(L.rmd_conv2d_strided_workspace_bytes(cin, cout, k, k) - 256
                             for cout, cin, k, _ in library.feature_encoder_convs(output_dim))
        assert L.rmd_feature_encoder_workspace_bytes(batch, ht, wd, output_dim) == packed + 6 * stat + 3 * one_map + proj + 256
        assert library.feature_encoder_unsupported_reason(output_dim, ht, wd) is None
    assert L.rmd_feature_encoder_workspace_regions(0, 4, 4, 256, (ctypes.c_size_t * 4)()) != 0
