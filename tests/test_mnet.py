"""The fused k x k MatchingNet without a GPU: the tests' float64 restatement (mnet_cases.py) against the reference's
fixtures and against F.conv_transpose2d, the operators' CPU composites against the module path, the `off` path
against the plain nn.Sequential (bitwise), folded() / foldable(), every fall-back reason of "auto" with the message
"on" raises, hooks, state-dict keys, the operator family, schemas and fake shapes, the host-only supported() and
workspace answers, the group a budget gives, and the C ABI's argument checks (which run before any launch, so they
need no device).

None of these passes without the feature: the operators, the arguments and the C entry points do not exist."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mnet_cases as cases

NORMS = ("batch", "none", "group", "instance")
WIDTHS = (64, 96, 128, 64, 32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _mnet(c_in=34, norm="batch", seed=3, **kwargs):
    """A MatchingNet in eval mode with non-trivial batch-norm state."""
    from rmd.blocks.dicl import MatchingNet
    torch.manual_seed(seed)
    m = MatchingNet(c_in, norm_type=norm, **kwargs)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_var.uniform_(0.5, 2.0)
                mod.running_mean.normal_(0.0, 0.3)
                mod.weight.uniform_(0.7, 1.3)
                mod.bias.normal_(0.0, 0.2)
    return m.eval()


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_restatement_against_the_fixtures(name):
    g, c = cases.fixture(name), cases.fixture_case(name)
    err = cases.max_norm_err(c["ref"], g["nodap.cost"])
    assert err <= 1e-5, (name, err)
    assert g["dap.cost"].shape == c["ref"].shape and np.array_equal(np.isnan(g["dap.cost"]), np.isnan(c["ref"]))


@pytest.mark.parametrize("shape", cases.TAIL_SHAPES, ids=cases.TAIL_IDS)
def test_transposed_restatement_against_aten_float64(shape):
    x, w5 = cases.tail_case(shape)["args"][:2]
    want = F.conv_transpose2d(_t(x).double(), _t(w5).double(), stride=2, padding=1).numpy()
    got = cases.tconv64(x, w5)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def test_emulated_modes_order_as_the_products():
    """One product is far from float64, three are near fp32: the emulation separates the modes."""
    for shape in cases.TAIL_SHAPES[:4]:
        e = cases.tail_case(shape)["e"]
        assert e["fp32"] < 1e-4 < 5e-4 < e["bf16"] < 2e-2, (shape, e)


@pytest.mark.parametrize("norm", ("batch", "none"))
def test_cpu_operators_against_the_module_path(norm):
    from rmd import ops
    m = _mnet(34, norm, scale=0.5)
    mvol = torch.randn(2, 3, 3, 34, 6, 10)
    with torch.no_grad():
        want = nn.Sequential.forward(m, mvol.view(18, 34, 6, 10)).view(2, 3, 3, 6, 10)
        weights, biases = m.folded()
        got = ops.matching_net(mvol, weights, biases)
        x = m[3](m[2](m[1](m[0](mvol.view(18, 34, 6, 10)))))
        tail = ops.mnet_tail(x, weights[4], biases[4], weights[5], biases[5], precision="bf16")
    assert got.shape == want.shape and got.dtype == torch.float32
    assert cases.max_norm_err(got.numpy(), want.numpy()) <= 1e-6
    assert cases.max_norm_err(tail.numpy(), want.reshape(18, 6, 10).numpy()) <= 1e-6
    ref = cases.net_ref(mvol.view(18, 34, 6, 10).numpy(), [w.detach().numpy() for w in weights],
                        [b.detach().numpy() for b in biases])
    assert cases.max_norm_err(got.reshape(18, 6, 10).numpy(), ref) <= 1e-5


@pytest.mark.parametrize("norm", NORMS)
def test_off_is_the_plain_sequential_bit_for_bit(norm):
    m = _mnet(16, norm)
    assert m.fused == "off" and m.precision == "fp32"
    mvol = torch.randn(1, 3, 3, 16, 4, 6)
    with torch.no_grad():
        want = nn.Sequential.forward(m, mvol.view(9, 16, 4, 6)).view(1, 3, 3, 4, 6)
        assert torch.equal(m(mvol), want)
        auto = _mnet(16, norm, fused="auto")
        auto.load_state_dict(m.state_dict())
        assert torch.equal(auto(mvol), want)                # on the CPU "auto" is the sequential path
    m.train()
    assert m(mvol).requires_grad


def test_folded_and_foldable():
    from rmd.blocks.dicl import MatchingNet
    for norm in NORMS:
        m = _mnet(10, norm, scale=0.25)
        assert m.foldable() == (norm in ("batch", "none")), norm
        if not m.foldable():
            with pytest.raises(RuntimeError, match="cannot be folded"):
                m.folded()
            continue
        weights, biases = m.folded()
        assert [tuple(w.shape) for w in weights] == [(24, 10, 3, 3), (32, 24, 3, 3), (32, 32, 3, 3), (16, 32, 3, 3),
                                                     (16, 8, 4, 4), (8, 3, 3)]
        assert [b.numel() for b in biases] == [24, 32, 32, 16, 8, 1]
        x = torch.randn(3, 10, 4, 6)
        with torch.no_grad():
            for i, stride in enumerate((1, 2, 1, 1)):
                want = m[i](x)
                got = F.relu(F.conv2d(x, weights[i], biases[i], stride=stride, padding=1))
                assert cases.max_norm_err(got.numpy(), want.numpy()) <= 1e-6, (norm, i)
                x = want
            # layer 5: the scale multiplies dim 1 of the transposed weight
            got = F.relu(F.conv_transpose2d(x, weights[4], biases[4], stride=2, padding=1))
            assert cases.max_norm_err(got.numpy(), m[4](x).numpy()) <= 1e-6, norm
        assert torch.equal(weights[5], m[5].weight[0]) and biases[5] is m[5].bias
    train = MatchingNet(10, "batch").train()
    assert not train.foldable()
    nostats = MatchingNet(10, "batch").eval()
    nostats[2][1] = nn.BatchNorm2d(nostats[2][0].out_channels, track_running_stats=False).eval()
    assert not nostats.foldable()


def test_fallback_reasons_and_on_errors():
    """Every reason "auto" falls back for, named by the RuntimeError of "on"; "auto" itself returns what "off" does."""
    from rmd.blocks.dicl import MatchingNet
    mvol = torch.randn(1, 1, 1, 34, 4, 6)

    def both(reason, make, x, ctx=torch.no_grad):
        on = make("on")
        with ctx(), pytest.raises(RuntimeError, match=reason):
            on(x)
        auto = make("auto")
        assert auto.fallback_reason(x) is not None
        with ctx():
            out = auto(x)
        return out

    for norm in ("group", "instance"):
        both("group, instance or train-mode batch norm", lambda f, norm=norm: _mnet(34, norm, fused=f), mvol)
    both("train-mode batch norm", lambda f: _mnet(34, "batch", fused=f).train(), mvol)
    with torch.no_grad(), pytest.raises(RuntimeError, match="not all float32"):
        _mnet(34, "none", fused="on").double()(mvol.double())
    assert _mnet(34, "none", fused="auto").double()(mvol.double()).dtype == torch.float64
    out = both("gradient", lambda f: _mnet(34, "none", fused=f), mvol, ctx=torch.enable_grad)
    assert out.requires_grad
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16), pytest.raises(RuntimeError, match="autocast"):
        _mnet(34, "none", fused="on")(mvol)
    odd = torch.randn(1, 1, 1, 34, 3, 4)
    with torch.no_grad(), pytest.raises(RuntimeError, match="a side of the 3 x 4 map is odd"):
        _mnet(34, "none", fused="on")(odd)
    with torch.no_grad(), pytest.raises(RuntimeError, match="shape"):      # the sequential path's view fails, as the reference's
        _mnet(34, "none", fused="auto")(odd)
    with torch.no_grad(), pytest.raises(RuntimeError, match="unsupported widths"):
        _mnet(34, "none", fused="on", scale=3)(mvol)         # c3 = 192, c4 = 96
    with torch.no_grad():
        assert _mnet(34, "none", fused="auto", scale=3)(mvol).shape == (1, 1, 1, 4, 6)
    both("not on the GPU", lambda f: _mnet(34, "batch", fused=f), mvol)
    for bad in (dict(fused="yes"), dict(precision="fp16")):
        with pytest.raises(ValueError, match="unknown"):
            MatchingNet(34, **bad)


def test_arguments_pass_through_the_correlation_modules():
    import rmd
    for ty, kw in (("dicl", dict(mnet_scale=0.5)), ("dicl-emb", {})):
        mod = rmd.corr.make_cmod(ty, 16, 2, fused="auto", precision="bf16", **kw)
        assert (mod.mnet.fused, mod.mnet.precision) == ("auto", "bf16")
        assert mod.mnet.widths()[0] == (34 if ty == "dicl-emb" else 32)
        assert rmd.corr.make_cmod(ty, 16, 2, **kw).mnet.fused == "off"
    ml = rmd.raft_dicl_ml.CorrelationModule(16, 3, 2, fused="on", precision="bf16")
    assert all((m.fused, m.precision) == ("on", "bf16") for m in ml.mnet)
    shared = rmd.raft_dicl_ml.CorrelationModule(16, 3, 2, share=True, fused="auto")
    assert shared.mnet.fused == "auto"
    # rmd.dicl.compute_cost takes whatever mnet it is given
    f = torch.randn(1, 16, 4, 6)
    with torch.no_grad():
        cost = rmd.dicl.compute_cost(_mnet(32, "batch", fused="auto"), f, f, (1, 1))
    assert cost.shape == (1, 3, 3, 4, 6)


def test_a_forward_hook_on_mnet_fires_once_and_state_dict_keys_are_the_references():
    for name in cases.FIXTURES[:3]:
        g = cases.fixture(name)
        for fused in ("off", "auto"):
            mod = cases.build_module(name, fused=fused)
            assert sorted(mod.state_dict().keys()) == sorted(g["sd.keys"].tolist()), (name, fused)
            calls = []
            mod.mnet.register_forward_hook(lambda m, i, o: calls.append(tuple(o.shape)))
            with torch.no_grad():
                out = mod(_t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"]))
            assert calls == [g["nodap.cost"].shape]
            assert cases.max_norm_err(out.numpy(), g["dap.out"]) <= 1e-5


def test_mnet_operators_are_a_family_of_their_own():
    from rmd import library
    assert library.mnet_operators() == cases.OPERATORS
    others = (library.operators, library.loss_operators, library.metric_operators, library.head_operators,
              library.attn_operators, library.match_operators, library.match_train_operators,
              library.update_operators, library.conv_operators, library.encoder_operators)
    for family in others:
        assert not set(family()) & set(cases.OPERATORS), family.__name__
    assert library.encoder_operators() == ["conv2d_norm_act", "feature_encoder", "instance_norm_stats", "residual_join"]
    assert library.conv_operators() == ["conv2d_act", "motion_encoder"]
    assert library.match_operators() == ["dicl_match_1x1"]
    schemas = {"matching_net": "rmd::matching_net(Tensor mvol, Tensor[] weights, Tensor[] biases, int group, "
                               "int compute) -> Tensor",
               "mnet_tail": "rmd::mnet_tail(Tensor x, Tensor weight5, Tensor bias5, Tensor weight6, Tensor bias6, "
                            "int compute) -> Tensor"}
    for name, schema in schemas.items():
        assert str(getattr(torch.ops.rmd, name).default._schema) == schema


def test_fake_kernels_give_the_shapes():
    import rmd  # noqa: F401
    from rmd import _lib

    def meta(*shape):
        return torch.empty(shape, device="meta")

    X3 = _lib.RMD_BF16X3
    for n, c3, c4, h2, w2 in cases.TAIL_SHAPES:
        out = torch.ops.rmd.mnet_tail(meta(n, c3, h2, w2), meta(c3, c4, 4, 4), meta(c4), meta(c4, 3, 3), meta(1), X3)
        assert out.shape == (n, 2 * h2, 2 * w2) and out.dtype == torch.float32
    for b, du, dv, c_in, scale, h, w in cases.NET_SHAPES:
        _, c1, c2, c3, c4 = cases.widths(c_in, scale)
        ws = [meta(c1, c_in, 3, 3), meta(c2, c1, 3, 3), meta(c2, c2, 3, 3), meta(c3, c2, 3, 3), meta(c3, c4, 4, 4),
              meta(c4, 3, 3)]
        bs = [meta(c1), meta(c2), meta(c2), meta(c3), meta(c4), meta(1)]
        out = torch.ops.rmd.matching_net(meta(b, du, dv, c_in, h, w), ws, bs, 3, X3)
        assert out.shape == (b, du, dv, h, w) and out.dtype == torch.float32
        with pytest.raises(ValueError, match="even"):
            torch.ops.rmd.matching_net(meta(b, du, dv, c_in, h + 1, w), ws, bs, 3, X3)
        with pytest.raises(ValueError, match="group"):
            torch.ops.rmd.matching_net(meta(b, du, dv, c_in, h, w), ws, bs, 0, X3)
        with pytest.raises(ValueError, match=r"weights\[2\]"):
            torch.ops.rmd.matching_net(meta(b, du, dv, c_in, h, w), ws[:2] + [ws[3]] + ws[3:], bs, 3, X3)


def test_supported_grid():
    from rmd import _lib, library
    lib = _lib.lib()
    for h, w, want in ((2, 2, 1), (48, 160, 1), (4, 6, 1), (3, 4, 0), (4, 5, 0), (1, 2, 0), (0, 4, 0), (2, 1 << 24, 0)):
        assert lib.rmd_matching_net_supported(*WIDTHS, h, w) == want, (h, w)
    for widths, want in (((34, 96, 128, 64, 32), 1), ((1, 1, 1, 1, 1), 1), ((512, 512, 512, 64, 32), 1),
                         ((513, 96, 128, 64, 32), 0), ((64, 96, 513, 64, 32), 0), ((64, 96, 128, 65, 32), 0),
                         ((64, 96, 128, 64, 33), 0), ((64, 0, 128, 64, 32), 0), ((32, 48, 64, 32, 16), 1)):
        assert lib.rmd_matching_net_supported(*widths, 8, 12) == want, widths
        assert library.mnet_supported(*widths, 8, 12) == bool(want)
    for c3, c4, h2, w2, want in ((64, 32, 1, 1, 1), (1, 1, 1, 1, 1), (24, 12, 2, 3, 1), (65, 32, 1, 1, 0), (64, 33, 1, 1, 0),
                                 (0, 32, 1, 1, 0), (64, 32, 0, 1, 0), (64, 32, 4096, 4096, 0), (63, 32, 4096, 4096, 1)):
        assert lib.rmd_mnet_tail_supported(c3, c4, h2, w2) == want, (c3, c4, h2, w2)
    assert lib.rmd_mnet_tail_workspace_bytes(65, 32) == 0 and lib.rmd_mnet_tail_workspace_bytes(64, 0) == 0


def _round(n, to=256):
    return -(-n // to) * to


def _frag_bytes(c, cout, taps):
    """Packed MFMA A fragments: 32-row tiles x taps x 16-channel k-steps x 64 lanes x 16 bytes x 2 parts."""
    return -(-cout // 32) * taps * -(-c // 16) * 64 * 16 * 2


def test_workspace_bytes_are_the_packed_weights_and_one_groups_maps():
    from rmd import _lib
    lib = _lib.lib()
    for widths, h, w in ((WIDTHS, 48, 160), ((34, 96, 128, 64, 32), 4, 6), ((16, 48, 64, 32, 16), 6, 10),
                         ((5, 7, 9, 11, 3), 2, 2)):
        c_in, c1, c2, c3, c4 = widths
        packed = (_frag_bytes(c_in, c1, 9) + _frag_bytes(c1, c2, 9) + _frag_bytes(c2, c2, 9) + _frag_bytes(c2, c3, 9)
                  + 16 * -(-c3 // 16) * 64 * 16 * 2)
        for group in (1, 4, 49):
            half = (h // 2) * (w // 2)
            maps = sum(_round(4 * group * n) for n in (c1 * h * w, c2 * half, c2 * half, c3 * half))
            assert lib.rmd_matching_net_workspace_bytes(group, *widths, h, w) == packed + maps + 256, (widths, group)
        assert lib.rmd_matching_net_workspace_bytes(0, *widths, h, w) == 0
        assert lib.rmd_matching_net_workspace_bytes(1, *widths, h + 1, w) == 0
        assert lib.rmd_mnet_tail_workspace_bytes(c3, c4) == 16 * -(-c3 // 16) * 64 * 16 * 2 + 256


def test_the_group_a_budget_gives():
    from rmd import library, ops
    h, w, n = 48, 160, 648
    one = library.mnet_workspace_bytes(1, *WIDTHS, h, w)
    for budget in (1, one - 1, one, 64 << 20, 128 << 20, 256 << 20, 512 << 20, 1 << 40):
        group = ops.mnet_group(n, WIDTHS, h, w, budget)
        assert 1 <= group <= n
        if group > 1:
            assert library.mnet_workspace_bytes(group, *WIDTHS, h, w) <= budget
        if group < n and budget >= one:
            assert library.mnet_workspace_bytes(group + 1, *WIDTHS, h, w) > budget
    assert ops.mnet_group(n, WIDTHS, h, w, 1) == 1 and ops.mnet_group(n, WIDTHS, h, w, 1 << 40) == n
    assert ops.mnet_group(n, WIDTHS, h, w) == ops.mnet_group(n, WIDTHS, h, w, ops.MNET_WORKSPACE_BYTES)
    assert ops.MNET_WORKSPACE_BYTES in (64 << 20, 128 << 20, 256 << 20, 512 << 20)
    with pytest.raises(ValueError, match="unsupported sizes"):
        ops.mnet_group(n, (64, 96, 128, 65, 32), h, w)


def test_the_c_abi_refuses_bad_arguments_before_any_launch():
    """Null pointers, overlaps, group < 1 and a bad compute mode are RMD_ERR_ARG (-1), unsupported sizes
    RMD_ERR_SHAPE (-2).  The checks precede the first launch, so host memory serves and nothing is written."""
    from rmd import _lib
    lib = _lib.lib()
    X3 = _lib.RMD_BF16X3
    widths = (4, 6, 8, 4, 2)
    shapes = [(6, 4, 3, 3), (8, 6, 3, 3), (8, 8, 3, 3), (4, 8, 3, 3), (4, 2, 4, 4), (2, 3, 3)]
    ws = [np.zeros(s, np.float32) for s in shapes]
    bs = [np.zeros(n, np.float32) for n in (6, 8, 8, 4, 2, 1)]
    x = np.zeros((2, 4, 4, 6), np.float32)
    cost = np.full((2, 4, 6), 7.0, np.float32)
    work = np.zeros(lib.rmd_matching_net_workspace_bytes(2, *widths, 4, 6), np.uint8)

    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def table(arrays):
        return (ctypes.c_void_p * 6)(*[None if a is None else a.ctypes.data for a in arrays])

    def net(x=x, ws=ws, bs=bs, cost=cost, work=work, images=2, group=2, widths=widths, h=4, w=6, compute=X3):
        rc = lib.rmd_matching_net(ptr(x), table(ws), table(bs), ptr(cost), ptr(work), images, group, *widths, h, w,
                                  compute, None)
        return rc, lib.rmd_last_error().decode()

    for kw, code, text in ((dict(x=None), -1, "null pointer"), (dict(cost=None), -1, "null pointer"),
                           (dict(work=None), -1, "null pointer"), (dict(ws=ws[:4] + [None] + ws[5:]), -1, "null weight or bias 4"),
                           (dict(bs=bs[:5] + [None]), -1, "null weight or bias 5"), (dict(group=0), -1, "group"),
                           (dict(group=-3), -1, "group"), (dict(compute=_lib.RMD_F32), -1, "compute"),
                           (dict(cost=x), -1, "overlap"), (dict(work=cost), -1, "overlap"),
                           (dict(ws=ws[:5] + [cost]), -1, "overlaps weight or bias 5"), (dict(images=0), -2, "bad sizes"),
                           (dict(h=5), -2, "unsupported"), (dict(w=7), -2, "unsupported"),
                           (dict(widths=(4, 6, 8, 65, 2)), -2, "unsupported"), (dict(widths=(4, 6, 8, 4, 33)), -2, "unsupported")):
        rc, msg = net(**kw)
        assert rc == code and text in msg, (kw.keys(), rc, msg)

    twork = np.zeros(lib.rmd_mnet_tail_workspace_bytes(4, 2), np.uint8)
    t = np.zeros((2, 4, 2, 3), np.float32)

    def tail(x=t, w5=ws[4], b5=bs[4], w6=ws[5], b6=bs[5], cost=cost, work=twork, c3=4, c4=2, h2=2, w2=3, compute=X3):
        rc = lib.rmd_mnet_tail(ptr(x), ptr(w5), ptr(b5), ptr(w6), ptr(b6), ptr(cost), ptr(work), 2, c3, c4, h2, w2, compute,
                               None)
        return rc, lib.rmd_last_error().decode()

    for kw, code, text in ((dict(b6=None), -1, "null pointer"), (dict(work=None), -1, "null pointer"),
                           (dict(cost=t), -1, "overlap"), (dict(work=ws[4]), -1, "overlap"),
                           (dict(compute=_lib.RMD_F16), -1, "compute"), (dict(c4=33), -2, "unsupported tail"),
                           (dict(c3=65), -2, "unsupported tail"), (dict(h2=0), -2, "bad sizes")):
        rc, msg = tail(**kw)
        assert rc == code and text in msg, (kw.keys(), rc, msg)
    assert (cost == 7.0).all() and not x.any() and not work.any() and not twork.any()
