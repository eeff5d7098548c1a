"""The fused k x k MatchingNet on the GPU: csrc/mnet.hip through torch.ops.rmd.mnet_tail and matching_net and the
drop-in modules with fused="on", against the tests' float64 restatement (mnet_cases.py) and the reference's
fixtures: the tail on seven shapes in both compute modes, one-hot weights against their closed forms (bitwise), the
whole network on four shapes, independence of the group size (bitwise), the fixtures with and without DAP, NaN and
inf, views, repeatability, opcheck, the no-host-synchronisation rule, the allocation bound and the argument checks.

Tolerance (mnet_cases.py): per case and mode max(1e-5, 3 e), e the error of the CPU float64 emulation of the mode (of
the emulated chain for the network) against float64 — never a figure of the kernel's.

A +-inf input gives NaN in its receptive field in the fp32 mode (inf - inf in the split's residual), where the
reference gives +-inf or NaN: the one documented deviation, as for the other fused convolutions.

Every test here calls the new operators: none can pass without the kernels."""

import numpy as np
import pytest
import torch

import mnet_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECISIONS = ("fp32", "bf16")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tail(args, precision):
    from rmd import ops
    return ops.mnet_tail(*(_t(a) for a in args), precision=precision)


def _net(args, precision, **kwargs):
    from rmd import ops
    mvol, weights, biases = args
    return ops.matching_net(_t(mvol), [_t(w) for w in weights], [_t(b) for b in biases], precision=precision, **kwargs)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", cases.TAIL_SHAPES, ids=cases.TAIL_IDS)
def test_tail_against_float64(shape, precision):
    c = cases.tail_case(shape)
    out = _tail(c["args"], precision)
    assert out.shape == c["ref"].shape and out.dtype == torch.float32 and out.is_contiguous()
    err = cases.max_norm_err(out.cpu().numpy(), c["ref"])
    print(f"{shape} [{precision}]: kernel {err:.3e}  emulation e {c['e'][precision]:.3e}  tolerance {c['tol'][precision]:.3e}")
    assert err <= c["tol"][precision], (shape, precision, err, c["tol"][precision])


def test_tail_samples_do_not_depend_on_the_batch_and_runs_repeat():
    args = cases.tail_case(cases.BATCH_TAIL)["args"]
    for precision in PRECISIONS:
        full = _tail(args, precision)
        assert torch.equal(_bits(full), _bits(_tail(args, precision)))
        for n in range(args[0].shape[0]):
            alone = _tail((args[0][n:n + 1],) + args[1:], precision)
            assert torch.equal(_bits(alone[0]), _bits(full[n])), (precision, n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_hot_transposed_weights_give_the_scattered_relu(precision):
    """A single W5'[c, o, ky, kx] = 1, t5 = 0, w6 one-hot at the centre of channel o: the cost is b6 + relu(x[c])
    scattered at stride 2 by the tap, bit for bit on dyadic data.  All 16 taps; the positions checked by name are an
    interior one, the four corners, an edge and one on the seam of two tiles; the whole map is compared."""
    n, c3, c4, h2, w2 = cases.ONEHOT_SHAPE
    rng = np.random.default_rng(5)
    x = cases.dyadic(rng, (n, c3, h2, w2))
    b6 = np.float32(0.25)
    k = 0
    for ky in range(4):
        for kx in range(4):
            c, o = (0, 15, 16, 23)[k % 4], (0, 11, 5)[k % 3]
            k += 1
            w5 = np.zeros((c3, c4, 4, 4), np.float32)
            w5[c, o, ky, kx] = 1.0
            w6 = np.zeros((c4, 3, 3), np.float32)
            w6[o, 1, 1] = 1.0
            got = _tail((x, w5, np.zeros(c4, np.float32), w6, np.array([b6])), precision).cpu().numpy()
            want = (cases.w5_onehot_expected(x, c, ky, kx) + np.float64(b6)).astype(np.float32)
            assert np.array_equal(got, want), (precision, ky, kx, np.argwhere(got != want)[:4])
            for iy, ix in cases.ONEHOT_POSITIONS:
                yy, xx = 2 * iy - 1 + ky, 2 * ix - 1 + kx
                if 0 <= yy < 2 * h2 and 0 <= xx < 2 * w2:
                    assert got[0, yy, xx] == np.float32(max(x[0, c, iy, ix], 0.0) + b6)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_hot_last_layer_sees_zero_padding_not_relu_of_the_bias(precision):
    """W5' = 0 and t5 = 0.5: u is 0.5 inside the map, and a tap of w6 that leaves the map must read zero — a ring
    of relu(t5) would give b6 + 0.5 on the border too.  All 9 taps, bit for bit."""
    shape = cases.ONEHOT_SHAPE
    n, c3, c4, h2, w2 = shape
    rng = np.random.default_rng(6)
    x = cases.dyadic(rng, (n, c3, h2, w2))
    b6 = np.float32(-0.75)
    for i in range(3):
        for j in range(3):
            o = (0, 11, 7)[(3 * i + j) % 3]
            w6 = np.zeros((c4, 3, 3), np.float32)
            w6[o, i, j] = 1.0
            got = _tail((x, np.zeros((c3, c4, 4, 4), np.float32), np.full(c4, 0.5, np.float32), w6, np.array([b6])),
                        precision).cpu().numpy()
            want = cases.w6_onehot_expected(shape, i, j, b6).astype(np.float32)
            assert np.array_equal(got, want), (precision, i, j, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", cases.NET_SHAPES, ids=cases.NET_IDS)
def test_whole_network_against_float64(shape, precision):
    c = cases.net_case(shape)
    out = _net(c["args"], precision)
    assert out.shape == c["ref"].shape and out.dtype == torch.float32
    err = cases.max_norm_err(out.cpu().numpy(), c["ref"])
    print(f"{shape} [{precision}]: kernel {err:.3e}  emulation e {c['e'][precision]:.3e}  tolerance {c['tol'][precision]:.3e}")
    assert err <= c["tol"][precision], (shape, precision, err, c["tol"][precision])


def test_the_result_does_not_depend_on_the_group():
    """49 images in groups of 4 (a last group of 1), of 49 and of 1: the same bits."""
    from rmd import _lib
    c = cases.net_case(cases.GROUP_SHAPE)
    mvol, ws, bs = _t(c["args"][0]), [_t(w) for w in c["args"][1]], [_t(b) for b in c["args"][2]]
    for compute, precision in ((_lib.RMD_BF16X3, "fp32"), (_lib.RMD_BF16, "bf16")):
        outs = [torch.ops.rmd.matching_net(mvol, ws, bs, group, compute) for group in (4, 49, 1, 4)]
        for o in outs[1:]:
            assert torch.equal(_bits(o), _bits(outs[0])), precision
        err = cases.max_norm_err(outs[0].cpu().numpy(), c["ref"])
        assert err <= c["tol"][precision], (precision, err)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", cases.FIXTURES)
def test_fixtures_through_the_fused_modules(name, precision):
    """The fixtures through fused="on" modules, with and without DAP.  The MatchingNet cost (a forward hook on
    `mnet`, which fires once per call) is held to the chain tolerance against the float64 restatement and has the
    reference's NaN positions.  Everything after the cost is the unchanged module code, so the module output must be,
    bit for bit, what the `off` module computes from that cost (a hook on its `mnet` hands it over)."""
    g, c = cases.fixture(name), cases.fixture_case(name)
    on, off = cases.build_module(name, DEV, fused="on", precision=precision), cases.build_module(name, DEV)
    args = (_t(g["fmap1"]), _t(g["fmap2"]), _t(g["coords"]))
    with torch.no_grad():
        for dap in (True, False):
            cap = []
            hook = on.mnet.register_forward_hook(lambda m, i, o: cap.append(o))
            out = on(*args, dap=dap)
            hook.remove()
            assert len(cap) == 1
            cost = cap[0].cpu().numpy()
            assert np.array_equal(np.isnan(cost), np.isnan(g["nodap.cost"])), "NaN positions differ from the reference's"
            err = cases.max_norm_err(cost, c["ref"])
            print(f"{name} [{precision}, dap={dap}]: kernel {err:.3e}  tolerance {c['tol'][precision]:.3e}")
            assert err <= c["tol"][precision], (name, precision, dap, err, c["tol"][precision])
            hook = off.mnet.register_forward_hook(lambda m, i, o: cap[0])
            want = off(*args, dap=dap)
            hook.remove()
            assert out.shape == want.shape == g["dap.out"].shape
            assert torch.equal(_bits(out), _bits(want))


def test_nan_positions_are_the_eager_modules_and_inf_gives_nan():
    """NaN costs where the `off` module on the CPU has them; a +inf entry of the stack gives NaN in its receptive
    field in the fp32 mode (the documented deviation) and nowhere else."""
    name = cases.NAN_FIXTURE
    g = cases.fixture(name)
    cpu = cases.build_module(name)
    with torch.no_grad():
        want = cpu.mnet(torch.from_numpy(cases.fixture_case(name)["args"][0]))
    assert torch.isnan(want).any()
    c = cases.fixture_case(name)
    for precision in PRECISIONS:
        got = _net(c["args"], precision).cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), precision
    clean = cases.net_case(cases.NET_SHAPES[0])
    mvol = clean["args"][0].copy()
    mvol[0, 1, 2, 5, 4, 7] = np.inf
    got = _net((mvol,) + clean["args"][1:], "fp32").cpu().numpy()
    assert np.isnan(got[0, 1, 2]).any() and np.isfinite(np.delete(got.reshape(9, 8, 12), 5, axis=0)).all()
    ref = cases.net_ref(mvol.reshape(9, 32, 8, 12), *clean["args"][1:]).reshape(got.shape)
    assert np.array_equal(np.isnan(got), ~np.isfinite(ref))


def test_views_give_the_results_of_their_contiguous_copies():
    from rmd import _lib
    c = cases.net_case(cases.NET_SHAPES[2])
    mvol, ws, bs = _t(c["args"][0]), [_t(w) for w in c["args"][1]], [_t(b) for b in c["args"][2]]
    ref = torch.ops.rmd.matching_net(mvol, ws, bs, 7, _lib.RMD_BF16X3)

    def offset(t):                                          # the same values one element into a larger buffer
        buf = torch.zeros(t.numel() + 1, device=DEV)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    def strided(t):                                         # a non-contiguous view with the same values
        return torch.stack([t, t], dim=-1)[..., 0]

    for view in (offset, strided):
        got = torch.ops.rmd.matching_net(view(mvol), [view(w) for w in ws], [view(b) for b in bs], 7, _lib.RMD_BF16X3)
        assert torch.equal(_bits(got), _bits(ref))
    t = cases.tail_case(cases.TAIL_SHAPES[2])
    targs = [_t(a) for a in t["args"]]
    tref = torch.ops.rmd.mnet_tail(*targs, _lib.RMD_BF16)
    for view in (offset, strided):
        assert torch.equal(_bits(torch.ops.rmd.mnet_tail(*[view(a) for a in targs], _lib.RMD_BF16)), _bits(tref))


def test_opcheck():
    import rmd  # noqa: F401
    from rmd import _lib
    t = [_t(a) for a in cases.tail_case(cases.TAIL_SHAPES[2])["args"]]
    c = cases.net_case(cases.NET_SHAPES[1])
    nargs = (_t(c["args"][0]), [_t(w) for w in c["args"][1]], [_t(b) for b in c["args"][2]])
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    for compute in (_lib.RMD_BF16X3, _lib.RMD_BF16):
        torch.library.opcheck(torch.ops.rmd.mnet_tail, (*t, compute), test_utils=utils)
        torch.library.opcheck(torch.ops.rmd.matching_net, (*nargs, 1, compute), test_utils=utils)
    assert not torch.ops.rmd.mnet_tail(t[0].clone().requires_grad_(True), *t[1:], _lib.RMD_BF16X3).requires_grad
    assert not torch.ops.rmd.matching_net(nargs[0].clone().requires_grad_(True), *nargs[1:], 2,
                                          _lib.RMD_BF16X3).requires_grad


def test_the_fused_network_never_waits_for_the_host_and_stays_in_its_workspace():
    """Sync-debug mode over fused calls of a batch-norm and a norm-free module (the batch norm is folded on the
    device), then the operator's peak allocation: the output and the workspace, nothing else."""
    import rmd  # noqa: F401
    from rmd import _lib
    names = (cases.FIXTURES[0], cases.FIXTURES[1])
    mods = [cases.build_module(n, DEV, fused="on") for n in names]
    args = [tuple(_t(cases.fixture(n)[k]) for k in ("fmap1", "fmap2", "coords")) for n in names]
    with torch.no_grad():
        for m, a in zip(mods, args):
            m(*a)                                           # the warm-up call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            for m, a in zip(mods, args):
                m(*a)
    finally:
        torch.cuda.set_sync_debug_mode("default")

    c = cases.net_case(cases.GROUP_SHAPE)
    mvol, ws, bs = _t(c["args"][0]), [_t(w) for w in c["args"][1]], [_t(b) for b in c["args"][2]]
    for group in (4, 49):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = torch.ops.rmd.matching_net(mvol, ws, bs, group, _lib.RMD_BF16X3)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        bound = out.numel() * 4 + _lib.lib().rmd_matching_net_workspace_bytes(group, 32, 96, 128, 64, 32, 4, 6)
        assert peak <= bound + 2 * 512, (group, peak, bound)    # the allocator rounds each of the two blocks up to 512 bytes


def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    import rmd  # noqa: F401
    from rmd import _lib, ops
    from rmd.blocks.dicl import MatchingNet
    X3 = _lib.RMD_BF16X3
    c = cases.net_case(cases.NET_SHAPES[1])
    mvol, ws, bs = _t(c["args"][0]), [_t(w) for w in c["args"][1]], [_t(b) for b in c["args"][2]]
    t = [_t(a) for a in cases.tail_case(cases.TAIL_SHAPES[2])["args"]]
    assert MatchingNet(34, "none", fused="auto").to(DEV)(mvol).requires_grad       # the sequential path, which trains
    on = {norm: MatchingNet(34, norm, fused="on").to(DEV).eval() for norm in ("none", "batch", "group", "instance")}
    supported = _lib.lib().rmd_matching_net_supported

    class NoLaunch:
        def __getattr__(self, name):
            if name == "rmd_matching_net_supported":
                return supported                            # host only
            raise AssertionError(f"reached {name}")

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="autocast"):
            on["none"](mvol)
    with pytest.raises(RuntimeError, match="gradient"):
        on["none"](mvol)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="train-mode batch norm"):
            on["batch"].train()(mvol)
        for norm in ("group", "instance"):
            with pytest.raises(RuntimeError, match="group, instance"):
                on[norm](mvol)
        with pytest.raises(RuntimeError, match="odd"):
            on["none"](torch.zeros(1, 1, 1, 34, 3, 4, device=DEV))
        with pytest.raises(RuntimeError, match="not all float32"):
            on["none"](mvol.double())
        with pytest.raises(RuntimeError, match="unsupported widths"):
            MatchingNet(34, "none", scale=3, fused="on").to(DEV)(mvol)      # c3 = 192
    cpu = torch.Tensor.cpu
    for fn in (lambda: torch.ops.rmd.matching_net(mvol, ws[:2] + [cpu(ws[2])] + ws[3:], bs, 1, X3),
               lambda: torch.ops.rmd.mnet_tail(t[0], t[1], cpu(t[2]), t[3], t[4], X3)):
        with pytest.raises(ValueError, match="must be on the GPU"):
            fn()
    with pytest.raises(ValueError, match="different devices"):
        ops.matching_net(mvol, ws, bs[:5] + [cpu(bs[5])])
    with pytest.raises(ValueError, match="need 6 weights"):
        torch.ops.rmd.matching_net(mvol, ws[:5], bs, 1, X3)
    with pytest.raises(ValueError, match="weights\\[4\\]"):
        torch.ops.rmd.matching_net(mvol, ws[:4] + [ws[4][:, :, :3].contiguous()] + ws[5:], bs, 1, X3)
    with pytest.raises(ValueError, match="group"):
        torch.ops.rmd.matching_net(mvol, ws, bs, 0, X3)
    with pytest.raises(ValueError, match="even"):
        torch.ops.rmd.matching_net(torch.zeros(1, 1, 1, 34, 3, 4, device=DEV), ws, bs, 1, X3)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.matching_net(mvol, ws, bs, 1, _lib.RMD_F32)
    with pytest.raises(ValueError, match="compute"):
        torch.ops.rmd.mnet_tail(*t, _lib.RMD_F32)
    with pytest.raises(ValueError, match="weight6"):
        torch.ops.rmd.mnet_tail(t[0], t[1], t[2], t[3][:, :2].contiguous(), t[4], X3)
    with pytest.raises(ValueError, match="precision"):
        ops.matching_net(mvol, ws, bs, precision="fp16")


def test_the_c_abi_checks_run_before_any_launch():
    """Null pointers, overlaps and group < 1 are RMD_ERR_ARG, unsupported sizes RMD_ERR_SHAPE; the launchers return
    before their first launch, so the buffers are never touched."""
    import ctypes
    import rmd  # noqa: F401
    from rmd import _lib
    from rmd.library import _pointers
    X3 = _lib.RMD_BF16X3
    widths = (4, 6, 8, 4, 2)
    rng = np.random.default_rng(0)
    x = torch.zeros(2, 4, 4, 6, device=DEV)
    cost = torch.full((2, 4, 6), 7.0, device=DEV)
    chans = [(6, 4, 3, 3), (8, 6, 3, 3), (8, 8, 3, 3), (4, 8, 3, 3), (4, 2, 4, 4), (2, 3, 3)]
    ws = [_t(rng.standard_normal(s).astype(np.float32)) for s in chans]
    bs = [torch.zeros(n, device=DEV) for n in (6, 8, 8, 4, 2, 1)]
    work = _lib.workspace("matching_net", x, 2, *widths, 4, 6)
    good = (x, _pointers(ws), _pointers(bs), cost, work, 2, 2, *widths, 4, 6, X3)

    def call(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        _lib.launch("rmd_matching_net", x, *args)

    with pytest.raises(_lib.RmdError, match=r"code -1\).*null pointer"):
        call(a3=None)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*null weight or bias 5"):
        call(a2=(ctypes.c_void_p * 6)(*[b.data_ptr() for b in bs[:5]], None))
    with pytest.raises(_lib.RmdError, match=r"code -1\).*overlap"):
        call(a3=x)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*overlap"):
        call(a4=cost)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*group"):
        call(a6=0)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*compute"):
        call(a14=_lib.RMD_F32)
    with pytest.raises(_lib.RmdError, match=r"code -2\).*unsupported"):
        call(a12=5)                                         # an odd height
    with pytest.raises(_lib.RmdError, match=r"code -2\).*unsupported"):
        call(a10=65)                                        # c3 above 64
    twork = _lib.workspace("mnet_tail", x, 4, 2)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*null pointer"):
        _lib.launch("rmd_mnet_tail", x, x, ws[4], bs[4], ws[5], None, cost, twork, 2, 4, 2, 4, 6, X3)
    with pytest.raises(_lib.RmdError, match=r"code -1\).*overlap"):
        _lib.launch("rmd_mnet_tail", x, x, ws[4], bs[4], ws[5], bs[5], x, twork, 2, 4, 2, 4, 6, X3)
    with pytest.raises(_lib.RmdError, match=r"code -2\).*unsupported tail"):
        _lib.launch("rmd_mnet_tail", x, x, ws[4], bs[4], ws[5], bs[5], cost, twork, 2, 4, 33, 4, 6, X3)
    lib = _lib.lib()
    assert lib.rmd_matching_net_workspace_bytes(0, *widths, 4, 6) == 0
    assert lib.rmd_matching_net_workspace_bytes(1, *widths, 5, 6) == 0
    assert lib.rmd_matching_net_supported(*widths, 4, 6) == 1 and lib.rmd_matching_net_supported(*widths, 4, 7) == 0
    assert lib.rmd_mnet_tail_supported(64, 32, 1, 1) == 1 and lib.rmd_mnet_tail_supported(65, 32, 1, 1) == 0
    assert lib.rmd_mnet_tail_workspace_bytes(4, 33) == 0
    torch.cuda.synchronize()
    assert torch.equal(cost, torch.full((2, 4, 6), 7.0, device=DEV)) and not x.any()
