"""Flow metrics on the GPU: the HIP path of the drop-in classes (csrc/metrics.hip through
torch.ops.rmd.flow_metrics) against the fixtures the reference's classes wrote
(tests/golden/gen_golden_metrics.py; the gate — exact counts, means no farther from the reference than
the reference is from float64 plus 1e-6 — is in metrics_cases.py), the planted on-threshold pixels, a
shape sweep against the CPU kernel, NaN / Inf / empty masks, determinism, dtypes, opcheck and the
no-host-synchronisation rule."""

import functools
import math

import numpy as np
import pytest
import torch

import metrics_cases
from metrics_cases import CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
SUM_SLOTS = [2, 4, 5, 6]


@pytest.mark.parametrize("name,index", CASES)
def test_hip_classes_reproduce_the_reference(name, index):
    """Every class, for the batch and per sample, from one FlowMetrics launch each."""
    import rmd
    c = metrics_cases.case(name)
    fm = rmd.FlowMetrics.from_config(c.configs[index])
    est, tgt, val = c.tensors(DEV)
    batch = fm(None, est, tgt, val, None)
    samples = fm.per_sample(None, est, tgt, val)
    metrics_cases.check_against_fixture(c, index, batch, samples)


@pytest.mark.parametrize("name", ["metrics_main", "metrics_small"])
def test_planted_pixels_fall_on_the_reference_side(name):
    """Pixels exactly ON a threshold: epe 5, 3, 1 and 0 count for `<= 5`, `<= 3`, `<= 1`; epe 3 is no outlier
    (`> 3` is false).  Checked by masking everything but the planted pixels of one sample."""
    from rmd import ops
    c = metrics_cases.case(name)
    est, tgt, _ = c.tensors(DEV)
    only = np.zeros_like(c.valid)
    for (b, y, x, _, _) in c.planted:
        only[b, y, x] = True
    s = ops.flow_metrics(est, tgt, torch.from_numpy(only).to(DEV)).host().stats[0]
    for b in range(c.batch):
        epes = sorted(math.hypot(d0, d1) for (pb, _, _, d0, d1) in c.planted if pb == b)
        assert s[b, 1] == len(epes)
        assert s[b, 2] == sum(epes)                                         # exact arithmetic
        assert s[b, 3] == sum(e > 3 for e in epes)                          # 0.05 * |(1.5, -2)| = 0.125 is far below
        assert [float(v) for v in s[b, 8:11]] == [sum(e <= d for e in epes) for d in (1, 3, 5)]


SWEEP = [(1, 1, 1), (1, 3, 5), (2, 4, 8), (3, 37, 53), (2, 20, 36), (1, 130, 257)]
DIST = (1.0, 3.0, 5.0, 0.5, 7.25)


@functools.lru_cache(maxsize=None)
def _sweep_inputs(shape):
    b, h, w = shape
    est, tgt, val = metrics_cases.fair_inputs((b, 2, h, w), 0.7, DIST, seed0=10 * h, scales=(1.0, 0.5))
    est2 = (est * 0.5).contiguous()
    ref = {o: torch.ops.rmd.flow_metrics([est, est2], tgt, val, list(DIST), 3.0, 0.05, o) for o in (2.0, 1.0, math.inf, 3.0)}
    return est, est2, tgt, val, ref


def _assert_stats(got, ref, label):
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape
    counts = [s for s in range(ref.shape[-1]) if s not in SUM_SLOTS]
    assert torch.equal(got[..., counts], ref[..., counts]), (label, got[..., counts], ref[..., counts])
    for s in SUM_SLOTS:
        err = ((got[..., s] - ref[..., s]).abs() / ref[..., s].abs()).max()
        print(f"{label} slot {s}: max relative {float(err):.3e}")
        assert torch.allclose(got[..., s], ref[..., s], rtol=1e-6, atol=0), (label, s)


@pytest.mark.parametrize("shape", SWEEP)
def test_shape_sweep_against_the_cpu_kernel(shape):
    """Counts exact, sums 1e-6 relative, every magnitude norm; (1,.,1,1) and the odd planes take the scalar
    path, (2,.,4,8) is less than one wave on the vector path, 37x53 two tiles per sample with a tail,
    130x257 many blocks."""
    est, est2, tgt, val, ref = _sweep_inputs(shape)
    for o, r in ref.items():
        got = torch.ops.rmd.flow_metrics([est.to(DEV), est2.to(DEV)], tgt.to(DEV), val.to(DEV), list(DIST), 3.0, 0.05, o)
        _assert_stats(got, r, f"{shape} ord {o}")


def _offset(t):
    """A contiguous copy of t whose storage starts one element past an aligned base."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view_as(t)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % (4 * t.element_size()) != 0
    return view


@pytest.mark.parametrize("which", ["estimate", "target", "valid"])
def test_offset_views_take_the_scalar_path(which):
    """H*W % 4 == 0 but one base pointer off its alignment: the scalar path, same numbers."""
    est, est2, tgt, val, ref = _sweep_inputs((2, 20, 36))
    args = {"estimate": est2.to(DEV), "target": tgt.to(DEV), "valid": val.to(DEV)}
    args[which] = _offset(args[which])
    got = torch.ops.rmd.flow_metrics([est.to(DEV), args["estimate"]], args["target"], args["valid"], list(DIST), 3.0, 0.05, 2.0)
    _assert_stats(got, ref[2.0], f"offset {which}")


def test_nan_inf_and_empty_mask():
    """NaN at an invalid pixel leaves slots 2, 3 and 8... of its sample as they were and reaches 4, 6, 7; at
    a valid pixel slot 2 of THAT sample is NaN and no other row changes; an all-false mask gives a 0
    count and NaN means."""
    from rmd import ops
    est, _, tgt, val, _ = _sweep_inputs((3, 37, 53))
    est, tgt, val = est.to(DEV), tgt.to(DEV), val.to(DEV)
    base = ops.flow_metrics(est, tgt, val).host().stats[0]
    vnp = val.cpu().numpy()
    y, x = [int(v[0]) for v in np.nonzero(~vnp[1])]
    bad = est.clone()
    bad[1, 0, y, x] = float("nan")
    s = ops.flow_metrics(bad, tgt, val).host().stats[0]
    assert torch.equal(s[[0, 2]], base[[0, 2]])
    assert torch.equal(s[1, [0, 1, 2, 3, 5, 8, 9, 10]], base[1, [0, 1, 2, 3, 5, 8, 9, 10]])
    assert torch.isnan(s[1, 4]) and torch.isnan(s[1, 6]) and s[1, 7] == 1 and base[1, 7] == 0
    y, x = [int(v[0]) for v in np.nonzero(vnp[2])]
    bad = est.clone()
    bad[2, 1, y, x] = float("nan")
    s = ops.flow_metrics(bad, tgt, val).host().stats[0]
    assert torch.equal(s[[0, 1]], base[[0, 1]])
    assert torch.isnan(s[2, 2]) and torch.isnan(s[2, 4]) and torch.isnan(s[2, 5]) and s[2, 7] == 1
    assert s[2, 3] == base[2, 3] - (1 if _is_outlier(est, tgt, 2, y, x) else 0)     # a comparison with NaN is false
    bad = est.clone()
    bad[0, 0, 0, 0] = float("inf")
    s = ops.flow_metrics(bad, tgt, val).host().stats[0]
    assert torch.isinf(s[0, 6]) and s[0, 7] == 1 and torch.equal(s[1:], base[1:])
    empty = val.clone()
    empty[1] = False
    r = ops.flow_metrics(est, tgt, empty).host()
    assert r.stats[0, 1, 1] == 0 and r.stats[0, 1, 2] == 0 and r.stats[0, 1, 3] == 0
    ps = r.per_sample()
    assert torch.isnan(ps["epe"][0, 1]) and torch.isnan(ps["fl_all"][0, 1]) and torch.isnan(ps["within"][0, 1]).all()
    assert torch.isfinite(ps["aae"][0, 1]) and torch.isfinite(ps["epe"][0, 0]) and torch.isfinite(r.batch()["epe"][0])


def _is_outlier(est, tgt, b, y, x):
    epe = float((est[b, :, y, x] - tgt[b, :, y, x]).norm())
    return epe > 3 and epe > 0.05 * float(tgt[b, :, y, x].norm())


def test_determinism():
    """Two runs are bitwise equal; N estimates in one call equal N single calls; batch() is the index-order
    sum of the per-sample rows."""
    from rmd import ops
    est, est2, tgt, val, _ = _sweep_inputs((3, 37, 53))
    ests = [est.to(DEV), est2.to(DEV), (est * 1.5).to(DEV)]
    tgt, val = tgt.to(DEV), val.to(DEV)
    a = ops.flow_metrics(ests, tgt, val)
    b = ops.flow_metrics(ests, tgt, val)
    assert torch.equal(a.stats, b.stats)
    for k, e in enumerate(ests):
        assert torch.equal(ops.flow_metrics(e, tgt, val).stats[0], a.stats[k])
    total = a.stats[:, 0] + a.stats[:, 1] + a.stats[:, 2]
    assert torch.equal(a.batch_stats(), total)
    assert torch.equal(a.batch()["epe"], total[:, 2] / total[:, 1])
    est, est2, tgt, val, _ = _sweep_inputs((2, 20, 36))                     # the vector path
    ests = [est.to(DEV), est2.to(DEV)]
    a = ops.flow_metrics(ests, tgt.to(DEV), val.to(DEV))
    assert torch.equal(ops.flow_metrics(ests[1], tgt.to(DEV), val.to(DEV)).stats[0], a.stats[1])
    assert torch.equal(ops.flow_metrics(ests, tgt.to(DEV), val.to(DEV)).stats, a.stats)


def test_dtypes_and_layouts():
    """fp16 / bf16 estimates are widened (the fixture's values are fp16-exact), uint8 masks equal bool masks,
    non-contiguous inputs are made contiguous, a single instance is a batch of one."""
    from rmd import ops
    c = metrics_cases.case("metrics_small")
    est, tgt, val = c.tensors(DEV)
    base = ops.flow_metrics(est, tgt, val).stats
    assert torch.equal(ops.flow_metrics(est.half(), tgt.half(), val).stats, base)
    bf = est.bfloat16()
    assert torch.equal(ops.flow_metrics(bf, tgt, val).stats, ops.flow_metrics(bf.float(), tgt, val).stats)
    assert torch.equal(ops.flow_metrics(est, tgt, val.to(torch.uint8) * 255).stats, base)
    wide = torch.zeros(2, 2, 20, 72, device=DEV)
    wide[..., ::2] = est
    assert torch.equal(ops.flow_metrics(wide[..., ::2], tgt, val).stats, base)
    assert torch.equal(ops.flow_metrics(est[1], tgt[1], val[1]).stats[:, 0], base[:, 1])


def test_opcheck_operator():
    c = metrics_cases.case("metrics_small")
    est, tgt, val = c.tensors(DEV)
    torch.library.opcheck(torch.ops.rmd.flow_metrics, ([est, est * 0.5], tgt, val, [1.0, 3.0], 3.0, 0.05, 2.0),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    assert not torch.ops.rmd.flow_metrics([est.clone().requires_grad_(True)], tgt, val, [], 3.0, 0.05, 2.0).requires_grad


def test_no_host_synchronisation():
    """ops.flow_metrics, per_sample() and batch() up to but excluding host() under sync-debug mode 'error'.
    The mode is shown to work on this build first: nonzero() (what the reference's epe[valid] launches)
    raises.  The loss rides in host()'s single copy."""
    from rmd import ops
    c = metrics_cases.case("metrics_main")
    est, tgt, val = c.tensors(DEV)
    loss = torch.tensor(0.75, device=DEV)
    ops.flow_metrics([est, est], tgt, val).batch()                          # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            val.nonzero()
        r = ops.flow_metrics([est, est.half()], tgt, val, distances=(1, 3, 5), extra=loss)
        ps, bt = r.per_sample(), r.batch()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    h = r.host()
    assert h.stats.device.type == "cpu" and float(h.extra) == 0.75
    assert torch.equal(h.per_sample()["epe"], ps["epe"].cpu()) and torch.equal(h.batch()["within"], bt["within"].cpu())
    ref = dict(c.results[0]["batch"][0]["result"])["EndPointError/mean"]
    assert abs(float(h.batch()["epe"][1]) - ref) <= 1e-5 * ref
