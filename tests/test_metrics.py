"""Flow metrics without a GPU: the CPU dispatch of the drop-in classes (rmd/metrics.py over rmd/cpu.py's
restatement of the reference's expressions) reproduces the fixtures the reference's own classes wrote
(tests/golden/gen_golden_metrics.py; the gate is in metrics_cases.py), the classes keep the
reference's type strings, configs and keys, the C ABI rejects bad arguments before any launch, and the
operator is registered in its own table with a fake kernel that propagates shapes."""

import ctypes
import json
import math

import numpy as np
import pytest
import torch

import metrics_cases
from metrics_cases import CASES


@pytest.mark.parametrize("name,index", CASES)
def test_cpu_classes_reproduce_the_reference(name, index):
    import rmd
    c = metrics_cases.case(name)
    fm = rmd.FlowMetrics.from_config(c.configs[index])
    est, tgt, val = c.tensors("cpu")
    batch = fm(None, est, tgt, val, None)
    samples = fm.per_sample(None, est, tgt, val)
    assert len(samples) == c.batch
    metrics_cases.check_against_fixture(c, index, batch, samples)


@pytest.mark.parametrize("name,index", CASES)
def test_config_and_type_match_the_reference(name, index):
    from rmd import metrics
    c = metrics_cases.case(name)
    for cfg, entry in zip(c.configs[index], c.results[index]["batch"]):
        m = metrics.Metric.from_config(cfg)
        assert m.type == cfg["type"] == entry["config"]["type"]
        assert json.loads(json.dumps(m.get_config())) == entry["config"]
        assert type(m).from_config(m.get_config()).get_config() == m.get_config()


def test_registry_and_defaults():
    """Defaults of argument-less instances (epe.py:22, fl_all.py:19, aae.py:19, flow.py:20, loss.py:18); the
    registry raises the reference's errors: KeyError for a type it does not hold, ValueError for a mismatch."""
    from rmd import metrics
    assert metrics.EndPointError().get_config() == {"type": "epe", "key": "EndPointError/", "distances": [1, 3, 5]}
    assert metrics.FlAll().get_config() == {"type": "fl-all", "key": "Fl-all"}
    assert metrics.AverageAngularError().get_config() == {"type": "aae", "key": "AverageAngularError"}
    assert metrics.FlowMagnitude().get_config() == {"type": "flow-magnitude", "key": "FlowMagnitude", "ord": 2}
    assert metrics.Loss().get_config() == {"type": "loss", "key": "Loss"}
    for t in ("grad-norm", "grad-mean", "grad-minmax", "param-norm", "param-mean", "param-minmax", "learning-rate"):
        with pytest.raises(KeyError):
            metrics.Metric.from_config({"type": t})
    with pytest.raises(ValueError, match="invalid metric type"):
        metrics.FlAll.from_config({"type": "epe"})
    assert metrics.EndPointError().reduce({"a": [1.0, 3.0], "b": [2.0]}) == {"a": 2.0, "b": 2.0}


def test_single_classes_single_instances_and_the_loss():
    """Each class's compute equals its share of the FlowMetrics result; (2, H, W) / (H, W) inputs are a batch
    of one; the default evaluation set (epe, fl-all, loss) keeps the reference's key order, the loss
    tensor's value passing through."""
    import rmd
    from rmd import metrics
    c = metrics_cases.case("metrics_main")
    est, tgt, val = c.tensors("cpu")
    fm = rmd.FlowMetrics.from_config(c.configs[1])
    whole = fm(None, est, tgt, val, None)
    for m in fm.metrics:
        part = m(None, None, est, tgt, val, None)
        assert all(whole[k] == v for k, v in part.items()) and len(part) >= 1
    samples = fm.per_sample(None, est, tgt, val)
    for b in range(c.batch):
        assert fm(None, est[b], tgt[b], val[b], None) == samples[b]
    default = rmd.FlowMetrics.from_config([{"type": "epe"}, {"type": "fl-all"}, {"type": "loss"}])
    loss = torch.tensor(1.25, dtype=torch.float32)
    out = default(None, est, tgt, val, loss)
    assert list(out) == ["EndPointError/mean", "EndPointError/1px", "EndPointError/3px", "EndPointError/5px", "Fl-all",
                         "Loss"]
    assert out["Loss"] == 1.25 and metrics.Loss()(None, None, est, tgt, val, loss) == {"Loss": 1.25}


def test_slot_table_of_the_cpu_kernel():
    """The raw statistics: counts are whole numbers, unused slots 0, fp16 / bf16 estimates are widened,
    uint8 masks equal bool masks, a non-contiguous estimate equals its contiguous copy, the result carries
    no graph, and more than 8 distances / 32 estimates are chunked."""
    from rmd import ops
    c = metrics_cases.case("metrics_small")
    est, tgt, val = c.tensors("cpu")
    r = ops.flow_metrics(est, tgt, val)
    raw = torch.ops.rmd.flow_metrics([est], tgt, val, [1.0, 3.0, 5.0], 3.0, 0.05, 2.0)
    assert raw.shape == (1, 2, 16) and raw.dtype == torch.float64 and torch.equal(raw[..., :11], r.stats)
    assert torch.equal(raw[..., 11:], torch.zeros(1, 2, 5, dtype=torch.float64))
    assert torch.equal(raw[0, :, 0], torch.full((2,), 20.0 * 36.0, dtype=torch.float64))
    assert torch.equal(raw[0, :, 1], val.sum(dim=(1, 2)).double())
    for slot in (3, 7, 8, 9, 10):
        assert torch.equal(raw[0, :, slot], raw[0, :, slot].round())
    assert torch.equal(ops.flow_metrics(est.half(), tgt, val).stats, r.stats)       # the fixture's values are fp16-exact
    assert ops.flow_metrics(est.bfloat16(), tgt, val).stats.shape == r.stats.shape
    assert torch.equal(ops.flow_metrics(est, tgt, val.to(torch.uint8)).stats, r.stats)
    wide = torch.zeros(2, 2, 20, 72)
    wide[..., ::2] = est
    assert not wide[..., ::2].is_contiguous()
    assert torch.equal(ops.flow_metrics(wide[..., ::2], tgt, val).stats, r.stats)
    assert not ops.flow_metrics(est.clone().requires_grad_(True), tgt, val).stats.requires_grad
    with pytest.raises(ValueError, match="bool or uint8"):
        ops.flow_metrics(est, tgt, val.float())
    with pytest.raises(ValueError, match="bad ord"):
        ops.flow_metrics(est, tgt, val, ord=0)
    with pytest.raises(ValueError, match="an estimate must be"):
        ops.flow_metrics(est[:, :, :10], tgt, val)
    dist = [0.25 * i for i in range(1, 12)]                     # 11 distances: two calls
    many = ops.flow_metrics([est + 0.125 * k for k in range(34)], tgt, val, distances=dist)      # 34: two calls
    assert many.stats.shape == (34, 2, 8 + 11)
    one = ops.flow_metrics(est + 0.125 * 33, tgt, val, distances=dist[8:])
    assert torch.equal(many.stats[33, :, :8], one.stats[0, :, :8])
    assert torch.equal(many.stats[33, :, 16:], one.stats[0, :, 8:])
    b = many.batch()
    assert b["epe"].shape == (34,) and b["within"].shape == (34, 11)
    assert torch.equal(many.batch_stats(), many.stats[:, 0] + many.stats[:, 1])
    assert many.per_sample()["within"].shape == (34, 2, 11)


def test_cpu_kernel_against_the_eager_expressions():
    """The slot kernel's derived values against the reference-form expressions evaluated value by value
    (cpu.flow_metrics_eager), batch and single sample."""
    from rmd import cpu, ops
    est, tgt, val = metrics_cases.fair_inputs((2, 2, 9, 14), 0.6, (1.0, 3.0, 5.0))
    r = ops.flow_metrics(est, tgt, val, ord=1).host()
    for sample, args in ((None, (est, tgt, val)), (1, (est[1], tgt[1], val[1]))):
        eager = cpu.flow_metrics_eager(*args, ord=1)
        from rmd.metrics import _values
        v = _values(r, sample)
        assert abs(v["epe"] - float(eager["epe/mean"])) <= 1e-6 * v["epe"]
        assert abs(v["magnitude"] - float(eager["flow-magnitude"])) <= 1e-6 * v["magnitude"]
        assert abs(v["aae"] - float(eager["aae"])) <= 1e-9 * v["aae"]
        assert abs(v["fl_all"] - float(eager["fl-all"])) <= 1e-6
        for d in (1, 3, 5):
            assert abs(v["within"][float(d)] - float(eager[f"epe/{d}px"])) <= 1e-6


def _abi_call(lib, nest=1, nd=3, batch=1, height=4, width=4, ord=2.0, null=()):
    buf = ctypes.create_string_buffer(64)          # stands in for device pointers: never dereferenced, the
    p = ctypes.cast(buf, ctypes.c_void_p)          # argument checks fail before any launch
    table = (ctypes.c_void_p * max(nest, 1))(*[p.value] * max(nest, 1))
    dist = (ctypes.c_float * 8)(1, 3, 5)
    arg = lambda name: None if name in null else p  # noqa: E731
    return lib.rmd_flow_metrics(None if "estimates" in null else table, nest, arg("target"), arg("valid"), batch,
                                height, width, None if "distances" in null else dist, nd, 3.0, 0.05, ord, arg("stats"),
                                arg("workspace"), None)


def test_abi_rejects_bad_arguments():
    from rmd import _lib
    lib = _lib.lib()
    assert (_lib.METRICS_MAX_ESTIMATES, _lib.METRICS_MAX_DISTANCES, _lib.METRICS_SLOTS) == (32, 8, 16)
    for name in ("estimates", "target", "valid", "stats", "workspace", "distances"):
        assert _abi_call(lib, null=(name,)) == -1 and b"null" in lib.rmd_last_error()
    assert _abi_call(lib, nest=0) == -1 and b"estimates" in lib.rmd_last_error()
    assert _abi_call(lib, nest=33) == -1
    assert _abi_call(lib, nd=-1) == -1 and b"distances" in lib.rmd_last_error()
    assert _abi_call(lib, nd=9) == -1
    assert _abi_call(lib, height=0) == -2 and b"sizes" in lib.rmd_last_error()
    assert _abi_call(lib, width=-3) == -2 and _abi_call(lib, batch=0) == -2
    for bad in (0.0, -1.0, -math.inf, math.nan):
        assert _abi_call(lib, ord=bad) == -1 and b"mag_ord" in lib.rmd_last_error()
    table = (ctypes.c_void_p * 2)(ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p).value, None)
    buf = ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p)
    assert lib.rmd_flow_metrics(table, 2, buf, buf, 1, 4, 4, None, 0, 3.0, 0.05, 2.0, buf, buf, None) == -1
    assert b"estimate 1" in lib.rmd_last_error()
    assert lib.rmd_flow_metrics_workspace_bytes(2, 37, 53, 33) == 0
    assert lib.rmd_flow_metrics_workspace_bytes(2, 0, 53, 5) == 0
    # samples * blocks per sample * estimates * 16 slots * 8 bytes: 37*53 pixels = 2 tiles of 1024
    assert lib.rmd_flow_metrics_workspace_bytes(3, 37, 53, 5) == 3 * 2 * 5 * 16 * 8
    assert lib.rmd_flow_metrics_workspace_bytes(8, 436, 1024, 12) == 8 * 256 * 12 * 16 * 8      # bounded grid


def test_operator_registered_and_fake_kernel_propagates_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from rmd import library
    assert library.metric_operators() == ["flow_metrics"]
    assert "flow_metrics" not in library.operators() and "flow_metrics" not in library.loss_operators()
    schema = torch.ops.rmd.flow_metrics.default._schema
    assert [a.name for a in schema.arguments] == ["estimates", "target", "valid", "distances", "fl_abs", "fl_rel",
                                                  "mag_ord"]
    assert str(schema.arguments[0].type) == "List[Tensor]" and str(schema.arguments[3].type) == "List[float]"
    assert len(schema.returns) == 1 and str(schema.returns[0].type) == "Tensor"
    with FakeTensorMode():
        dev = "cuda"
        ests = [torch.empty(2, 2, 48, 80, device=dev) for _ in range(3)]
        target = torch.empty(2, 2, 48, 80, device=dev)
        valid = torch.empty(2, 48, 80, device=dev, dtype=torch.bool)
        stats = torch.ops.rmd.flow_metrics(ests, target, valid, [1.0, 3.0], 3.0, 0.05, 2.0)
        assert stats.shape == (3, 2, 16) and stats.dtype == torch.float64 and stats.device.type == "cuda"
        with pytest.raises(ValueError, match="valid must be"):
            torch.ops.rmd.flow_metrics(ests, target, valid[:, :4], [], 3.0, 0.05, 2.0)
        with pytest.raises(ValueError, match="mag_ord"):
            torch.ops.rmd.flow_metrics(ests, target, valid, [], 3.0, 0.05, -2.0)
        with pytest.raises(ValueError, match="distances"):
            torch.ops.rmd.flow_metrics(ests, target, valid, [1.0] * 9, 3.0, 0.05, 2.0)
    c = metrics_cases.case("metrics_small")
    est, tgt, val = c.tensors("cpu")
    torch.library.opcheck(torch.ops.rmd.flow_metrics, ([est, est * 0.5], tgt, val, [1.0, 3.0], 3.0, 0.05, 2.0),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    assert np.isfinite(torch.ops.rmd.flow_metrics([est], tgt, val, [], 3.0, 0.05, math.inf).numpy()).all()
