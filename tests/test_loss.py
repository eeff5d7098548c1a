"""Sequence losses without a GPU: the CPU dispatch of the four drop-in classes (rmd/loss.py over
rmd/cpu.py's restatement of the reference's ATen calls) reproduces the fixtures the reference's own
classes wrote (tests/golden/gen_golden_loss.py), the classes keep the reference's type strings and
configs, the C ABI rejects bad arguments before any launch, and the operators are registered with
fake kernels that propagate shapes."""

import ctypes
import json

import pytest
import torch

import loss_cases
from loss_cases import CASES


@pytest.mark.parametrize("name,tag", CASES)
def test_cpu_classes_reproduce_the_reference(name, tag):
    """Loss within 1e-6 relative, every prediction's gradient within the fp32 gate, equal NaN and zero
    patterns."""
    c = loss_cases.case(name, tag)
    obj, loss, flows = loss_cases.run(c, "cpu")
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss_cases.check_against_fixture(c, loss, flows, loss_rtol=1e-6)


@pytest.mark.parametrize("name,tag", CASES)
def test_config_and_type_match_the_reference(name, tag):
    c = loss_cases.case(name, tag)
    cls = loss_cases.loss_class(c.type)
    assert cls.type == c.type == c.config["type"]
    obj = cls.from_config({"type": c.type, "arguments": c.arguments})
    assert json.loads(json.dumps(obj.get_config())) == c.config
    with pytest.raises(ValueError, match="invalid loss type"):
        cls.from_config({"type": "no/such-loss"})


def test_default_configs():
    """get_config() of an argument-less instance: the reference's defaults (raft.py:609, mlseq.py:22-27,
    raft_dicl_ctf_l3.py:416-423, dicl.py:429)."""
    import rmd
    assert rmd.SequenceLoss().get_config() == {
        "type": "raft/sequence", "arguments": {"ord": 1, "gamma": 0.8, "include_invalid": False}}
    assert rmd.MultiLevelSequenceLoss().get_config() == {
        "type": "raft+dicl/mlseq", "arguments": {"ord": 1, "gamma": 0.8, "alpha": (1.0, 0.5), "scale": 1.0}}
    assert rmd.RestrictedMultiLevelSequenceLoss().get_config() == {
        "type": "raft+dicl/mlseq-restricted",
        "arguments": {"ord": 1, "gamma": 0.85, "alpha": (0.38, 0.6, 1.0), "scale": 1.0, "delta_range": (128, 64, 32),
                      "delta_mode": "bilinear"}}
    assert rmd.MultiscaleLoss().get_config() == {"type": "dicl/multiscale",
                                                 "arguments": {"ord": 2, "mode": "bilinear"}}


def test_call_merges_arguments():
    """__call__ merges the stored arguments with the call's keywords, the call's winning (model.py:82-83)."""
    import rmd
    g = torch.Generator().manual_seed(1)
    target = torch.randn(1, 2, 6, 8, generator=g)
    flows = [torch.randn(1, 2, 6, 8, generator=g) for _ in range(3)]
    valid = torch.ones(1, 6, 8, dtype=torch.bool)
    loss = rmd.SequenceLoss({"gamma": 0.5})
    ref = sum(0.5 ** (2 - i) * (f - target).abs().sum(1).mean() for i, f in enumerate(flows))
    assert torch.allclose(loss(None, flows, target, valid), ref, rtol=1e-6)
    ref2 = sum(0.25 ** (2 - i) * (f - target).abs().sum(1).mean() for i, f in enumerate(flows))
    assert torch.allclose(loss(None, flows, target, valid, gamma=0.25), ref2, rtol=1e-6)
    # uint8 validity is accepted like bool
    assert torch.equal(loss(None, flows, target, valid.to(torch.uint8)), loss(None, flows, target, valid))


def test_mixed_devices_and_bad_arguments_raise():
    from rmd import ops
    target, valid = torch.zeros(1, 2, 4, 4), torch.ones(1, 4, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="different devices"):
        ops.sequence_loss([torch.zeros(1, 2, 4, 4, device="meta")], target, valid, [1.0])
    with pytest.raises(ValueError, match="weights"):
        ops.sequence_loss([torch.zeros(1, 2, 4, 4)], target, valid, [1.0, 2.0])
    with pytest.raises(ValueError, match="must be"):
        ops.sequence_loss([torch.zeros(1, 3, 4, 4)], target, valid, [1.0])
    with pytest.raises(ValueError, match="bool or uint8"):
        from rmd import library
        library._u8(torch.zeros(1, 4, 4))
    # an ord the HIP kernels do not have: GPU tensors raise and name the supported ones (checked on fake
    # GPU tensors: the check comes before any launch); CPU tensors run the reference's generic norm
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        tg, va = torch.empty(1, 2, 4, 4, device="cuda"), torch.empty(1, 4, 4, device="cuda", dtype=torch.bool)
        with pytest.raises(ValueError, match="'absmean', 'robust'"):
            ops.sequence_loss([torch.empty(1, 2, 4, 4, device="cuda")], tg, va, [1.0], ord=3)
        with pytest.raises(ValueError, match="mode 'bilinear'"):
            ops.sequence_loss([torch.empty(1, 2, 2, 2, device="cuda")], tg, va, [1.0], mode="nearest")
    f = torch.ones(1, 2, 4, 4)
    assert torch.allclose(ops.sequence_loss([f], target, valid, [1.0], ord=3), torch.tensor(2.0 ** (1 / 3)))


def _dummy_call(lib, npred=1, norm=1, height=4, width=4, pheight=4, pwidth=4):
    from rmd import _lib
    buf = ctypes.create_string_buffer(64)          # stands in for device pointers: never dereferenced, the
    p = ctypes.cast(buf, ctypes.c_void_p)          # argument checks fail before any launch
    table = (_lib.LossPrediction * max(npred, 1))()
    for e in table:
        e.flow, e.height, e.width, e.weight = p.value, pheight, pwidth, 1.0
    return lib.rmd_sequence_loss(table, npred, p, p, 1, height, width, norm, 0, 0, 1.0, p, p, p, None)


def test_abi_rejects_bad_arguments():
    from rmd import _lib
    lib = _lib.lib()
    assert _lib.LOSS_MAX_PREDICTIONS == 32
    assert _dummy_call(lib, norm=7) == -1 and b"norm" in lib.rmd_last_error()
    assert _dummy_call(lib, norm=0) == -1
    assert _dummy_call(lib, npred=33) == -1 and b"predictions" in lib.rmd_last_error()
    assert _dummy_call(lib, npred=0) == -1
    assert _dummy_call(lib, height=0) == -2 and b"sizes" in lib.rmd_last_error()
    assert _dummy_call(lib, width=-3) == -2
    assert _dummy_call(lib, pwidth=0) == -2 and b"prediction 0" in lib.rmd_last_error()
    table = (_lib.LossPrediction * 1)()
    assert lib.rmd_sequence_loss(table, 1, None, None, 1, 4, 4, 1, 0, 0, 1.0, None, None, None, None) == -1
    assert lib.rmd_sequence_loss_backward(table, 1, None, None, 1, 4, 4, 1, 0, 1.0, None, None, None) == -1
    assert lib.rmd_sequence_loss_workspace_bytes(2, 37, 53, 33) == 0
    assert lib.rmd_sequence_loss_workspace_bytes(2, 0, 53, 5) == 0
    # blocks * K * (one double + one 64-bit count): 2*37*53 pixels = 16 blocks of 256
    assert lib.rmd_sequence_loss_workspace_bytes(2, 37, 53, 5) == 16 * 5 * 16
    assert lib.rmd_sequence_loss_workspace_bytes(8, 436, 1024, 32) == 2048 * 32 * 16       # bounded grid


def test_operators_registered_and_fake_kernels_propagate_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from rmd import library
    assert library.loss_operators() == ["sequence_loss", "sequence_loss_backward"]
    for name in library.loss_operators():
        assert hasattr(torch.ops.rmd, name)
    with FakeTensorMode():
        dev = "cuda"
        flows = [torch.empty(2, 2, 6, 10, device=dev), torch.empty(2, 2, 48, 80, device=dev)]
        target = torch.empty(2, 2, 48, 80, device=dev)
        valid = torch.empty(2, 48, 80, device=dev, dtype=torch.bool)
        mask = torch.empty(2, 48, 80, device=dev, dtype=torch.uint8)
        loss, counts = torch.ops.rmd.sequence_loss(flows, target, valid, [mask], [-1, 0], [0.5, 1.0], 2, False, True, 1.0)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == "cuda"
        assert counts.shape == (2,) and counts.dtype == torch.int64
        grads = torch.ops.rmd.sequence_loss_backward(loss, flows, target, valid, [mask], [-1, 0], [0.5, 1.0], counts,
                                                     [True, False], 2, False, 1.0)
        assert grads[0].shape == (2, 2, 6, 10) and grads[0].dtype == torch.float32 and grads[1].numel() == 0
        with pytest.raises(ValueError, match="norm 9"):
            torch.ops.rmd.sequence_loss(flows, target, valid, [], [-1, -1], [0.5, 1.0], 9, False, False, 1.0)
        with pytest.raises(ValueError, match="valid must be"):
            torch.ops.rmd.sequence_loss(flows, target, valid[:, :4], [], [-1, -1], [0.5, 1.0], 1, False, False, 1.0)
