"""Sequence losses on the GPU: the HIP path of the drop-in classes (csrc/loss.hip through
torch.ops.rmd.sequence_loss) against the fixtures the reference's classes wrote
(tests/golden/gen_golden_loss.py), plus masking, determinism, gradient selection, a mid-size case
against the CPU kernels, opcheck and the no-host-synchronisation rule.

Parity gate: |loss - ref| <= 1e-5 |ref| — every term is non-negative, each dist carries about
10 ulp * (|f| + |target|), which for the fixtures' independent normal inputs is about 1e-6 relative;
the gate leaves 8x over that.  Gradients pass conftest.assert_fp32_gate per prediction; NaN and zero
patterns are identical."""

import numpy as np
import pytest
import torch

import loss_cases
from loss_cases import CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("name,tag", CASES)
def test_hip_classes_reproduce_the_reference(name, tag):
    c = loss_cases.case(name, tag)
    obj, loss, flows = loss_cases.run(c, DEV)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.device.type == "cuda"
    for f in flows:
        assert f.grad is not None and f.grad.device.type == "cuda"
    loss_cases.check_against_fixture(c, loss, flows, loss_rtol=1e-5)


def _seq_inputs():
    c = loss_cases.case("loss_seq", "ord1")
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return c, [t(f) for f in c.flows], t(c.target), t(c.valid)


def test_nan_at_an_invalid_pixel_is_selected_away():
    """Masked mode selects (raft.py:639): a NaN at an invalid pixel does not reach the sum; include_invalid
    multiplies (raft.py:633): it does.  A NaN at a valid pixel makes the loss NaN in both."""
    from rmd import ops
    c, flows, target, valid = _seq_inputs()
    w = [0.8 ** (4 - i) for i in range(5)]
    base = ops.sequence_loss(flows, target, valid, w, ord=1)
    b, y, x = [int(v[0]) for v in np.nonzero(~c.valid)]
    assert not c.valid[b, y, x]
    bad = [f.clone() for f in flows]
    bad[2][b, 1, y, x] = float("nan")
    assert torch.equal(ops.sequence_loss(bad, target, valid, w, ord=1), base)
    assert torch.isnan(ops.sequence_loss(bad, target, valid, w, ord=1, include_invalid=True))
    assert torch.isfinite(ops.sequence_loss(flows, target, valid, w, ord=1, include_invalid=True))
    b, y, x = [int(v[0]) for v in np.nonzero(c.valid)]
    bad = [f.clone() for f in flows]
    bad[4][b, 0, y, x] = float("nan")
    assert torch.isnan(ops.sequence_loss(bad, target, valid, w, ord=1))
    assert torch.isnan(ops.sequence_loss(bad, target, valid, w, ord=2, include_invalid=True))


@pytest.mark.parametrize("name,tag", [("loss_mlseq", "ord2"), ("loss_mlseq_ragged", "ord1"), ("loss_many", "ord1")])
def test_two_runs_are_bitwise_equal(name, tag):
    c = loss_cases.case(name, tag)
    _, l1, f1 = loss_cases.run(c, DEV)
    _, l2, f2 = loss_cases.run(c, DEV)
    assert torch.equal(l1, l2) or (torch.isnan(l1) and torch.isnan(l2))
    for a, b in zip(f1, f2):
        assert torch.equal(a.grad, b.grad)


def test_prediction_without_requires_grad_gets_no_gradient():
    c = loss_cases.case("loss_mlseq", "ord1")
    _, l_all, f_all = loss_cases.run(c, DEV)
    need = [i not in (1, 6) for i in range(len(c.flows))]          # one coarse, one full-resolution
    _, l_some, f_some = loss_cases.run(c, DEV, requires_grad=need)
    assert torch.equal(l_all, l_some)
    for i, (a, b) in enumerate(zip(f_all, f_some)):
        if need[i]:
            assert torch.equal(a.grad, b.grad)
        else:
            assert b.grad is None


def test_other_dtypes_and_upstream_gradient():
    """fp16 flows are cast (the _f32 convention) and get fp16 gradients; the upstream gradient scales
    every gradient (read on the device)."""
    from rmd import ops
    c, flows, target, valid = _seq_inputs()
    w = [1.0] * 5
    f32 = [f.clone().requires_grad_(True) for f in flows]
    (3.0 * ops.sequence_loss(f32, target, valid, w, ord=2)).backward()
    f16 = [f.half().requires_grad_(True) for f in flows]         # the fixture's values are fp16-exact
    loss = ops.sequence_loss(f16, target, valid, w, ord=2)
    loss.backward()
    for a, b in zip(f32, f16):
        assert b.grad.dtype == torch.float16
        assert torch.allclose(a.grad / 3.0, b.grad.float(), rtol=2e-3, atol=1e-7)


def _midsize(seed):
    g = torch.Generator().manual_seed(seed)
    b, h, w = 2, 96, 160
    target = 3.0 * torch.randn(b, 2, h, w, generator=g)
    valid = torch.rand(b, h, w, generator=g) < 0.7
    flows = [target + torch.randn(b, 2, h, w, generator=g) for _ in range(12)]
    for ch, cw in ((12, 20), (12, 20), (24, 40), (24, 40)):
        flows.append(torch.randn(b, 2, ch, cw, generator=g) * 2.0)
    return flows, target, valid


def test_midsize_against_the_cpu_kernels():
    """B=2, 96x160, 12 full-resolution and 4 coarse predictions, ord 2, HIP against the CPU kernels.  The
    inputs are redrawn until ||d|| >= 1e-3 on every valid pixel of the upsampled predictions (checked
    on the CPU side), so d/||d|| does not hinge on interpolation rounding."""
    from rmd import cpu, ops
    for seed in range(20):
        flows, target, valid = _midsize(seed)
        if all(((cpu.loss_upsample(f, target.shape) - target).norm(dim=1)[valid] >= 1e-3).all() for f in flows[12:]):
            break
    else:
        raise AssertionError("no seed met the fixture condition")
    w = [0.85 ** (len(flows) - i - 1) for i in range(len(flows))]
    fc = [f.clone().requires_grad_(True) for f in flows]
    ref = ops.sequence_loss(fc, target, valid, w, ord=2, scale=0.5)
    ref.backward()
    fg = [f.to(DEV).requires_grad_(True) for f in flows]
    got = ops.sequence_loss(fg, target.to(DEV), valid.to(DEV), w, ord=2, scale=0.5)
    got.backward()
    got_v, ref_v = float(got.detach()), float(ref.detach())
    print(f"midsize: loss {got_v!r} cpu {ref_v!r}")
    assert abs(got_v - ref_v) <= 1e-5 * abs(ref_v)
    from conftest import assert_fp32_gate
    for a, b in zip(fg, fc):
        assert_fp32_gate(a.grad.cpu().numpy(), b.grad.numpy())


def test_unaligned_views_take_the_scalar_path():
    """W % 4 == 0 but a base pointer off 16 bytes: same numbers as the aligned call."""
    from rmd import ops
    g = torch.Generator().manual_seed(3)
    b, h, w = 2, 8, 16
    target = torch.randn(b, 2, h, w, generator=g).to(DEV)
    valid = (torch.rand(b, h, w, generator=g) < 0.6).to(DEV)
    flow = torch.randn(b, 2, h, w, generator=g).to(DEV)
    buf = torch.zeros(flow.numel() + 1, device=DEV)
    off = buf[1:].view_as(flow)
    off.copy_(flow)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    fa, fb = flow.clone().requires_grad_(True), off.detach().requires_grad_(True)
    la = ops.sequence_loss([fa], target, valid, [1.0], ord=2)
    lb = ops.sequence_loss([fb], target, valid, [1.0], ord=2)
    la.backward()
    lb.backward()
    assert torch.allclose(la, lb, rtol=1e-6) and torch.allclose(fa.grad, fb.grad, rtol=1e-6, atol=0)


def test_opcheck_forward_operator():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
    target, valid = r(2, 2, 12, 20), (torch.rand(2, 12, 20, generator=g) < 0.7).to(DEV)
    mask = (torch.rand(2, 12, 20, generator=g) < 0.5).to(DEV).to(torch.uint8)
    flows = [r(2, 2, 3, 5), r(2, 2, 12, 20)]
    torch.library.opcheck(torch.ops.rmd.sequence_loss,
                          (flows, target, valid, [mask], [-1, 0], [0.5, 1.0], 2, False, True, 0.5),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_no_host_synchronisation():
    """Forward and backward of a multi-level loss under sync-debug mode 'error'.  The mode is shown to work
    on this build first: nonzero() (what the reference's dist[valid] launches) raises."""
    import rmd
    c = loss_cases.case("loss_mlseq", "ord1")
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    flows = [t(f).requires_grad_(True) for f in c.flows]
    target, valid = t(c.target), t(c.valid)
    loss_obj = rmd.loss.MultiLevelSequenceLoss(c.arguments)
    loss_obj(None, c.result(flows), target, valid).backward()      # warm-up: library load, allocator
    for f in flows:
        f.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            valid.nonzero()
        loss = loss_obj(None, c.result(flows), target, valid)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert abs(float(loss.detach()) - c.loss) <= 1e-5 * abs(c.loss)
