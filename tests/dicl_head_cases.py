"""Shared helpers of test_dicl_head.py / test_gpu_dicl_head.py: the fixtures of
tests/golden/gen_golden_dicl_head.py (loaded once per process and never modified), the tests' own numpy
float64 restatement of the DICL flow head (forward and analytic backward), the gate, the shape sweep
and a FlowLevel built from the package's blocks for the level fixture.

Gate: conftest.rel_max_err (max |got - ref| / max |ref|, NaN positions identical) <= 1e-5 for flow,
entropy and grad_cost — the project's gate for its fp32 softmax kernels (test_gpu_heads.py).  The
reference's own fp32 formulas, evaluated on the CPU against the float64 restatement below, stay at or
below 6.5e-7 for all three quantities on the mixed-scale sweep inputs, so the gate leaves the kernel
an order of magnitude for the device's expf / logf and its summation order.
"""

import functools

import numpy as np
import torch
import torch.nn as nn

from conftest import load_golden

GATE = 1e-5
LEVEL_GATE = 1e-4           # north_star's fp32 tolerance: the level runs the DAP in split-bf16 on the GPU
EPS = 1e-9

HEAD_FIXTURES = ["dicl_head_b2_r3x3_6x10", "dicl_head_b2_r2x4_5x7", "dicl_head_peaked_b1_r3x3_4x9",
                 "dicl_head_nonfinite_b1_r1x1_3x5"]
LEVEL_FIXTURE = "dicl_level_b2_c8_8x12"

# (b, ru, rv, h, w): one pixel; odd sizes on the register path (r = 3, r = 4: more than one block); a
# rectangular and a zero range, the largest range and a plain r = 3 row longer than a block's 64 lanes
# with a tail on the generic / register paths; D = 1
SWEEP = [(1, 1, 1, 1, 1), (2, 3, 3, 5, 13), (1, 4, 4, 3, 67), (3, 2, 5, 7, 9), (1, 0, 3, 4, 5), (2, 8, 8, 2, 3),
         (1, 3, 3, 1, 257), (1, 0, 0, 2, 3)]
SCALES = (0.3, 1.0, 8.0, 40.0)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_golden(name)


def _softmax64(cost):
    b, du, dv, h, w = cost.shape
    x = cost.astype(np.float64).reshape(b, du * dv, h, w)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))        # NaN / +inf / all -inf: NaN for the whole pixel
        return (e / e.sum(axis=1, keepdims=True)).reshape(b, du, dv, h, w)


def _constants(du, dv, eps):
    """The clamp bounds and log(D) as the reference's float32 arithmetic sees them (1 - 1e-9 is 1)."""
    lo = float(np.float32(eps))
    hi = float(np.float32(1.0) - np.float32(eps))
    return lo, hi, float(np.float32(np.log(du * dv)))


def _offsets(du, dv):
    u = np.arange(du, dtype=np.float64) - (du - 1) // 2
    v = np.arange(dv, dtype=np.float64) - (dv - 1) // 2
    return u.reshape(1, du, 1, 1, 1), v.reshape(1, 1, dv, 1, 1)


def forward64(cost, flow_coarse=None, eps=EPS):
    """float64: (flow (B, 2, h, w), entropy (B, h, w)) of cost (B, du, dv, h, w); dim 1 is the u offset."""
    _, du, dv, _, _ = cost.shape
    p = _softmax64(cost)
    lo, hi, log_d = _constants(du, dv, eps)
    u, v = _offsets(du, dv)
    with np.errstate(all="ignore"):
        flow = np.stack([(p * u).sum(axis=(1, 2)), (p * v).sum(axis=(1, 2))], axis=1)
        if flow_coarse is not None:
            flow = flow + flow_coarse.astype(np.float64)
        entropy = -(p * np.log(np.clip(p, lo, hi))).sum(axis=(1, 2)) / log_d
    return flow, entropy


def backward64(cost, grad_flow, grad_entropy, eps=EPS):
    """float64 analytic gradient: grad_cost_k = p_k (g_k - sum_j p_j g_j), g_k = gu u_k + gv v_k
    - gH (log(clamp(p_k)) + [eps <= p_k <= 1 - eps]) / log(D) (the bracket: torch's clamp subgradient)."""
    _, du, dv, _, _ = cost.shape
    p = _softmax64(cost)
    lo, hi, log_d = _constants(du, dv, eps)
    u, v = _offsets(du, dv)
    gu = grad_flow[:, 0].astype(np.float64)[:, None, None]
    gv = grad_flow[:, 1].astype(np.float64)[:, None, None]
    gh = grad_entropy.astype(np.float64)[:, None, None]
    with np.errstate(all="ignore"):
        inside = ((p >= lo) & (p <= hi)).astype(np.float64)
        g = gu * u + gv * v - gh * (np.log(np.clip(p, lo, hi)) + inside) / log_d
        return p * (g - (p * g).sum(axis=(1, 2), keepdims=True))


@functools.lru_cache(maxsize=None)
def sweep_case(shape):
    """Seeded inputs of one SWEEP shape, every tensor mixing the per-pixel cost scales SCALES, with their
    float64 results (with and without the coarse flow).  Shared; never modified."""
    b, ru, rv, h, w = shape
    du, dv = 2 * ru + 1, 2 * rv + 1
    rng = np.random.default_rng(1000 * ru + 100 * rv + 10 * h + w + b)
    scale = np.asarray(SCALES, dtype=np.float32)[np.arange(h * w) % len(SCALES)].reshape(1, 1, 1, h, w)
    cost = (rng.standard_normal((b, du, dv, h, w), dtype=np.float32) * scale).astype(np.float32)
    coarse = (3.0 * rng.standard_normal((b, 2, h, w), dtype=np.float32)).astype(np.float32)
    grad = rng.standard_normal((b, 3, h, w), dtype=np.float32)
    flow, entropy = forward64(cost)
    flow_c, _ = forward64(cost, coarse)
    return dict(cost=cost, coarse=coarse, grad=grad, flow=flow, flow_coarse=flow_c, entropy=entropy,
                grad_cost=backward64(cost, grad[:, :2], grad[:, 2]),
                grad_cost_flow_only=backward64(cost, grad[:, :2], np.zeros_like(grad[:, 2])),
                grad_cost_entropy_only=backward64(cost, np.zeros_like(grad[:, :2]), grad[:, 2]))


# ---- a DICL level from the package's blocks (the modules a reference FlowLevel holds, dicl.py:150-169) ----

def _context_net(feature_channels):
    """The level 2 / 3 context network: six dilated 3x3 conv blocks and a biased 3x3 output conv
    (flow 2 + entropy 1 + features + image 3 input channels)."""
    from rmd.blocks.dicl import ConvBlock
    widths = [feature_channels + 6, 64, 128, 128, 96, 64, 32]
    dilations = [1, 2, 4, 8, 16, 1]
    blocks = [ConvBlock(widths[i], widths[i + 1], kernel_size=3, padding=d, dilation=d)
              for i, d in enumerate(dilations)]
    return nn.Sequential(*blocks, nn.Conv2d(32, 2, kernel_size=3, padding=1))


def make_level(feature_channels, level, maxdisp):
    """class FlowLevel(rmd.dicl.FlowLevelMixin, <base with the reference's sub-modules>)."""
    import rmd
    from rmd.blocks.dicl import DisplacementAwareProjection, MatchingNet
    assert level in (2, 3)

    class _Base(nn.Module):
        def __init__(self):
            super().__init__()
            self.level = level
            self.maxdisp = maxdisp
            self.mnet = MatchingNet(2 * feature_channels)
            self.dap = DisplacementAwareProjection(maxdisp)
            self.flow = rmd.dicl.FlowRegression()
            self.entropy = rmd.dicl.FlowEntropy()
            self.ctxnet = _context_net(feature_channels)

    class FlowLevel(rmd.dicl.FlowLevelMixin, _Base):
        pass

    return FlowLevel()


def run_level(device):
    """The level fixture through FlowLevelMixin on `device` -> dict of numpy results named as in the fixture."""
    from detinit import det_init
    g = fixture(LEVEL_FIXTURE)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    lvl = det_init(make_level(int(g["channels"]), int(g["level"]), tuple(int(m) for m in g["maxdisp"]))).eval().to(device)
    f1, f2 = t(g["feat1"]).requires_grad_(True), t(g["feat2"]).requires_grad_(True)
    flow, flow_raw = lvl(t(g["img1"]), f1, f2, t(g["flow_coarse"]), raw=True, dap=True, ctx=True,
                         scale=float(g["scale"]))
    params = [lvl.dap.conv1.weight, lvl.ctxnet[0][0].weight]
    grads = torch.autograd.grad((flow, flow_raw), [f1, f2] + params, (t(g["grad_flow"]), t(g["grad_flow_raw"])))
    names = ["grad_feat1", "grad_feat2", "grad_dap_conv1", "grad_ctxnet_conv0"]
    out = {"flow": flow, "flow_raw": flow_raw, **dict(zip(names, grads))}
    return {k: v.detach().cpu().numpy() for k, v in out.items()}, sorted(lvl.state_dict().keys())
