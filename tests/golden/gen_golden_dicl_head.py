#!/usr/bin/env python3
"""Golden vectors for the DICL flow head, produced by RUNNING the reference.

Test infrastructure only; same import recipe as gen_golden.py (inert stubs for the reference's
absent non-hot-path imports) and the name-keyed weights of detinit.  Functions exercised (reference
file:line):
  * impls.dicl.FlowEntropy       src/models/impls/dicl.py:31-50
  * impls.dicl.FlowRegression    src/models/impls/dicl.py:53-85
  * impls.dicl.FlowLevel         src/models/impls/dicl.py:150-241 (forward with a coarse flow, raw=True,
                                 DAP and context network on; eval mode)

Head fixtures hold the cost, both modules' outputs and the cost gradient of seeded upstream gradients
(one backward through both modules); the level fixture the inputs, flow, flow_raw, four gradients and
the state-dict keys.  Weights are never stored.
Usage:  python tests/golden/gen_golden_dicl_head.py     (writes tests/golden/dicl_head_*.npz, dicl_level_*.npz)
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detinit import det_init  # noqa: E402
from gen_golden import OUT, _import_reference  # noqa: E402


def main():
    import torch
    ref = _import_reference()["dicl"]
    torch.manual_seed(0)
    rng = np.random.default_rng(20250)
    t = torch.from_numpy

    def save(name, **arrays):
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}.npz  {os.path.getsize(path) / 1e3:.1f} kB  keys={sorted(arrays)}")

    def head_case(name, cost):
        tc = t(cost).requires_grad_(True)
        flow = ref.FlowRegression()(tc)
        entropy = ref.FlowEntropy()(tc)
        gf = rng.standard_normal(flow.shape, dtype=np.float32)
        ge = rng.standard_normal(entropy.shape, dtype=np.float32)
        (dc,) = torch.autograd.grad((flow, entropy), tc, (t(gf), t(ge)))
        save(name, cost=cost, flow=flow.detach().numpy(), entropy=entropy.detach().numpy(), grad_flow=gf,
             grad_entropy=ge, grad_cost=dc.numpy())

    head_case("dicl_head_b2_r3x3_6x10", (2.0 * rng.standard_normal((2, 7, 7, 6, 10))).astype(np.float32))
    head_case("dicl_head_b2_r2x4_5x7", (2.0 * rng.standard_normal((2, 5, 9, 5, 7))).astype(np.float32))

    # per-pixel cost scales: flat softmaxes, and peaked ones whose tails sit on the eps clamp or underflow to 0
    scale = np.asarray([0.3, 1.0, 8.0, 40.0], dtype=np.float32)[np.arange(36) % 4].reshape(1, 1, 1, 4, 9)
    head_case("dicl_head_peaked_b1_r3x3_4x9", rng.standard_normal((1, 7, 7, 4, 9), dtype=np.float32) * scale)

    cost = rng.standard_normal((1, 3, 3, 3, 5), dtype=np.float32)
    cost[0, 1, 2, 0, 0] = np.nan                        # a NaN cost: the whole pixel is NaN
    cost[0, 0, 1, 0, 2] = np.inf                        # +inf: inf - inf
    cost[0, 2, 0, 1, 1] = -np.inf                       # a single -inf: p = 0, gradient 0
    cost[0, :, :, 2, 3] = -np.inf                       # all -inf
    head_case("dicl_head_nonfinite_b1_r1x1_3x5", cost)

    # ---- a whole level: cost -> DAP -> flow (+ coarse), entropy -> context network -----------------
    b, c, h, w, level, maxdisp, scale = 2, 8, 8, 12, 3, (3, 3), 0.75
    lvl = det_init(ref.FlowLevel(c, level, maxdisp)).eval()
    img1 = rng.random((b, 3, 2 * h, 2 * w), dtype=np.float32)
    f1 = rng.standard_normal((b, c, h, w), dtype=np.float32)
    f2 = rng.standard_normal((b, c, h, w), dtype=np.float32)
    coarse = (1.5 * rng.standard_normal((b, 2, h // 2, w // 2))).astype(np.float32)
    tf1, tf2 = t(f1).requires_grad_(True), t(f2).requires_grad_(True)
    flow, flow_raw = lvl(t(img1), tf1, tf2, t(coarse), raw=True, dap=True, ctx=True, scale=scale)
    g1 = rng.standard_normal(flow.shape, dtype=np.float32)
    g2 = rng.standard_normal(flow_raw.shape, dtype=np.float32)
    d1, d2, ddap, dctx = torch.autograd.grad((flow, flow_raw), (tf1, tf2, lvl.dap.conv1.weight, lvl.ctxnet[0][0].weight),
                                             (t(g1), t(g2)))
    save("dicl_level_b2_c8_8x12", img1=img1, feat1=f1, feat2=f2, flow_coarse=coarse, channels=np.int32(c),
         level=np.int32(level), maxdisp=np.int32(maxdisp), scale=np.float32(scale), flow=flow.detach().numpy(),
         flow_raw=flow_raw.detach().numpy(), grad_flow=g1, grad_flow_raw=g2, grad_feat1=d1.numpy(),
         grad_feat2=d2.numpy(), grad_dap_conv1=ddap.numpy(), grad_ctxnet_conv0=dctx.numpy(),
         keys=np.asarray(sorted(lvl.state_dict().keys())))


if __name__ == "__main__":
    main()
