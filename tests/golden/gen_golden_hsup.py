#!/usr/bin/env python3
"""Golden vectors for the hidden-state upsamplers, produced by RUNNING the reference.

Test infrastructure only; same import recipe as gen_golden.py (inert stubs for the reference's
absent non-hot-path imports) and the name-keyed weights of detinit.  Classes exercised (reference
file:line):
  * common.hsup.HUpCrossAttn     src/models/common/hsup.py:36-97
  * common.hsup.HUpBilinear      src/models/common/hsup.py:16-33

Module fixtures hold h_prev, h_init, the output, the gradients of both inputs and of every parameter
for a seeded upstream gradient, and the state-dict keys; weights are never stored (detinit).  The core
fixture feeds q, k and v straight to the attention lines (hsup.py:66-92): the instance's five
convolutions are replaced by modules that hand back the given tensors (conv_v_init: zeros, conv_out:
the identity), so that non-finite values sit exactly where they were put.
Usage:  python tests/golden/gen_golden_hsup.py     (writes tests/golden/hsup_*.npz)
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detinit import det_init  # noqa: E402
from gen_golden import OUT, _import_reference  # noqa: E402


def main():
    import torch
    import torch.nn as nn
    _import_reference()
    from src.models.common import hsup as ref
    torch.manual_seed(0)
    rng = np.random.default_rng(20251)
    t = torch.from_numpy

    def save(name, **arrays):
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}.npz  {os.path.getsize(path) / 1e3:.1f} kB  keys={sorted(arrays)}")

    def module_case(name, cls, channels, b, h2, w2, fy, fx):
        m = det_init(cls(channels))
        h_prev = rng.standard_normal((b, channels, h2, w2), dtype=np.float32)
        h_init = rng.standard_normal((b, channels, h2 * fy, w2 * fx), dtype=np.float32)
        tp, ti = t(h_prev).requires_grad_(True), t(h_init).requires_grad_(True)
        out = m(tp, ti)
        grad = rng.standard_normal(out.shape, dtype=np.float32)
        names, params = zip(*m.named_parameters())
        grads = torch.autograd.grad(out, (tp, ti) + params, t(grad))
        save(name, channels=np.int32(channels), h_prev=h_prev, h_init=h_init, out=out.detach().numpy(), grad=grad,
             grad_h_prev=grads[0].numpy(), grad_h_init=grads[1].numpy(),
             keys=np.asarray(sorted(m.state_dict().keys())),
             **{"grad_" + n: g.numpy() for n, g in zip(names, grads[2:])})

    module_case("hsup_crossattn_b2_c8_3x5_f2x2", ref.HUpCrossAttn, 8, 2, 3, 5, 2, 2)
    module_case("hsup_crossattn_b1_c6_3x2_f1x4", ref.HUpCrossAttn, 6, 1, 3, 2, 1, 4)
    module_case("hsup_bilinear_b2_c5_3x4_f2x2", ref.HUpBilinear, 5, 2, 3, 4, 2, 2)

    class Given(nn.Module):
        def __init__(self, value):
            super().__init__()
            self.value = value

        def forward(self, x):
            return self.value

    # the attention core with non-finite inputs, one in each corner of a map large enough to keep a finite middle
    b, ck, cv, h2, w2, fy, fx = 1, 4, 3, 6, 9, 2, 2
    h, w = h2 * fy, w2 * fx
    q = rng.standard_normal((b, ck, h, w), dtype=np.float32)
    k = rng.standard_normal((b, ck, h2, w2), dtype=np.float32)
    v = rng.standard_normal((b, cv, h2, w2), dtype=np.float32)
    q[0, :, h - 1, w - 1] = np.nan              # one q pixel (bottom-right corner)
    k[0, :, h2 - 1, 0] = np.nan                 # one k cell (bottom-left)
    v[0, :, 0, w2 - 1] = np.nan                 # one v cell (top-right)
    v[0, 1, 0, 0] = np.inf                      # one v element (top-left)
    tq, tk, tv = (t(a).requires_grad_(True) for a in (q, k, v))
    m = ref.HUpCrossAttn(cv)
    m.conv_q, m.conv_k, m.conv_v_prev = Given(tq), Given(tk), Given(tv)
    m.conv_v_init, m.conv_out = Given(torch.zeros(b, cv, h, w)), nn.Identity()
    out = m(torch.zeros(b, cv, h2, w2), torch.zeros(b, cv, h, w))
    grad = rng.standard_normal(out.shape, dtype=np.float32)
    dq, dk, dv = torch.autograd.grad(out, (tq, tk, tv), t(grad))
    save("hsup_core_nonfinite_b1_6x9_f2x2", q=q, k=k, v=v, out=out.detach().numpy(), grad=grad, grad_q=dq.numpy(),
         grad_k=dk.numpy(), grad_v=dv.numpy())


if __name__ == "__main__":
    main()
