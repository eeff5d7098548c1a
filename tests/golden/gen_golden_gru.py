#!/usr/bin/env python3
"""Golden vectors for the update block's recurrent unit, produced by RUNNING the reference.

Test infrastructure only; same import recipe as gen_golden_hsup.py (inert stubs for the reference's
absent non-hot-path imports) and the name-keyed, He-scaled weights of detinit.det_init_fanin, which are
never stored.  Classes exercised (reference file:line):
  * raft.SepConvGru          src/models/impls/raft.py:228-259
  * raft.BasicUpdateBlock    src/models/impls/raft.py:276-296

Inputs: h = tanh(N(0, 1)) (a hidden state), x = relu(N(0, 1)) (context and motion features).
  gru_b2_h128_x256_6x10      h, x, out of SepConvGru(128, 256), the state-dict keys
  gru_block_b1_6x10          h, x, corr (a random lookup, 324 planes), flow -> (h', d) of BasicUpdateBlock(324)
  gru_nan_b1_h32_x16_7x9     SepConvGru(32, 16) with one NaN in h and one in x, away from the border.  A NaN reaches
                             +-4 along each axis (z and r read +-2, and q reads r.h at +-2 again), so on this map
                             every output is NaN
  gru_nan_b1_h32_x16_12x14   the same on a map that keeps finite outputs outside the two 9 x 9 squares
Usage:  python tests/golden/gen_golden_gru.py     (writes tests/golden/gru_*.npz)
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detinit import det_init_fanin  # noqa: E402
from gen_golden import OUT, _import_reference  # noqa: E402

# (b, channel, y, x) of the NaN in h and of the one in x, per fixture
NANS = {"gru_nan_b1_h32_x16_7x9": ((7, 9), (0, 5, 3, 4), (0, 9, 2, 6)),
        "gru_nan_b1_h32_x16_12x14": ((12, 14), (0, 5, 2, 3), (0, 9, 8, 10))}


def main():
    import torch
    ref = _import_reference()["raft"]
    torch.manual_seed(0)
    rng = np.random.default_rng(20252)
    t = torch.from_numpy

    def save(name, **arrays):
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}.npz  {os.path.getsize(path) / 1e3:.1f} kB  keys={sorted(arrays)}")

    def inputs(b, hd, xd, h, w):
        return (np.tanh(rng.standard_normal((b, hd, h, w))).astype(np.float32),
                np.maximum(rng.standard_normal((b, xd, h, w)), 0).astype(np.float32))

    with torch.no_grad():
        m = det_init_fanin(ref.SepConvGru(128, 256)).eval()
        h, x = inputs(2, 128, 256, 6, 10)
        save("gru_b2_h128_x256_6x10", h=h, x=x, out=m(t(h), t(x)).numpy(),
             keys=np.asarray(sorted(m.state_dict().keys())))

        m = det_init_fanin(ref.BasicUpdateBlock(324)).eval()
        h, x = inputs(1, 128, 128, 6, 10)
        corr = rng.standard_normal((1, 324, 6, 10)).astype(np.float32)
        flow = (2.0 * rng.standard_normal((1, 2, 6, 10))).astype(np.float32)
        h_out, d = m(t(h), t(x), t(corr), t(flow))
        save("gru_block_b1_6x10", h=h, x=x, corr=corr, flow=flow, h_out=h_out.numpy(), d=d.numpy(),
             keys=np.asarray(sorted(m.state_dict().keys())))

        m = det_init_fanin(ref.SepConvGru(32, 16)).eval()
        for name, ((ht, wd), nan_h, nan_x) in NANS.items():
            h, x = inputs(1, 32, 16, ht, wd)
            h[nan_h] = np.nan
            x[nan_x] = np.nan
            save(name, h=h, x=x, out=m(t(h), t(x)).numpy(), nan_h=np.asarray(nan_h), nan_x=np.asarray(nan_x),
                 keys=np.asarray(sorted(m.state_dict().keys())))


if __name__ == "__main__":
    main()
