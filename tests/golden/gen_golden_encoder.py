#!/usr/bin/env python3
"""Golden vectors for RAFT's feature / context encoder, produced by RUNNING the reference.

Test infrastructure only; same import recipe as gen_golden_gru.py and the name-keyed, He-scaled weights of
detinit.det_init_fanin, which are never stored (for the batch norm they include non-trivial gamma, beta and running
statistics).  Class exercised (reference file:line):
  * encoders.raft.s3.FeatureEncoder   src/models/common/encoders/raft/s3.py:8-72 (ResidualBlock: blocks/raft.py:13-46)

One input, N(0, 1) of (2, 3, 36, 140): the maps are 18 x 70, 9 x 35 and 5 x 18 — an odd side entering a stride-2
convolution, more than one 32-wide tile at 1/2 and 1/4 resolution.  Per norm type (eval mode):
  encoder_instance_b2_36x140, encoder_batch_b2_36x140, encoder_none_b2_36x140
      x, the state-dict keys, out (fp32), out64 (the same module run in float64 on the same fp32 parameters) and
      ref_err = max|out - out64| / max|out64|, the reference's own fp32 error
Usage:  python tests/golden/gen_golden_encoder.py     (writes tests/golden/encoder_*.npz)
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detinit import det_init_fanin  # noqa: E402
from gen_golden import OUT, _import_reference  # noqa: E402

NORMS = ("instance", "batch", "none")
SHAPE = (2, 3, 36, 140)


def main():
    import torch
    _import_reference()
    from src.models.common.encoders.raft import s3
    torch.manual_seed(0)
    rng = np.random.default_rng(20257)
    x = rng.standard_normal(SHAPE).astype(np.float32)
    with torch.no_grad():
        for norm in NORMS:
            m = det_init_fanin(s3.FeatureEncoder(256, norm)).eval()
            keys = np.asarray(sorted(m.state_dict().keys()))
            out = m(torch.from_numpy(x)).numpy()
            out64 = m.double()(torch.from_numpy(x).double()).numpy()
            ref_err = float(np.abs(out - out64).max() / np.abs(out64).max())
            name = f"encoder_{norm}_b2_36x140"
            path = os.path.join(OUT, name + ".npz")
            np.savez_compressed(path, x=x, out=out, out64=out64, ref_err=np.float64(ref_err), keys=keys)
            print(f"{name}.npz  {os.path.getsize(path) / 1e3:.1f} kB  out {out.shape}  reference fp32 error {ref_err:.2e}")


if __name__ == "__main__":
    main()
