#!/usr/bin/env python3
"""Golden vectors for the eval-mode 'dicl' and 'dicl-emb' correlation modules (test infrastructure): what the fused
k x k MatchingNet path has to reproduce.

Runs the reference's own corr.dicl.CorrelationModule (src/models/common/corr/dicl.py:8-61) and
corr.dicl_emb.CorrelationModule (src/models/common/corr/dicl_emb.py:32-104) from a checkout of qzed/raft-meets-dicl
v2 (gen_golden's reference path), in .eval(), with the name-keyed weights of detinit.det_init and
the seeded, non-trivial batch-norm state of gen_golden_dicl_match.seed_norm_state, which IS stored (`sd.<key>`: the
norm entries only; every other weight is rebuilt with det_init).  Stored per case: the inputs, the MatchingNet output
(forward hook) and the module output with dap=True and dap=False.

  mnet_bn_b2_c16_r2_8x12        'dicl', b2, C16, 8x12, r2, batch norm; coords = grid + N(0, 1.5^2): windows leave the map
  mnet_none_b1_c8_r3_6x10_s05   'dicl', b1, C8, 6x10, r3, no norm, mnet_scale 0.5: widths 48, 64, 32, 16
  mnet_emb_b1_c16_r2_4x6        'dicl-emb', b1, C16, 4x6, r2, batch norm: 34 input channels
  mnet_nan_b1_c16_r2_8x12       the first case's module and first sample, one pixel's coordinate NaN and one +inf

Usage:  python tests/golden/gen_golden_mnet.py   (writes tests/golden/mnet_*.npz)
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detinit import det_init  # noqa: E402
from gen_golden import _grid, _import_reference, _state_keys  # noqa: E402
from gen_golden_dicl_match import seed_norm_state  # noqa: E402

OUT = HERE

CASES = (
    # name, module type, b, c, h, w, r, norm, mnet_scale, poison
    ("mnet_bn_b2_c16_r2_8x12", "dicl", 2, 16, 8, 12, 2, "batch", 1, False),
    ("mnet_none_b1_c8_r3_6x10_s05", "dicl", 1, 8, 6, 10, 3, "none", 0.5, False),
    ("mnet_emb_b1_c16_r2_4x6", "dicl-emb", 1, 16, 4, 6, 2, "batch", 1, False),
    ("mnet_nan_b1_c16_r2_8x12", "dicl", 1, 16, 8, 12, 2, "batch", 1, True),
)
POISON = ((0, 2, 5, np.nan), (0, 6, 3, np.inf))       # (batch, y, x, value of the x coordinate)


def main():
    import torch
    _import_reference()
    from src.models.common.corr import dicl, dicl_emb
    t = torch.from_numpy
    for name, cmod, b, c, h, w, r, norm, scale, poison in CASES:
        rng = np.random.default_rng(20241021)           # the first and the last case share weights and inputs
        torch.manual_seed(0)
        if cmod == "dicl":
            mod = dicl.CorrelationModule(feature_dim=c, radius=r, dap_init="standard", norm_type=norm, mnet_scale=scale)
        else:
            mod = dicl_emb.CorrelationModule(feature_dim=c, radius=r, dap_init="standard", norm_type=norm)
        mod = det_init(mod)
        stored = seed_norm_state(mod, rng)
        mod.eval()
        f1 = rng.standard_normal((2, c, h, w), dtype=np.float32)[:b]
        f2 = rng.standard_normal((2, c, h, w), dtype=np.float32)[:b]
        co = (_grid(2, h, w) + rng.normal(0.0, 1.5, size=(2, 2, h, w))).astype(np.float32)[:b]
        if poison:
            for pb, py, px, v in POISON:
                co[pb, 0, py, px] = v
        arrays = dict(fmap1=f1, fmap2=f2, coords=co, radius=np.int32(r), norm_type=np.asarray(norm),
                      cmod=np.asarray(cmod), mnet_scale=np.float64(scale), **_state_keys(mod, "sd."), **stored)
        with torch.no_grad():
            for dap in (True, False):
                cap = {}
                hook = mod.mnet.register_forward_hook(lambda m, i, o: cap.update(cost=o))
                out = mod(t(f1), t(f2), t(co), dap=dap)
                hook.remove()
                tag = "dap" if dap else "nodap"
                arrays[f"{tag}.out"] = out.numpy()
                arrays[f"{tag}.cost"] = cap["cost"].numpy()
        nan = np.isnan(arrays["nodap.cost"])
        print(f"  NaN costs: {int(nan.sum())} of {nan.size}")
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{os.path.basename(path)}  {os.path.getsize(path) / 1e6:.2f} MB  {len(arrays)} arrays")


if __name__ == "__main__":
    main()
