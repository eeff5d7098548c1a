#!/usr/bin/env python3
"""Golden vectors for the eval-mode 'dicl-1x1' correlation module (test infrastructure): what the fused
dicl_match_1x1 path has to reproduce.

Runs the reference's own corr.dicl_1x1.CorrelationModule (src/models/common/corr/dicl_1x1.py:33-86) from
/root/reference (qzed/raft-meets-dicl v2) in the build container, in .eval(), with the name-keyed weights
of detinit.det_init and seeded, non-trivial batch-norm state — running variance in [0.5, 2], running mean,
gamma and beta — which IS stored (`sd.<key>`: the norm entries only; every other weight is rebuilt with
det_init).  Stored per case: the inputs, the MatchingNet output (forward hook) and the module output with
dap=True and dap=False.

  match_bn_b2_c16_8x12      b2, C16, 8x12, r3, batch norm; coords = grid + N(0, 1.5^2): windows leave the map
  match_none_b1_c32_6x10    b1, C32, 6x10, r4, no norm, mnet_scale 0.5: hidden widths 48, 64, 32
  match_nan_b2_c16_8x12     as the first, one pixel's coordinate NaN and one +inf

Usage:  python tests/golden/gen_golden_dicl_match.py   (writes tests/golden/match_*.npz)
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detinit import det_init  # noqa: E402
from gen_golden import _grid, _import_reference, _state_keys  # noqa: E402

OUT = HERE

CASES = (
    # name, b, c, h, w, r, norm, mnet_scale, poison
    ("match_bn_b2_c16_8x12", 2, 16, 8, 12, 3, "batch", 1, False),
    ("match_none_b1_c32_6x10", 1, 32, 6, 10, 4, "none", 0.5, False),
    ("match_nan_b2_c16_8x12", 2, 16, 8, 12, 3, "batch", 1, True),
)
POISON = ((0, 2, 5, np.nan), (1, 6, 3, np.inf))       # (batch, y, x, value of the x coordinate)


def seed_norm_state(mod, rng):
    """Non-trivial batch-norm state, returned as the arrays to store."""
    import torch
    stored = {}
    with torch.no_grad():
        for key, val in mod.state_dict().items():
            if key.endswith("running_var"):
                a = rng.uniform(0.5, 2.0, tuple(val.shape))
            elif key.endswith("running_mean"):
                a = rng.normal(0.0, 0.3, tuple(val.shape))
            elif ".1." in key and key.endswith(".weight") and val.dim() == 1:
                a = rng.uniform(0.7, 1.3, tuple(val.shape))
            elif ".1." in key and key.endswith(".bias") and val.dim() == 1:
                a = rng.normal(0.0, 0.2, tuple(val.shape))
            else:
                continue
            a = a.astype(np.float32)
            val.copy_(torch.from_numpy(a))
            stored["sd." + key] = a
    return stored


def main():
    import torch
    ref = _import_reference()
    from src.models.common.corr import dicl_1x1
    del ref
    t = torch.from_numpy
    for name, b, c, h, w, r, norm, scale, poison in CASES:
        rng = np.random.default_rng(20240612)           # cases (a) and (c) share inputs and weights
        torch.manual_seed(0)
        mod = det_init(dicl_1x1.CorrelationModule(feature_dim=c, radius=r, dap_init="standard", norm_type=norm,
                                                  mnet_scale=scale))
        stored = seed_norm_state(mod, rng)
        mod.eval()
        f1 = rng.standard_normal((b, c, h, w), dtype=np.float32)
        f2 = rng.standard_normal((b, c, h, w), dtype=np.float32)
        co = (_grid(b, h, w) + rng.normal(0.0, 1.5, size=(b, 2, h, w))).astype(np.float32)
        if poison:
            for pb, py, px, v in POISON:
                co[pb, 0, py, px] = v
        arrays = dict(fmap1=f1, fmap2=f2, coords=co, radius=np.int32(r), norm_type=np.asarray(norm),
                      mnet_scale=np.float64(scale), **_state_keys(mod, "sd."), **stored)
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
        print(f"  NaN costs: {int(nan.sum())} at pixels {sorted(set(zip(*np.nonzero(nan.any(axis=(1, 2))))))}")
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{os.path.basename(path)}  {os.path.getsize(path) / 1e6:.2f} MB  {len(arrays)} arrays")


if __name__ == "__main__":
    main()
