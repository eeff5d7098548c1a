#!/usr/bin/env python3
"""Golden gradients for the eval-mode 'dicl-1x1' correlation module (test infrastructure): what the fused
path with fused_backward=True has to reproduce.

Runs the reference's own corr.dicl_1x1.CorrelationModule (src/models/common/corr/dicl_1x1.py:33-86) from
/root/reference (qzed/raft-meets-dicl v2) in the build container, in .eval(), on the inputs, det_init
weights and stored norm state of the forward fixtures (gen_golden_dicl_match.py; those files are only
read), and stores its autograd gradients.  One fixture per forward fixture:

  match_grad_bn_b2_c16_8x12, match_grad_none_b1_c32_6x10, match_grad_nan_b2_c16_8x12

Stored per case: the inputs again, `keep` (B, d, d, h, w) — 0 on the ReLU-guarded columns of
tests/dicl_match_grad_cases.py, 1 elsewhere — and for dap=True / dap=False (`dap.` / `nodap.`):
  grad_out            the gradient of the module's output (B, d*d, h, w): seeded normal; for dap=False it is
                      the guarded grad_cost itself
  grad.fmap1, grad.fmap2, grad.<parameter>   the reference's gradients, the DAP weight included
The gradient entering the mnet's cost is multiplied by `keep` (a tensor hook on the mnet's output,
dicl_match_grad_cases.module_gradients), so guarded columns contribute nothing with the DAP in front either.

Usage:  python tests/golden/gen_golden_dicl_match_grad.py   (writes tests/golden/match_grad_*.npz)
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from detinit import det_init  # noqa: E402
from gen_golden import _import_reference  # noqa: E402

OUT = HERE


def main():
    import torch
    import conftest  # noqa: F401  (the tests' path setup)
    import dicl_match_cases as fwd
    import dicl_match_grad_cases as cases
    ref = _import_reference()
    from src.models.common.corr import dicl_1x1
    del ref
    for name in cases.FIXTURES:
        fname = cases.FORWARD_FIXTURE[name]
        g = fwd.fixture(fname)
        c, r = g["fmap1"].shape[1], int(g["radius"])
        torch.manual_seed(0)
        mod = det_init(dicl_1x1.CorrelationModule(feature_dim=c, radius=r, dap_init="standard",
                                                  norm_type=str(g["norm_type"]), mnet_scale=float(g["mnet_scale"])))
        stored = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.") and k != "sd.keys"}
        mod.load_state_dict(stored, strict=False)
        mod.eval()
        grad, frac = cases.guarded_grad(fwd.fixture_case(fname)["args"], cases.fixture_seed(name))
        b, d, _, h, w = grad.shape
        rng = np.random.default_rng(cases.fixture_seed(name) + 1)
        arrays = dict(fmap1=g["fmap1"], fmap2=g["fmap2"], coords=g["coords"], radius=g["radius"],
                      keep=1.0 - cases.guard(fwd.fixture_case(fname)["args"]).astype(np.float32))
        arrays["nodap.grad_out"] = grad.reshape(b, d * d, h, w)
        arrays["dap.grad_out"] = rng.standard_normal((b, d * d, h, w)).astype(np.float32)
        for dap in (True, False):
            tag = "dap" if dap else "nodap"
            grads, calls = cases.module_gradients(mod, arrays, dap)
            assert len(calls) == 1
            for k, v in grads.items():
                arrays[f"{tag}.grad.{k}"] = v
            nan = {k: int(np.isnan(v).sum()) for k, v in grads.items() if np.isnan(v).any()}
            print(f"  {tag}: {len(grads)} gradients, NaN entries {nan}")
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{os.path.basename(path)}  guarded {frac:.3f}  {os.path.getsize(path) / 1e6:.2f} MB  {len(arrays)} arrays")


if __name__ == "__main__":
    main()
