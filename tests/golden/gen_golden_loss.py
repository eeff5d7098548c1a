#!/usr/bin/env python3
"""Golden vectors for the sequence losses, produced by RUNNING the reference's four Loss classes.

Test infrastructure only; same import recipe as gen_golden.py.  Classes exercised (reference file:line):
  * impls.raft.SequenceLoss                              src/models/impls/raft.py:596-644
  * common.loss.mlseq.MultiLevelSequenceLoss             src/models/common/loss/mlseq.py:7-67
  * impls.raft_dicl_ctf_l3.RestrictedMultiLevelSequenceLoss   src/models/impls/raft_dicl_ctf_l3.py:401-473
  * impls.dicl.MultiscaleLoss                            src/models/impls/dicl.py:416-472
Each file holds one set of inputs (float16-representable values, stored as float16 and widened by the
tests: half the bytes, the same float32 numbers on both sides), the class's `type`, and per variant
`<tag>/...` its arguments and get_config() as JSON, the loss and every prediction's gradient (CPU fp32).

Fair-gate conditions, asserted HERE on the reference side (a new seed is drawn until they hold): on
every masked pixel of an UPSAMPLED prediction |d_c| >= 1e-4 (ord 1, absmean, robust) resp.
||d|| >= 1e-3 (ord 2), so sign(d) and d/||d|| never hinge on interpolation rounding.  Exact zeros
are planted only in full-resolution predictions, where d is one IEEE subtraction.

Usage:  python tests/golden/gen_golden_loss.py        (writes tests/golden/loss_*.npz)
"""

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, _import_reference  # noqa: E402


def _h(x):
    """float16-representable float32 values."""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def _leaves(result, pairs):
    """Flattened (prev, flow) leaves of a result structure in the order the loss visits them."""
    if pairs:
        return [(p, f) for level in result for (p, f) in level]
    if result and isinstance(result[0], (list, tuple)):
        return [(None, f) for level in result for f in level]
    return [(None, f) for f in result]


def main():
    import torch
    import torch.nn.functional as F
    _import_reference()
    from src.models.impls.raft import SequenceLoss
    from src.models.common.loss.mlseq import MultiLevelSequenceLoss
    from src.models.impls.raft_dicl_ctf_l3 import RestrictedMultiLevelSequenceLoss
    from src.models.impls.dicl import MultiscaleLoss
    t = torch.from_numpy
    total = [0]

    def up(flow, shape, mode="bilinear"):
        fh, fw = flow.shape[-2:]
        th, tw = shape[-2:]
        flow = F.interpolate(flow, (th, tw), mode=mode, align_corners=None if mode == "nearest" else True)
        return flow * torch.tensor([tw / fw, th / fh]).view(1, 2, 1, 1)

    def fair(leaves, masks, target, ord):
        """The gate conditions on the upsampled predictions' masked pixels."""
        for (_, f), m in zip(leaves, masks):
            if f.shape == target.shape:
                continue
            d = (up(t(f), target.shape) - t(target)).numpy()
            sel = np.broadcast_to(m[:, None], d.shape)
            if not sel.any():
                continue
            if ord == 2:
                if not (np.sqrt((d ** 2).sum(1))[m] >= 1e-3).all():
                    return False
            elif not (np.abs(d)[sel] >= 1e-4).all():
                return False
        return True

    def run(name, cls, variants, make, pairs=False):
        """One file: the inputs of make(rng) -> (result, target, valid) once, and per variant
        (tag, arguments, masks_of) the reference's loss and gradients under the prefix `<tag>/`.
        masks_of(result, target, valid) -> per-leaf numpy masks (None: the shared valid)."""
        seed = 1000
        while True:
            rng = np.random.default_rng(seed)
            result, target, valid = make(rng)
            leaves = _leaves(result, pairs)
            if all(fair(leaves, masks_of(result, target, valid) if masks_of else [valid] * len(leaves), target,
                        arguments["ord"]) for _, arguments, masks_of in variants):
                break
            seed += 1
        nested = pairs or isinstance(result[0], (list, tuple))
        arrays = dict(target=target.astype(np.float16), valid=valid, seed=np.int64(seed), type=np.array(cls.type),
                      variants=np.array(json.dumps([v[0] for v in variants])),
                      structure=np.array(json.dumps({"pairs": pairs, "levels": (
                          [len(level) for level in result] if nested else None)})))
        assert np.array_equal(target, _h(target))
        for i, (p, f) in enumerate(leaves):
            assert np.array_equal(f, _h(f))
            arrays[f"flow_{i}"] = f.astype(np.float16)
            if p is not None:
                assert np.array_equal(p, _h(p))
                arrays[f"prev_{i}"] = p.astype(np.float16)
        losses = []
        for tag, arguments, _ in variants:
            loss_obj = cls.from_config({"type": cls.type, "arguments": arguments})
            flows = [t(f).requires_grad_(True) for _, f in leaves]
            it = iter(flows)
            if pairs:
                res = [[(t(p), next(it)) for (p, _) in level] for level in result]
            elif nested:
                res = [[next(it) for _ in level] for level in result]
            else:
                res = [next(it) for _ in result]
            loss = loss_obj(None, res, t(target), t(valid))
            grads = torch.autograd.grad(loss, flows, allow_unused=True)
            arrays[f"{tag}/loss"] = np.float32(loss.item())
            arrays[f"{tag}/arguments"] = np.array(json.dumps(arguments))
            arrays[f"{tag}/config"] = np.array(json.dumps(loss_obj.get_config()))
            for i, g in enumerate(grads):
                arrays[f"{tag}/grad_{i}"] = (torch.zeros_like(flows[i]) if g is None else g).numpy()
            losses.append(f"{tag} {loss.item():.6g}")
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        total[0] += os.path.getsize(path)
        print(f"{name}.npz  {os.path.getsize(path) / 1e3:.1f} kB  seed {seed}  loss {', '.join(losses)}")

    def target_valid(rng, b, h, w, frac, sigma=3.0):
        return _h(sigma * rng.standard_normal((b, 2, h, w))), rng.random((b, h, w)) < frac

    def pred(rng, target, h, w, noise=1.0):
        """A prediction at (h, w): the (area-)downsampled target in its own units plus noise."""
        th, tw = target.shape[-2:]
        if (h, w) == (th, tw):
            return _h(target + noise * rng.standard_normal(target.shape))
        small = F.interpolate(t(target), (h, w), mode="bilinear", align_corners=True).numpy()
        small = small * np.float32([w / tw, h / th]).reshape(1, 2, 1, 1)
        return _h(small + noise * rng.standard_normal(small.shape))

    # ---- seq: B=2, 37x53 (odd W, a tail block, several blocks), 5 full-resolution predictions, ~70 % valid;
    #      exact flow == target pixels (valid and invalid ones) in every prediction ----------------------
    def make_seq(rng):
        target, valid = target_valid(rng, 2, 37, 53, 0.7)
        result = [pred(rng, target, 37, 53) for _ in range(5)]
        for k, f in enumerate(result):
            f[0, :, 3 + k, 5:9] = target[0, :, 3 + k, 5:9]              # both components equal
            f[1, 0, 20, 10 + k] = target[1, 0, 20, 10 + k]              # one component equal
        valid[0, 3:8, 5:7] = True
        valid[0, 3:8, 7:9] = False
        valid[1, 20, 10:15] = True
        return result, target, valid

    run("loss_seq", SequenceLoss, [("ord1", {"ord": 1}, None), ("ord2", {"ord": 2, "gamma": 0.85}, None),
                                   ("absmean", {"ord": "absmean"}, None),
                                   ("invalid", {"ord": 1, "include_invalid": True}, None)], make_seq)

    # ---- mlseq: target 2x2x48x80, levels [3 @ 3x5], [2 @ 6x10], [3 @ 48x80] -----------------------------
    def make_ml(sizes):
        def make(rng):
            b, h, w = sizes[0]
            target, valid = target_valid(rng, b, h, w, 0.5)
            return [[pred(rng, target, lh, lw) for _ in range(n)] for (n, lh, lw) in sizes[1]], target, valid
        return make

    ml = ((2, 48, 80), ((3, 3, 5), (2, 6, 10), (3, 48, 80)))
    run("loss_mlseq", MultiLevelSequenceLoss,
        [(f"ord{o}", {"ord": o, "gamma": 0.85, "alpha": (0.38, 0.6, 1.0), "scale": 0.5}, None) for o in (1, 2)],
        make_ml(ml))

    # ---- mlseq-ragged: 23x29 with a non-integer ratio, in = 1 in y, in = 1 in x, and full size ----------
    rag = ((2, 23, 29), ((2, 5, 7), (1, 1, 4), (1, 3, 1), (2, 23, 29)))
    run("loss_mlseq_ragged", MultiLevelSequenceLoss,
        [(f"ord{o}", {"ord": o, "gamma": 0.8, "alpha": (0.3, 0.5, 0.7, 1.0)}, None) for o in (1, 2)], make_ml(rag))

    # ---- empty: valid all false (NaN loss, zero gradients); valid false for one image only -------------
    def make_empty(which):
        def make(rng):
            result, target, valid = make_ml(((2, 12, 20), ((2, 3, 5), (2, 12, 20))))(rng)
            if which == "all":
                valid[:] = False
            else:
                valid[1] = False
            return result, target, valid
        return make

    for which in ("all", "one"):
        run(f"loss_empty_{which}", MultiLevelSequenceLoss,
            [("ord1", {"ord": 1, "gamma": 0.8, "alpha": (0.5, 1.0)}, None)], make_empty(which))

    # ---- restricted: 2x2x32x48, (flow_prev, flow) pairs at 4x6, 8x12, 32x48; level 0 keeps a part of its
    #      pixels, level 1 none (the skip branch), level 2 most -------------------------------------------
    def make_restricted(rng):
        target, valid = target_valid(rng, 2, 32, 48, 0.7, sigma=4.0)
        result = []
        for (n, h, w, off) in ((2, 4, 6, 0.0), (2, 8, 12, 40.0), (2, 32, 48, 0.0)):
            level = []
            for _ in range(n):
                prev = pred(rng, target, h, w, noise=0.5)
                prev = _h(prev + off * np.float32([w / 48, h / 32]).reshape(1, 2, 1, 1))   # +off px at full size
                level.append((prev, pred(rng, target, h, w)))
            result.append(level)
        return result, target, valid

    delta_range = (3.0, 6.0, 1.5)

    def restricted_masks(mode):
        def masks_of(result, target, valid):
            out = []
            for i, level in enumerate(result):
                for prev, _ in level:
                    p = t(prev) if prev.shape == target.shape else up(t(prev), target.shape, mode)
                    d = (t(target) - p).abs().numpy()
                    out.append((d[:, 0] <= delta_range[i]) & (d[:, 1] <= delta_range[i]) & valid)
            kept = [int(m.sum()) for m in out]
            assert 0 < kept[0] < valid.sum() and kept[2] == kept[3] == 0 and kept[4] > 0, kept
            return out
        return masks_of

    run("loss_restricted", RestrictedMultiLevelSequenceLoss,
        [(mode, {"ord": 1, "gamma": 0.85, "alpha": (0.38, 0.6, 1.0), "scale": 1.0, "delta_range": delta_range,
                 "delta_mode": mode}, restricted_masks(mode)) for mode in ("bilinear", "nearest")],
        make_restricted, pairs=True)

    # ---- multiscale: four levels with weights, ord 2 and robust, valid_range given and None -----------
    def make_ms(rng):
        target, valid = target_valid(rng, 2, 24, 32, 0.7)
        return [pred(rng, target, h, w) for (h, w) in ((3, 4), (6, 8), (12, 16), (24, 32))], target, valid

    weights = (0.25, 0.5, 0.75, 1.0)
    ranges = ((2.5, 2.0), (4.0, 3.5), (6.0, 6.0), (100.0, 100.0))

    def ms_masks(vr):
        def masks_of(result, target, valid):
            if vr is None:
                return [valid] * len(result)
            return [valid & (np.abs(target[:, 0]) < vr[i][0]) & (np.abs(target[:, 1]) < vr[i][1])
                    for i in range(len(result))]
        return masks_of

    variants = []
    for o in (2, "robust"):
        for tag, vr in (("range", ranges), ("norange", None)):
            args = {"weights": weights, "ord": o}
            if vr is not None:
                args["valid_range"] = vr
            variants.append((f"ord{o}_{tag}", args, ms_masks(vr)))
    run("loss_multiscale", MultiscaleLoss, variants, make_ms)

    # ---- many: 40 predictions at 2x2x8x12 (more than one 32-entry chunk) ------------------------------
    def make_many(rng):
        target, valid = target_valid(rng, 2, 8, 12, 0.7)
        return [pred(rng, target, 8, 12) for _ in range(40)], target, valid

    run("loss_many", SequenceLoss, [("ord1", {"ord": 1, "gamma": 0.95}, None)], make_many)
    print(f"total {total[0] / 1e3:.1f} kB")
    assert total[0] < 900e3


if __name__ == "__main__":
    main()
