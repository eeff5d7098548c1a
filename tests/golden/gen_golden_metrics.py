#!/usr/bin/env python3
"""Golden vectors for the flow metrics, produced by RUNNING the reference's metric classes on CPU.

Test infrastructure only; same import recipe as gen_golden.py.  Classes exercised (reference file:line):
  * metrics.epe.EndPointError          src/metrics/epe.py:10-57
  * metrics.fl_all.FlAll               src/metrics/fl_all.py:7-48
  * metrics.aae.AverageAngularError    src/metrics/aae.py:7-48, fed movedim(-3, -1) views: the class indexes
                                       the last axis, so channel-last views give it the flow components
  * metrics.flow.FlowMagnitude         src/metrics/flow.py:7-40
Each file holds one set of inputs (float16-representable values, stored as float16 and widened by the
tests), `configs` (JSON: a list of metric-config lists, the form of cfg/eval/*.yaml `metrics`) and
`results` (JSON): per config list and per scope ("batch", "s0", "s1", ...: the whole batch, every sample
alone) one entry per metric, {"config": get_config(), "result": [[key, value], ...]} in the class's order.

Fair-gate conditions, asserted HERE on the reference side (a new seed is drawn until they hold): on every
valid pixel that is finite and not planted, the float64 epe is at least 1e-5 relative away from every
distance of the file's configs, from the absolute outlier threshold 3 and from 0.05f * ||target||: about
50x fp32's rounding of the epe expression, so no count hinges on it.

Planted pixels (listed in `planted`: b, y, x, d0, d1), exempt from the gate: valid pixels with
estimate = target + d in exactly representable arithmetic, d = (3, 4) (epe 5), (0, 3), (0, 1), (0, 0),
which sit exactly ON a threshold (`<=` holds, `>` does not); the reference's answer for them does not
depend on rounding.

Usage:  python tests/golden/gen_golden_metrics.py        (writes tests/golden/metrics_*.npz)
"""

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, _import_reference  # noqa: E402

DEFAULT = [{"type": "epe"}, {"type": "fl-all"}, {"type": "aae"}, {"type": "flow-magnitude"}]
VARIANT = [{"type": "epe", "key": "epe/", "distances": [0.5, 2, 10]}, {"type": "fl-all", "key": "fl"},
           {"type": "aae", "key": "angle"}, {"type": "flow-magnitude", "ord": 1, "key": "l1"},
           {"type": "flow-magnitude", "ord": float("inf"), "key": "max"}]
PLANT = [(3.0, 4.0), (0.0, 3.0), (0.0, 1.0), (0.0, 0.0)]
FL_ABS, FL_REL = 3.0, float(np.float32(0.05))


def _h(x):
    """float16-representable float32 values."""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def fair(estimate, target, valid, planted, distances):
    """The gate condition -> (holds, smallest relative gap)."""
    d = estimate.astype(np.float64) - target.astype(np.float64)
    epe = np.sqrt((d ** 2).sum(1))
    tgt = np.sqrt((target.astype(np.float64) ** 2).sum(1))
    sel = valid & np.isfinite(epe)
    for (b, y, x, _, _) in planted:
        sel[b, y, x] = False
    gap = np.inf
    for thr in [np.full_like(epe, t) for t in sorted(set(distances) | {FL_ABS})] + [FL_REL * tgt]:
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(epe - thr)[sel] / thr[sel]
        if rel.size:
            gap = min(gap, float(rel.min()))
    return gap >= 1e-5, gap


def main():
    import torch
    _import_reference()
    from src.metrics import Metric
    t = torch.from_numpy
    total = [0]

    def run_reference(cfg, estimate, target, valid):
        """One metric class on one (batch or single-instance) input -> its entry."""
        metric = Metric.from_config(cfg)
        e, g = t(estimate), t(target)
        if cfg["type"] == "aae":
            e, g = e.movedim(-3, -1), g.movedim(-3, -1)
        result = metric(None, None, e, g, t(valid), None)
        return {"config": metric.get_config(), "result": [[k, float(v)] for k, v in result.items()]}

    def run(name, make, configs):
        distances = set()
        for cfg_list in configs:
            for cfg in cfg_list:
                if cfg["type"] == "epe":
                    distances |= {float(d) for d in cfg.get("distances", [1, 3, 5])}
        seed = 2000
        while True:
            rng = np.random.default_rng(seed)
            estimate, target, valid, planted = make(rng)
            ok, gap = fair(estimate, target, valid, planted, distances)
            if ok:
                break
            seed += 1
        assert np.array_equal(target, _h(target)) and np.array_equal(estimate, _h(estimate), equal_nan=True)
        for (b, y, x, d0, d1) in planted:            # exact arithmetic on the planted pixels
            assert valid[b, y, x]
            assert estimate[b, 0, y, x] - target[b, 0, y, x] == d0 and estimate[b, 1, y, x] - target[b, 1, y, x] == d1
        results = []
        for cfg_list in configs:
            scopes = {"batch": [run_reference(c, estimate, target, valid) for c in cfg_list]}
            for b in range(target.shape[0]):
                scopes[f"s{b}"] = [run_reference(c, estimate[b], target[b], valid[b]) for c in cfg_list]
            results.append(scopes)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, estimate=estimate.astype(np.float16), target=target.astype(np.float16), valid=valid,
                            planted=np.asarray(planted, dtype=np.float32).reshape(-1, 5), seed=np.int64(seed),
                            min_gap=np.float64(gap), configs=np.array(json.dumps(configs)),
                            results=np.array(json.dumps(results)))
        total[0] += os.path.getsize(path)
        print(f"{name}.npz  {os.path.getsize(path) / 1e3:.1f} kB  seed {seed}  min gap {gap:.2e}  "
              f"batch {[r['result'][0][1] for r in results[0]['batch']]}")

    def inputs(rng, b, h, w, frac, sigma=3.0, noise=2.0):
        target = _h(sigma * rng.standard_normal((b, 2, h, w)))
        estimate = _h(target + noise * rng.standard_normal((b, 2, h, w)))
        return estimate, target, rng.random((b, h, w)) < frac

    def plant(estimate, target, valid, b, y, x0):
        """The four on-threshold pixels in row y of sample b from column x0 on."""
        out = []
        for i, (d0, d1) in enumerate(PLANT):
            x = x0 + i
            target[b, :, y, x] = (1.5, -2.0)
            estimate[b, :, y, x] = (1.5 + d0, -2.0 + d1)
            valid[b, y, x] = True
            out.append((b, y, x, d0, d1))
        return out

    # ---- main: (3, 2, 37, 53), ~70 % valid, default and non-default configs, planted pixels in two samples
    def make_main(rng):
        estimate, target, valid = inputs(rng, 3, 37, 53, 0.7)
        return estimate, target, valid, plant(estimate, target, valid, 0, 4, 7) + plant(estimate, target, valid, 2, 30, 40)

    run("metrics_main", make_main, [DEFAULT, VARIANT])

    # ---- small: (2, 2, 20, 36), a plane that is a multiple of 4 pixels -------------------------------
    def make_small(rng):
        estimate, target, valid = inputs(rng, 2, 20, 36, 0.5, sigma=1.0, noise=3.0)
        return estimate, target, valid, plant(estimate, target, valid, 1, 10, 16)

    run("metrics_small", make_small, [DEFAULT])

    # ---- empty: the second sample's mask is all false (NaN means for it, finite batch values) --------
    def make_empty(rng):
        estimate, target, valid = inputs(rng, 2, 12, 20, 0.7)
        valid[1] = False
        return estimate, target, valid, []

    run("metrics_empty", make_empty, [DEFAULT])

    # ---- nonfinite: NaN at a valid pixel (s0), +Inf at an invalid one (s1), NaN at an invalid one (s2),
    #      -Inf at a valid one (s3) ---------------------------------------------------------------------
    def make_nonfinite(rng):
        estimate, target, valid = inputs(rng, 4, 10, 12, 0.7)
        valid[0, 2, 3], valid[1, 4, 5], valid[2, 6, 7], valid[3, 8, 9] = True, False, False, True
        estimate[0, 1, 2, 3] = np.nan
        estimate[1, 0, 4, 5] = np.inf
        estimate[2, 0, 6, 7] = np.nan
        estimate[3, 1, 8, 9] = -np.inf
        return estimate, target, valid, []

    run("metrics_nonfinite", make_nonfinite, [DEFAULT, VARIANT])
    print(f"total {total[0] / 1e3:.1f} kB")
    assert total[0] < 800e3


if __name__ == "__main__":
    main()
