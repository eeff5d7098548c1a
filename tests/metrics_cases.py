"""Shared helpers of test_metrics.py / test_gpu_metrics.py: the metric fixtures of
tests/golden/gen_golden_metrics.py (loaded once per process and never modified), the tests' own numpy
float64 evaluation of their inputs, and the gate both devices are held to.

Gate (per value of every class, for the batch and for every sample alone):
  * a ratio of counts (`<d>px`, Fl-all): round(ref * n_valid) == round(ours * n_valid), and ours is an
    exact count over n_valid.  The reference's ratio is an fp32 mean of zeros and ones, at most 6e-8
    relative off count / n_valid, far below half a pixel at these sizes; the fixtures keep every
    unplanted valid pixel 1e-5 relative away from every threshold, so the count does not hinge on the
    epe's fp32 rounding.
  * a mean (epe, angle, magnitude): |ours - ref| <= |ref - f64| + 1e-6 |f64| with f64 the numpy float64
    evaluation below: no farther from the reference than the reference is from the truth, plus our
    own bound (an fp32 epe or norm is <= 3 roundings ~ 2e-7 relative per pixel, all terms positive,
    accumulation in double; the angle is evaluated in double).
  * a non-finite reference value (NaN, +-Inf) is reproduced as such.
"""

import functools
import json
import math

import numpy as np
import torch

from conftest import load_golden

# fixture file -> number of config lists (tests/golden/gen_golden_metrics.py)
FILES = {"metrics_main": 2, "metrics_small": 1, "metrics_empty": 1, "metrics_nonfinite": 2}
CASES = [(f, i) for f, n in FILES.items() for i in range(n)]
FL_ABS, FL_REL = 3.0, float(np.float32(0.05))


class Case:
    def __init__(self, name):
        g = load_golden(name)
        self.name = name
        self.estimate = g["estimate"].astype(np.float32)
        self.target = g["target"].astype(np.float32)
        self.valid = g["valid"]
        self.planted = [(int(b), int(y), int(x), float(d0), float(d1)) for b, y, x, d0, d1 in g["planted"]]
        self.configs = json.loads(str(g["configs"]))
        self.results = json.loads(str(g["results"]))
        self.batch = self.target.shape[0]

    def scopes(self):
        return ["batch"] + [f"s{b}" for b in range(self.batch)]

    def arrays(self, scope):
        if scope == "batch":
            return self.estimate, self.target, self.valid
        b = int(scope[1:])
        return self.estimate[b:b + 1], self.target[b:b + 1], self.valid[b:b + 1]

    def tensors(self, device):
        t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        return t(self.estimate), t(self.target), t(self.valid)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def truth(cfg, estimate, target, valid):
    """numpy float64 evaluation of one metric config -> [(key, value, kind)], kind 'mean' or 'ratio'."""
    e, t = estimate.astype(np.float64), target.astype(np.float64)
    with np.errstate(all="ignore"):
        if cfg["type"] in ("epe", "fl-all"):
            epe = np.sqrt(((e - t) ** 2).sum(1))[valid]
            n = epe.size
            if cfg["type"] == "fl-all":
                tgt = np.sqrt((t ** 2).sum(1))[valid]
                bad = (epe > FL_ABS) & (epe > FL_REL * tgt)
                return [(cfg.get("key", "Fl-all"), bad.mean() if n else math.nan, "ratio")]
            key = cfg.get("key", "EndPointError/")
            out = [(f"{key}mean", epe.mean() if n else math.nan, "mean")]
            return out + [(f"{key}{d}px", (epe <= d).mean() if n else math.nan, "ratio")
                          for d in cfg.get("distances", [1, 3, 5])]
        if cfg["type"] == "aae":
            cos = ((e * t).sum(1) + 1) / (np.sqrt((e ** 2).sum(1)) * np.sqrt((t ** 2).sum(1)) + 1)
            cos = np.where(np.isnan(cos), cos, np.clip(cos, -1.0, 1.0))
            return [(cfg.get("key", "AverageAngularError"), np.degrees(np.arccos(cos).mean()), "mean")]
        if cfg["type"] == "flow-magnitude":
            mag = np.linalg.norm(e, ord=cfg.get("ord", 2), axis=1)
            if cfg.get("ord", 2) == math.inf:                    # np.max drops no NaN, as torch's norm
                mag = np.abs(e).max(1)
            return [(cfg.get("key", "FlowMagnitude"), mag.mean(), "mean")]
    raise KeyError(cfg["type"])


def check_entry(cfg, entry, ours, arrays, label):
    """One metric's result dict `ours` against the fixture entry of the same scope."""
    estimate, target, valid = arrays
    n_valid = int(valid.sum())
    ref = entry["result"]
    assert list(ours.keys()) == [k for k, _ in ref], (label, list(ours.keys()), ref)
    for (key, ref_v), (tkey, f64, kind) in zip(ref, truth(cfg, estimate, target, valid)):
        assert key == tkey
        got = ours[key]
        assert isinstance(got, float)
        print(f"{label} {key}: ours {got!r} ref {ref_v!r} f64 {float(f64)!r}")
        if not math.isfinite(ref_v):
            assert (math.isnan(got) and math.isnan(ref_v)) or got == ref_v, (label, key, got, ref_v)
        elif kind == "ratio":
            count = got * n_valid
            assert abs(count - round(count)) <= 1e-6, (label, key, count)
            assert round(count) == round(ref_v * n_valid), (label, key, got, ref_v, n_valid)
        else:
            assert abs(got - ref_v) <= abs(ref_v - f64) + 1e-6 * abs(f64), (label, key, got, ref_v, float(f64))


def check_against_fixture(c, index, batch_result, sample_results):
    """FlowMetrics results (the batch dict, the per-sample list) against the fixture's config list `index`."""
    cfgs = c.configs[index]
    for scope, ours in zip(c.scopes(), [batch_result] + list(sample_results)):
        entries = c.results[index][scope]
        assert list(ours.keys()) == [k for entry in entries for k, _ in entry["result"]], "key order"
        for cfg, entry in zip(cfgs, entries):
            part = {k: ours[k] for k, _ in entry["result"]}
            check_entry(cfg, entry, part, c.arrays(scope), f"{c.name}[{index}]/{scope}")


def fair_inputs(shape, frac, distances, seed0=0, scales=(1.0,)):
    """Random inputs for shape (B, 2, H, W), redrawn until every valid pixel's float64 epe is 1e-5
    relative away from every threshold (the fixtures' gate condition), for the estimate times every one
    of `scales` -> torch CPU tensors."""
    b, _, h, w = shape
    for seed in range(seed0, seed0 + 50):
        rng = np.random.default_rng(seed)
        target = (3.0 * rng.standard_normal(shape)).astype(np.float32)
        estimate = (target + 2.0 * rng.standard_normal(shape)).astype(np.float32)
        valid = rng.random((b, h, w)) < frac
        tgt = np.sqrt((target.astype(np.float64) ** 2).sum(1))
        thrs = [np.full_like(tgt, t) for t in set(distances) | {FL_ABS}] + [FL_REL * tgt]
        epes = [np.sqrt(((estimate * np.float32(s) - target.astype(np.float64)) ** 2).sum(1)) for s in scales]
        if all((np.abs(epe - thr)[valid] >= 1e-5 * thr[valid]).all() for thr in thrs for epe in epes):
            return torch.from_numpy(estimate), torch.from_numpy(target), torch.from_numpy(valid)
    raise AssertionError("no seed met the gate condition")
