#!/usr/bin/env python3
"""The fused flow metrics (rmd.metrics / rmd.ops.flow_metrics, csrc/metrics.hip) against the eager
composite they replace, timed in one process:

  shape 1   1 estimate  (8, 2, 436, 1024): FlowMetrics with epe + fl-all + aae + flow-magnitude, for the
            whole batch (__call__) and per sample (per_sample: one launch, one readback, 8 dicts)
  shape 2  12 estimates at that size: ops.flow_metrics(list).host(), batch and per-sample values derived
            on the host from the one copy

  eager     the reference-form expressions of rmd/cpu.py (flow_metrics_eager) on the same GPU tensors
            with the reference's read-back pattern, one .item() per value: once per batch, and once per
            sample as the evaluator's loop does (src/evaluation/evaluator.py:29-37), for every estimate

Host-clock times around work that ends in a read-back (so launches, the copy and the host-side
derivation are included), median over `steps` after `warmup`; `kernel_ms` is the fused operator alone
between device events.  Algorithmic bytes: (8 N + 9) per pixel (N estimates, target, validity); the
fractions are of the 8 TB/s HBM peak — for the host-clock times an end-to-end rate, not a kernel's
share.  The work runs in a child process under its own time limit.

usage: python3 tools/metrics_probe.py [--warmup 5] [--steps 25] [--out profiles/metrics_r08.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raft-meets-dicl_amd"), ROOT):
    sys.path.insert(0, p)

HBM_PEAK = 8e12
LEG_TIMEOUT = 400
CONFIG = [{"type": "epe"}, {"type": "fl-all"}, {"type": "aae"}, {"type": "flow-magnitude"}]


def leg(warmup, steps):
    import statistics
    import time

    import torch
    import rmd
    from rmd import cpu, ops
    from rmd.metrics import _values
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    b, h, w = 8, 436, 1024
    target = (3.0 * torch.randn(b, 2, h, w, generator=g)).to(dev)
    valid = (torch.rand(b, h, w, generator=g) < 0.8).to(dev)
    estimates = [(target + torch.randn(b, 2, h, w, generator=g).to(dev)) for _ in range(12)]
    fm = rmd.FlowMetrics.from_config(CONFIG)

    def host_ms(fn):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def kernel_ms(ests):
        ev = []
        for i in range(warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.flow_metrics(ests, target, valid)
            e1.record()
            if i >= warmup:
                ev.append((e0, e1))
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(c) for a, c in ev)

    def eager(ests, per_sample):
        out = []
        for est in ests:
            if per_sample:
                for s in range(b):
                    out.append({k: v.item() for k, v in cpu.flow_metrics_eager(est[s], target[s], valid[s]).items()})
            else:
                out.append({k: v.item() for k, v in cpu.flow_metrics_eager(est, target, valid).items()})
        return out

    def fused_many(ests, per_sample):
        host = ops.flow_metrics(ests, target, valid).host()
        if per_sample:
            return [_values(host, s, k) for k in range(len(ests)) for s in range(b)]
        return [_values(host, None, k) for k in range(len(ests))]

    legs = []
    for n in (1, 12):
        ests = estimates[:n]
        nbytes = (8 * n + 9) * b * h * w
        if n == 1:
            fused_batch = lambda: fm(None, ests[0], target, valid, None)                    # noqa: E731
            fused_samples = lambda: fm.per_sample(None, ests[0], target, valid)             # noqa: E731
        else:
            fused_batch = lambda: fused_many(ests, False)                                   # noqa: E731
            fused_samples = lambda: fused_many(ests, True)                                  # noqa: E731
        ours, theirs = fused_many(ests, False)[0], eager(ests, False)[0]
        out = {"shape": f"{n} x ({b}, 2, {h}, {w})", "estimates": n, "warmup": warmup, "steps": steps,
               "algorithmic_bytes": nbytes,
               "fused": {"kernel_ms": kernel_ms(ests), "batch_ms": host_ms(fused_batch),
                         "per_sample_ms": host_ms(fused_samples)},
               "eager": {"batch_ms": host_ms(lambda: eager(ests, False)),
                         "per_sample_ms": host_ms(lambda: eager(ests, True))},
               "epe_fused": ours["epe"], "epe_eager": theirs["epe/mean"],
               "aae_fused": ours["aae"], "aae_eager": theirs["aae"]}
        for path in ("fused", "eager"):
            for k in list(out[path]):
                out[path][k.replace("_ms", "_hbm_fraction")] = nbytes / (out[path][k] * 1e-3) / HBM_PEAK
        out["eager_over_fused_batch"] = out["eager"]["batch_ms"] / out["fused"]["batch_ms"]
        out["eager_over_fused_per_sample"] = out["eager"]["per_sample_ms"] / out["fused"]["per_sample_ms"]
        legs.append(out)
    print("METRICS_PROBE " + json.dumps(legs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_r08.json"))
    ap.add_argument("--leg", action="store_true", help="internal: run the measurement in this process")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (a median over fewer steps is not reported)")
    if a.leg:
        leg(a.warmup, a.steps)
        return 0
    # a fresh child under its own time limit
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--warmup", str(a.warmup), "--steps",
                        str(a.steps)], capture_output=True, text=True, timeout=LEG_TIMEOUT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("METRICS_PROBE ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"metrics_probe: failed (exit {r.returncode})")
        return 1
    legs = json.loads(line[len("METRICS_PROBE "):])
    for lg in legs:
        print(f"metrics_probe: {lg['shape']}: fused kernel {lg['fused']['kernel_ms']:.3f} ms, batch "
              f"{lg['fused']['batch_ms']:.3f} ms vs eager {lg['eager']['batch_ms']:.3f} ms, per sample "
              f"{lg['fused']['per_sample_ms']:.3f} ms vs eager {lg['eager']['per_sample_ms']:.3f} ms")
    import torch
    doc = {"tool": "tools/metrics_probe.py", "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK, "legs": legs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"metrics_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
