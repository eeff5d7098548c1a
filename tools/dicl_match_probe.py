#!/usr/bin/env python3
"""The fused dicl-1x1 cost (rmd.ops.dicl_match_1x1, csrc/dicl_match.hip) against the path it replaces, timed in
one process between device events:

  shapes    the three levels of raft+dicl/ctf-l3 at cfg4 on a batch of 8 (1/8: 48x160, 1/16: 24x80, 1/32:
            12x40), C = 32, r = 4, mnet scale 1, eval-mode batch norm with non-trivial running statistics
  fused     dicl_1x1.CorrelationModule(fused="on") with precision "fp32" (three split-bf16 products per
            layer) and "bf16" (one), dap=False: the fold of the norm layers, the weight repack and the kernel
  today     the same module with fused="off": rmd_dicl_stack, then four MIOpen 1x1 convolutions with their
            norm and ReLU passes — the parent commit's behaviour
  graph     the fused forward, GRAPH_CALLS calls captured in one graph and replayed
  memory    peak bytes of one forward above its start, every side
  error     max |side - float64| / max |float64| on SAMPLES random (pixel, displacement) columns, the
            float64 values from oracle.dicl.dicl_stack_at and a float64 MLP of the folded parameters
  cases     for every case of tests/dicl_match_cases.py (fixtures and sweep): the emulation error e of each
            mode (CPU), the tolerance max(1e-5, 3 e) and the kernel's measured error

The sides alternate inside one loop (the machine is shared); median over `steps` after `warmup`.
Algorithmic FLOPs: 2 x 26,688 MAC per column; the fraction is of the 2.5 PFLOP/s dense bf16 MFMA peak (the
three-product mode issues three times the MFMAs for the same algorithmic FLOPs).  The work runs in a child
process under its own time limit.

usage: python3 tools/dicl_match_probe.py [--warmup 20] [--steps 50] [--out profiles/dicl_match_r12.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "raft-meets-dicl_amd"), ROOT):
    sys.path.insert(0, p)

MFMA_PEAK = 2.5e15
LEG_TIMEOUT = 540
GRAPH_CALLS = 10
SAMPLES = 60000
BATCH, CHANNELS, RADIUS = 8, 32, 4
SHAPES = [("ctf-l3 1/8", 48, 160), ("ctf-l3 1/16", 24, 80), ("ctf-l3 1/32", 12, 40)]


def leg(warmup, steps):
    import statistics

    import numpy as np
    import torch
    import rmd
    import dicl_match_cases as cases
    from detinit import det_init_fanin
    from oracle.dicl import dicl_stack_at
    from rmd import ops
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)

    def interleaved_ms(fns):
        ev = [[] for _ in fns]
        for i in range(warmup + steps):
            for n, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                if i >= warmup:
                    ev[n].append((e0, e1))
        torch.cuda.synchronize()
        return [statistics.median(a.elapsed_time(c) for a, c in e) for e in ev]

    def peak_bytes(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        del out
        return peak

    def module(fused, precision="fp32"):
        torch.manual_seed(0)
        m = det_init_fanin(rmd.corr.make_cmod("dicl-1x1", CHANNELS, RADIUS, fused=fused, precision=precision))
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for block in list(m.mnet)[:3]:
                block[1].running_var.copy_(torch.rand(block[1].running_var.shape, generator=g) * 1.5 + 0.5)
        return m.eval().to(dev)

    sides = {"fused_fp32": module("on", "fp32"), "fused_bf16": module("on", "bf16"), "today": module("off")}
    weights, biases = (([t.detach().cpu().numpy().astype(np.float64) for t in part]) for part in sides["today"].mnet.folded())
    d = 2 * RADIUS + 1
    macs = sum(w.size for w in weights)
    legs = []
    for name, h, w in SHAPES:
        f1 = rng.standard_normal((BATCH, CHANNELS, h, w), dtype=np.float32)
        f2 = rng.standard_normal((BATCH, CHANNELS, h, w), dtype=np.float32)
        co = cases.grid_coords(rng, BATCH, h, w, 2.0).astype(np.float32)
        t1, t2, tc = (torch.from_numpy(a).to(dev) for a in (f1, f2, co))
        fns = {}
        for side, m in sides.items():
            def fn(m=m):
                with torch.no_grad():
                    return m(t1, t2, tc, dap=False)
            fns[side] = fn
        # float64 on sampled columns
        idx = (rng.integers(0, BATCH, SAMPLES), rng.integers(0, d, SAMPLES), rng.integers(0, d, SAMPLES),
               rng.integers(0, h, SAMPLES), rng.integers(0, w, SAMPLES))
        x = dicl_stack_at(f1.astype(np.float64), f2.astype(np.float64), co.astype(np.float64), RADIUS, idx).T
        for wt, t in zip(weights[:3], biases[:3]):
            x = cases.relu64(wt @ x + t.reshape(-1, 1))
        ref = (weights[3].reshape(1, -1) @ x + biases[3].reshape(-1)[0]).reshape(-1)
        error = {}
        for side, fn in fns.items():
            got = fn().view(BATCH, d, d, h, w).cpu().numpy()[idx].astype(np.float64)
            error[side] = float(np.abs(got - ref).max() / np.abs(ref).max())
        order = list(fns)
        t = dict(zip(order, interleaved_ms([fns[s] for s in order])))
        graph_ms = {}
        for side in ("fused_fp32", "fused_bf16"):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep = [fns[side]() for _ in range(GRAPH_CALLS)]
            graph_ms[side] = interleaved_ms([graph.replay])[0] / GRAPH_CALLS
            del keep, graph
        columns = BATCH * d * d * h * w
        flops = 2.0 * macs * columns
        legs.append({"shape": f"{name}: fmaps ({BATCH}, {CHANNELS}, {h}, {w}), r = {RADIUS}, cost ({BATCH}, {d}, {d}, {h}, {w})",
                     "columns": columns, "algorithmic_flops": flops, "warmup": warmup, "steps": steps,
                     "forward_ms": t, "today_over_fused": {s: t["today"] / t[s] for s in ("fused_fp32", "fused_bf16")},
                     "graph_replay": {"calls_per_graph": GRAPH_CALLS, "forward_ms": graph_ms,
                                      "mfma_peak_fraction": {s: flops / (ms * 1e-3) / MFMA_PEAK for s, ms in graph_ms.items()}},
                     "forward_peak_bytes": {s: peak_bytes(fn) for s, fn in fns.items()},
                     "max_normalised_error_vs_float64": {"samples": SAMPLES, **error}})
    # the tests' cases: emulation error, tolerance and the kernel's error
    table = []
    for label, get in cases.all_cases():
        c = get()
        f1, f2, co, r, ws, ts = c["args"]
        row = {"case": label}
        for precision in cases.PRODUCTS:
            out = ops.dicl_match_1x1(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (f1, f2, co)), r,
                                     [torch.from_numpy(a).to(dev) for a in ws], [torch.from_numpy(a).to(dev) for a in ts],
                                     precision=precision)
            row[precision] = {"emulation_e": c["e"][precision], "tolerance": c["tol"][precision],
                              "kernel_error": cases.max_norm_err(out.cpu().numpy(), c["ref"])}
        table.append(row)
    print("DICL_MATCH_PROBE " + json.dumps({"legs": legs, "cases": table}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dicl_match_r12.json"))
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
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("DICL_MATCH_PROBE ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"dicl_match_probe: failed (exit {r.returncode})")
        return 1
    res = json.loads(line[len("DICL_MATCH_PROBE "):])
    for lg in res["legs"]:
        t, g = lg["forward_ms"], lg["graph_replay"]
        print(f"dicl_match_probe: {lg['shape']}: fused fp32 {t['fused_fp32']:.3f} ms, bf16 {t['fused_bf16']:.3f} ms, today "
              f"{t['today']:.3f} ms; graph replay fp32 {g['forward_ms']['fused_fp32']:.3f} ms "
              f"({100 * g['mfma_peak_fraction']['fused_fp32']:.1f} % of the bf16 MFMA peak), bf16 "
              f"{g['forward_ms']['fused_bf16']:.3f} ms ({100 * g['mfma_peak_fraction']['fused_bf16']:.1f} %); peak "
              f"{lg['forward_peak_bytes']['fused_fp32'] / 1e6:.1f} MB vs {lg['forward_peak_bytes']['today'] / 1e6:.1f} MB; "
              f"error vs float64 {lg['max_normalised_error_vs_float64']}")
    import torch
    doc = {"tool": "tools/dicl_match_probe.py", "torch": torch.__version__, "mfma_peak_flops_per_s": MFMA_PEAK, **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"dicl_match_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
