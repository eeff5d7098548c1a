#!/usr/bin/env python3
"""The fused DICL flow head (rmd.ops.dicl_flow_head, csrc/dicl_head.hip) against the eager composite it
replaces, timed in one process between device events:

  shapes    the five cfg3 levels (batch 8; 96x128, 48x64, 24x32, 12x16, 6x8; D = 49) and the cfg4 shape
            (batch 8, D = 81, 47x155), each with a coarse flow
  fused     forward: one rmd_dicl_flow_head launch; forward + backward: that launch and one
            rmd_dicl_flow_head_backward launch through autograd (upstream gradients on flow and entropy)
  eager     the reference-form expressions of rmd/cpu.py (dicl_flow_head_eager: FlowRegression, the
            coarse-flow addition, FlowEntropy) on the same GPU tensors, and their autograd backward

  graph     the fused forward, the fused backward operator and the eager forward again, 20 calls captured
            in one graph and replayed: the per-call time without the host's launch work.  At these sizes
            an eagerly launched call is host-bound (the launch work of one operator call, or of an
            autograd pass, takes longer than the kernels), so the fused / eager event times compare
            launch counts and vary with the host; the graph figures are the device's

Median over `steps` after `warmup`.  Algorithmic bytes per pixel: forward 4 D + 12 (+ 8 with the coarse
flow), backward 8 D + 12; the fractions are of the 8 TB/s HBM peak.  The work runs in a child process
under its own time limit.

usage: python3 tools/dicl_head_probe.py [--warmup 30] [--steps 50] [--out profiles/dicl_head_r09.json]
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
LEG_TIMEOUT = 300
GRAPH_CALLS = 20
# (name, batch, ru, rv, h, w)
SHAPES = [("cfg3 level 2", 8, 3, 3, 96, 128), ("cfg3 level 3", 8, 3, 3, 48, 64), ("cfg3 level 4", 8, 3, 3, 24, 32),
          ("cfg3 level 5", 8, 3, 3, 12, 16), ("cfg3 level 6", 8, 3, 3, 6, 8), ("cfg4", 8, 4, 4, 47, 155)]


def leg(warmup, steps):
    import statistics

    import torch
    import rmd  # noqa: F401
    from rmd import cpu, ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(9)

    def event_ms(fn):
        ev = []
        for i in range(warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if i >= warmup:
                ev.append((e0, e1))
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(c) for a, c in ev)

    def graph_ms(fn):
        """Per-call time of GRAPH_CALLS captured calls replayed as one graph: the launches without the host."""
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = [fn() for _ in range(GRAPH_CALLS)]
        ms = event_ms(graph.replay) / GRAPH_CALLS
        del keep, graph
        return ms

    legs = []
    for name, b, ru, rv, h, w in SHAPES:
        du, dv = 2 * ru + 1, 2 * rv + 1
        d, pixels = du * dv, b * h * w
        cost = (2.0 * torch.randn(b, du, dv, h, w, generator=gen)).to(dev).requires_grad_(True)
        coarse = torch.randn(b, 2, h, w, generator=gen).to(dev)
        g_flow = torch.randn(b, 2, h, w, generator=gen).to(dev)
        g_ent = torch.randn(b, 1, h, w, generator=gen).to(dev)

        def fused_fwd():
            with torch.no_grad():
                return ops.dicl_flow_head(cost, coarse)

        def eager_fwd():
            with torch.no_grad():
                return cpu.dicl_flow_head_eager(cost, coarse, 1e-9)

        def fused_both():
            return torch.autograd.grad(ops.dicl_flow_head(cost, coarse), cost, (g_flow, g_ent))

        def eager_both():
            return torch.autograd.grad(cpu.dicl_flow_head_eager(cost, coarse, 1e-9), cost, (g_flow, g_ent))

        def fused_bwd():
            return torch.ops.rmd.dicl_flow_head_backward(g_out, cost.detach(), 1e-9)

        g_out = torch.cat((g_flow, g_ent), 1)
        (ours,), (theirs,) = fused_both(), eager_both()
        fwd_bytes = (4 * d + 12 + 8) * pixels
        bwd_bytes = (8 * d + 12) * pixels
        both_bytes = fwd_bytes + bwd_bytes
        out = {"shape": f"{name}: ({b}, {du}, {dv}, {h}, {w})", "displacements": d, "pixels": pixels,
               "warmup": warmup, "steps": steps,
               "forward_bytes": fwd_bytes, "forward_backward_bytes": both_bytes,
               "fused": {"forward_ms": event_ms(fused_fwd), "forward_backward_ms": event_ms(fused_both)},
               "eager": {"forward_ms": event_ms(eager_fwd), "forward_backward_ms": event_ms(eager_both)},
               "grad_max_abs_difference": float((ours - theirs).abs().max())}
        dv_ = {"fused_forward_ms": graph_ms(fused_fwd), "fused_backward_ms": graph_ms(fused_bwd),
               "eager_forward_ms": graph_ms(eager_fwd)}
        dv_["fused_forward_hbm_fraction"] = fwd_bytes / (dv_["fused_forward_ms"] * 1e-3) / HBM_PEAK
        dv_["fused_backward_hbm_fraction"] = bwd_bytes / (dv_["fused_backward_ms"] * 1e-3) / HBM_PEAK
        out["graph_replay"] = dv_
        for path in ("fused", "eager"):
            t = out[path]
            t["forward_hbm_fraction"] = fwd_bytes / (t["forward_ms"] * 1e-3) / HBM_PEAK
            t["forward_backward_hbm_fraction"] = both_bytes / (t["forward_backward_ms"] * 1e-3) / HBM_PEAK
        out["eager_over_fused_forward"] = out["eager"]["forward_ms"] / out["fused"]["forward_ms"]
        out["eager_over_fused_forward_backward"] = (out["eager"]["forward_backward_ms"]
                                                    / out["fused"]["forward_backward_ms"])
        legs.append(out)
    print("DICL_HEAD_PROBE " + json.dumps(legs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dicl_head_r09.json"))
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
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("DICL_HEAD_PROBE ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"dicl_head_probe: failed (exit {r.returncode})")
        return 1
    legs = json.loads(line[len("DICL_HEAD_PROBE "):])
    for lg in legs:
        print(f"dicl_head_probe: {lg['shape']}: forward {lg['fused']['forward_ms']:.4f} ms vs eager "
              f"{lg['eager']['forward_ms']:.4f} ms, forward + backward {lg['fused']['forward_backward_ms']:.4f} ms vs "
              f"eager {lg['eager']['forward_backward_ms']:.4f} ms")
    import torch
    doc = {"tool": "tools/dicl_head_probe.py", "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK, "legs": legs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"dicl_head_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
