#!/usr/bin/env python3
"""The fused local cross-attention of HUpCrossAttn (rmd.ops.local_cross_attn, csrc/hsup.hip) against the
eager composition it replaces, timed in one process between device events:

  shapes    the two level transitions of raft+dicl/ctf-l3 on a 448x1024 batch of 8 with ck = 64, cv = 128:
            1/16 -> 1/8 (q 56x128 from 28x64) and 1/32 -> 1/16 (q 28x64 from 14x32), 3x3 window
  fused     forward: one rmd_local_cross_attn launch; forward + backward: that launch and the two
            launches of rmd_local_cross_attn_backward through autograd
  eager     the reference-form expressions of rmd/cpu.py (local_cross_attn_eager: unfold, expand to
            (B, c, 9, h, w), matmul, softmax, product and sum) on the same GPU tensors, and their
            autograd backward
  graph     the fused forward, the fused backward operator and the eager forward, GRAPH_CALLS calls
            captured in one graph and replayed: the per-call time without the host's launch work
  memory    bytes a forward holds for its backward (allocated after the forward, output included, minus
            before) and the forward's peak above its start, fused and eager

Fused and eager steps alternate inside one loop (the machine is shared); median over `steps` after
`warmup`.  Algorithmic bytes: forward q + k + v + out, backward grad + q + k + v + the three
gradients, 4 bytes each; the fractions are of the 8 TB/s HBM peak.  The work runs in a child process
under its own time limit.

usage: python3 tools/hsup_probe.py [--warmup 20] [--steps 50] [--out profiles/hsup_r11.json]
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
GRAPH_CALLS = 10
# (name, batch, ck, cv, h2, w2, fy, fx)
SHAPES = [("ctf-l3 1/16 -> 1/8", 8, 64, 128, 28, 64, 2, 2), ("ctf-l3 1/32 -> 1/16", 8, 64, 128, 14, 32, 2, 2)]
WINDOW = (3, 3)


def leg(warmup, steps):
    import statistics

    import torch
    import rmd  # noqa: F401
    from rmd import _lib, cpu, ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(11)

    def interleaved_ms(fns):
        """Median time of each callable, one call of each per step in turn."""
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

    def graphs_ms(fns):
        """Per-call time of GRAPH_CALLS captured calls of each callable replayed as one graph."""
        graphs, keep = [], []
        for fn in fns:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep.append([fn() for _ in range(GRAPH_CALLS)])
            graphs.append(graph)
        ms = [t / GRAPH_CALLS for t in interleaved_ms([g.replay for g in graphs])]
        del keep, graphs
        return ms

    def forward_memory(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        held, peak = torch.cuda.memory_allocated(dev) - base, torch.cuda.max_memory_allocated(dev) - base
        del out
        return {"held_for_backward_bytes": held, "forward_peak_bytes": peak}

    legs = []
    for name, b, ck, cv, h2, w2, fy, fx in SHAPES:
        h, w = h2 * fy, w2 * fx
        scale = 3.0 ** 0.5 / ck ** 0.25                         # logits of standard deviation 3
        q = (scale * torch.randn(b, ck, h, w, generator=gen)).to(dev).requires_grad_(True)
        k = (scale * torch.randn(b, ck, h2, w2, generator=gen)).to(dev).requires_grad_(True)
        v = torch.randn(b, cv, h2, w2, generator=gen).to(dev).requires_grad_(True)
        grad = torch.randn(b, cv, h, w, generator=gen).to(dev)
        route = _lib.lib().rmd_local_cross_attn_kernel(b, ck, cv, h, w, h2, w2, *WINDOW).decode()

        def fused_fwd():
            with torch.no_grad():
                return ops.local_cross_attn(q, k, v, WINDOW)

        def eager_fwd():
            with torch.no_grad():
                return cpu.local_cross_attn_eager(q, k, v, WINDOW)

        def fused_both():
            return torch.autograd.grad(ops.local_cross_attn(q, k, v, WINDOW), (q, k, v), grad)

        def eager_both():
            return torch.autograd.grad(cpu.local_cross_attn_eager(q, k, v, WINDOW), (q, k, v), grad)

        def fused_bwd():
            return torch.ops.rmd.local_cross_attn_backward(grad, q.detach(), k.detach(), v.detach(), *WINDOW)

        ours, theirs = fused_both(), eager_both()
        diff = {n: float((a - c).abs().max() / c.abs().max()) for n, a, c in zip(("grad_q", "grad_k", "grad_v"), ours, theirs)}
        diff["out"] = float((fused_fwd() - eager_fwd()).abs().max() / eager_fwd().abs().max())
        del ours, theirs
        fwd_bytes = 4 * (q.numel() + k.numel() + v.numel() + grad.numel())
        bwd_bytes = 4 * (grad.numel() + 2 * (q.numel() + k.numel() + v.numel()))
        t = interleaved_ms([fused_fwd, eager_fwd, fused_both, eager_both])
        g = graphs_ms([fused_fwd, fused_bwd, eager_fwd])
        out = {"shape": f"{name}: q ({b}, {ck}, {h}, {w}), k ({b}, {ck}, {h2}, {w2}), v ({b}, {cv}, {h2}, {w2})",
               "window": list(WINDOW), "route": route, "warmup": warmup, "steps": steps,
               "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes,
               "fused": {"forward_ms": t[0], "forward_backward_ms": t[2]},
               "eager": {"forward_ms": t[1], "forward_backward_ms": t[3]},
               "eager_over_fused_forward": t[1] / t[0], "eager_over_fused_forward_backward": t[3] / t[2],
               "graph_replay": {"calls_per_graph": GRAPH_CALLS, "fused_forward_ms": g[0], "fused_backward_ms": g[1],
                                "eager_forward_ms": g[2],
                                "fused_forward_hbm_fraction": fwd_bytes / (g[0] * 1e-3) / HBM_PEAK,
                                "fused_backward_hbm_fraction": bwd_bytes / (g[1] * 1e-3) / HBM_PEAK,
                                "eager_forward_hbm_fraction": fwd_bytes / (g[2] * 1e-3) / HBM_PEAK},
               "memory": {"fused": forward_memory(lambda: ops.local_cross_attn(q, k, v, WINDOW)),
                          "eager": forward_memory(lambda: cpu.local_cross_attn_eager(q, k, v, WINDOW))},
               "max_normalised_difference_fused_vs_eager": diff}
        legs.append(out)
    print("HSUP_PROBE " + json.dumps(legs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hsup_r11.json"))
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
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("HSUP_PROBE ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"hsup_probe: failed (exit {r.returncode})")
        return 1
    legs = json.loads(line[len("HSUP_PROBE "):])
    for lg in legs:
        print(f"hsup_probe: {lg['shape']}: forward {lg['fused']['forward_ms']:.4f} ms vs eager "
              f"{lg['eager']['forward_ms']:.4f} ms, forward + backward {lg['fused']['forward_backward_ms']:.4f} ms vs "
              f"eager {lg['eager']['forward_backward_ms']:.4f} ms; held for backward "
              f"{lg['memory']['fused']['held_for_backward_bytes'] / 1e6:.1f} MB vs "
              f"{lg['memory']['eager']['held_for_backward_bytes'] / 1e6:.1f} MB")
    import torch
    doc = {"tool": "tools/hsup_probe.py", "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK, "legs": legs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"hsup_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
