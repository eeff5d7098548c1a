#!/usr/bin/env python3
"""Forward + backward of the fused sequence loss (rmd.loss, csrc/loss.hip) against the eager composite
it replaces, timed with HIP events in one process per shape:

  shape 1  raft/sequence: 12 full-resolution predictions at 436x1024, batch 8; the composite is the
           formula of raft.py:616-644 (ord 1, gamma 0.8)
  shape 2  raft+dicl/mlseq on the cfg5 result structure at 384x512, batch 6, iterations (4, 3, 3):
           [4 @ 12x16], [3 @ 24x32], [3 @ 384x512]; the composite is tests/e2e/ctf_l3_net.mlseq_loss

Per path: median over `steps` steps after `warmup` (forward alone, and forward + backward), the
algorithmic bytes (forward: K flows + target + valid; backward: that plus K gradient writes), the
fraction of the 8 TB/s HBM peak they imply, and the peak of torch.cuda.max_memory_allocated over one
step above the inputs.  Each shape runs in a child process of its own under its own time limit, both
paths in that one process; a failing child ends the run.

usage: python3 tools/loss_probe.py [--warmup 5] [--steps 25] [--out profiles/loss_r07.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raft-meets-dicl_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

HBM_PEAK = 8e12
LEG_TIMEOUT = 240


def sequence_eager(result, target, valid, ord=1, gamma=0.8):
    """SequenceLoss.compute (raft.py:616-644), masked mode."""
    import torch
    n = len(result)
    loss = 0.0
    for i, flow in enumerate(result):
        dist = torch.linalg.vector_norm(flow - target, ord=ord, dim=-3)
        loss = loss + gamma ** (n - i - 1) * dist[valid].mean()
    return loss


def leg(shape, warmup, steps):
    import statistics

    import torch
    import rmd
    from e2e.ctf_l3_net import mlseq_loss
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)

    def rand(*s):
        return torch.randn(*s, generator=g).to(dev)

    if shape == 1:
        b, h, w = 8, 436, 1024
        target = 3.0 * rand(b, 2, h, w)
        result = [(target + rand(b, 2, h, w)).requires_grad_(True) for _ in range(12)]
        flows = result
        fused_obj = rmd.loss.SequenceLoss({"ord": 1, "gamma": 0.8})
        fused = lambda: fused_obj(None, result, target, valid)                              # noqa: E731
        eager = lambda: sequence_eager(result, target, valid)                               # noqa: E731
        name = "raft/sequence 12 x (8, 2, 436, 1024)"
    else:
        b, h, w = 6, 384, 512
        target = 3.0 * rand(b, 2, h, w)
        sizes = [(4, h // 32, w // 32), (3, h // 16, w // 16), (3, h, w)]
        result = [[rand(b, 2, lh, lw).requires_grad_(True) for _ in range(n)] for n, lh, lw in sizes]
        flows = [f for level in result for f in level]
        args = {"ord": 1, "gamma": 0.85, "alpha": (0.38, 0.6, 1.0), "scale": 1.0}
        fused_obj = rmd.loss.MultiLevelSequenceLoss(args)
        fused = lambda: fused_obj(None, result, target, valid)                              # noqa: E731
        eager = lambda: mlseq_loss(result, target, valid, **args)                           # noqa: E731
        name = "raft+dicl/mlseq cfg5 [4 @ 12x16], [3 @ 24x32], [3 @ 384x512], batch 6"
    valid = (torch.rand(b, h, w, generator=g) < 0.8).to(dev)

    flow_bytes = sum(f.numel() * 4 for f in flows)
    fwd_bytes = flow_bytes + target.numel() * 4 + valid.numel()
    bwd_bytes = fwd_bytes + flow_bytes

    def timed(fn, backward):
        def step():
            for f in flows:
                f.grad = None
            loss = fn()
            if backward:
                loss.backward()
            return loss
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        ev = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for a, b in ev)

    def peak(fn):
        for f in flows:
            f.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    out = {"shape": name, "warmup": warmup, "steps": steps, "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes}
    losses = {}
    for path, fn in (("fused", fused), ("eager", eager)):
        losses[path] = float(fn().detach())
        fwd_ms = timed(fn, False)
        both_ms = timed(fn, True)
        out[path] = {"loss": losses[path], "forward_ms": fwd_ms, "forward_backward_ms": both_ms,
                     "forward_hbm_fraction": fwd_bytes / (fwd_ms * 1e-3) / HBM_PEAK,
                     "forward_backward_hbm_fraction": (fwd_bytes + bwd_bytes) / (both_ms * 1e-3) / HBM_PEAK,
                     "peak_memory_bytes_above_inputs": peak(fn)}
    out["loss_rel_diff"] = abs(losses["fused"] - losses["eager"]) / abs(losses["eager"])
    out["eager_over_fused_forward_backward"] = out["eager"]["forward_backward_ms"] / out["fused"]["forward_backward_ms"]
    out["eager_over_fused_forward"] = out["eager"]["forward_ms"] / out["fused"]["forward_ms"]
    print("LOSS_PROBE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_r07.json"))
    ap.add_argument("--leg", type=int, default=0, help="internal: run one shape in this process")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (a median over fewer steps is not reported)")
    if a.leg:
        leg(a.leg, a.warmup, a.steps)
        return 0
    legs = []
    for shape in (1, 2):
        # a fresh child per shape under its own time limit; nothing more is started after a failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", str(shape), "--warmup", str(a.warmup),
                            "--steps", str(a.steps)], capture_output=True, text=True, timeout=LEG_TIMEOUT)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LOSS_PROBE ")), None)
        if r.returncode != 0 or line is None:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"loss_probe: shape {shape} failed (exit {r.returncode}); stopping")
            return 1
        legs.append(json.loads(line[len("LOSS_PROBE "):]))
        print(f"loss_probe: {legs[-1]['shape']}: fused {legs[-1]['fused']['forward_backward_ms']:.3f} ms, eager "
              f"{legs[-1]['eager']['forward_backward_ms']:.3f} ms (forward + backward)")
    import torch
    doc = {"tool": "tools/loss_probe.py", "torch": torch.__version__, "hbm_peak_bytes_per_s": HBM_PEAK, "legs": legs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"loss_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
