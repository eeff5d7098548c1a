#!/usr/bin/env python3
"""The differentiable fused dicl-1x1 cost (rmd.ops.dicl_match_1x1(differentiable=True), csrc/dicl_match_grad.hip)
against the training path it replaces, timed in one process on one GPU.

Both sides are the same dicl_1x1.CorrelationModule (C = 32, r = 4, eval-mode batch norm, dap on):
  fused   fused="on", fused_backward=True: rmd_dicl_match_1x1 forward, rmd_dicl_match_1x1_backward
  off     fused="off": rmd_dicl_stack + the MIOpen MatchingNet1x1 under autograd (the stack and every hidden
          activation kept for the backward)

Per shape — the three ctf-l3 levels of the cfg5 training shape (b6: 48x64, 24x32, 12x16) and the cfg4 1/8
level at b8 (48x160) if the off side fits in memory:
  step_ms        forward + backward between device events, the two sides alternating in one loop, median
  backward_ms    the fused backward operator alone (pack + MFMA kernel + reduction, grad_fmap2's memset),
                 replayed from a graph of 5 calls; per-kernel times are not split out
  peak_mb        peak memory above the inputs of a forward kept for backward, and of the backward
  grad_err       max-normalised difference of the fused gradients from the off side's (fp32 autograd) on
                 fmap1, fmap2 and every parameter

usage: python3 tools/dicl_match_grad_probe.py [--warmup 5] [--steps 20] [--out profiles/dicl_match_grad_r13.json]
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-meets-dicl_amd"))

SHAPES = (
    ("cfg5 ctf-l3 1/8 (b6)", (6, 32, 48, 64)),
    ("cfg5 ctf-l3 1/16 (b6)", (6, 32, 24, 32)),
    ("cfg5 ctf-l3 1/32 (b6)", (6, 32, 12, 16)),
    ("cfg4 ctf-l3 1/8 (b8)", (8, 32, 48, 160)),
)
RADIUS = 4


def build(torch, rmd, c, **kw):
    torch.manual_seed(7)
    mod = rmd.corr.make_cmod("dicl-1x1", c, RADIUS, dap_init="standard", **kw).cuda()
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 2.0)
                m.running_mean.normal_(0.0, 0.3)
                m.weight.uniform_(0.7, 1.3)
                m.bias.normal_(0.0, 0.2)
    return mod.eval()


def inputs(torch, shape):
    b, c, h, w = shape
    gen = torch.Generator(device="cuda").manual_seed(11)
    f1 = torch.randn(b, c, h, w, device="cuda", generator=gen).requires_grad_(True)
    f2 = torch.randn(b, c, h, w, device="cuda", generator=gen).requires_grad_(True)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    co = (torch.stack([xs, ys]).float()[None] + 2.0 * torch.randn(b, 2, h, w, device="cuda", generator=gen)).contiguous()
    go = torch.randn(b, (2 * RADIUS + 1) ** 2, h, w, device="cuda", generator=gen)
    return f1, f2, co, go


def step(mod, f1, f2, co, go):
    for t in (f1, f2, *mod.parameters()):
        t.grad = None
    mod(f1, f2, co).backward(go)


def grads(mod, f1, f2):
    out = {"fmap1": f1.grad, "fmap2": f2.grad}
    out.update({k: p.grad for k, p in mod.named_parameters()})
    return {k: v.detach().clone() for k, v in out.items()}


def measure(torch, rmd, label, shape, warmup, steps):
    res = {"shape": f"{label}: fmaps {shape}, r = {RADIUS}"}
    f1, f2, co, go = inputs(torch, shape)
    sides = {"fused": build(torch, rmd, shape[1], fused="on", fused_backward=True), "off": build(torch, rmd, shape[1])}
    sides["off"].load_state_dict(sides["fused"].state_dict())
    try:
        step(sides["off"], f1, f2, co, go)
        torch.cuda.synchronize()
    except torch.OutOfMemoryError as e:
        res["off"] = f"does not fit in memory: {str(e)[:120]}"
        sides.pop("off")
        torch.cuda.empty_cache()
    got = {}
    for name, mod in sides.items():
        step(mod, f1, f2, co, go)
        got[name] = grads(mod, f1, f2)
    if "off" in sides:
        res["grad_err_fused_vs_off"] = {
            k: float((got["fused"][k] - v).abs().max() / v.abs().max()) for k, v in got["off"].items()}
    del got
    res["peak_mb"] = {}
    for name, mod in sides.items():
        for t in (f1, f2, *mod.parameters()):
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = mod(f1, f2, co)
        torch.cuda.synchronize()
        fwd_peak, kept = torch.cuda.max_memory_allocated() - before, torch.cuda.memory_allocated() - before
        torch.cuda.reset_peak_memory_stats()
        out.backward(go)
        torch.cuda.synchronize()
        res["peak_mb"][name] = {"forward_peak": fwd_peak / 1e6, "kept_for_backward": kept / 1e6,
                                "backward_peak": (torch.cuda.max_memory_allocated() - before) / 1e6}
        del out
    times = {name: [] for name in sides}
    for i in range(warmup + steps):
        for name, mod in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(mod, f1, f2, co, go)
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    res["step_ms"] = {name: statistics.median(v) for name, v in times.items()}
    if "off" in sides:
        res["step_speedup_fused_over_off"] = res["step_ms"]["off"] / res["step_ms"]["fused"]
    # the fused backward operator alone, from a graph of 5 calls
    from rmd import ops
    with torch.no_grad():
        ws, ts = ops._pad_match(*sides["fused"].mnet.folded())
        gc = torch.randn(shape[0], 2 * RADIUS + 1, 2 * RADIUS + 1, *shape[2:], device="cuda")
        args = (gc, f1.detach(), f2.detach(), co, RADIUS, ws, ts, [True, True, True])
        fwd_args = args[1:-1]
        for what, fn in (("backward_ms", lambda: torch.ops.rmd.dicl_match_1x1_backward(*args)),
                         ("forward_ms", lambda: torch.ops.rmd.dicl_match_1x1_train(*fwd_args))):
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(5):
                    fn()
            reps = []
            for i in range(3 + 10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                graph.replay()
                b.record()
                b.synchronize()
                if i >= 3:
                    reps.append(a.elapsed_time(b) / 5)
            res[what] = statistics.median(reps)
            del graph
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dicl_match_grad_r13.json"))
    a = ap.parse_args()
    import torch
    import rmd
    doc = {"tool": "tools/dicl_match_grad_probe.py", "torch": torch.__version__, "device": torch.cuda.get_device_name(0),
           "warmup": a.warmup, "steps": a.steps, "levels": []}
    for label, shape in SHAPES:
        r = measure(torch, rmd, label, shape, a.warmup, a.steps)
        doc["levels"].append(r)
        print(f"dicl_match_grad_probe: {r['shape']}: step {r['step_ms']}, fused backward {r['backward_ms']:.3f} ms, "
              f"fused forward {r['forward_ms']:.3f} ms, peak {r['peak_mb']}", flush=True)
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"dicl_match_grad_probe: wrote {a.out}")


if __name__ == "__main__":
    main()
