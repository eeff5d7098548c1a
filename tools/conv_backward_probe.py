#!/usr/bin/env python3
"""Training through the fused k x k convolutions (rmd.ops.conv2d_act(differentiable=True), csrc/conv.hip +
csrc/conv_backward.hip) against the MIOpen paths they replace (fused="off": the parent's behaviour), forward +
backward, timed in one process between device events:

  shapes    the cfg5 training maps (b6: 48x64, 24x32, 12x16) and cfg2 (b8, 55x128), corr_planes 324 throughout
  convs     each of the nine convolutions of BasicMotionEncoder, FlowHead and Up8Network's mask head, forward +
            backward to the input, weight and bias: the differentiable operator against the eager Conv2d (+ ReLU).
            Then the backward operator by its parts, each a call of torch.ops.rmd.conv2d_act_backward that launches
            only those kernels: data (repack + conv_kernel), weight (conv_wgrad_kernel + reduce; its fraction of the
            dense bf16 MFMA peak by algorithmic FLOPs, three products per useful one), mask_bias (the ReLU mask +
            bias-gradient pass) and its share of the whole backward call
  modules   BasicMotionEncoder, FlowHead, Up8Network, forward + backward, fused="on", fused_backward=True against
            fused="off"; the memory kept for backward and the backward's peak on both paths
  step      one BasicUpdateBlock training step (forward + backward, the recurrent unit eager on both sides) at the
            cfg5 1/8 shape

Fused and eager alternate inside one loop (the machine is shared), eager first; median over `steps` after `warmup`.
Algorithmic FLOPs of a gradient: 2 x kh x kw x Cin x Cout per pixel; the fraction is of the 2.5 PFLOP/s dense bf16
MFMA peak.  The work runs in a child process under its own time limit.

The share of the backward kernels' time that the weight repack takes comes from a kernel trace:
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/conv_backward_probe.py --trace-leg
  python3 tools/conv_backward_probe.py --kernel-stats DIR/.../*_kernel_stats.csv      (adds "kernel_trace" to --out;
                                                     a rocpd *_results.db, rocprofv3's other output format, works too)

usage: python3 tools/conv_backward_probe.py [--warmup 10] [--steps 20] [--out profiles/conv_backward_r20.json]
"""
import argparse
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "raft-meets-dicl_amd"), ROOT):
    sys.path.insert(0, p)

MFMA_PEAK = 2.5e15
LEG_TIMEOUT = 840
PLANES = 324
SHAPES = [("cfg5 1/8", 6, 48, 64), ("cfg5 1/16", 6, 24, 32), ("cfg5 1/32", 6, 12, 16), ("cfg2 1/8", 8, 55, 128)]
# (module path, C0, C1, Cout, k, activation)
CONVS = [("enc.convc1", PLANES, 0, 256, 1, "relu"), ("enc.convc2", 256, 0, 192, 3, "relu"),
         ("enc.convf1", 2, 0, 128, 7, "relu"), ("enc.convf2", 128, 0, 64, 3, "relu"), ("enc.conv", 192, 64, 126, 3, "relu"),
         ("flow.conv1", 128, 0, 256, 3, "relu"), ("flow.conv2", 256, 0, 2, 3, "none"), ("up8.conv1", 128, 0, 256, 3, "relu"),
         ("up8.conv2", 256, 0, 576, 1, "none")]
TRACE_CALLS = 20
KERNELS = ("conv_mask_bias_kernel", "conv_pack_transposed_kernel", "conv_kernel", "conv_wgrad_kernel",
           "conv_wgrad_reduce_kernel", "conv_pack_kernel")


def _modules(dev, **kw):
    import rmd.raft
    from detinit import det_init_fanin
    blk = det_init_fanin(rmd.raft.BasicUpdateBlock(PLANES, **kw)).train().to(dev)
    up = det_init_fanin(rmd.raft.Up8Network(128, **kw)).train().to(dev)
    return {"enc": blk.enc, "flow": blk.flow, "up8": up, "block": blk}


def trace_leg():
    """TRACE_CALLS training steps of the fused BasicUpdateBlock and Up8Network at cfg5 1/8, for a kernel trace."""
    import torch
    dev = torch.device("cuda", 0)
    mods = _modules(dev, fused="on", fused_backward=True)
    _, b, h, w = SHAPES[0]
    gen = torch.Generator().manual_seed(20)
    hid, ctx, corr, flow = (torch.randn(b, c, h, w, generator=gen).to(dev) for c in (128, 128, PLANES, 2))
    for _ in range(TRACE_CALLS):
        hh, d = mods["block"](hid, ctx, corr, flow)
        out = mods["up8"](hh, d)
        (hh.sum() + d.sum() + out.sum()).backward()
    torch.cuda.synchronize()


def kernel_stats(path):
    """Time per kernel of the fused training step, and the repack's share, from a rocprofv3 kernel_stats.csv or
    rocpd results.db."""
    if path.endswith(".db"):                            # rocprofv3's rocpd output: the `kernels` view
        import sqlite3
        with sqlite3.connect(path) as db:
            rows = db.execute("select name, sum(end - start) from kernels group by name").fetchall()
    else:
        with open(path) as f:
            rows = [(r["Name"], int(r["TotalDurationNs"])) for r in csv.DictReader(f)]
    per = {}
    for name, ns in rows:
        for key in KERNELS:
            if key + "<" in name or key + "(" in name:
                per[key] = per.get(key, 0) + int(ns)
    backward = sum(per.get(k, 0) for k in KERNELS if k != "conv_pack_kernel")
    return {"shape": f"{SHAPES[0][0]}: BasicUpdateBlock + Up8Network, fused='on', fused_backward=True, {TRACE_CALLS} training "
                     "steps; conv_kernel holds the forward and the data gradient",
            "kernel_ns": per,
            "transposed_repack_over_conv_kernels": per.get("conv_pack_transposed_kernel", 0) / backward if backward else None,
            "mask_bias_over_conv_kernels": per.get("conv_mask_bias_kernel", 0) / backward if backward else None}


def leg(warmup, steps):
    import statistics

    import torch
    import torch.nn.functional as F
    from rmd import ops
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(20)

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

    def timed(sides):
        order = ["eager"] + [s for s in sides if s != "eager"]
        t = dict(zip(order, interleaved_ms([sides[s] for s in order])))
        return {"forward_backward_ms": t, "eager_over_fused": {s: t["eager"] / t[s] for s in order[1:]}}

    def memory(fn_forward, grads):
        """bytes kept between forward and backward, and the backward's peak above what the forward left"""
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        outs = fn_forward()
        torch.cuda.synchronize()
        kept = torch.cuda.memory_allocated() - before - sum(o.numel() * 4 for o in outs)
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
        return {"kept_for_backward_bytes": kept, "backward_peak_bytes": torch.cuda.max_memory_allocated() - held}

    off, fused = _modules(dev), _modules(dev, fused="on", fused_backward=True)
    legs = []
    for name, b, h, w in SHAPES:
        def rand(c, grad=False):
            return torch.randn(b, c, h, w, generator=gen).to(dev).requires_grad_(grad)
        row = {"shape": f"{name}: ({b}, ., {h}, {w})", "warmup": warmup, "steps": steps, "convs": {}, "modules": {}}
        for path, c0, c1, cout, k, act in CONVS:
            owner, attr = path.split(".")
            conv = getattr(off[owner], attr)
            x0, x1 = rand(c0, True), (rand(c1, True) if c1 else None)
            g = rand(cout)
            code = ops.CONV_ACTS[act]

            def eager(conv=conv, x0=x0, x1=x1, g=g, act=act):
                x = x0 if x1 is None else torch.cat([x0, x1], dim=1)
                y = conv(x)
                (F.relu(y) if act == "relu" else y).backward(g)

            def train(conv=conv, x0=x0, x1=x1, g=g, act=act):
                ops.conv2d_act(x0, x1, conv.weight, conv.bias, act, "fp32", differentiable=True).backward(g)

            r = timed({"eager": eager, "fused": train})
            with torch.no_grad():
                y = ops.conv2d_act(x0, x1, conv.weight, conv.bias, act)
                yy = y if code else None
                wt = conv.weight.detach()
                calls = {"all": lambda: torch.ops.rmd.conv2d_act_backward(g, yy, x0, x1, wt, code, [True] * 4),
                         "data": lambda: torch.ops.rmd.conv2d_act_backward(g, None, x0, x1, wt, 0, [True, True, False, False]),
                         "weight": lambda: torch.ops.rmd.conv2d_act_backward(g, None, x0, x1, wt, 0, [False, False, True, False]),
                         "mask_bias": lambda: torch.ops.rmd.conv2d_act_backward(g, yy, x0, x1, wt, code, [False, False, False, True])}
                parts = dict(zip(calls, interleaved_ms(list(calls.values()))))
            flops = 2.0 * k * k * (c0 + c1) * cout * b * h * w
            r["backward_operator_ms"] = parts
            r["mask_bias_share_of_backward"] = parts["mask_bias"] / parts["all"]
            r["algorithmic_flops_per_gradient"] = flops
            r["weight_gradient_mfma_peak_fraction"] = flops / (parts["weight"] * 1e-3) / MFMA_PEAK
            r["data_gradient_mfma_peak_fraction"] = flops / (parts["data"] * 1e-3) / MFMA_PEAK
            row["convs"][f"{path} {k}x{k} {c0}+{c1}->{cout} {act}"] = r
        inputs = {"enc": [rand(2, True), rand(PLANES, True)], "flow": [rand(128, True)], "up8": [rand(128, True), rand(2, True)],
                  "block": [rand(128, True), rand(128, True), rand(PLANES, True), rand(2, True)]}
        for key in ("enc", "flow", "up8") + (("block",) if name == SHAPES[0][0] else ()):
            def forward(m, key=key):
                out = m(*inputs[key])
                return list(out) if isinstance(out, tuple) else [out]
            with torch.no_grad():
                grads = [torch.randn(o.shape, generator=gen).to(dev) for o in forward(off[key])]

            def step(m, key=key, grads=grads, forward=forward):
                torch.autograd.backward(forward(m), grads)

            r = timed({"eager": lambda: step(off[key]), "fused": lambda: step(fused[key])})
            r["memory"] = {"eager": memory(lambda: forward(off[key]), grads), "fused": memory(lambda: forward(fused[key]), grads)}
            row["modules"][key] = r
        legs.append(row)
    print("CONV_BACKWARD_PROBE " + json.dumps({"legs": legs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_backward_r20.json"))
    ap.add_argument("--leg", action="store_true", help="internal: run the measurement in this process")
    ap.add_argument("--trace-leg", action="store_true", help="fused training steps at cfg5 1/8, for a kernel trace")
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats.csv (or rocpd results.db) of --trace-leg: add the kernels' times to --out")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (a median over fewer steps is not reported)")
    if a.trace_leg:
        trace_leg()
        return 0
    if a.leg:
        leg(a.warmup, a.steps)
        return 0
    if a.kernel_stats:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_trace"] = kernel_stats(a.kernel_stats)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(f"conv_backward_probe: kernel trace {doc['kernel_trace']} -> {a.out}")
        return 0
    # a fresh child under its own time limit
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--warmup", str(a.warmup), "--steps",
                        str(a.steps)], capture_output=True, text=True, timeout=LEG_TIMEOUT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("CONV_BACKWARD_PROBE ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"conv_backward_probe: failed (exit {r.returncode})")
        return 1
    res = json.loads(line[len("CONV_BACKWARD_PROBE "):])
    for lg in res["legs"]:
        for name, c in lg["convs"].items():
            t, p = c["forward_backward_ms"], c["backward_operator_ms"]
            print(f"conv_backward_probe: {lg['shape']} {name}: eager {t['eager']:.3f} ms, fused {t['fused']:.3f} ms "
                  f"(x{c['eager_over_fused']['fused']:.2f}); backward {p['all']:.3f} = data {p['data']:.3f} + weight "
                  f"{p['weight']:.3f} ({100 * c['weight_gradient_mfma_peak_fraction']:.2f} % of peak) + mask/bias "
                  f"{p['mask_bias']:.3f}")
        for key, m in lg["modules"].items():
            print(f"conv_backward_probe: {lg['shape']} {key}: {m['forward_backward_ms']}  eager / fused "
                  f"{m['eager_over_fused']['fused']:.2f}  memory {m['memory']}")
    import torch
    doc = {"tool": "tools/conv_backward_probe.py", "torch": torch.__version__, "mfma_peak_flops_per_s": MFMA_PEAK, **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"conv_backward_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
