#!/usr/bin/env python3
"""The fused SepConvGRU (rmd.ops.sepconv_gru, csrc/gru.hip) against the path it replaces, timed in one process
between device events:

  shapes    cfg2 (b8, 55x128) and the three cfg4 ctf levels (b8, 48x160, 24x80, 12x40), hidden 128, input 256
  fused     rmd.raft.SepConvGru(fused="on") with precision "fp32" (three split-bf16 products) and "bf16" (one):
            the weight repack and the four kernels
  eager     the same module with fused="off": six MIOpen fp32 convolutions, two cats, the pointwise passes — the
            parent commit's only path
  graph     each side, GRAPH_CALLS calls captured in one graph and replayed
  memory    peak bytes of one forward above its start, every side
  error     at cfg2, max |side - float64| / max |float64| on SAMPLES random outputs, the float64 values from the
            module's composition in float64 on the CPU
  model     tests/e2e RaftNet (rmd correlation and Up8) at 436x1024 (padded 440x1024) b8, 12 iterations, with the
            eager unit and with the fused one in both modes: frame pairs/s; and the e2e fixture at b1:
            max |EPE - EPE_ref| over the iterations and the sampled flow difference, every side

The sides alternate inside one loop (the machine is shared); median over `steps` after `warmup`.  Algorithmic
FLOPs: 2 x 6 x 5 x (Hd + Xd) x Hd per pixel; the fraction is of the 2.5 PFLOP/s dense bf16 MFMA peak (the
three-product mode issues three times the MFMAs for the same algorithmic FLOPs).  The work runs in a child process
under its own time limit.

usage: python3 tools/gru_probe.py [--warmup 10] [--steps 20] [--out profiles/gru_r14.json]
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
LEG_TIMEOUT = 840
GRAPH_CALLS = 10
SAMPLES = 60000
BATCH, HIDDEN, INPUT = 8, 128, 256
SHAPES = [("cfg2 1/8", 55, 128), ("ctf-l3 1/8", 48, 160), ("ctf-l3 1/16", 24, 80), ("ctf-l3 1/32", 12, 40)]
SIDES = {"fused_fp32": ("on", "fp32"), "fused_bf16": ("on", "bf16"), "eager": ("off", "fp32")}


def leg(warmup, steps):
    import copy
    import statistics
    import time

    import numpy as np
    import torch
    import rmd.raft
    from conftest import load_golden
    from detinit import det_init_fanin
    from e2e.raft_net import RaftNet
    from synth import epe, frame_pair
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(14)

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

    def unit(fused, precision):
        return det_init_fanin(rmd.raft.SepConvGru(HIDDEN, INPUT, fused=fused, precision=precision)).eval().to(dev)

    sides = {side: unit(*how) for side, how in SIDES.items()}
    exact = copy.deepcopy(sides["eager"]).cpu().double()
    macs = 6 * 5 * (HIDDEN + INPUT) * HIDDEN
    legs = []
    for name, h, w in SHAPES:
        hid = np.tanh(rng.standard_normal((BATCH, HIDDEN, h, w))).astype(np.float32)
        inp = np.maximum(rng.standard_normal((BATCH, INPUT, h, w)), 0).astype(np.float32)
        th, tx = torch.from_numpy(hid).to(dev), torch.from_numpy(inp).to(dev)
        fns = {}
        for side, m in sides.items():
            def fn(m=m):
                with torch.no_grad():
                    return m(th, tx)
            fns[side] = fn
        error = None
        if name.startswith("cfg2"):
            with torch.no_grad():
                ref = exact(torch.from_numpy(hid).double(), torch.from_numpy(inp).double()).numpy().reshape(-1)
            idx = rng.integers(0, ref.size, SAMPLES)
            error = {"samples": SAMPLES}
            for side, fn in fns.items():
                got = fn().cpu().numpy().reshape(-1)[idx].astype(np.float64)
                error[side] = float(np.abs(got - ref[idx]).max() / np.abs(ref[idx]).max())
        order = list(fns)
        t = dict(zip(order, interleaved_ms([fns[s] for s in order])))
        graph_ms = {}
        for side in order:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep = [fns[side]() for _ in range(GRAPH_CALLS)]
            graph_ms[side] = interleaved_ms([graph.replay])[0] / GRAPH_CALLS
            del keep, graph
        flops = 2.0 * macs * BATCH * h * w
        row = {"shape": f"{name}: h ({BATCH}, {HIDDEN}, {h}, {w}), x ({BATCH}, {INPUT}, {h}, {w})",
               "algorithmic_flops": flops, "warmup": warmup, "steps": steps, "forward_ms": t,
               "eager_over_fused": {s: t["eager"] / t[s] for s in ("fused_fp32", "fused_bf16")},
               "graph_replay": {"calls_per_graph": GRAPH_CALLS, "forward_ms": graph_ms,
                                "eager_over_fused": {s: graph_ms["eager"] / graph_ms[s] for s in ("fused_fp32", "fused_bf16")},
                                "mfma_peak_fraction": {s: flops / (graph_ms[s] * 1e-3) / MFMA_PEAK
                                                       for s in ("fused_fp32", "fused_bf16")}},
               "forward_peak_bytes": {s: peak_bytes(fn) for s, fn in fns.items()}}
        if error:
            row["max_normalised_error_vs_float64"] = error
        legs.append(row)
        del th, tx

    # the whole network
    g = load_golden("e2e_raft_436x1024")
    fh, fw, iters = int(g["height"]), int(g["width"]), int(g["iterations"])
    img1, img2, gt = frame_pair(fh, fw)
    one = (torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev))
    low = torch.rand(BATCH, 3, 55, 128, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    b1 = torch.nn.functional.interpolate(low, size=(440, 1024), mode="bilinear", align_corners=True).to(dev)
    b2 = torch.roll(b1, shifts=(3, 5), dims=(2, 3))
    model = {}
    for side, (fused, precision) in SIDES.items():
        net = RaftNet(rmd.raft.CorrBlock, precision="fp32", upnet_cls=rmd.raft.Up8Network)
        net.update_block.gru = rmd.raft.SepConvGru(HIDDEN, INPUT, fused=fused, precision=precision)
        net = det_init_fanin(net).eval().to(dev)
        with torch.no_grad():
            flows = [f.cpu().numpy() for f in net(*one, iters)]
            d_epe = max(abs(epe(f, gt) - float(r)) for f, r in zip(flows, g["epe"]))
            d_flow = max(float(np.abs(flows[k - 1][0, :, :fh, :fw].reshape(2, -1)[:, g["pixels"]] - g[f"flow_it{k}"]).max())
                         for k in (1, 4, 12))
            for _ in range(2):
                net(b1, b2, iters)
            torch.cuda.synchronize()
            reps = 3
            t0 = time.perf_counter()
            for _ in range(reps):
                net(b1, b2, iters)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
        model[side] = {"frame_pairs_per_s": BATCH * reps / el, "ms_per_batch": el / reps * 1e3,
                       "e2e_max_abs_epe_diff_px": d_epe, "e2e_max_flow_diff_px": d_flow}
        del net
        torch.cuda.empty_cache()
    print("GRU_PROBE " + json.dumps({"legs": legs, "model_436x1024_b8_12_iterations": model}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_r14.json"))
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
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("GRU_PROBE ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"gru_probe: failed (exit {r.returncode})")
        return 1
    res = json.loads(line[len("GRU_PROBE "):])
    for lg in res["legs"]:
        t, gr = lg["forward_ms"], lg["graph_replay"]
        print(f"gru_probe: {lg['shape']}: fused fp32 {t['fused_fp32']:.3f} ms, bf16 {t['fused_bf16']:.3f} ms, eager "
              f"{t['eager']:.3f} ms; graph replay fp32 {gr['forward_ms']['fused_fp32']:.3f} ms "
              f"({100 * gr['mfma_peak_fraction']['fused_fp32']:.1f} % of the bf16 MFMA peak), bf16 "
              f"{gr['forward_ms']['fused_bf16']:.3f} ms ({100 * gr['mfma_peak_fraction']['fused_bf16']:.1f} %), eager "
              f"{gr['forward_ms']['eager']:.3f} ms; peak {lg['forward_peak_bytes']['fused_fp32'] / 1e6:.1f} MB vs "
              f"{lg['forward_peak_bytes']['eager'] / 1e6:.1f} MB; error vs float64 "
              f"{lg.get('max_normalised_error_vs_float64')}")
    for side, m in res["model_436x1024_b8_12_iterations"].items():
        print(f"gru_probe: model {side}: {m['frame_pairs_per_s']:.1f} pairs/s, e2e dEPE {m['e2e_max_abs_epe_diff_px']:.2e} px, "
              f"flow {m['e2e_max_flow_diff_px']:.2e} px")
    import torch
    doc = {"tool": "tools/gru_probe.py", "torch": torch.__version__, "mfma_peak_flops_per_s": MFMA_PEAK, **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"gru_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
