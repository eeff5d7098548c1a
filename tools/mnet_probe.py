#!/usr/bin/env python3
"""The fused k x k MatchingNet (rmd.ops.matching_net / mnet_tail, csrc/mnet.hip) against the MIOpen nn.Sequential it
replaces (MatchingNet(fused="off"): the parent commit's behaviour), timed in one process between device events:

  levels    the module forward on a ready displacement stack at the three ctf-l3 levels of cfg4 on b8 (648 images of
            64 channels at 48x160, 24x80, 12x40) and the five DICL levels of cfg3 on b8 (392 images of 64 channels at
            6x8 .. 96x128): off / fused fp32 / fused bf16, eval-mode batch norm (folded on the device inside the
            timed call), the peak memory allocated during a call on each path and the difference from `off`
  layers    at the cfg4 1/8 level: each of layers 1-4 (conv2d_norm_act with its ReLU, repack included) against its
            ConvBlock, and the tail (mnet_tail) against ConvBlockTransposed + Conv2d, on all 648 images
  budgets   the whole network at the cfg4 1/8 level with workspace budgets of 64, 128, 256 and 512 MiB (the group
            each gives), both modes: the source of rmd.ops.MNET_WORKSPACE_BYTES
  graph     the fused operator at the cfg4 1/8 level replayed from a captured graph: time per replay and the share
            of the 2.5 PFLOP/s dense bf16 MFMA peak by algorithmic FLOPs (2 x taps x Cin x Cout per output pixel;
            the three-product mode issues three times the MFMAs for the same algorithmic FLOPs)
  model     tests/e2e CtfL3Net at 384x1280 b1, iterations (4, 3, 3): off / fused fp32 / fused bf16

The sides alternate inside one loop (the machine is shared), `off` first; median over `steps` after `warmup`.  The
compiler's figures for the tail kernel (csrc `make resource-usage`) are passed through --resources.  The work runs in
a child process under its own time limit.

usage: python3 tools/mnet_probe.py [--warmup 3] [--steps 20] [--out profiles/mnet_r18.json]
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
LEG_TIMEOUT = 900
TAG = "MNET_PROBE "
CFG4 = [("cfg4 1/8", 81, 48, 160), ("cfg4 1/16", 81, 24, 80), ("cfg4 1/32", 81, 12, 40)]
CFG3 = [(f"cfg3 level {l}", 49, 384 >> l, 512 >> l) for l in (2, 3, 4, 5, 6)]
BUDGETS_MIB = (64, 128, 256, 512)
WIDTHS = (64, 96, 128, 64, 32)


def net_flops(images, h, w):
    c_in, c1, c2, c3, c4 = WIDTHS
    full, half = h * w, (h // 2) * (w // 2)
    macs = full * 9 * c_in * c1 + half * 9 * (c1 * c2 + c2 * c2 + c2 * c3) + full * 4 * c3 * c4 + full * 9 * c4
    return 2.0 * images * macs


def leg(warmup, steps):
    import statistics

    import torch
    import rmd
    from detinit import det_init_fanin
    from e2e.ctf_l3_net import CtfL3Net
    from rmd import ops
    from rmd.blocks.dicl import MatchingNet
    from synth import frame_pair
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(18)

    def interleaved_ms(fns):
        ev = [[] for _ in fns]
        with torch.no_grad():
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
        order = ["off"] + [s for s in sides if s != "off"]
        t = dict(zip(order, interleaved_ms([sides[s] for s in order])))
        return {"forward_ms": t, "off_over_fused": {s: t["off"] / t[s] for s in order[1:]}}

    def peak_bytes(fn):
        with torch.no_grad():
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - before

    def seeded(mod):
        """eval-mode batch norm with non-trivial state."""
        with torch.no_grad():
            for m in mod.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_var.uniform_(0.5, 2.0)
                    m.running_mean.normal_(0.0, 0.3)
                    m.weight.uniform_(0.7, 1.3)
                    m.bias.normal_(0.0, 0.2)
        return mod.eval()

    torch.manual_seed(18)
    off = seeded(MatchingNet(WIDTHS[0])).to(dev)
    mods = {"off": off}
    for side, precision in (("fused_fp32", "fp32"), ("fused_bf16", "bf16")):
        mods[side] = MatchingNet(WIDTHS[0], fused="on", precision=precision).to(dev).eval()
        mods[side].load_state_dict(off.state_dict())

    levels = []
    for name, disp, h, w in CFG4 + CFG3:
        d = int(disp ** 0.5)
        mvol = torch.randn(8, d, d, WIDTHS[0], h, w, generator=gen).to(dev)
        r = {"level": name, "images": 8 * disp, "channels": WIDTHS[0], "height": h, "width": w,
             "group": ops.mnet_group(8 * disp, WIDTHS, h, w)}
        r.update(timed({s: (lambda m=m: m(mvol)) for s, m in mods.items()}))
        r["peak_allocated_bytes"] = {s: peak_bytes(lambda m=m: m(mvol)) for s, m in mods.items()}
        with torch.no_grad():
            ref = mods["off"](mvol)
            r["max_norm_diff_from_off"] = {s: float((mods[s](mvol) - ref).abs().max() / ref.abs().max())
                                           for s in ("fused_fp32", "fused_bf16")}
        flops = net_flops(8 * disp, h, w)
        r["algorithmic_gflop"] = flops / 1e9
        r["mfma_peak_fraction"] = {s: flops / (r["forward_ms"][s] * 1e-3) / MFMA_PEAK for s in ("fused_fp32", "fused_bf16")}
        levels.append(r)
        del mvol
        torch.cuda.empty_cache()

    # ---- per layer at the cfg4 1/8 level ---------------------------------------------------------------
    name, disp, h, w = CFG4[0]
    n = 8 * disp
    with torch.no_grad():
        weights, biases = [[t.contiguous() for t in ts] for ts in mods["fused_fp32"].folded()]
    layers = []
    x = torch.randn(n, WIDTHS[0], h, w, generator=gen).to(dev)
    for i, stride in enumerate((1, 2, 1, 1)):
        block = off[i]
        r = {"layer": i + 1, "in": list(x.shape), "stride": stride}
        r.update(timed({"off": lambda: block(x),
                        "fused_fp32": lambda: ops.conv2d_norm_act(x, weights[i], biases[i], stride=stride, act="relu"),
                        "fused_bf16": lambda: ops.conv2d_norm_act(x, weights[i], biases[i], stride=stride, act="relu",
                                                                  precision="bf16")}))
        layers.append(r)
        with torch.no_grad():
            x = block(x)
    r = {"layer": "5 + 6 (tail)", "in": list(x.shape)}
    r.update(timed({"off": lambda: off[5](off[4](x)),
                    "fused_fp32": lambda: ops.mnet_tail(x, weights[4], biases[4], weights[5], biases[5]),
                    "fused_bf16": lambda: ops.mnet_tail(x, weights[4], biases[4], weights[5], biases[5], precision="bf16")}))
    layers.append(r)
    del x
    torch.cuda.empty_cache()

    # ---- workspace budgets -----------------------------------------------------------------------------
    d = int(disp ** 0.5)
    mvol = torch.randn(8, d, d, WIDTHS[0], h, w, generator=gen).to(dev)
    sides, groups = {"off": lambda: off(mvol)}, {}
    for mib in BUDGETS_MIB:
        groups[mib] = ops.mnet_group(n, WIDTHS, h, w, mib << 20)
        for precision in ("fp32", "bf16"):
            sides[f"{mib}MiB_{precision}"] = (lambda mib=mib, precision=precision: ops.matching_net(
                mvol, weights, biases, precision=precision, workspace_bytes=mib << 20))
    budgets = {"level": name, "images": n, "groups": groups}
    budgets.update(timed(sides))

    # ---- graph replay ----------------------------------------------------------------------------------
    graph = {}
    flops = net_flops(n, h, w)
    for precision in ("fp32", "bf16"):
        with torch.no_grad():
            fn = lambda: ops.matching_net(mvol, weights, biases, precision=precision)      # noqa: E731
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                fn()
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
        (ms,) = interleaved_ms([g.replay])
        graph[precision] = {"replay_ms": ms, "mfma_peak_fraction": flops / (ms * 1e-3) / MFMA_PEAK}
    graph["algorithmic_gflop"] = flops / 1e9
    del mvol
    torch.cuda.empty_cache()

    # ---- the ctf-l3 forward ------------------------------------------------------------------------------
    def make(**kw):
        def cmod(*args, **kwargs):
            return rmd.corr.make_cmod(*args, **kwargs, **kw)
        return det_init_fanin(CtfL3Net(cmod, rmd.corr.make_flow_regression, upnet_cls=rmd.raft.Up8Network),
                              head_gain=0.02).to(dev).eval()
    nets = {"off": make(), "fused_fp32": make(fused="on"), "fused_bf16": make(fused="on", precision="bf16")}
    img1, img2, _ = frame_pair(384, 1280)
    i1, i2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
    model = {"shape": "384x1280 b1, iterations (4, 3, 3)"}
    model.update(timed({s: (lambda m=m: m(i1, i2, (4, 3, 3))) for s, m in nets.items()}))
    with torch.no_grad():
        ref = nets["off"](i1, i2, (4, 3, 3))[2][-1]
        model["max_flow_diff_px"] = {s: float((nets[s](i1, i2, (4, 3, 3))[2][-1] - ref).abs().max())
                                     for s in ("fused_fp32", "fused_bf16")}

    print(TAG + json.dumps({"warmup": warmup, "steps": steps, "levels": levels, "layers_cfg4_1_8": layers,
                            "budgets": budgets, "graph_cfg4_1_8": graph, "model_ctf_l3": model,
                            "default_workspace_bytes": ops.MNET_WORKSPACE_BYTES,
                            "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnet_r18.json"))
    ap.add_argument("--resources", default=None, help="JSON file with the compiler's figures for the tail kernels")
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (a median over fewer steps is not reported)")
    if a.leg:
        leg(a.warmup, a.steps)
        return 0
    # a fresh child under its own time limit
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--warmup", str(a.warmup), "--steps",
                        str(a.steps)], capture_output=True, text=True, timeout=LEG_TIMEOUT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith(TAG)), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"mnet_probe: failed (exit {r.returncode})")
        return 1
    res = json.loads(line[len(TAG):])
    for lv in res["levels"]:
        t = lv["forward_ms"]
        print(f"mnet_probe: {lv['level']} ({lv['images']} x {lv['height']}x{lv['width']}, group {lv['group']}): off "
              f"{t['off']:.3f} ms, fused fp32 {t['fused_fp32']:.3f} ms (x{lv['off_over_fused']['fused_fp32']:.2f}), bf16 "
              f"{t['fused_bf16']:.3f} ms (x{lv['off_over_fused']['fused_bf16']:.2f}); peak bytes "
              f"{lv['peak_allocated_bytes']}; diff {lv['max_norm_diff_from_off']}")
    for ly in res["layers_cfg4_1_8"]:
        print(f"mnet_probe: layer {ly['layer']}: {ly['forward_ms']}  off / fused {ly['off_over_fused']}")
    print(f"mnet_probe: budgets (groups {res['budgets']['groups']}): {res['budgets']['forward_ms']}")
    print(f"mnet_probe: graph replay: {res['graph_cfg4_1_8']}")
    print(f"mnet_probe: ctf-l3: {res['model_ctf_l3']}")
    import torch
    doc = {"tool": "tools/mnet_probe.py", "torch": torch.__version__, "mfma_peak_flops_per_s": MFMA_PEAK, **res}
    if a.resources:
        with open(a.resources) as f:
            doc["compiler_resource_usage"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"mnet_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
