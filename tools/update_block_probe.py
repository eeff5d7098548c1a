#!/usr/bin/env python3
"""The fused k x k convolutions (rmd.ops.conv2d_act / motion_encoder, csrc/conv.hip) and the modules built on them
against the MIOpen paths they replace, timed in one process between device events:

  shapes    cfg2 (b8, 55x128) and the three cfg4 ctf levels (b8, 48x160, 24x80, 12x40) — the shapes of
            profiles/gru_r14.json —, corr_planes 324 throughout
  convs     each of the nine convolutions of BasicMotionEncoder, FlowHead and Up8Network's mask head:
            ops.conv2d_act in precision "fp32" (three split-bf16 products) and "bf16" (one), weight repack included,
            against the eager Conv2d (+ ReLU)
  modules   ops.motion_encoder against the eager BasicMotionEncoder; the whole BasicUpdateBlock and Up8Network,
            eager / GRU fused (the parent's path) / everything fused, both precisions
  model     tests/e2e RaftNet (rmd correlation) at 436x1024 (padded 440x1024) b8, 12 iterations: eager; GRU fused;
            GRU + block fused; GRU + block + Up8 fused (fp32 mode, and the last also in bf16): frame pairs/s; and
            the e2e fixture at b1: max |EPE - EPE_ref| over the iterations and the sampled flow difference
  split     the eager network's batch time by module, between device events recorded in forward hooks: the two
            encoders, the update block's convolutions (motion encoder + flow head), the recurrent unit, Up8 and
            the hot path (correlation pyramid + 12 lookups); the rest is the glue between them

Fused and eager alternate inside one loop (the machine is shared), eager first; median over `steps` after `warmup`.
Algorithmic FLOPs: 2 x kh x kw x Cin x Cout per pixel; the fraction is of the 2.5 PFLOP/s dense bf16 MFMA peak (the
three-product mode issues three times the MFMAs for the same algorithmic FLOPs).  The work runs in a child process
under its own time limit.

The share of a call that the weight repack takes comes from a kernel trace:
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/update_block_probe.py --trace-leg
  python3 tools/update_block_probe.py --pack-stats DIR/.../*_kernel_stats.csv      (adds "pack_share" to --out)

usage: python3 tools/update_block_probe.py [--warmup 10] [--steps 20] [--out profiles/update_block_r16.json]
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
BATCH, PLANES = 8, 324
SHAPES = [("cfg2 1/8", 55, 128), ("ctf-l3 1/8", 48, 160), ("ctf-l3 1/16", 24, 80), ("ctf-l3 1/32", 12, 40)]
# (module path, Cin, Cout, k, activation)
CONVS = [("enc.convc1", PLANES, 256, 1, "relu"), ("enc.convc2", 256, 192, 3, "relu"), ("enc.convf1", 2, 128, 7, "relu"),
         ("enc.convf2", 128, 64, 3, "relu"), ("enc.conv", 256, 126, 3, "relu"), ("flow.conv1", 128, 256, 3, "relu"),
         ("flow.conv2", 256, 2, 3, "none"), ("up8.conv1", 128, 256, 3, "relu"), ("up8.conv2", 256, 576, 1, "none")]
TRACE_CALLS = 20


def _modules(dev):
    import rmd.raft
    from detinit import det_init_fanin

    def block(**kw):
        return det_init_fanin(rmd.raft.BasicUpdateBlock(PLANES, **kw)).eval().to(dev)

    def up8(**kw):
        return det_init_fanin(rmd.raft.Up8Network(128, **kw)).eval().to(dev)

    blocks = {"eager": block(), "gru_fused": block(gru_fused="on"),
              "all_fused_fp32": block(gru_fused="on", fused="on"),
              "all_fused_bf16": block(gru_fused="on", gru_precision="bf16", fused="on", precision="bf16")}
    ups = {"eager": up8(), "fused_fp32": up8(fused="on"), "fused_bf16": up8(fused="on", precision="bf16")}
    return blocks, ups


def trace_leg():
    """TRACE_CALLS calls of the fully fused block and Up8Network at cfg2 (fp32 mode), for a kernel trace."""
    import torch
    dev = torch.device("cuda", 0)
    blocks, ups = _modules(dev)
    _, h, w = SHAPES[0]
    gen = torch.Generator().manual_seed(16)
    hid, ctx, corr, flow = (torch.randn(BATCH, c, h, w, generator=gen).to(dev) for c in (128, 128, PLANES, 2))
    with torch.no_grad():
        for _ in range(TRACE_CALLS):
            hh, d = blocks["all_fused_fp32"](hid, ctx, corr, flow)
            ups["fused_fp32"](hh, d)
    torch.cuda.synchronize()


def pack_share(path):
    """Share of the conv.hip kernels' time that the repack takes, from a rocprofv3 kernel_stats.csv."""
    total, pack, per = 0, 0, {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            for key in ("conv_pack_kernel", "conv_kernel", "conv_copy_kernel", "gru_pack_kernel", "gru_kernel"):
                if key + "<" in name or key + "(" in name:
                    per[key] = per.get(key, 0) + int(r["TotalDurationNs"])
    total = sum(per.get(k, 0) for k in ("conv_pack_kernel", "conv_kernel", "conv_copy_kernel"))
    pack = per.get("conv_pack_kernel", 0)
    return {"shape": f"{SHAPES[0][0]}: fully fused BasicUpdateBlock + Up8Network, fp32 mode, {TRACE_CALLS} calls",
            "kernel_ns": per, "conv_pack_over_conv_kernels": pack / total if total else None}


def leg(warmup, steps):
    import statistics
    import time

    import numpy as np
    import torch
    import torch.nn.functional as F
    import rmd.raft
    from conftest import load_golden
    from detinit import det_init_fanin
    from e2e.raft_net import RaftNet
    from rmd import ops
    from synth import epe, frame_pair
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(16)

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
        """{side: fn}, eager first -> {side: ms} and the eager-over-side ratios."""
        order = ["eager"] + [s for s in sides if s != "eager"]
        t = dict(zip(order, interleaved_ms([sides[s] for s in order])))
        return {"forward_ms": t, "eager_over_fused": {s: t["eager"] / t[s] for s in order[1:]}}

    blocks, ups = _modules(dev)
    parts = {"enc": blocks["eager"].enc, "flow": blocks["eager"].flow, "up8": ups["eager"]}
    legs = []
    for name, h, w in SHAPES:
        def rand(c):
            return torch.randn(BATCH, c, h, w, generator=gen).to(dev)
        row = {"shape": f"{name}: ({BATCH}, ., {h}, {w})", "warmup": warmup, "steps": steps, "convs": {}}
        for path, cin, cout, k, act in CONVS:
            owner, attr = path.split(".")
            conv = getattr(parts[owner], attr)
            x = rand(cin)
            sides = {"eager": (lambda conv=conv, x=x: F.relu(conv(x))) if act == "relu" else (lambda conv=conv, x=x: conv(x))}
            for p in ("fp32", "bf16"):
                sides["fused_" + p] = lambda conv=conv, x=x, act=act, p=p: ops.conv2d_act(x, None, conv.weight, conv.bias, act, p)
            r = timed(sides)
            flops = 2.0 * k * k * cin * cout * BATCH * h * w
            r["algorithmic_flops"] = flops
            r["mfma_peak_fraction"] = {s: flops / (r["forward_ms"][s] * 1e-3) / MFMA_PEAK for s in ("fused_fp32", "fused_bf16")}
            row["convs"][f"{path} {k}x{k} {cin}->{cout} {act}"] = r
        hid, ctx, corr, flow = rand(128), rand(128), rand(PLANES), rand(2)
        enc = parts["enc"]
        ws, bs = [c.weight for c in enc._convs()], [c.bias for c in enc._convs()]
        row["motion_encoder"] = timed({"eager": lambda: enc(flow, corr),
                                       "fused_fp32": lambda: ops.motion_encoder(flow, corr, ws, bs, "fp32"),
                                       "fused_bf16": lambda: ops.motion_encoder(flow, corr, ws, bs, "bf16")})
        row["basic_update_block"] = timed({s: (lambda m=m: m(hid, ctx, corr, flow)) for s, m in blocks.items()})
        row["up8_network"] = timed({s: (lambda m=m: m(hid, flow)) for s, m in ups.items()})
        legs.append(row)

    # the whole network
    g = load_golden("e2e_raft_436x1024")
    fh, fw, iters = int(g["height"]), int(g["width"]), int(g["iterations"])
    img1, img2, gt = frame_pair(fh, fw)
    one = (torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev))
    low = torch.rand(BATCH, 3, 55, 128, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    b1 = F.interpolate(low, size=(440, 1024), mode="bilinear", align_corners=True).to(dev)
    b2 = torch.roll(b1, shifts=(3, 5), dims=(2, 3))
    configs = {"eager": ({}, {}), "gru_fused": ({"gru_fused": "on"}, {}),
               "gru_block_fused": ({"gru_fused": "on", "fused": "on"}, {}),
               "gru_block_up8_fused": ({"gru_fused": "on", "fused": "on"}, {"fused": "on"}),
               "gru_block_up8_fused_bf16": ({"gru_fused": "on", "gru_precision": "bf16", "fused": "on", "precision": "bf16"},
                                            {"fused": "on", "precision": "bf16"})}

    def network(block_kw, up_kw, corr_block=rmd.raft.CorrBlock):
        net = RaftNet(corr_block, precision="fp32", upnet_cls=rmd.raft.Up8Network)
        net.update_block = rmd.raft.BasicUpdateBlock(PLANES, **block_kw)
        net.upnet = rmd.raft.Up8Network(128, **up_kw)
        return det_init_fanin(net).eval().to(dev)

    model = {}
    for side, (block_kw, up_kw) in configs.items():
        net = network(block_kw, up_kw)
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

    # the eager batch by module
    spans = {}

    def span(key):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        spans.setdefault(key, []).append((e0, e1))
        return e0, e1

    class TimedCorr:
        def __init__(self, *a, **k):
            e0, e1 = span("hot_path")
            e0.record()
            self.inner = rmd.raft.CorrBlock(*a, **k)
            e1.record()

        def __call__(self, coords):
            e0, e1 = span("hot_path")
            e0.record()
            out = self.inner(coords)
            e1.record()
            return out

    net = network({}, {}, TimedCorr)
    watched = {"encoders": [net.fnet, net.cnet], "update_block_convolutions": [net.update_block.enc, net.update_block.flow],
               "gru": [net.update_block.gru], "up8": [net.upnet]}
    open_spans = {}
    for key, mods in watched.items():
        for m in mods:
            def pre(mod, inputs, key=key):
                e0, e1 = span(key)
                open_spans[id(mod)] = e1
                e0.record()

            def post(mod, inputs, output):
                open_spans.pop(id(mod)).record()
            m.register_forward_pre_hook(pre)
            m.register_forward_hook(post)
    with torch.no_grad():
        for _ in range(2):
            net(b1, b2, iters)
        torch.cuda.synchronize()
        spans.clear()
        reps = 3
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            net(b1, b2, iters)
        t1.record()
        torch.cuda.synchronize()
    total = t0.elapsed_time(t1) / reps
    split = {k: sum(a.elapsed_time(b) for a, b in v) / reps for k, v in spans.items()}
    split["glue"] = total - sum(split.values())
    split_doc = {"ms_per_batch": total, "ms": split, "share": {k: v / total for k, v in split.items()}}
    print("UPDATE_BLOCK_PROBE " + json.dumps({"legs": legs, "model_436x1024_b8_12_iterations": model,
                                              "eager_batch_by_module": split_doc}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_block_r16.json"))
    ap.add_argument("--leg", action="store_true", help="internal: run the measurement in this process")
    ap.add_argument("--trace-leg", action="store_true", help="the fully fused block and Up8 at cfg2, for a kernel trace")
    ap.add_argument("--pack-stats", help="a rocprofv3 kernel_stats.csv of --trace-leg: add the repack's share to --out")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 (a median over fewer steps is not reported)")
    if a.trace_leg:
        trace_leg()
        return 0
    if a.leg:
        leg(a.warmup, a.steps)
        return 0
    if a.pack_stats:
        with open(a.out) as f:
            doc = json.load(f)
        doc["pack_share"] = pack_share(a.pack_stats)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(f"update_block_probe: pack share {doc['pack_share']['conv_pack_over_conv_kernels']} -> {a.out}")
        return 0
    # a fresh child under its own time limit
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--warmup", str(a.warmup), "--steps",
                        str(a.steps)], capture_output=True, text=True, timeout=LEG_TIMEOUT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("UPDATE_BLOCK_PROBE ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"update_block_probe: failed (exit {r.returncode})")
        return 1
    res = json.loads(line[len("UPDATE_BLOCK_PROBE "):])
    for lg in res["legs"]:
        for name, c in lg["convs"].items():
            t = c["forward_ms"]
            print(f"update_block_probe: {lg['shape']} {name}: eager {t['eager']:.3f} ms, fused fp32 {t['fused_fp32']:.3f} ms "
                  f"(x{c['eager_over_fused']['fused_fp32']:.2f}, {100 * c['mfma_peak_fraction']['fused_fp32']:.1f} % of peak), "
                  f"bf16 {t['fused_bf16']:.3f} ms (x{c['eager_over_fused']['fused_bf16']:.2f})")
        for key in ("motion_encoder", "basic_update_block", "up8_network"):
            print(f"update_block_probe: {lg['shape']} {key}: {lg[key]['forward_ms']}  eager / fused {lg[key]['eager_over_fused']}")
    for side, m in res["model_436x1024_b8_12_iterations"].items():
        print(f"update_block_probe: model {side}: {m['frame_pairs_per_s']:.1f} pairs/s ({m['ms_per_batch']:.1f} ms), e2e dEPE "
              f"{m['e2e_max_abs_epe_diff_px']:.2e} px, flow {m['e2e_max_flow_diff_px']:.2e} px")
    print(f"update_block_probe: eager batch by module: {res['eager_batch_by_module']}")
    import torch
    doc = {"tool": "tools/update_block_probe.py", "torch": torch.__version__, "mfma_peak_flops_per_s": MFMA_PEAK, **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"update_block_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
