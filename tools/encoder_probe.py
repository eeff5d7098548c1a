#!/usr/bin/env python3
"""The fused feature / context encoder (rmd.ops.conv2d_norm_act / instance_norm_stats / residual_join /
feature_encoder, csrc/encoder.hip) against the MIOpen paths it replaces, timed in one process between device events:

  convs     each of the encoder's 16 convolutions at its real size (a 440x1024 input): on 16 images as fnet runs
            it (instance norm) and on 8 as cnet does (eval batch norm).  Eager: Conv2d + norm + ReLU (no ReLU after
            a projection or the last convolution).  Fused, batch norm: the folded convolution with its ReLU
            epilogue.  Fused, instance norm: the raw convolution + instance_norm_stats — the normalisation and
            ReLU themselves happen while the next convolution stages its input.  Precision "fp32" (three split-bf16
            products) and "bf16" (one), weight repack included
  passes    instance_norm_stats and residual_join on their own at (16, 64, 220, 512)
  encoders  fnet (instance) on 8 and 16 images and cnet (batch) on 8: eager / fused fp32 / fused bf16, with the
            peak memory allocated during a call on each path
  model     tests/e2e RaftNet (rmd correlation) at 436x1024 (padded 440x1024) b8, 12 iterations: eager; the
            parent's best setting (GRU + block + Up8 fused, fp32 mode); that plus the encoders in fp32; that plus
            the encoders in bf16: frame pairs/s; and the e2e fixture at b1: max |EPE - EPE_ref| over the iterations
            and the sampled flow difference

Fused and eager alternate inside one loop (the machine is shared), eager first; median over `steps` after `warmup`.
Algorithmic FLOPs: 2 x k x k x Cin x Cout per output pixel; the fraction is of the 2.5 PFLOP/s dense bf16 MFMA peak
(the three-product mode issues three times the MFMAs for the same algorithmic FLOPs).  The work runs in a child
process under its own time limit.

usage: python3 tools/encoder_probe.py [--warmup 10] [--steps 20] [--out profiles/encoder_r17.json]
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
LEG_TIMEOUT = 1000
HEIGHT, WIDTH, PLANES = 440, 1024, 324
TAG = "ENCODER_PROBE "


def leg(warmup, steps):
    import statistics
    import time

    import numpy as np
    import torch
    import torch.nn.functional as F
    import rmd.encoders
    import rmd.raft
    from conftest import load_golden
    from detinit import det_init_fanin
    from e2e.raft_net import RaftNet
    from rmd import library, ops
    from rmd.blocks.raft import folded
    from synth import epe, frame_pair
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(17)

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

    def encoder(norm, **kw):
        return det_init_fanin(rmd.encoders.FeatureEncoder(256, norm, **kw)).eval().to(dev)

    def peak_bytes(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        return peak

    # ---- the 16 convolutions --------------------------------------------------------------------------
    convs = []
    for norm, batch in (("instance", 16), ("batch", 8)):
        m = encoder(norm)
        pairs = m.conv_norms()
        ht, wd = HEIGHT, WIDTH
        sizes = []                                          # the input size of each convolution
        for cout, cin, k, stride in library.feature_encoder_convs(256):
            if k == 1 and stride == 2:
                sizes.append(sizes[-2])                     # the projection reads its block's input
                continue
            sizes.append((ht, wd))
            ht, wd = library.out_side(ht, stride), library.out_side(wd, stride)
        for g, ((conv, nrm), (cout, cin, k, stride), (h, w)) in enumerate(zip(pairs, library.feature_encoder_convs(256), sizes)):
            x = torch.randn(batch, cin, h, w, generator=gen).to(dev)
            relu = nrm is not None and not (k == 1 and stride == 2)
            with torch.no_grad():
                wt, bs = folded(conv, nrm)
                wt, bs = wt.contiguous(), bs.contiguous()

            def eager(conv=conv, nrm=nrm, x=x, relu=relu):
                y = conv(x) if nrm is None else nrm(conv(x))
                return F.relu(y) if relu else y
            sides = {"eager": eager}
            for p in ("fp32", "bf16"):
                if norm == "instance" and nrm is not None:
                    sides["fused_" + p] = lambda x=x, wt=wt, bs=bs, stride=stride, p=p: ops.instance_norm_stats(
                        ops.conv2d_norm_act(x, wt, bs, stride=stride, precision=p))
                else:
                    sides["fused_" + p] = lambda x=x, wt=wt, bs=bs, stride=stride, p=p, relu=relu: ops.conv2d_norm_act(
                        x, wt, bs, stride=stride, act="relu" if relu else "none", precision=p)
            r = timed(sides)
            flops = 2.0 * k * k * cin * cout * batch * library.out_side(h, stride) * library.out_side(w, stride)
            r["algorithmic_flops"] = flops
            r["mfma_peak_fraction"] = {s: flops / (r["forward_ms"][s] * 1e-3) / MFMA_PEAK for s in ("fused_fp32", "fused_bf16")}
            r["conv"] = f"#{g} {k}x{k} stride {stride} {cin}->{cout} on ({batch}, {cin}, {h}, {w}), {norm} norm"
            convs.append(r)
            del x
        del m
        torch.cuda.empty_cache()

    # ---- the statistics and the join on their own -----------------------------------------------------
    y = torch.randn(16, 64, 220, 512, generator=gen).to(dev)
    x = torch.randn(16, 64, 220, 512, generator=gen).to(dev)
    stats = ops.instance_norm_stats(y)
    passes = {"shape": "(16, 64, 220, 512)",
              "instance_norm_stats": timed({"eager": lambda: torch.var_mean(y, dim=(2, 3), unbiased=False),
                                            "fused": lambda: ops.instance_norm_stats(y)}),
              "residual_join": timed({"eager": lambda: F.relu(x + F.relu(F.instance_norm(y))),
                                      "fused": lambda: ops.residual_join(y, x, stats)})}
    passes["note"] = "eager statistics: torch.var_mean alone; eager join: instance norm + ReLU + add + ReLU"
    del x, y, stats
    torch.cuda.empty_cache()

    # ---- the encoders ---------------------------------------------------------------------------------
    encoders = {}
    for name, norm, batch in (("fnet_b8", "instance", 8), ("fnet_b16", "instance", 16), ("cnet_b8", "batch", 8)):
        img = (torch.rand(batch, 3, HEIGHT, WIDTH, generator=gen) * 2 - 1).to(dev)
        mods = {"eager": encoder(norm), "fused_fp32": encoder(norm, fused="on"),
                "fused_bf16": encoder(norm, fused="on", precision="bf16")}
        r = timed({s: (lambda m=m: m(img)) for s, m in mods.items()})
        r["peak_allocated_bytes"] = {s: peak_bytes(lambda m=m: m(img)) for s, m in mods.items()}
        r["workspace_bytes"] = library._lib.lib().rmd_feature_encoder_workspace_bytes(batch, HEIGHT, WIDTH, 256)
        with torch.no_grad():
            ref = mods["eager"](img).double()
            r["max_norm_diff_from_eager"] = {s: float((mods[s](img).double() - ref).abs().max() / ref.abs().max())
                                             for s in ("fused_fp32", "fused_bf16")}
        encoders[name] = r
        del mods, img, ref
        torch.cuda.empty_cache()

    # ---- the whole network ----------------------------------------------------------------------------
    g = load_golden("e2e_raft_436x1024")
    fh, fw, iters = int(g["height"]), int(g["width"]), int(g["iterations"])
    img1, img2, gt = frame_pair(fh, fw)
    one = (torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev))
    low = torch.rand(8, 3, 55, 128, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    b1 = F.interpolate(low, size=(HEIGHT, WIDTH), mode="bilinear", align_corners=True).to(dev)
    b2 = torch.roll(b1, shifts=(3, 5), dims=(2, 3))
    best = ({"gru_fused": "on", "fused": "on"}, {"fused": "on"})
    configs = {"eager": ({}, {}, None), "gru_block_up8_fused": (*best, None),
               "gru_block_up8_encoders_fused": (*best, "fp32"), "gru_block_up8_fused_encoders_bf16": (*best, "bf16")}

    def network(block_kw, up_kw, enc_precision):
        net = RaftNet(rmd.raft.CorrBlock, precision="fp32", upnet_cls=rmd.raft.Up8Network)
        if enc_precision:
            net.fnet = rmd.encoders.FeatureEncoder(256, "instance", fused="on", precision=enc_precision)
            net.cnet = rmd.encoders.FeatureEncoder(256, "batch", fused="on", precision=enc_precision)
        net.update_block = rmd.raft.BasicUpdateBlock(PLANES, **block_kw)
        net.upnet = rmd.raft.Up8Network(128, **up_kw)
        return det_init_fanin(net).eval().to(dev)

    model = {}
    nets = {side: network(*cfg) for side, cfg in configs.items()}
    with torch.no_grad():
        for side, net in nets.items():
            flows = [f.cpu().numpy() for f in net(*one, iters)]
            d_epe = max(abs(epe(f, gt) - float(r)) for f, r in zip(flows, g["epe"]))
            d_flow = max(float(np.abs(flows[k - 1][0, :, :fh, :fw].reshape(2, -1)[:, g["pixels"]] - g[f"flow_it{k}"]).max())
                         for k in (1, 4, 12))
            model[side] = {"e2e_max_abs_epe_diff_px": d_epe, "e2e_max_flow_diff_px": d_flow}
            for _ in range(2):
                net(b1, b2, iters)
        torch.cuda.synchronize()
        reps, rounds = 2, 3                                  # the settings alternate: rounds x (reps batches each)
        times = {side: [] for side in nets}
        for _ in range(rounds):
            for side, net in nets.items():
                t0 = time.perf_counter()
                for _ in range(reps):
                    net(b1, b2, iters)
                torch.cuda.synchronize()
                times[side].append((time.perf_counter() - t0) / reps)
    for side, t in times.items():
        ms = statistics.median(t) * 1e3
        model[side].update({"frame_pairs_per_s": 8 / (ms * 1e-3), "ms_per_batch": ms})
    print(TAG + json.dumps({"warmup": warmup, "steps": steps, "convs": convs, "passes": passes, "encoders": encoders,
                            "model_436x1024_b8_12_iterations": model}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_r17.json"))
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
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith(TAG)), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"encoder_probe: failed (exit {r.returncode})")
        return 1
    res = json.loads(line[len(TAG):])
    for c in res["convs"]:
        t = c["forward_ms"]
        print(f"encoder_probe: {c['conv']}: eager {t['eager']:.3f} ms, fused fp32 {t['fused_fp32']:.3f} ms "
              f"(x{c['eager_over_fused']['fused_fp32']:.2f}, {100 * c['mfma_peak_fraction']['fused_fp32']:.1f} % of peak), "
              f"bf16 {t['fused_bf16']:.3f} ms (x{c['eager_over_fused']['fused_bf16']:.2f})")
    for key in ("instance_norm_stats", "residual_join"):
        print(f"encoder_probe: {key} {res['passes']['shape']}: {res['passes'][key]['forward_ms']}")
    for name, e in res["encoders"].items():
        print(f"encoder_probe: {name}: {e['forward_ms']}  eager / fused {e['eager_over_fused']}  peak bytes "
              f"{e['peak_allocated_bytes']}  diff from eager {e['max_norm_diff_from_eager']}")
    for side, m in res["model_436x1024_b8_12_iterations"].items():
        print(f"encoder_probe: model {side}: {m['frame_pairs_per_s']:.1f} pairs/s ({m['ms_per_batch']:.1f} ms), e2e dEPE "
              f"{m['e2e_max_abs_epe_diff_px']:.2e} px, flow {m['e2e_max_flow_diff_px']:.2e} px")
    import torch
    doc = {"tool": "tools/encoder_probe.py", "torch": torch.__version__, "mfma_peak_flops_per_s": MFMA_PEAK, **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"encoder_probe: wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
