#!/usr/bin/env python3
"""Launch times of the two forms of the bf16 correlation pyramid at cfg2 (B=8, 55x128, C=256, 4 levels), alternating
in one process: legacy = rmd_corr_prepare (prep_pair) + rmd_corr_pyramid_prepared (corr_pyramid_w8, A operand from
the workspace), staged = rmd_corr_prepare_queries (prep_queries) + rmd_corr_pyramid_staged (corr_pyramid_w8_f32, A
tiles built from fmap2).  HIP events around each of the four launches, and around each pair, reps times; before
every timed pair a cache-sized buffer is rewritten so that the feature maps come from HBM as they do in a model.
Prints one JSON line: medians and minima in microseconds, and whether the two pyramids are bit-identical.
usage: python3 tools/w8_stage_time.py [reps]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-meets-dicl_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from rmd import _lib, library  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    f1, f2, _ = bench.synthetic(8, 256, 55, 128, 12, 1234, "cuda")
    c, scale, compute = 256, 1.0 / 16, _lib.RMD_BF16
    d, data_old, ws = library.pyramid_buffers(f1, 4, compute, _lib.RMD_F16)
    data_new = torch.empty_like(data_old)
    data_old.zero_()
    data_new.zero_()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")       # > L2 + Infinity Cache
    ref = ctypes.byref(d)

    def legacy():
        return [("prep_pair", lambda: _lib.launch("rmd_corr_prepare", f1, f1, f2, c, scale, ref, compute, ws)),
                ("gemm_legacy", lambda: _lib.launch("rmd_corr_pyramid_prepared", f1, c, scale, ref, compute, data_old, ws))]

    def staged():
        return [("prep_queries", lambda: _lib.launch("rmd_corr_prepare_queries", f1, f1, c, ref, compute, ws)),
                ("gemm_staged", lambda: _lib.launch("rmd_corr_pyramid_staged", f1, f2, c, scale, ref, compute, data_new, ws))]

    times = {}
    for rep in range(reps + 3):                                             # 3 warm-up rounds
        for form, pair in (("legacy", legacy()), ("staged", staged())):
            flush.fill_(rep & 1)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            pair[0][1]()
            ev[1].record()
            pair[1][1]()
            ev[2].record()
            torch.cuda.synchronize()
            if rep >= 3:
                times.setdefault(pair[0][0], []).append(ev[0].elapsed_time(ev[1]))
                times.setdefault(pair[1][0], []).append(ev[1].elapsed_time(ev[2]))
                times.setdefault(form + "_pair", []).append(ev[0].elapsed_time(ev[2]))
    res = {"lib": os.path.basename(os.environ.get("RMD_LIBRARY", "librmd.so")), "reps": reps,
           "bit_identical": bool(torch.equal(data_old.view(torch.int16), data_new.view(torch.int16)))}
    for k, v in times.items():
        v.sort()
        res[k] = {"median_us": round(v[len(v) // 2] * 1e3, 2), "min_us": round(v[0] * 1e3, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
