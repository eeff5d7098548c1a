#!/usr/bin/env python3
"""Static instruction counts of one kernel in a `hipcc -S` listing: VALU (v_*), SALU (s_*), memory, VGPRs,
and the most frequent mnemonics.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -Iinclude -Icsrc --cuda-device-only -S \
           csrc/corr_lookup.hip -o lookup.s
       python3 tools/lookup_asm_stats.py lookup.s [kernel-name substring, default the headline lookup] [top N]
"""
import collections
import json
import re
import sys

HEADLINE = "corr_lookup_kernelI6__halfLi4ELi3ELi1ELb1E"     # <__half, 4, 3, TILES, BUF>


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else HEADLINE
    top = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    name, ops, out = None, collections.Counter(), []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            name, ops = m.group(1), collections.Counter()
            continue
        if name is None or want not in name:
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)\b", line)
        if m and not line.lstrip().startswith("."):
            ops[m.group(1)] += 1
        m = re.match(r"^; NumVgprs: (\d+)", line)
        if m:
            mem = sum(n for o, n in ops.items() if o.startswith(("buffer_", "global_", "flat_", "ds_", "scratch_")))
            valu = sum(n for o, n in ops.items() if o.startswith("v_"))
            salu = sum(n for o, n in ops.items() if o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop")))
            out.append({"kernel": name, "vgprs": int(m.group(1)), "valu": valu, "salu": salu, "mem": mem,
                        "waitcnt": ops["s_waitcnt"], "top": dict(ops.most_common(top))})
            name = None
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
