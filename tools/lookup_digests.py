#!/usr/bin/env python3
"""Record or compare the lookup bit-exactness digests (tests/lookup_digest_cases.py) for the library in
RMD_LIBRARY (default: the product).  MI355X only.

usage: python3 tools/lookup_digests.py --record tests/golden/lookup_digests.json   (from a known-good build)
       python3 tools/lookup_digests.py                                             (compare; exit 1 on a mismatch)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raft-meets-dicl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "lookup_digests.json")


def main():
    import torch

    import lookup_digest_cases as lc
    from rmd import _lib, library
    dev = torch.device("cuda:0")
    got, pyrs = {}, {}
    for kind, radius, shape in lc.all_cases():
        if (kind, shape) not in pyrs:
            pyr = lc.build_pyramid(kind, shape, dev)
            dtype, tiles = lc.EXPECT[kind]
            assert str(pyr.data.dtype) == "torch." + dtype, (kind, pyr.data.dtype)
            assert (library.pyramid_layout(pyr.data) == _lib.RMD_LAYOUT_TILES) == tiles, kind
            pyrs[kind, shape] = pyr
        got[lc.case_id(kind, radius, shape)] = lc.digest(pyrs[kind, shape], shape, radius, dev)
    if len(sys.argv) > 2 and sys.argv[1] == "--record":
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"recorded {len(got)} digests -> {sys.argv[2]}")
        return 0
    want = json.load(open(GOLDEN))
    bad = sorted(k for k in want if got.get(k) != want[k])
    print(json.dumps({"lib": os.path.basename(os.environ.get("RMD_LIBRARY", "librmd.so")), "cases": len(want),
                      "mismatch": bad}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
