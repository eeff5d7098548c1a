#!/usr/bin/env python3
"""Record or compare the dicl-1x1 match kernels' bit-exactness digests (tests/dicl_match_digest_cases.py) for
the library in RMD_LIBRARY (default: the product).  MI355X only.

usage: python3 tools/dicl_match_digests.py --record tests/golden/match_digests.json   (from a known-good build)
       python3 tools/dicl_match_digests.py                                            (compare; exit 1 on a mismatch)

The recorded file keeps the rmd_source_hash of the library it was recorded from.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "raft-meets-dicl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "match_digests.json")


def main():
    import torch

    import dicl_match_digest_cases as dc
    from rmd import _lib
    dev = torch.device("cuda:0")
    got = {dc.case_id(s): dc.digests(s, dev) for s in dc.CASES}
    source_hash = _lib.lib().rmd_source_hash().decode()
    if len(sys.argv) > 2 and sys.argv[1] == "--record":
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump({"source_hash": source_hash, "digests": got}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"recorded {sum(len(v) for v in got.values())} digests of {len(got)} cases from library "
              f"{source_hash} -> {sys.argv[2]}")
        return 0
    want = json.load(open(GOLDEN))
    bad = sorted(f"{c}:{n}" for c, names in want["digests"].items() for n in names if got.get(c, {}).get(n) != names[n])
    print(json.dumps({"lib": os.path.basename(os.environ.get("RMD_LIBRARY", "librmd.so")), "source_hash": source_hash,
                      "recorded_from": want["source_hash"], "cases": len(want["digests"]), "mismatch": bad}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
