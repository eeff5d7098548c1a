#!/usr/bin/env python3
"""Prove that a refactor leaves the compiled kernels unchanged: device assembly of REV against this tree.

    python tools/device_asm_diff.py REV

Extracts REV's raft-meets-dicl_amd/csrc and include into a temporary directory, builds the device assembly of
every .hip source there and here (csrc/Makefile's build/asm/%.s rule, this tree's Makefile for both), drops
the lines that carry the per-compilation __hip_cuid_ symbol and prints, per source, the line count and the
number of differing lines.  Exit status 1 if any source differs.  Needs hipcc, no GPU.
"""
import pathlib
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = "raft-meets-dicl_amd/csrc"


def build_asm(csrc):
    """{source name: assembly lines without the __hip_cuid_ ones} of every .hip in `csrc`"""
    names = sorted(p.stem for p in csrc.glob("*.hip"))
    targets = [f"build/asm/{n}.s" for n in names]
    subprocess.run(["make", "-f", str(ROOT / CSRC / "Makefile"), "-C", str(csrc), "-j16", *targets],
                   check=True, stdout=subprocess.DEVNULL)
    return {n: [l for l in (csrc / f"build/asm/{n}.s").read_text().splitlines() if "__hip_cuid_" not in l]
            for n in names}


def differing(a, b):
    """lines that diff(1) reports as removed from a or added in b"""
    if a == b:
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, lines in (("a", a), ("b", b)):
            pathlib.Path(tmp, name).write_text("\n".join(lines) + "\n")
        out = subprocess.run(["diff", "a", "b"], cwd=tmp, stdout=subprocess.PIPE, text=True).stdout
    return sum(l.startswith(("<", ">")) for l in out.splitlines())


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        archive = subprocess.run(["git", "-C", str(ROOT), "archive", rev, CSRC, "include"], check=True,
                                 stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=archive, check=True)
        old = build_asm(pathlib.Path(tmp) / CSRC)
    new = build_asm(ROOT / CSRC)
    bad = 0
    print(f"{'source':<24}{rev:>12}{'this tree':>12}{'differing':>12}")
    for n in sorted(set(old) | set(new)):
        a, b = old.get(n, []), new.get(n, [])
        d = differing(a, b)
        bad += d != 0
        print(f"{n + '.hip':<24}{len(a):>12}{len(b):>12}{d:>12}")
    print("identical" if not bad else f"{bad} source(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
