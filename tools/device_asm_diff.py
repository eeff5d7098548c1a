#!/usr/bin/env python3
"""Prove that a refactor leaves the compiled kernels unchanged: device assembly of REV against this tree,
kernel by kernel, so a kernel may move to another source.

    python tools/device_asm_diff.py REV [--rename OLD=NEW ...] [--rename-re PATTERN=REPL ...]

Extracts REV's raft-meets-dicl_amd/csrc and include into a temporary directory and builds the device assembly
of every .hip source there and here (csrc/Makefile's build/asm/%.s rule, this tree's Makefile for both).  Every
function of every source is collected: its symbol line up to its .Lfunc_end label plus, for a kernel, its
.amdhsa_kernel block.  Lines that carry the per-compilation __hip_cuid_ symbol are dropped and the
translation-unit ordinal in local labels (.LBB<n>_<m>, .Lfunc_end<n>) becomes a fixed token, since it changes
when a function moves.  Functions are matched by mangled name, and by source too where two sources define the
same name, and fall into one class each:

    identical   same text
    reordered   same .amdhsa_ block (registers, LDS, scratch), same number of body lines, same multiset of
                instruction mnemonics: a pure rescheduling
    different   anything else
    missing     in REV only
    new         in this tree only

--rename OLD=NEW (repeatable) replaces the mangled name OLD by NEW throughout REV's assembly before the functions
are matched, so a kernel whose symbol changed (it lost a template parameter, say) is still compared body for body.
--rename-re PATTERN=REPL does the same with a regular expression (re.sub), for a whole family of instantiations:

    --rename-re '(otf_lookup_kernelI(?:DF16b|f)Lb[01]ELi\\d+ELi\\d+E)Li1E=\\1'

drops the fifth template argument, a constant 1, from every otf_lookup_kernel instantiation.

Prints the counts per source of this tree (REV's source for a missing one) and names every function that is not
identical.  Exit status 1 unless all are identical or reordered.  Needs hipcc, no GPU.
"""
import collections
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = "raft-meets-dicl_amd/csrc"
CLASSES = ("identical", "reordered", "different", "missing", "new")

Function = collections.namedtuple("Function", "source body amdhsa")


def build_asm(csrc):
    """{source name: assembly lines} of every .hip in `csrc`"""
    names = sorted(p.stem for p in csrc.glob("*.hip"))
    targets = [f"build/asm/{n}.s" for n in names]
    subprocess.run(["make", "-f", str(ROOT / CSRC / "Makefile"), "-C", str(csrc), "-j16", *targets],
                   check=True, stdout=subprocess.DEVNULL)
    return {n: (csrc / f"build/asm/{n}.s").read_text().splitlines() for n in names}


def normalised(line):
    """`line` with the translation-unit ordinal of local labels (in comments too) as '#'; the ordinal's width
    moves the comment column, so the padding before a comment becomes one space"""
    line = re.sub(r"(\.L|\b)(BB|JTI)\d+_(\d+)", r"\1\2#_\3", line)
    line = re.sub(r"(\.Lfunc_(?:begin|end))\d+", r"\1#", line)
    return re.sub(r"\s+;", " ;", line)


def functions(source, lines):
    """[(mangled name, Function)] of one source's assembly"""
    lines = [normalised(l) for l in lines if "__hip_cuid_" not in l]
    bodies, blocks = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):\s*; @", lines[i])
        k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m or k:
            end = r"\.Lfunc_end#:" if m else r"\s*\.end_amdhsa_kernel"
            j = i
            while not re.match(end, lines[j]):
                j += 1
            (bodies if m else blocks)[(m or k).group(1)] = lines[i:j + 1]
            # where the assembler's output has the kernel's descriptor before .Lfunc_end, it lies in the body
            inner = [n for n in range(i, j) if m and re.match(r"\s*\.(end_)?amdhsa_kernel", lines[n])]
            if inner:
                blocks[m.group(1)] = lines[inner[0]:inner[-1] + 1]
            i = j
        i += 1
    assert set(blocks) <= set(bodies), f"{source}: .amdhsa_kernel block without a body"
    return [(name, Function(source, body, blocks.get(name, []))) for name, body in bodies.items()]


def collect(asm):
    """{key: Function}; the key is the mangled name, or (name, source) where two sources define the name"""
    found = [f for source, lines in sorted(asm.items()) for f in functions(source, lines)]
    count = collections.Counter(name for name, _ in found)
    return {(name if count[name] == 1 else (name, f.source)): f for name, f in found}


def mnemonics(body):
    """multiset of the instruction mnemonics of a function body"""
    ops = collections.Counter()
    for line in body:
        s = line.strip()
        if s and not s.startswith((";", ".")) and not s.split(";")[0].rstrip().endswith(":"):
            ops[s.split()[0]] += 1
    return ops


def classify(a, b):
    if a is None or b is None:
        return "new" if a is None else "missing"
    if a.body == b.body and a.amdhsa == b.amdhsa:
        return "identical"
    if a.amdhsa == b.amdhsa and len(a.body) == len(b.body) and mnemonics(a.body) == mnemonics(b.body):
        return "reordered"
    return "different"


def main():
    args, renames = sys.argv[1:], []
    for flag, literal in (("--rename", True), ("--rename-re", False)):
        while flag in args[:-1]:
            i = args.index(flag)
            was, _, now = args[i + 1].partition("=")
            renames.append((re.escape(was), now.replace("\\", r"\\")) if literal else (was, now))
            del args[i:i + 2]
    if len(args) != 1 or args[0].startswith("-") or not all(was and now for was, now in renames):
        sys.exit(__doc__)
    rev = args[0]
    with tempfile.TemporaryDirectory() as tmp:
        archive = subprocess.run(["git", "-C", str(ROOT), "archive", rev, CSRC, "include"], check=True,
                                 stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=archive, check=True)
        asm = build_asm(pathlib.Path(tmp) / CSRC)
    for was, now in renames:
        asm = {n: [re.sub(was, now, l) for l in lines] for n, lines in asm.items()}
    old = collect(asm)
    new = collect(build_asm(ROOT / CSRC))
    # a name keyed with its source on one side only (it was unique there) is keyed alike on both
    for side, other in ((old, new), (new, old)):
        for key in [k for k in side if isinstance(k, tuple) and k not in other]:
            if key[0] in other and other[key[0]].source == key[1]:
                other[key] = other.pop(key[0])
    table = collections.defaultdict(collections.Counter)
    named = []
    for key in sorted(set(old) | set(new), key=str):
        a, b = old.get(key), new.get(key)
        cls = classify(a, b)
        table[(b or a).source][cls] += 1
        if cls != "identical":
            named.append(f"  {cls:<10}{(b or a).source}.hip  {key if isinstance(key, str) else key[0]}")
    print(f"{'source':<28}{'kernels':>9}" + "".join(f"{c:>11}" for c in CLASSES))
    total = collections.Counter()
    for source in sorted(table):
        total += table[source]
        print(f"{source + '.hip':<28}{sum(table[source].values()):>9}" + "".join(f"{table[source][c]:>11}" for c in CLASSES))
    print(f"{'all':<28}{sum(total.values()):>9}" + "".join(f"{total[c]:>11}" for c in CLASSES))
    print("\n".join(named))
    bad = total["different"] + total["missing"] + total["new"]
    print(f"{bad} function(s) different, missing or new vs {rev}" if bad else f"every function identical or reordered vs {rev}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
