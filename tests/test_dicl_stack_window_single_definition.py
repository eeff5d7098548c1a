"""The LDS window of the stack backward kernels has one definition, csrc/dicl_stack_window.h, and the former
dicl.hip is one source per operator.

These tests read the sources: a kernel that copies the window's zero loop, its lowest-row rule or its flush
instead of calling the header fails here, and so does one that adds into the window on its own without being
listed below with the reason.
"""

import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "raft-meets-dicl_amd", "csrc")
HEADER = "dicl_stack_window.h"
BACKWARD = "dicl_stack_backward.hip"

# Kernels that add into the window with their own text, and why.  Both add one patch row per step through a row
# pointer; with that row form in the header (as a member taking the row's values, or a callable) the compiler
# tests the columns once for both targets and the kernel comes out with other instruction counts, which
# tools/device_asm_diff.py classes as different.  Their LDS and global adds stay in separate branches, as the
# header's comment demands (tests/test_asm_audit.py::test_dicl_backward_has_no_flat_atomics watches that).
OWN_WINDOW_ADD = {
    "dicl_stack_patch_backward_kernel": "row add of K values per patch row, zeros included",
    "dicl_stack_sep_backward_kernel": "row add of K values per patch row, zeros left out",
}


def _sources():
    """{file name: text} of every source and header in csrc/"""
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h", ".cpp")))
    assert HEADER in names and BACKWARD in names and len(names) > 10
    return {n: open(os.path.join(CSRC, n)).read() for n in names}


def _occurrences(pattern):
    """{file name: count} over the files where `pattern` occurs"""
    return {n: len(re.findall(pattern, text)) for n, text in _sources().items() if re.search(pattern, text)}


def _kernels(text):
    """{kernel name: body} of the __global__ functions of one source"""
    heads = list(re.finditer(r"__global__[^;{]*?\b(\w+_kernel)\(", text))
    return {m.group(1): text[m.start():(heads[i + 1].start() if i + 1 < len(heads) else len(text))]
            for i, m in enumerate(heads)}


def test_window_zero_loop_is_in_the_header_only():
    assert _occurrences(r"win\[\w+\] = 0\.f") == {HEADER: 1}
    assert _occurrences(r"wmin = 1 << 30") == {HEADER: 1}


def test_lowest_row_rule_is_in_the_header_only():
    assert _occurrences(r"atomicMin\(&wmin") == {HEADER: 1}
    assert _occurrences(r"wy0 = min\(wmin") == {HEADER: 1}
    assert _occurrences(r"wrows = min\(") == {HEADER: 1}


def test_flush_loop_is_in_the_header_only():
    assert _occurrences(r"= win\[\w+\];") == {HEADER: 1}
    assert _occurrences(r"k < wrows \* ") == {HEADER: 1}


def test_chain_link_rule_is_in_the_header_only():
    # the wave_shl:1 shift that tells a lane whether the next one continues its chain
    assert _occurrences(r"update_dpp\(0, \(int\)link, 0x130") == {HEADER: 1}
    # The chain sums stay in the two two-pixel kernels, one each: written once with the step as a parameter,
    # dicl_stack_sep_backward2_kernel<8, *> compiles to other instruction counts.
    assert _occurrences(r"\(link \? up : 0\.f\)") == {BACKWARD: 2}


def test_every_window_kernel_runs_the_protocol():
    kernels = {n: b for n, b in _kernels(_sources()[BACKWARD]).items() if "__shared__ float win[" in b}
    assert len(kernels) == 5
    for name, body in kernels.items():
        for call in ("window_zero(win, wmin)", "window_rows<WIN>(wmin, ", "W.flush(win)"):
            assert body.count(call) == 1, (name, call)


def test_only_the_listed_kernels_add_into_the_window_themselves():
    own = {n for n, b in _kernels(_sources()[BACKWARD]).items() if re.search(r"\bwin \+|atomicAdd\(win\b", b)}
    assert own == set(OWN_WINDOW_ADD)
    others = [n for n, text in _sources().items()
              if n not in (HEADER, BACKWARD) and re.search(r"__shared__ float win\[", text)]
    assert others == []


def test_one_source_per_operator():
    src = _sources()
    assert "dicl.hip" not in src
    for name in ("dicl_stack.hip", BACKWARD, "dicl_int.hip", "dap.hip"):
        assert name in src, name

    def includes(name, seen=()):
        direct = [i for i in re.findall(r'#\s*include\s*"([^"]+)"', src[name]) if i in src and i not in seen]
        return set(direct).union(*(includes(i, (*seen, name)) for i in direct))

    for name, text in src.items():
        if re.search(r"\bdap_\w+\(", text) and "__global__" in text:
            assert "dicl_taps.h" not in includes(name), name
    assert re.search(r"\bdap_x3_kernel\(", src["dap.hip"]) and re.search(r"\bdap_wgrad_kernel\(", src["dap.hip"])
