"""The split-bf16 MFMA arithmetic has one definition, csrc/mfma_bf16.h, and the host helpers that moved to
rmd_common.h with it left every workspace size as it was.

The first four tests read the sources: a new kernel that copies the split, the product or the vector types
instead of including the header fails here.  The last pins the workspace-size entry points (pure host code,
no GPU) to the values of the build before the helpers were shared.
"""

import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "raft-meets-dicl_amd", "csrc")
HEADER = "mfma_bf16.h"


def _sources():
    """{file name: text} of every source and header in csrc/"""
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h", ".cpp")))
    assert HEADER in names and len(names) > 10
    return {n: open(os.path.join(CSRC, n)).read() for n in names}


def _files_matching(pattern):
    return sorted(n for n, text in _sources().items() if re.search(pattern, text))


def test_lo_part_expression_is_in_the_header_only():
    # lo = (__bf16)(v - (float)hi), in any spelling of v and hi
    assert _files_matching(r"\(__bf16\)\([^;\n]* - \(float\)") == [HEADER]


def test_32x32x16_bf16_mfma_is_issued_from_the_header_or_the_single_product_gemm():
    assert _files_matching(r"__builtin_amdgcn_mfma_f32_32x32x16_bf16") == [
        "corr_pyramid_stationary.hip", "corr_pyramid_tiled.hip", "corr_pyramid_w8.hip", HEADER]


def test_bf16_and_f32x16_vector_types_are_declared_in_the_header_only():
    bf16_vec = r"ext_vector_type\([^)]*\)\)\)\s*__bf16|__bf16\s+__attribute__\(\(ext_vector_type"
    f32x16 = r"ext_vector_type\(\s*16\s*\)\)\)\s*float|float\s+__attribute__\(\(ext_vector_type\(\s*16\s*\)"
    assert _files_matching(bf16_vec) == [HEADER]
    assert _files_matching(f32x16) == [HEADER]


def test_gru_does_not_depend_on_the_matching_net():
    gru = _sources()["gru.hip"]
    assert '#include "mfma_bf16.h"' in gru
    assert not re.search(r"#\s*include\s*[\"<]dicl_match", gru)


def test_workspace_sizes_are_those_of_the_build_before_the_shared_helpers():
    from rmd import _lib
    L = _lib.lib()
    x3, bf16, f32 = _lib.RMD_BF16X3, _lib.RMD_BF16, _lib.RMD_F32
    # the GRU golden fixture (gru_nan_b1_h32_x16_7x9) and the cfg2 shape
    assert L.rmd_sepconv_gru_workspace_bytes(1, 32, 16, 7, 9) == 209536
    assert L.rmd_sepconv_gru_workspace_bytes(8, 128, 256, 55, 128) == 92406784
    # dicl-1x1 backward at match_grad_none_b1_c32_6x10: radius 4, widths 48 / 64 / 32 padded to 64 / 64 / 32
    assert L.rmd_dicl_match_1x1_backward_workspace_bytes(1, 32, 6, 10, 4, 64, 64, 32) == 170240
    # on-the-fly lookup at corr_fs_b2_c16_16x24_nonfinite (4 levels), every compute mode
    assert L.rmd_corr_otf_workspace_bytes(2, 16, 16, 24, 4, x3) == 335616
    assert L.rmd_corr_otf_workspace_bytes(2, 16, 16, 24, 4, bf16) == 175872
    assert L.rmd_corr_otf_workspace_bytes(2, 16, 16, 24, 4, f32) == 335616
    # its backward at corr_fs_bwd_b1_c48_21x35_l3r3 (3 levels, radius 3)
    assert L.rmd_corr_otf_record_bytes(1, 21, 35, 3, 3) == 582400
    assert L.rmd_corr_otf_backward_workspace_bytes(1, 48, 21, 35, 3, x3) == 1163520
    assert L.rmd_corr_otf_backward_workspace_bytes(1, 48, 21, 35, 3, bf16) == 854272
    # the warped DICL volume at warp_dicl_cost_b2_c16_10x12
    assert L.rmd_dicl_stack_int_warped_workspace_bytes(2, 16, 10, 12) == 15872
    # the host code that moved out of dicl.hip with its operators (dicl_int.hip, dap.hip): the unwarped volume
    # at the same shape, the DAP weight gradient at D = 81 on a few pixels and at the 'full' D = 324 of cfg4
    assert L.rmd_dicl_stack_int_workspace_bytes(2, 10, 12) == 240
    assert L.rmd_dap_weight_grad_workspace_bytes(2, 81, 120) == 147456
    assert L.rmd_dap_weight_grad_workspace_bytes(8, 324, 7680) == 11894784
