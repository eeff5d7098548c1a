"""Host side of the fp32-staging correlation GEMM's C ABI (include/rmd.h: rmd_corr_pyramid_fused and its two halves
rmd_corr_prepare_queries / rmd_corr_pyramid_staged): the symbols exist, null pointers and descriptors of another GEMM
return RMD_ERR_ARG before anything is launched, and the fused entry sends a call the w8 GEMM does not serve down
rmd_corr_pyramid's own two halves.  The results are compared on the GPU in test_gpu_w8_stage_f32.py."""

import ctypes

import pytest
import torch

from rmd import _lib

ERR_ARG, ERR_LAUNCH = -1, -3
P = ctypes.c_void_p
# (channels, storage, compute) of calls the w8 GEMM does not serve, and the GEMM that does
OTHER_GEMMS = [(256, _lib.RMD_F32, _lib.RMD_BF16, b"tiled"),        # fp32 storage
               (320, _lib.RMD_F16, _lib.RMD_BF16, b"tiled"),        # C > 256
               (256, _lib.RMD_F32, _lib.RMD_BF16X3, b"x3")]


def _desc(c, storage, compute, b=1, h=8, w=8, levels=2):
    return _lib.describe_for(b, h, w, levels, storage, c, compute)


def _err():
    return _lib.lib().rmd_last_error().decode()


def test_symbols_exist_and_are_bound():
    lib = _lib.lib()
    for name in ("rmd_corr_pyramid_fused", "rmd_corr_prepare_queries", "rmd_corr_pyramid_staged"):
        assert hasattr(lib, name) and name in _lib.symbols()
    # the legacy halves stay: they are the oracle of the new path
    for name in ("rmd_corr_pyramid", "rmd_corr_prepare", "rmd_corr_pyramid_prepared"):
        assert hasattr(lib, name)


def test_workspace_size_is_unchanged_by_the_new_path():
    """The describe functions report the legacy path's workspace (both operands): it must still fit there."""
    d = _desc(256, _lib.RMD_F16, _lib.RMD_BF16, b=8, h=55, w=128, levels=4)
    n = 55 * 128
    assert _lib.lib().rmd_corr_pyramid_workspace_bytes(ctypes.byref(d), 256, _lib.RMD_BF16) == 8 * 2 * n * 256 * 2 + 32 * 1024


@pytest.mark.parametrize("missing", range(4))
def test_fused_rejects_null_pointers(missing):
    d = _desc(256, _lib.RMD_F16, _lib.RMD_BF16)
    ptrs = [P(16)] * 4                      # fmap1, fmap2, pyramid, workspace: never dereferenced
    ptrs[missing] = None
    rc = _lib.lib().rmd_corr_pyramid_fused(ptrs[0], ptrs[1], 256, 0.0625, ctypes.byref(d), _lib.RMD_BF16, ptrs[2], ptrs[3],
                                           None)
    assert rc == ERR_ARG and "rmd_corr_pyramid_fused: null pointer" in _err()


def test_halves_reject_null_pointers_and_null_desc():
    lib = _lib.lib()
    d = _desc(256, _lib.RMD_F16, _lib.RMD_BF16)
    for args in ((None, P(16)), (P(16), None)):
        assert lib.rmd_corr_prepare_queries(args[0], 256, ctypes.byref(d), _lib.RMD_BF16, args[1], None) == ERR_ARG
        assert "rmd_corr_prepare_queries: null pointer" in _err()
    for args in ((None, P(16), P(16)), (P(16), None, P(16)), (P(16), P(16), None)):
        assert lib.rmd_corr_pyramid_staged(args[0], 256, 0.0625, ctypes.byref(d), _lib.RMD_BF16, args[1], args[2],
                                           None) == ERR_ARG
        assert "rmd_corr_pyramid_staged: null pointer" in _err()
    assert lib.rmd_corr_prepare_queries(P(16), 256, None, _lib.RMD_BF16, P(16), None) == ERR_ARG
    assert lib.rmd_corr_pyramid_staged(P(16), 256, 0.0625, None, _lib.RMD_BF16, P(16), P(16), None) == ERR_ARG
    assert lib.rmd_corr_pyramid_fused(P(16), P(16), 256, 0.0625, None, _lib.RMD_BF16, P(16), P(16), None) == ERR_ARG


@pytest.mark.parametrize("c,storage,compute,kernel", OTHER_GEMMS)
def test_halves_reject_descriptors_of_another_gemm(c, storage, compute, kernel):
    lib = _lib.lib()
    d = _desc(c, storage, compute)
    assert lib.rmd_corr_gemm_kernel(ctypes.byref(d), c, compute) == kernel
    assert lib.rmd_corr_prepare_queries(P(16), c, ctypes.byref(d), compute, P(16), None) == ERR_ARG
    assert "the w8 GEMM only" in _err()
    assert lib.rmd_corr_pyramid_staged(P(16), c, 0.0625, ctypes.byref(d), compute, P(16), P(16), None) == ERR_ARG
    assert "the w8 GEMM only" in _err()


def test_halves_check_the_descriptor_like_rmd_corr_pyramid():
    lib = _lib.lib()
    rows = _lib.describe(1, 8, 8, 2, _lib.RMD_F16)          # the w8 GEMM writes the tiles layout
    assert lib.rmd_corr_pyramid_fused(P(16), P(16), 256, 0.0625, ctypes.byref(rows), _lib.RMD_BF16, P(16), P(16),
                                      None) == ERR_ARG
    assert "layout" in _err()
    d = _desc(256, _lib.RMD_F16, _lib.RMD_BF16)
    assert lib.rmd_corr_prepare_queries(P(16), 0, ctypes.byref(d), _lib.RMD_BF16, P(16), None) == -2     # RMD_ERR_SHAPE
    assert lib.rmd_corr_pyramid_staged(P(16), 256, 0.0625, ctypes.byref(d), 7, P(16), P(16), None) == ERR_ARG


@pytest.mark.parametrize("c,storage,compute,kernel", OTHER_GEMMS)
def test_fused_takes_the_legacy_route_off_the_w8_gemm(c, storage, compute, kernel):
    """Without a GPU the first launcher the call reaches fails with RMD_ERR_LAUNCH and names itself: rmd_corr_prepare's,
    not rmd_corr_prepare_queries'.  With one, the call runs and gives rmd_corr_pyramid's pyramid bit for bit."""
    lib = _lib.lib()
    if not torch.cuda.is_available():
        d = _desc(c, storage, compute)
        rc = lib.rmd_corr_pyramid_fused(P(16), P(16), c, 0.0625, ctypes.byref(d), compute, P(16), P(16), None)
        assert rc == ERR_LAUNCH and _err().startswith("rmd_corr_prepare") and "queries" not in _err()
        w8 = _desc(256, _lib.RMD_F16, _lib.RMD_BF16)
        rc = lib.rmd_corr_pyramid_fused(P(16), P(16), 256, 0.0625, ctypes.byref(w8), _lib.RMD_BF16, P(16), P(16), None)
        assert rc == ERR_LAUNCH and _err().startswith("rmd_corr_prepare_queries")
        return
    from rmd import library
    g = torch.Generator().manual_seed(5)
    f1, f2 = (torch.randn(1, c, 8, 8, generator=g).cuda() for _ in range(2))
    got = []
    for entry in ("rmd_corr_pyramid_fused", "rmd_corr_pyramid"):
        d, data, ws = library.pyramid_buffers(f1, 2, compute, storage)
        data.zero_()
        _lib.launch(entry, f1, f1, f2, c, 0.0625, ctypes.byref(d), compute, data, ws)
        got.append(data)
    assert torch.equal(got[0].view(torch.uint8), got[1].view(torch.uint8))
