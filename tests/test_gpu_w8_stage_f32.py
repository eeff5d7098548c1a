"""The fp32-staging correlation GEMM (rmd_corr_pyramid_fused: prep_queries + corr_pyramid_w8_f32, which builds its
A tiles in LDS from fmap2 itself) against the two-call ABI it replaces on the operator's path (rmd_corr_prepare +
rmd_corr_pyramid_prepared: prep_pair + corr_pyramid_w8 reading the bf16 A operand from the workspace).

The legacy path stays in the library and is the oracle: both pyramids are written into buffers pre-filled with the
same pattern and must be equal bit for bit over the raw storage (so is every byte neither path writes), and so
must one lookup of each.  No tolerance is involved.  Shapes are the smallest at which each branch of the staging can go
wrong; channels pad to 256 in all of them (the w8 GEMM's condition).
"""

import ctypes

import pytest
import torch

from rmd import _lib, library, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
COMPUTE, STORAGE, LEVELS, RADIUS = _lib.RMD_BF16, _lib.RMD_F16, 4, 3

# (id, B, C, H, W, scale, plant non-finite values)
CASES = [
    ("24x32_b2_paired", 2, 256, 24, 32, None, False),       # paired last block row of 8 rows, second image's offsets
    ("18x32_b2_paired", 2, 256, 18, 32, None, False),       # paired last block row of 2 rows
    ("20x48_unpaired", 1, 256, 20, 48, None, False),        # odd column-block count, last block row of 4 rows
    ("13x22_scalar", 1, 256, 13, 22, None, False),          # W % 4 != 0: scalar loads, slots of no pixel, odd H
    ("20x48_c250", 1, 250, 20, 48, None, False),            # channels no multiple of 8, zero-filled padding
    ("13x22_c250_scalar", 1, 250, 13, 22, None, False),     # the same on the scalar path
    ("18x32_scale0.3", 2, 256, 18, 32, 0.3, False),         # a scale that is no power of two, folded before rounding
    ("24x32_nonfinite", 2, 256, 24, 32, None, True),        # NaN and +-inf in fmap2
    ("20x48_nonfinite_c250_neg", 1, 250, 20, 48, -0.17, True),   # ... and a negative scale (-0 in the padding)
]


def _inputs(b, c, h, w, nonfinite):
    g = torch.Generator().manual_seed(1000 * h + w + c)
    f1 = torch.randn(b, c, h, w, generator=g)
    f2 = torch.randn(b, c, h, w, generator=g)
    if nonfinite:
        flat = f2.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:48]
        flat[idx[:16]] = float("nan")
        flat[idx[16:32]] = float("inf")
        flat[idx[32:]] = float("-inf")
        f2[-1, c - 1, h - 1, w - 1] = float("nan")          # the last element the staging reads
        f2[0, 0, 0, 0] = float("-inf")
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coords = torch.stack([xs, ys])[None] + 2.5 * torch.randn(b, 2, h, w, generator=g)
    return f1.to(DEV), f2.to(DEV), coords.to(DEV)


def _pyramid(f1, f2, scale, fused):
    """(desc, raw pyramid) through the fused entry or the legacy two calls, into a pre-filled buffer"""
    c = f1.shape[1]
    d, data, ws = library.pyramid_buffers(f1, LEVELS, COMPUTE, STORAGE)
    assert _lib.lib().rmd_corr_gemm_kernel(ctypes.byref(d), c, COMPUTE) == b"w8" and d.layout == _lib.RMD_LAYOUT_TILES
    data.view(torch.int16).fill_(0x5a5a)
    ws.fill_(0xa5)
    if fused:
        _lib.launch("rmd_corr_pyramid_fused", f1, f1, f2, c, scale, ctypes.byref(d), COMPUTE, data, ws)
    else:
        _lib.launch("rmd_corr_prepare", f1, f1, f2, c, scale, ctypes.byref(d), COMPUTE, ws)
        _lib.launch("rmd_corr_pyramid_prepared", f1, c, scale, ctypes.byref(d), COMPUTE, data, ws)
    return d, data


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_pyramid_and_lookup_equal_the_legacy_path_bit_for_bit(case):
    _, b, c, h, w, scale, nonfinite = case
    f1, f2, coords = _inputs(b, c, h, w, nonfinite)
    scale = 1.0 / c ** 0.5 if scale is None else scale
    d_new, new = _pyramid(f1, f2, scale, fused=True)
    d_old, old = _pyramid(f1, f2, scale, fused=False)
    torch.cuda.synchronize()
    assert new.shape == old.shape and new.dtype == old.dtype == torch.float16
    assert torch.equal(_bits(new), _bits(old))
    if nonfinite:
        assert bool(torch.isnan(old).any()) and bool(torch.isinf(old).any())      # the planted values reached the pyramid
    else:
        assert bool(torch.isfinite(old).all())
    # the hand-off: one lookup of each pyramid, and of the operator's and the timed split form's (which run the new path)
    look_old = ops.corr_lookup(ops.Pyramid(old, d_old, c, scale), coords, RADIUS)
    look_new = ops.corr_lookup(ops.Pyramid(new, d_new, c, scale), coords, RADIUS)
    look_op = ops.corr_lookup(ops.corr_pyramid(f1, f2, LEVELS, "bf16", scale=scale), coords, RADIUS)
    events = []
    look_split = ops.corr_lookup(ops.corr_pyramid(f1, f2, LEVELS, "bf16", events=events, scale=scale), coords, RADIUS)
    torch.cuda.synchronize()
    assert len(events) == 1 and events[0][0].elapsed_time(events[0][1]) > 0
    for got in (look_new, look_op, look_split):
        assert got.shape == look_old.shape == (b, LEVELS * (2 * RADIUS + 1) ** 2, h, w)
        assert torch.equal(_bits(got), _bits(look_old))


@pytest.mark.parametrize("c,storage,compute", [(256, _lib.RMD_F32, _lib.RMD_BF16), (320, _lib.RMD_F16, _lib.RMD_BF16),
                                               (256, _lib.RMD_F32, _lib.RMD_BF16X3)],
                         ids=["f32_storage", "c320", "bf16x3"])
def test_fused_entry_off_the_w8_gemm_is_rmd_corr_pyramid(c, storage, compute):
    g = torch.Generator().manual_seed(c + storage)
    f1, f2 = (torch.randn(2, c, 18, 32, generator=g).to(DEV) for _ in range(2))
    got = []
    for entry in ("rmd_corr_pyramid_fused", "rmd_corr_pyramid"):
        d, data, ws = library.pyramid_buffers(f1, LEVELS, compute, storage)
        assert _lib.lib().rmd_corr_gemm_kernel(ctypes.byref(d), c, compute) != b"w8"
        data.zero_()
        _lib.launch(entry, f1, f1, f2, c, 0.0625, ctypes.byref(d), compute, data, ws)
        got.append(data)
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.uint8), got[1].view(torch.uint8))
