"""Inputs and digests of the lookup bit-exactness cases: tests/test_gpu_lookup_digest.py compares against
tests/golden/lookup_digests.json, which tools/lookup_digests.py --record writes from a known-good build.

Every case is batch 2, 16 real channels, 4 levels, on a 16 x 24 map (levels 16x24, 8x12, 4x6, 2x3) or
a 15 x 20 map (15x20, 7x10, 3x5, 1x2: an odd last chunk row and a 1-pixel level).  Pyramid kinds:

  bf16-tiles  fp16 tiles layout (the w8 GEMM: the 16 channels zero-padded to 256, scale 1/sqrt(16) —
              the w8 GEMM, which alone writes the tiles layout, takes 193..256 channels)
  bf16-rows   fp16 row layout (the tiled GEMM at 16 channels)
  fp32        S24 rows (the x3 GEMM)
  fp32-f32    f32 rows (the x3 GEMM)

Inputs are dyadic rationals from integer draws, so they do not depend on a normal-variate algorithm.
"""
import hashlib
from functools import lru_cache

import numpy as np

BATCH, CHANNELS, LEVELS = 2, 16, 4
SHAPES = ((16, 24), (15, 20))
RADII = (1, 3, 4, 8)
KINDS = ("bf16-tiles", "bf16-rows", "fp32", "fp32-f32")
_PRECISION = {"bf16-tiles": "bf16", "bf16-rows": "bf16", "fp32": "fp32", "fp32-f32": "fp32-f32"}
# kind -> (storage dtype name, tiles layout?) the case must really exercise
EXPECT = {"bf16-tiles": ("float16", True), "bf16-rows": ("float16", False), "fp32": ("uint8", False),
          "fp32-f32": ("float32", False)}


def case_id(kind, radius, shape):
    return f"{kind}-r{radius}-{shape[0]}x{shape[1]}"


def all_cases():
    return [(k, r, s) for k in KINDS for r in RADII for s in SHAPES]


@lru_cache(maxsize=None)
def features(shape):
    h, w = shape
    rng = np.random.default_rng(1000 * h + w)
    f1 = (rng.integers(-64, 65, (BATCH, CHANNELS, h, w)) / 32.0).astype(np.float32)
    f2 = (rng.integers(-64, 65, (BATCH, CHANNELS, h, w)) / 32.0).astype(np.float32)
    return f1, f2


def special_points(h, w):
    """(x, y) of the hand-placed queries: inside, the four edges, off the map, every (quad phase, row
    parity) of levels 0 and 1, and the non-finite ones."""
    pts = [(w / 2 + 0.25, h / 2 + 0.5)]
    pts += [(-0.5, h / 2 + 0.125), (w - 0.5, h / 2 - 0.375), (w / 2 + 0.75, -0.75), (w / 2 - 0.25, h - 0.25)]
    pts += [(-1.0, -1.0), (w - 1.0, h - 1.0), (0.0, 0.0), (w - 1.0, 0.0)]           # integer coordinates, corners
    pts += [(-100.0, 5.0), (1000.0, 5.0), (5.0, -100.0), (5.0, 1000.0), (1.0e7, -1.0e7), (-3.0e9, 2.0), (2.0, 3.0e38)]
    pts += [(sx + 0.375, sy + 0.625) for sy in range(4, 8) for sx in range(4, 12)]  # xs mod 8, ys mod 4
    pts += [(float("nan"), 3.0), (4.0, float("inf")), (float("-inf"), 2.5), (float("nan"), float("inf"))]
    return pts


@lru_cache(maxsize=None)
def coords(shape):
    h, w = shape
    rng = np.random.default_rng(77 * h + w)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    co = np.stack([xs, ys])[None].repeat(BATCH, 0).astype(np.float64)
    co[0] += rng.integers(-24, 25, (2, h, w)) / 8.0            # a few pixels: inside and edge windows
    co[1] += rng.integers(-160, 161, (2, h, w)) / 8.0          # up to 20 pixels: edge and off-map windows
    flat = co.reshape(BATCH, 2, h * w)
    pts = special_points(h, w)
    # spread the special queries over image 0 (stride 5: several waves, both query rows of a tile)
    for i, (x, y) in enumerate(pts):
        k = (5 * i) % (h * w)
        flat[0, 0, k], flat[0, 1, k] = x, y
    return co.astype(np.float32)


def phase_coverage(shape, radius):
    """{(level, xs mod 4, ys mod 2)} over the finite queries of `coords(shape)`, levels 0 and 1."""
    co = coords(shape).astype(np.float64)
    seen = set()
    for lvl in (0, 1):
        x, y = co[:, 0] / 2 ** lvl, co[:, 1] / 2 ** lvl
        ok = np.isfinite(x) & np.isfinite(y) & (np.abs(x) < 1e6) & (np.abs(y) < 1e6)
        xs = np.floor(x[ok]).astype(np.int64) - radius
        ys = np.floor(y[ok]).astype(np.int64) - radius
        seen |= {(lvl, int(a), int(b)) for a, b in zip(xs % 4, ys % 2)}
    return seen


def build_pyramid(kind, shape, device):
    import torch

    from rmd import ops
    f1, f2 = (torch.from_numpy(f).to(device) for f in features(shape))
    scale = 1.0 / float(CHANNELS) ** 0.5
    if kind == "bf16-tiles":
        pad = (0, 0, 0, 0, 0, 256 - CHANNELS)
        f1, f2 = torch.nn.functional.pad(f1, pad), torch.nn.functional.pad(f2, pad)
    return ops.corr_pyramid(f1.contiguous(), f2.contiguous(), LEVELS, _PRECISION[kind], scale=scale)


def digest(pyr, shape, radius, device):
    """sha256 of the lookup's output bytes, and of the same lookup with level 1 masked."""
    import torch

    from rmd import ops
    co = torch.from_numpy(coords(shape)).to(device)
    h = hashlib.sha256()
    h.update(ops.corr_lookup(pyr, co, radius).cpu().numpy().tobytes())
    h.update(ops.corr_lookup(pyr, co, radius, mask_costs=[4]).cpu().numpy().tobytes())    # cost level 4 = level 1
    return h.hexdigest()
