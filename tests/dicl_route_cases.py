"""Shared table of test_dicl_routes.py / test_gpu_dicl_routes.py: one small shape per kernel route of
rmd_dicl_stack / rmd_dicl_stack_backward, with the route each shape must take, and the inputs the
GPU parity tests feed them (built once per process and never modified).

The expected routes restate the dispatch rule of csrc/dicl_stack.h by hand (radius, grid scale
sx = (wl-1)/(nw-1), sy = (hl-1)/(nh-1), LDS window estimate against 4096 / 12288 floats, stack size);
they were not read back from the library.  A row whose route moves (a retuned window threshold, a
new kernel) fails test_dicl_routes.py: move the shape so the route stays covered.

Names (include/rmd.h, rmd_dicl_stack_kernel): forward patch/R, separable/R/K, general; backward
patch2/R/small|large, patch1/R/small|large, separable2/K/small|large, separable1/10/small|large,
general/small|large, fallback.
"""

import functools
from typing import NamedTuple

import numpy as np
import torch


class Row(NamedTuple):
    h: int
    w: int
    hl: int
    wl: int
    nh: int
    nw: int
    level: int
    r: int
    fwd: str
    bwd: str
    b: int = 2
    c: int = 3
    extra: bool = False
    lattice: bool = False        # coordinates on a 2^-6 lattice: sample positions exact in fp32 (wide maps)

    @property
    def id(self):
        s = f"{self.h}x{self.w}"
        if (self.hl, self.wl, self.nh, self.nw) != (self.h, self.w, self.h, self.w):
            s += f"-l{self.hl}x{self.wl}-n{self.nh}x{self.nw}"
        return s + f"-r{self.r}" + ("-extra" if self.extra else "")

    @property
    def args(self):
        """(batch, channels, height, width, level_height, level_width, radius, level, norm_height,
        norm_width, extra_delta): the integer arguments of the C calls, in their order."""
        return (self.b, self.c, self.h, self.w, self.hl, self.wl, self.r, self.level, self.nh, self.nw,
                int(self.extra))


def _same(h, w, r, fwd, bwd, **kw):
    return Row(h, w, h, w, h, w, 0, r, fwd, bwd, **kw)


ROWS = (
    # unit steps, small window: the one-pixel forward patch kernels and the two-pixel backward
    [_same(18, 30, r, f"patch/{r}", f"patch2/{r}/small") for r in (1, 2, 3, 4)]
    # r = 0 and r > 4 at unit steps: the general forward; r = 0 fits the K = 4 separable backward
    + [_same(18, 30, 0, "general", "separable2/4/small"),
       _same(18, 30, 5, "general", "general/small", extra=True)]
    # odd widths: the two-pixel backward pairs the last pixel of a row with the first of the next
    + [_same(h, w, r, f"patch/{r}", f"patch2/{r}/small") for h, w in ((12, 21), (8, 13)) for r in (4, 2)]
    # unit steps, 48 KiB window (w >= 200 at r = 4)
    + [_same(4, 304, r, f"patch/{r}", f"patch2/{r}/large", lattice=True) for r in (1, 2, 3, 4)]
    + [_same(4, 304, 6, "general", "general/large", lattice=True)]
    # either side of the window threshold, so that a retuned kWinSmall or row estimate fails the routing test:
    # two pixels per lane at r = 4, (2r + 512/w + 10) w = 18 w + 512 <= 4096 up to w = 199; one pixel per lane
    # at r = 5, (2r + 256/w + 10) w = 20 w + 256 <= 4096 up to w = 192
    + [_same(4, 199, 4, "patch/4", "patch2/4/small", lattice=True),
       _same(4, 200, 4, "patch/4", "patch2/4/large", lattice=True),
       _same(4, 191, 5, "general", "general/small", lattice=True),
       _same(4, 193, 5, "general", "general/large", lattice=True)]
    # scaled grids (raft_dicl_ml levels): K = 4 (1/8), K = 6 (1/2), K = 8 (ceil(w/2) at odd w: scale 0.5
    # exactly; 0.75 at r = 3), K = 10 (one pixel per lane backward, general forward)
    + [Row(24, 40, 3, 5, 24, 40, 3, r, f"separable/{r}/4", "separable2/4/small") for r in (3, 4)]
    + [Row(12, 20, 6, 10, 12, 20, 1, r, f"separable/{r}/6", "separable2/6/small") for r in (3, 4)]
    + [Row(12, 20, 6, 10, 12, 20, 1, r, "general", "separable2/4/small") for r in (1, 2)]
    + [Row(12, 21, 6, 11, 12, 21, 1, 4, "separable/4/8", "separable2/8/small"),
       Row(12, 21, 9, 16, 12, 21, 0, 3, "separable/3/8", "separable2/8/small"),
       Row(12, 21, 10, 17, 12, 21, 0, 4, "general", "separable1/10/small")]
    # scaled grids, 48 KiB window; dyadic scales (0.375 / 0.25, 0.5, 0.25, 0.75)
    + [Row(4, 641, 4, 241, 13, 641, 0, 4, "separable/4/6", "separable2/6/large", lattice=True),
       Row(4, 641, 4, 321, 7, 641, 0, 4, "separable/4/8", "separable2/8/large", lattice=True),
       Row(4, 1041, 4, 261, 13, 1041, 0, 3, "separable/3/4", "separable2/4/large", lattice=True),
       Row(4, 321, 4, 241, 5, 321, 0, 4, "general", "separable1/10/large", lattice=True)]
    # sy = 1 with sx < 1 (K = 12: no separable kernel), and a scale above 1
    + [Row(12, 20, 12, 10, 12, 20, 0, 4, "general", "general/small"),
       Row(12, 20, 24, 40, 12, 20, 0, 2, "general", "general/small")]
    # the last resort: sx = inf, sx = NaN (1-pixel normalisation maps), a level wider than the 48 KiB window
    + [Row(4, 8, 4, 8, 4, 1, 0, 2, "general", "fallback"),
       Row(4, 1, 4, 1, 4, 1, 0, 2, "general", "fallback"),
       _same(2, 12292, 5, "general", "fallback", b=1, c=1, lattice=True)]
)
assert len({r.id for r in ROWS}) == len(ROWS)

# rows whose grid scale is not finite: the whole f2 half is NaN, grad_fmap2 is zero
NONFINITE_SCALE = [r for r in ROWS if r.nw == 1]

# Routes no row reaches, written out: the one-pixel-per-lane unit-step backward serves stacks of
# >= 4 GiB per image only (32-bit lane offsets end there), which is no small shape.  It stays untested.
EXEMPT_BACKWARD = {f"patch1/{r}/{win}" for r in (1, 2, 3, 4) for win in ("small", "large")}
EXEMPT_FORWARD = set()

# shapes of the non-finite coordinate test: one per forward family (patch, separable, general)
NONFINITE_COORD_IDS = ("18x30-r4", "12x20-l6x10-n12x20-r4", "18x30-r5-extra")
# (batch, y, x, component, value) planted into single coordinates
NONFINITE_COORDS = ((0, 3, 5, 0, np.nan), (0, 7, 11, 1, np.inf), (1, 2, 9, 0, -np.inf), (1, 9, 18, 1, np.nan),
                    (0, 10, 2, 0, 3e9), (1, 5, 14, 1, -1e30), (1, 11, 19, 0, np.inf))
HUGE_FINITE = tuple(p for p in NONFINITE_COORDS if np.isfinite(p[4]))


def row(row_id):
    return next(r for r in ROWS if r.id == row_id)


def query(lib, r, backward):
    return lib.rmd_dicl_stack_kernel(*r.args, int(backward)).decode()


def flow_fields(r, rng):
    """(B, 2, h, w) float64: image 0 a smooth field (a constant plus a slow ramp: neighbouring windows start
    at consecutive columns, so the backward's merges and chains happen; at an odd width a pair that
    straddles a row end sits next to merged ones), the last image a graded field (low-resolution noise
    upsampled: window origins step by 0, 1 or 2 columns and change rows), and a pixel block of +-40 whose
    windows leave the map."""
    ys, xs = np.meshgrid(np.arange(r.h), np.arange(r.w), indexing="ij")
    flow = np.empty((r.b, 2, r.h, r.w))
    flow[:, 0] = 2.3 + 0.01 * xs
    flow[:, 1] = -1.6 + 0.02 * ys
    low = torch.from_numpy(rng.standard_normal((1, 2, max(2, -(-r.h // 8)), max(2, -(-r.w // 8)))) * 3.0)
    flow[-1] += torch.nn.functional.interpolate(low, size=(r.h, r.w), mode="bilinear", align_corners=True)[0].numpy()
    y0, x0 = r.h // 2, min(2, r.w - 1)
    flow[0, 0, y0:y0 + 2, x0:x0 + 5] += 40.0
    flow[-1, 1, :2, r.w // 2:r.w // 2 + 3] -= 40.0
    return flow


class Inputs(NamedTuple):
    f1: np.ndarray           # float32
    f2: np.ndarray
    coords: np.ndarray
    grad: np.ndarray         # upstream gradient of the stack (B, d, d, 2C [+2], h, w)


@functools.lru_cache(maxsize=None)
def inputs(row_id, nonfinite=False):
    r = row(row_id)
    rng = np.random.default_rng(sum(map(ord, row_id)))
    d = 2 * r.r + 1
    f1 = rng.standard_normal((r.b, r.c, r.h, r.w)).astype(np.float32)
    f2 = rng.standard_normal((r.b, r.c, r.hl, r.wl)).astype(np.float32)
    flow = flow_fields(r, rng)
    if r.lattice:
        flow = np.round(flow * 64.0) / 64.0
    ys, xs = np.meshgrid(np.arange(r.h), np.arange(r.w), indexing="ij")
    coords = (np.stack([xs, ys])[None] + flow).astype(np.float32)
    if r.lattice:
        assert np.array_equal(coords.astype(np.float64) * 64.0, np.round(coords.astype(np.float64) * 64.0))
    if nonfinite:
        for b, y, x, k, v in NONFINITE_COORDS:
            coords[b, k, y, x] = v
    grad = rng.standard_normal((r.b, d, d, 2 * r.c + (2 if r.extra else 0), r.h, r.w)).astype(np.float32)
    for a in (f1, f2, coords, grad):
        a.setflags(write=False)
    return Inputs(f1, f2, coords, grad)


class Reference(NamedTuple):
    stack: np.ndarray        # float64 (B, d, d, 2C, h, w): f1 half, f2 half
    grad_f1: np.ndarray
    grad_f2: np.ndarray


@functools.lru_cache(maxsize=None)
def reference(row_id, nonfinite=False):
    """The float64 oracle on inputs(row_id, nonfinite)."""
    import oracle
    r, x = row(row_id), inputs(row_id, nonfinite)
    co = x.coords.astype(np.float64)
    with np.errstate(invalid="ignore"):          # non-finite positions: NaN weights, casts of NaN / inf
        stack = oracle.dicl_stack(x.f1.astype(np.float64), x.f2.astype(np.float64), co, r.r, level=r.level,
                                  norm_hw=(r.nh, r.nw))
        g = x.grad[:, :, :, :2 * r.c].astype(np.float64)
        g1, g2 = oracle.dicl_stack_backward(x.f2.shape, co, r.r, g, level=r.level, norm_hw=(r.nh, r.nw))
    for a in (stack, g1, g2):
        a.setflags(write=False)
    return Reference(stack, g1, g2)


# ---- integer volume (rmd_dicl_stack_int, plain and warped): shapes off the 4-pixel lanes and the 8-channel
# unroll.  (B, C, h, w, ru, rv): widths that are no multiple of 4 (a quad crosses a row end), channel
# tails (C % 8 != 0), ru != rv, a zero radius; |ru| < w and |rv| < h (the reference itself fails beyond).
INT_EDGE_CASES = [(2, 5, 6, 10, 2, 1), (1, 33, 4, 6, 0, 3), (2, 32, 6, 10, 3, 3), (1, 12, 4, 7, 1, 0)]


def int_edge_inputs(b, c, h, w):
    """(rng, fmap1, fmap2) of an integer-volume edge case; fmap2 has a zeroed strip (occlusion holes)."""
    rng = np.random.default_rng(1000 * c + 10 * h + w)
    f1 = rng.standard_normal((b, c, h, w)).astype(np.float32)
    f2 = rng.standard_normal((b, c, h, w)).astype(np.float32)
    f2[:, :, 1:3, 2:5] = 0
    return rng, f1, f2
