"""Inputs and digests of the dicl-1x1 match kernels' bit-exactness cases: tests/test_gpu_dicl_match_digest.py
compares against tests/golden/match_digests.json, which tools/dicl_match_digests.py --record wrote from the
build before csrc/dicl_match.hip and csrc/dicl_match_grad.hip came to share csrc/dicl_match_common.h.

Shapes: dicl_match_cases.SWEEP (EXACT, guarded 2/2/2/1, guarded 4/4/4/4 with the weights in LDS, a strip
remainder, dsplit > 1, 2C = 128), WIDEST (weights from global memory) and dicl_match_grad_cases.MORE_THAN_GRID
(the fixed-order reduction over a full grid).  Nothing larger.

Inputs are dyadic rationals from integer draws, so they do not depend on a normal-variate algorithm: features
and grad_cost integers / 32, weights integers / 64 divided by the power of two at or above 0.5 sqrt(fan-in),
biases integers / 32 in [0.1875, 1.25] — hidden pre-activations are then of order 1 and mostly positive, so
that few units are masked (MASKED_CAP, asserted on the CPU emulation by the test that needs no GPU) and a
changed bit anywhere reaches the outputs.  Coordinates: the pixel grid plus integers / 8, with hand-placed
positions (off every border, far away, one NaN and one inf coordinate).

A NaN sample makes gW2, gW3, gw4 and the f2 half of gW1 NaN whatever grad_cost is, so the backward is
digested a third time on `finite_coords` (the two non-finite positions moved onto the map).

Outputs of one case (OUTPUT_NAMES): the forward in both computes, the training forward, and every
deterministic backward output (dicl_match_grad_cases.DETERMINISTIC: grad_fmap2 is float atomics) with all
gradients requested, with the parameter gradients off, and on the finite coordinates.
"""
import functools
import hashlib
import zlib

import numpy as np

import dicl_match_cases as fwd
import dicl_match_grad_cases as grad

CASES = fwd.SWEEP + [fwd.WIDEST, grad.MORE_THAN_GRID]
MASKED_CAP = 0.10
WIDTH_STEP = 32          # the kernels take hidden widths in whole 32-row MFMA tiles (rmd.ops pads the same way)

OUTPUT_NAMES = (("fwd.bf16x3", "fwd.bf16", "train")
                + tuple(f"bwd.{n}" for n in grad.DETERMINISTIC)
                + ("bwd_noparams.grad_fmap1",)
                + tuple(f"bwd_finite.{n}" for n in grad.DETERMINISTIC))


def case_id(shape):
    b, c, h, w, r, widths = shape
    return f"b{b}-c{c}-{h}x{w}-r{r}-" + "x".join(str(v) for v in widths)


def _pow2_at_least(v):
    return 2.0 ** int(np.ceil(np.log2(v)))


def special_points(h, w):
    """(x, y): off each of the four borders (half a pixel, and further than the radius), far away, then the
    NaN and the inf coordinate (the last two: `finite_coords` replaces them)."""
    return [(-0.5, h / 2 + 0.125), (w - 0.5, h / 2 - 0.375), (w / 2 + 0.75, -0.75), (w / 2 - 0.25, h - 0.25),
            (-6.5, 1.0), (w + 5.25, 0.5), (1.0, -7.125), (0.5, h + 6.0),
            (1.0e7, -1.0e7), (float("nan"), 1.0), (1.5, float("inf"))]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(f1, f2, coords, radius, weights, biases, grad_cost) as float32 numpy; shared, never modified."""
    b, c, h, w, r, widths = shape
    rng = np.random.default_rng(zlib.crc32(("digest" + repr(shape)).encode()))
    f1 = (rng.integers(-64, 65, (b, c, h, w)) / 32.0).astype(np.float32)
    f2 = (rng.integers(-64, 65, (b, c, h, w)) / 32.0).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    co = np.stack([xs, ys])[None].repeat(b, 0).astype(np.float64)
    co += rng.integers(-24, 25, (b, 2, h, w)) / 8.0
    pix = co.transpose(0, 2, 3, 1).reshape(b * h * w, 2)             # a copy, (pixel, xy)
    pts = special_points(h, w)
    # spread over all images, at distinct pixels (the smallest case has 12)
    where = (np.arange(len(pts))[::-1] * max(1, (b * h * w) // len(pts)) + 1) % (b * h * w)
    assert len(set(where)) == len(pts)
    for k, pt in zip(where, pts):
        pix[k] = pt
    co = pix.reshape(b, h, w, 2).transpose(0, 3, 1, 2)
    weights, biases, cin = [], [], 2 * c
    for cout in widths + (1,):
        div = 64.0 * _pow2_at_least(0.5 * np.sqrt(cin))
        weights.append((rng.integers(-32, 33, (cout, cin)) / div).astype(np.float32))
        biases.append((rng.integers(6, 41, cout) / 32.0).astype(np.float32))
        cin = cout
    weights[3] = weights[3].reshape(-1)
    d = 2 * r + 1
    g = (rng.integers(-64, 65, (b, d, d, h, w)) / 32.0).astype(np.float32)
    return f1, f2, np.ascontiguousarray(co, dtype=np.float32), r, weights, biases, g


@functools.lru_cache(maxsize=None)
def finite_coords(shape):
    """inputs(shape)'s coordinates with the non-finite positions moved to the middle of the map."""
    _, _, h, w, _, _ = shape
    co = inputs(shape)[2].copy()
    bad = ~np.isfinite(co).all(axis=1)
    assert bad.sum() == 2
    co[:, 0][bad], co[:, 1][bad] = w / 2 + 0.375, h / 2 - 0.125
    return co


def padded(weights, biases):
    """Zero rows, and the matching zero columns of the next layer, up to whole 32-row tiles."""
    ws = [np.asarray(v).reshape(v.shape[0], -1) for v in weights[:3]] + [np.asarray(weights[3]).reshape(1, -1)]
    ts = [np.asarray(t).reshape(-1) for t in biases]
    for i in range(3):
        extra = -ws[i].shape[0] % WIDTH_STEP
        ws[i] = np.pad(ws[i], ((0, extra), (0, 0)))
        ts[i] = np.pad(ts[i], (0, extra))
        ws[i + 1] = np.pad(ws[i + 1], ((0, 0), (0, extra)))
    return ws[:3] + [ws[3].reshape(-1)], ts


def masked_fraction(shape):
    """Share of the (real, unpadded) hidden units that the CPU emulation of the three-product forward
    masks to zero, over every column of the case; a NaN unit is not masked."""
    f1, f2, co, r, weights, biases, _ = inputs(shape)
    x, _ = fwd._columns(f1, f2, co, r)
    _, acts = grad.forward_emulated(x, weights, biases)
    zero = sum(int((a == 0).sum()) for a in acts[1:])
    return zero / sum(a.size for a in acts[1:])


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(shape, device):
    """{output name: sha256 of the output's bytes} of one case, through the torch operators."""
    import torch

    import rmd  # noqa: F401
    from rmd import _lib
    f1, f2, co, r, weights, biases, g = inputs(shape)
    ws, ts = padded(weights, biases)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tf1, tf2, tco, tg = t(f1), t(f2), t(co), t(g)
    tws, tts = [t(v) for v in ws], [t(v) for v in ts]
    out = {"fwd.bf16x3": _sha(torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco, r, tws, tts, _lib.RMD_BF16X3)),
           "fwd.bf16": _sha(torch.ops.rmd.dicl_match_1x1(tf1, tf2, tco, r, tws, tts, _lib.RMD_BF16)),
           "train": _sha(torch.ops.rmd.dicl_match_1x1_train(tf1, tf2, tco, r, tws, tts))}
    for tag, coords, needs in (("bwd", tco, [True, True, True]), ("bwd_noparams", tco, [True, True, False]),
                               ("bwd_finite", t(finite_coords(shape)), [True, True, True])):
        got = torch.ops.rmd.dicl_match_1x1_backward(tg, tf1, tf2, coords, r, tws, tts, needs)
        for name, val in zip(grad.OUTPUTS, got):
            if f"{tag}.{name}" in OUTPUT_NAMES:
                out[f"{tag}.{name}"] = _sha(val)
    assert sorted(out) == sorted(OUTPUT_NAMES)
    return out
