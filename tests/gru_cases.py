"""Shared helpers of test_gru.py / test_gpu_gru.py: the fixtures of tests/golden/gen_golden_gru.py (loaded
once per process, never modified), the tests' own float64 restatement of the separable convolutional GRU
(raft.py:228-259), a float64 emulation of the kernel's two compute modes, the tolerance rule, the shapes and
the one-hot closed form.

Restatement: each convolution as five shifted float64 matrix products over a zero-padded map (tap t reads
position p + t - 2), sigmoid and tanh in float64.  Emulation of a compute mode: weights and the staged
[h ; x] / [r.h ; x] maps rounded to fp32 and split into the bfloat16 hi part and the bfloat16 of the
residual, the products the mode keeps (hi.hi, and for three products hi.lo and lo.hi) summed in float64; z,
r.h and h' rounded to fp32, as the kernel stores them.

Tolerance: for each case and mode, e = max|emulation - float64| / max|float64| (CPU only), and the kernel is
gated at max(1e-5, 3 e) max-normalised against float64, as rows f9 / f10.  Nothing here comes from the kernel.
"""

import functools
import zlib

import numpy as np

from conftest import load_golden
from dicl_match_cases import FACTOR, FLOOR, PRODUCTS, split_bf16
from dicl_match_cases import max_norm_err as _max_norm_err

FIXTURE, BLOCK_FIXTURE = "gru_b2_h128_x256_6x10", "gru_block_b1_6x10"
# one NaN in h and one in x.  A NaN reaches +-4 along each axis (z and r read +-2, then q reads r.h at +-2 again): on
# the 7 x 9 map every output is NaN, the 12 x 14 map keeps finite outputs outside the two 9 x 9 squares
NAN_FIXTURES = ("gru_nan_b1_h32_x16_7x9", "gru_nan_b1_h32_x16_12x14")
NAN_REACH = 4
GATES = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")

# (B, Hd, Xd, H, W)
SHAPES = [
    (2, 128, 256, 6, 10),       # the models' widths, both map sides just over 5
    (1, 32, 16, 1, 1),          # every tap but the centre is padding
    (1, 32, 48, 3, 4),          # both sides under 5
    (2, 64, 80, 5, 37),         # a 32-pixel tile plus a remainder of 5; nine k-steps per tap
    (1, 96, 32, 37, 5),         # the same, vertically
    (3, 128, 256, 9, 70),       # two tiles plus a remainder; three images
    (1, 128, 384, 4, 33),       # the largest Hd + Xd
]


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_golden(name)


def max_norm_err(got, ref):
    """dicl_match_cases.max_norm_err (NaN positions identical, then max|got - ref| / max|ref| over the finite
    reference entries); 0 where the reference holds no finite entry."""
    if not np.isfinite(ref).any():
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions differ"
        return 0.0
    return _max_norm_err(got, ref)


def nan_squares(g):
    """(H, W) mask of the outputs a NaN fixture's two NaNs reach."""
    ht, wd = g["h"].shape[2:]
    ys, xs = np.mgrid[:ht, :wd]
    return np.logical_or.reduce([(abs(ys - y) <= NAN_REACH) & (abs(xs - x) <= NAN_REACH)
                                 for _, _, y, x in (g["nan_h"], g["nan_x"])])


def _shift(a, t, axis):
    """a (B, C, H, W) -> the map tap t reads: a at position p + t - 2 along W (axis 0) or H (axis 1), zero outside."""
    d = t - 2
    out = np.zeros_like(a)
    n = a.shape[3 if axis == 0 else 2]
    if abs(d) >= n:
        return out
    src = slice(max(d, 0), n + min(d, 0))
    dst = slice(max(-d, 0), n + min(-d, 0))
    if axis == 0:
        out[:, :, :, dst] = a[:, :, :, src]
    else:
        out[:, :, dst, :] = a[:, :, src, :]
    return out


def conv64(parts, a, bias, axis):
    """sum over the (weight part, map part) pairs of `parts` of the 5-tap convolution, float64.  weight (Hd, C, 1, 5)
    or (Hd, C, 5, 1) -> taps (5, Hd, C)."""
    acc = 0.0
    with np.errstate(all="ignore"):
        for wt, m in parts:
            taps = np.asarray(wt, np.float64).reshape(wt.shape[0], wt.shape[1], 5).transpose(2, 0, 1)
            for t in range(5):
                acc = acc + np.einsum("oc,bchw->bohw", taps[t], _shift(m, t, axis))
    return acc + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)


def _sigmoid(v):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def half64(h, x, weights, biases, axis, products=None):
    """One half-step in float64; products = None: exact, 1 or 3: the emulation of that compute mode (fp32 in, fp32 out)."""
    f32 = (lambda v: v.astype(np.float32).astype(np.float64)) if products else (lambda v: v)

    def conv(g, a):
        if not products:
            return conv64([(weights[g], a)], a, biases[g], axis)
        wh, wl = split_bf16(weights[g])
        ah, al = split_bf16(a.astype(np.float32))
        parts = [(wh, ah)] + ([(wh, al), (wl, ah)] if products == 3 else [])
        return conv64(parts, a, np.asarray(biases[g], np.float32), axis)

    h, x = np.asarray(h, np.float64), np.asarray(x, np.float64)
    hx = np.concatenate([h, x], axis=1)
    z = f32(_sigmoid(conv(0, hx)))
    rh = f32(_sigmoid(conv(1, hx)) * h)
    with np.errstate(all="ignore"):
        q = np.tanh(conv(2, np.concatenate([rh, x], axis=1)))
        return f32((1.0 - z) * h + z * q)


def gru64(h, x, weights, biases, products=None):
    """Both halves: weights / biases in the order z1, r1, q1, z2, r2, q2."""
    h = half64(h, x, weights[:3], biases[:3], 0, products)
    return half64(h, x, weights[3:], biases[3:], 1, products)


def module_params(mod):
    """weights, biases of a SepConvGru in the operator's order, as numpy."""
    return ([getattr(mod, g).weight.detach().cpu().numpy().copy() for g in GATES],
            [getattr(mod, g).bias.detach().cpu().numpy().copy() for g in GATES])


@functools.lru_cache(maxsize=None)
def fixture_params(hd, xd):
    """det_init_fanin parameters of SepConvGru(hd, xd), the generator's own (weights are never stored)."""
    import rmd.raft
    from detinit import det_init_fanin
    return module_params(det_init_fanin(rmd.raft.SepConvGru(hd, xd)))


def _with_tolerances(case):
    h, x, ws, bs = case["args"]
    case["ref"] = gru64(h, x, ws, bs)
    case["ref_half"] = [half64(h, x, ws[:3], bs[:3], 0), half64(h, x, ws[3:], bs[3:], 1)]
    case["e"], case["tol"], case["tol_half"] = {}, {}, {}
    for precision, products in PRODUCTS.items():
        e = max_norm_err(gru64(h, x, ws, bs, products), case["ref"])
        case["e"][precision] = e
        case["tol"][precision] = max(FLOOR, FACTOR * e)
        case["tol_half"][precision] = [
            max(FLOOR, FACTOR * max_norm_err(half64(h, x, ws[3 * a:3 * a + 3], bs[3 * a:3 * a + 3], a, products),
                                             case["ref_half"][a])) for a in (0, 1)]
    return case


@functools.lru_cache(maxsize=None)
def shape_case(shape):
    """Seeded inputs of one shape — h = tanh(N(0, 1)), x = relu(N(0, 1)), He-scaled weights, N(0, 0.1^2) biases —
    with the float64 results (both halves together and each alone), the per-mode emulation error e and the
    tolerances.  Shared; never modified."""
    b, hd, xd, ht, wd = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    h = np.tanh(rng.standard_normal((b, hd, ht, wd))).astype(np.float32)
    x = np.maximum(rng.standard_normal((b, xd, ht, wd)), 0).astype(np.float32)
    c = hd + xd
    ws = [(rng.standard_normal((hd, c, 1, 5) if g < 3 else (hd, c, 5, 1)) * np.sqrt(2.0 / (5 * c))).astype(np.float32)
          for g in range(6)]
    bs = [(rng.standard_normal(hd) * 0.1).astype(np.float32) for _ in range(6)]
    return _with_tolerances({"args": (h, x, ws, bs)})


# ---- one-hot weights --------------------------------------------------------------------------------

ONEHOT_SHAPE = (1, 32, 32, 7, 9)     # Hd = 32: the h | x seam is at channel 32, a k-step boundary at 16 and 48


def exact_split(a):
    """a rounded so that it equals its bfloat16 hi part plus the bfloat16 of the residual exactly: the three-product
    mode then carries it without rounding, and the closed form below is exact up to the fp32 epilogue."""
    hi, lo = split_bf16(np.asarray(a, np.float32))
    return (hi + lo).astype(np.float32)


def onehot_cases():
    """(gate, out channel, in channel, tap): every tap, input channels on both sides of each 16-channel k-step
    boundary and of the h | x seam, all three gates of both halves."""
    _, hd, xd, _, _ = ONEHOT_SHAPE
    cases = []
    for gate in range(6):
        for tap in range(5):
            for cin in (0, 15, 16, hd - 1, hd, hd + 15, hd + 16, hd + xd - 1):
                cases.append((gate, (7 * cin + 3 * tap + gate) % hd, cin, tap))
    return cases


def onehot_expected(h, x, gate, cout, cin, tap):
    """The unit with all weights and biases zero but W_gate[cout, cin, tap] = 1, in closed form (float64).
    With zero pre-activations z = r = 1/2 and q = 0, so a half-step maps h to h / 2 except in channel cout of the
    half that holds the one-hot gate, where the pre-activation is the tap's shifted input channel."""
    h, x = np.asarray(h, np.float64), np.asarray(x, np.float64)
    for half in (0, 1):
        z = np.full_like(h, 0.5)
        rh = 0.5 * h
        q = np.zeros_like(h)
        if gate // 3 == half:
            g = gate % 3
            src = np.concatenate([rh if g == 2 else h, x], axis=1)
            pre = _shift(src[:, cin:cin + 1], tap, half)[:, 0]
            if g == 0:
                z[:, cout] = _sigmoid(pre)
            elif g == 2:
                q[:, cout] = np.tanh(pre)
            # g == 1: r enters the output only through q's weights, which are zero: h / 2 everywhere, and a
            # kernel that lets r's weights leak into z or q shows
        h = (1.0 - z) * h + z * q
    return h
