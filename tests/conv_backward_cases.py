"""Shared helpers of test_conv_backward.py / test_gpu_conv_backward.py: the tests' own float64 restatement of the
backward of the fused k x k convolution (csrc/conv_backward.hip), a float64 emulation of its three-product
arithmetic, the tolerance rule, the shapes, the one-hot cases and exact-integer data.

Restatement, with x = cat(x0, x1), y = act(conv(x, W) + b), g = dL/dy and gm = g where !(y <= 0) and 0 elsewhere
(ReLU; a NaN in y keeps the gradient) or gm = g (no activation):
    gb[o]          = sum_{b,y,x} gm[b, o, y, x]
    gx[b, c, y, x] = sum_{o,i,j} W[o, c, i, j] gm[b, o, y - i + kh/2, x - j + kw/2]
    gW[o, c, i, j] = sum_{b,y,x} gm[b, o, y, x] x[b, c, y + i - kh/2, x + j - kw/2]        (zero outside the map)
as kh kw shifted float64 matrix products.  Emulation: gm and W (data gradient) or gm and x (weight gradient)
rounded to fp32 and split into the bfloat16 hi part and the bfloat16 of the residual (dicl_match_cases.split_bf16),
hi.hi + hi.lo + lo.hi summed in float64, the result rounded to fp32.

Tolerance: per case e = max|emulation - float64| / max|float64| (CPU only), and the kernel is gated at
max(FLOOR, FACTOR e) = max(1e-5, 3 e) max-normalised against float64; the bias gradient (float64 sums of fp32
values in the kernel) at 1e-5.  The operator takes y as an argument, and the tests pass the oracle's own y (the
float64 forward rounded to fp32), so both sides use the same mask.  Nothing here comes from a kernel.
"""

import functools
import zlib

import numpy as np

from conv_cases import conv64, max_norm_err, tolerance  # noqa: F401  (re-exported)
from dicl_match_cases import FACTOR, FLOOR, PRODUCTS, split_bf16  # noqa: F401  (re-exported)
from dicl_match_grad_cases import E_MAX  # noqa: F401  (re-exported)

ACTS = ("none", "relu")
BIAS_TOL = 1e-5

# (B, C0, C1, Cout, kh, kw, H, W)
SHAPES = [
    (1, 324, 0, 256, 1, 1, 6, 10),      # a last k-step of 4 channels in the forward direction, a 60-pixel K in gW
    (1, 2, 0, 128, 7, 7, 6, 10),        # C below one tile column, 49 taps, a kernel taller than the map
    (2, 256, 0, 192, 3, 3, 5, 37),      # a pixel tile plus a remainder, two images summed in gW
    (1, 128, 0, 256, 3, 3, 37, 5),      # the same, vertically
    (1, 20, 13, 40, 3, 3, 4, 33),       # a source seam inside a tile, nothing aligned, gx0 / gx1 split
    (1, 192, 64, 126, 3, 3, 9, 70),     # two sources, Cout not a multiple of 32
    (1, 256, 0, 2, 3, 3, 3, 4),         # Cout = 2
    (1, 256, 0, 576, 1, 1, 4, 33),      # the data gradient contracts over 576 channels
    (1, 16, 0, 32, 5, 3, 1, 1),         # every tap but the centre is padding
    (3, 40, 0, 64, 3, 3, 9, 70),        # three images, more pixel slices than one workgroup takes
]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
EXACT_SHAPES = [SHAPES[4], SHAPES[5], SHAPES[9]]
BATCH_SHAPE = SHAPES[9]

# the nine convolutions next to the recurrent unit: (kh, kw, C0, C1, Cout); `conv` reads (cor, flo) as two sources
NINE = [(1, 1, 324, 0, 256), (3, 3, 256, 0, 192), (7, 7, 2, 0, 128), (3, 3, 128, 0, 64), (3, 3, 192, 64, 126),
        (3, 3, 128, 0, 256), (3, 3, 256, 0, 2), (3, 3, 128, 0, 256), (1, 1, 256, 0, 576)]


def mask64(g, y, act):
    """gm: g where !(y <= 0), exactly 0 elsewhere (act "relu"); g itself (act "none")."""
    g = np.asarray(g, np.float64)
    if act == "none":
        return g
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(y) <= 0, 0.0, g)


def data_grad64(parts):
    """sum over the (weight part (Cout, C, kh, kw), gm part (B, Cout, H, W)) pairs of the data gradient
    (B, C, H, W): tap (i, j) reads gm at (y - i + kh/2, x - j + kw/2), zero outside the map."""
    acc = 0.0
    with np.errstate(all="ignore"):
        for wt, gm in parts:
            wt, gm = np.asarray(wt, np.float64), np.asarray(gm, np.float64)
            cout, c, kh, kw = wt.shape
            b, _, ht, wd = gm.shape
            padded = np.pad(gm, ((0, 0), (0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2)))
            for i in range(kh):
                for j in range(kw):
                    cols = padded[:, :, kh - 1 - i:kh - 1 - i + ht, kw - 1 - j:kw - 1 - j + wd].reshape(b, cout, ht * wd)
                    acc = acc + np.matmul(wt[:, :, i, j].T, cols).reshape(b, c, ht, wd)
    return acc


def weight_grad64(parts, kh, kw):
    """sum over the (gm part (B, Cout, H, W), map part (B, C, H, W)) pairs of the weight gradient (Cout, C, kh, kw)."""
    acc = 0.0
    with np.errstate(all="ignore"):
        for gm, m in parts:
            gm, m = np.asarray(gm, np.float64), np.asarray(m, np.float64)
            b, cout, ht, wd = gm.shape
            c = m.shape[1]
            padded = np.pad(m, ((0, 0), (0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2)))
            out = np.zeros((cout, c, kh, kw))
            for i in range(kh):
                for j in range(kw):
                    cols = padded[:, :, i:i + ht, j:j + wd].reshape(b, c, ht * wd)
                    out[:, :, i, j] = np.einsum("bop,bcp->oc", gm.reshape(b, cout, ht * wd), cols)
            acc = acc + out
    return acc


def backward_ref(g, y, x, weight, act, products=None):
    """(gx, gW, gb) of one convolution over the map x (the concatenation already made); products = None: exact
    float64, 3: the emulation of the kernel's arithmetic (fp32 in, fp32 out)."""
    kh, kw = weight.shape[2:]
    gm = mask64(g, y, act)
    with np.errstate(all="ignore"):
        gb = gm.sum(axis=(0, 2, 3))
    if not products:
        return data_grad64([(weight, gm)]), weight_grad64([(gm, x)], kh, kw), gb
    gh, gl = split_bf16(gm.astype(np.float32))
    wh, wl = split_bf16(weight)
    xh, xl = split_bf16(np.asarray(x, np.float32))
    gx = data_grad64([(wh, gh), (wh, gl), (wl, gh)])
    gw = weight_grad64([(gh, xh), (gh, xl), (gl, xh)], kh, kw)
    return tuple(a.astype(np.float32).astype(np.float64) for a in (gx, gw, gb))


@functools.lru_cache(maxsize=None)
def shape_case(shape):
    """Seeded inputs of one shape — N(0, 1) maps and output gradients, He-scaled weights, N(0, 0.1^2) biases — with,
    per activation, the oracle's y (fp32; None without an activation), the float64 gradients, the emulation error
    e of gx and gW and their tolerances.  Shared; never modified."""
    b, c0, c1, cout, kh, kw, ht, wd = shape
    rng = np.random.default_rng(zlib.crc32(repr(("backward",) + shape).encode()))
    x0 = rng.standard_normal((b, c0, ht, wd)).astype(np.float32)
    x1 = rng.standard_normal((b, c1, ht, wd)).astype(np.float32) if c1 else None
    c = c0 + c1
    weight = (rng.standard_normal((cout, c, kh, kw)) * np.sqrt(2.0 / (kh * kw * c))).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    g = rng.standard_normal((b, cout, ht, wd)).astype(np.float32)
    x = x0 if x1 is None else np.concatenate([x0, x1], axis=1)
    case = {"args": (x0, x1, weight, bias), "g": g, "x": x, "y": {}, "ref": {}, "e": {}, "tol": {}}
    for act in ACTS:
        y = None if act == "none" else conv64([(weight, x)], bias, act).astype(np.float32)
        case["y"][act] = y
        case["ref"][act] = backward_ref(g, y, x, weight, act)
        emulated = backward_ref(g, y, x, weight, act, 3)
        for k, name in enumerate(("gx", "gw")):
            case["e"][act, name], case["tol"][act, name] = tolerance(emulated[k], case["ref"][act][k])
    return case


def split_sources(gx, c0):
    """(gx0, gx1 or None) of the gradient of the concatenation."""
    return gx[:, :c0], (gx[:, c0:] if gx.shape[1] > c0 else None)


def workspace_bytes(b, c0, c1, cout, kh, kw, ht, wd):
    """include/rmd.h's formula of rmd_conv2d_backward_workspace_bytes, restated."""
    def up(v, m):
        return -(-v // m) * m
    c = c0 + c1
    gm = up(4 * b * cout * ht * wd, 256)
    packed = sum(up(n, 32) * kh * kw * up(cout, 16) * 2 * 2 + up(4 * up(n, 32), 256) for n in (c0, c1) if n)
    slices = max(1, min(b * ht, 32, -(-1024 // (-(-cout // 128) * -(-c // 32) * kh))))
    return gm + packed + up(4 * slices * cout * c * kh * kw, 256) + 256


# ---- one-hot cases -----------------------------------------------------------------------------------

# (B, C0, C1, Cout, H, W): the channel boundaries of conv_cases.ONEHOT_SHAPE on a map wider than one 64-pixel row
# segment of the weight gradient, each of whose rows is a pixel slice of its own
ONEHOT_SHAPE = (1, 20, 13, 70, 6, 70)
ONEHOT_CIN = (0, 15, 16, 19, 20, 31, 32)
ONEHOT_COUT = (0, 31, 32, 63, 64, 69)
# (y, x): the four corners, both sides of the segment boundary inside a row and of a slice boundary between rows,
# the tail of a row
ONEHOT_PIXELS = ((0, 0), (0, 69), (5, 0), (5, 69), (2, 63), (2, 64), (3, 64), (3, 10), (4, 66))


def exact_ints(rng, shape, bound):
    """Integers in [-bound, bound] as float32: every product and sum of a few thousand of them is exact in fp32 and
    in the split-bf16 arithmetic (hi holds them, lo is zero)."""
    return rng.integers(-bound, bound + 1, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact_case(shape):
    """Integer data of one shape: x in [-4, 4], W in {-2..2}, bias in {-2..2}, g in [-3, 3]."""
    b, c0, c1, cout, kh, kw, ht, wd = shape
    rng = np.random.default_rng(zlib.crc32(repr(("exact",) + shape).encode()))
    x0 = exact_ints(rng, (b, c0, ht, wd), 4)
    x1 = exact_ints(rng, (b, c1, ht, wd), 4) if c1 else None
    weight = exact_ints(rng, (cout, c0 + c1, kh, kw), 2)
    bias = exact_ints(rng, (cout,), 2)
    g = exact_ints(rng, (b, cout, ht, wd), 3)
    return x0, x1, weight, bias, g


# ---- exact-integer modules ---------------------------------------------------------------------------

def int_init(module, seed, nonzeros=3):
    """Integer parameters under which a chain of convolutions stays exact: every weight row (one output channel)
    holds `nonzeros` entries of +-1 and zeros elsewhere, every bias is in {-1, 0, 1}; the recurrent unit's
    parameters are zero (z = 1/2, q = 0: each half halves h, exactly).  Returns module."""
    import torch
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            if ".gru." in "." + name or name.startswith("gru."):
                p.zero_()
            elif p.dim() == 4:
                wt = np.zeros(p.shape, np.float32).reshape(p.shape[0], -1)
                for o in range(wt.shape[0]):
                    at = rng.choice(wt.shape[1], size=min(nonzeros, wt.shape[1]), replace=False)
                    wt[o, at] = rng.choice([-1.0, 1.0], size=len(at))
                p.copy_(torch.from_numpy(wt.reshape(p.shape)))
            else:
                p.copy_(torch.from_numpy(exact_ints(rng, tuple(p.shape), 1)))
    return module


def saturate_up8(up):
    """Mask-head biases that make Up8Network's softmax over the nine taps exactly one-hot in fp32 (a margin of 1024
    / temperature, far past where exp underflows): channel 64 k + s of tap k and sub-pixel s gets 1024 where
    k = s mod 9.  The convex combination and its backward are then exact selections, the same on every device;
    the gradient that reaches the mask is exactly zero.  Returns up."""
    import torch
    with torch.no_grad():
        bias = torch.zeros(9, 64)
        for s in range(64):
            bias[s % 9, s] = 1024.0
        up.conv2.bias.copy_(bias.reshape(-1))
    return up
