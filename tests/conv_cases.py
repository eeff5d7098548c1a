"""Shared helpers of test_conv.py / test_gpu_conv.py: the tests' own float64 restatement of the fused k x k
convolution (csrc/conv.hip) and of the modules built on it (BasicMotionEncoder, FlowHead, Up8Network's mask head:
raft.py:193-225, 262-273, 299-331), a float64 emulation of the kernel's two compute modes, the tolerance rule, the
shapes and the one-hot cases.

Restatement: kh kw shifted float64 matrix products over the zero-padded map (tap (i, j) reads position
(y + i - kh/2, x + j - kw/2)), a ReLU that keeps NaN.  Emulation of a compute mode: weights and inputs rounded to
fp32 and split into the bfloat16 hi part and the bfloat16 of the residual (dicl_match_cases.split_bf16), the
products the mode keeps (hi.hi, and for three products hi.lo and lo.hi) summed in float64, every tensor the kernel
stores rounded to fp32.

Tolerance: for each case and mode, e = max|emulation - float64| / max|float64| (CPU only; for a chain of
convolutions the error of the emulated chain), and the kernel is gated at max(FLOOR, FACTOR e) max-normalised
against float64, as rows f9 - f11.  Nothing here comes from the kernel.
"""

import functools
import zlib

import numpy as np

from dicl_match_cases import FACTOR, FLOOR, PRODUCTS, relu64, split_bf16
from gru_cases import exact_split, fixture, gru64, max_norm_err, module_params  # noqa: F401  (re-exported)

BLOCK_FIXTURE, UP8_FIXTURE = "gru_block_b1_6x10", "heads_up8_b2_h32_6x9"
ENCODER_CONVS = ("convc1", "convc2", "convf1", "convf2", "conv")
ACTS = ("none", "relu")

# (B, C0, C1, Cout, kh, kw, H, W)
SHAPES = [
    (1, 324, 0, 256, 1, 1, 6, 10),      # convc1: a last k-step of 4 channels
    (1, 2, 0, 128, 7, 7, 6, 10),        # convf1: Cin below one k-step, a kernel taller than the map
    (2, 256, 0, 192, 3, 3, 5, 37),      # a pixel tile plus a remainder, two images
    (1, 128, 0, 256, 3, 3, 37, 5),      # the same, vertically
    (1, 192, 64, 126, 3, 3, 9, 70),     # two sources, Cout not a multiple of 32, more than one tile
    (1, 20, 13, 40, 3, 3, 4, 33),       # a source seam inside a k-step, nothing aligned
    (1, 256, 0, 2, 3, 3, 3, 4),         # FlowHead.conv2: Cout = 2, both sides under a tile
    (1, 256, 0, 576, 1, 1, 4, 33),      # Up8's conv2: more output rows than one workgroup pass holds
    (1, 16, 0, 32, 5, 3, 1, 1),         # a non-square kernel, every tap but the centre is padding
    (3, 128, 0, 64, 3, 3, 9, 70),       # sample independence
]
BATCH_SHAPE = SHAPES[9]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


def conv64(parts, bias, act):
    """sum over the (weight part (Cout, C, kh, kw), map part (B, C, H, W)) pairs of `parts` of the 'same'-padded
    convolution as kh kw shifted matrix products, + bias, then the activation ("none" / "relu"); float64."""
    acc = 0.0
    with np.errstate(all="ignore"):
        for wt, m in parts:
            wt, m = np.asarray(wt, np.float64), np.asarray(m, np.float64)
            cout, _, kh, kw = wt.shape
            b, c, ht, wd = m.shape
            padded = np.pad(m, ((0, 0), (0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2)))
            for i in range(kh):
                for j in range(kw):
                    cols = padded[:, :, i:i + ht, j:j + wd].reshape(b, c, ht * wd)
                    acc = acc + np.matmul(wt[:, :, i, j], cols).reshape(b, cout, ht, wd)
        out = acc + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    return relu64(out) if act == "relu" else out


def conv_ref(x, weight, bias, act, products=None):
    """One convolution over the map x (the concatenation already made); products = None: exact float64, 1 or 3: the
    emulation of that compute mode (fp32 in, fp32 out)."""
    if not products:
        return conv64([(weight, x)], bias, act)
    wh, wl = split_bf16(weight)
    xh, xl = split_bf16(np.asarray(x, np.float32))
    parts = [(wh, xh)] + ([(wh, xl), (wl, xh)] if products == 3 else [])
    return conv64(parts, np.asarray(bias, np.float32), act).astype(np.float32).astype(np.float64)


def encoder_ref(flow, corr, weights, biases, products=None):
    """BasicMotionEncoder.forward; parameters in the order of ENCODER_CONVS."""
    cor = conv_ref(corr, weights[0], biases[0], "relu", products)
    cor = conv_ref(cor, weights[1], biases[1], "relu", products)
    flo = conv_ref(flow, weights[2], biases[2], "relu", products)
    flo = conv_ref(flo, weights[3], biases[3], "relu", products)
    out = conv_ref(np.concatenate([cor, flo], axis=1), weights[4], biases[4], "relu", products)
    return np.concatenate([out, np.asarray(flow, np.float64)], axis=1)


def two_conv_ref(x, weights, biases, products=None):
    """conv2(relu(conv1(x))): FlowHead and Up8Network's mask head."""
    return conv_ref(conv_ref(x, weights[0], biases[0], "relu", products), weights[1], biases[1], "none", products)


def conv_params(mod, names):
    """weights, biases of the Conv2d sub-modules `names` of mod, as numpy."""
    return ([getattr(mod, n).weight.detach().cpu().numpy().copy() for n in names],
            [getattr(mod, n).bias.detach().cpu().numpy().copy() for n in names])


def tolerance(emulated, ref):
    """(e, max(FLOOR, FACTOR e)) of an emulated result against the float64 one."""
    e = max_norm_err(emulated, ref)
    return e, max(FLOOR, FACTOR * e)


@functools.lru_cache(maxsize=None)
def shape_case(shape):
    """Seeded inputs of one shape — N(0, 1) maps, He-scaled weights, N(0, 0.1^2) biases — with, per activation, the
    float64 result and per mode the emulation error e and the tolerance.  Shared; never modified."""
    b, c0, c1, cout, kh, kw, ht, wd = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    x0 = rng.standard_normal((b, c0, ht, wd)).astype(np.float32)
    x1 = rng.standard_normal((b, c1, ht, wd)).astype(np.float32) if c1 else None
    c = c0 + c1
    weight = (rng.standard_normal((cout, c, kh, kw)) * np.sqrt(2.0 / (kh * kw * c))).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    x = x0 if x1 is None else np.concatenate([x0, x1], axis=1)
    case = {"args": (x0, x1, weight, bias), "ref": {}, "e": {}, "tol": {}}
    for act in ACTS:
        case["ref"][act] = conv_ref(x, weight, bias, act)
        for precision, products in PRODUCTS.items():
            case["e"][act, precision], case["tol"][act, precision] = tolerance(
                conv_ref(x, weight, bias, act, products), case["ref"][act])
    return case


@functools.lru_cache(maxsize=None)
def encoder_params():
    """det_init_fanin parameters of BasicMotionEncoder(324), the generator's own."""
    import rmd.raft
    from detinit import det_init_fanin
    return conv_params(det_init_fanin(rmd.raft.BasicUpdateBlock(324)).enc, ENCODER_CONVS)


# ---- one-hot weights --------------------------------------------------------------------------------

# (B, C0, C1, Cout, H, W): k-step boundaries at channels 16 and 32, the source seam at 20, a padded tail after
# channel 32 (a last k-step of one channel); 32-row tile boundaries at 32 and 64, a padded tail after row 69
ONEHOT_SHAPE = (1, 20, 13, 70, 6, 10)
ONEHOT_CIN = (0, 15, 16, 19, 20, 31, 32)
ONEHOT_COUT = (0, 31, 32, 63, 64, 69)


def onehot_cases():
    """(k, out channel, in channel, tap row, tap column): every (tap, input channel) pair of a 3 x 3 kernel, and
    every tap of a 7 x 7 kernel with the input channels in turn; the output channels in turn in both."""
    cases, n = [], 0
    for i in range(3):
        for j in range(3):
            for cin in ONEHOT_CIN:
                cases.append((3, ONEHOT_COUT[n % len(ONEHOT_COUT)], cin, i, j))
                n += 1
    for i in range(7):
        for j in range(7):
            cases.append((7, ONEHOT_COUT[n % len(ONEHOT_COUT)], ONEHOT_CIN[n % len(ONEHOT_CIN)], i, j))
            n += 1
    return cases


def onehot_expected(x, k, cin, i, j):
    """The one non-zero output channel: input channel cin read at (y + i - k/2, x + j - k/2), zero outside."""
    p = k // 2
    ht, wd = x.shape[2:]
    return np.pad(x[:, cin], ((0, 0), (p, p), (p, p)))[:, i:i + ht, j:j + wd]
