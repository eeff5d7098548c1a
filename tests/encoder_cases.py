"""Shared helpers of test_encoder.py / test_gpu_encoder.py: the tests' own float64 restatement of the strided,
normalising convolution, the instance-norm statistics, the residual join and the whole feature encoder
(csrc/encoder.hip; encoders/raft/s3.py:8-72, blocks/raft.py:13-46), a float64 emulation of the kernels' two compute
modes, the tolerance rule, the shapes, the one-hot cases and the fixtures of tests/golden/gen_golden_encoder.py.

Restatement: conv_cases.conv64 (kh kw shifted float64 matrix products over the zero-padded map) read at every
stride-th position — tap (i, j) of output (y, x) reads (s y + i - k/2, s x + j - k/2) —, the instance norm as
(x - mean) / sqrt(var + eps) with the biased variance, ReLUs that keep NaN.  Emulation of a compute mode: what the
kernels do, in float64: inputs and weights rounded to fp32 and split with split_bf16, the transform on load
relu(x a + d) rounded to fp32 before the split (one rounding, as the fused multiply-add), the kept products summed
in float64, every tensor the kernels store rounded to fp32, the statistics taken in float64 of the fp32-rounded map
and rounded to fp32.

Tolerance (the project's rule, dicl_match_cases.FLOOR / FACTOR): e = max|emulation - float64| / max|float64| on the
CPU, and the kernels are gated at max(1e-5, 3 e) max-normalised against float64.  Nothing here comes from a kernel.
"""

import functools
import zlib

import numpy as np

from conv_cases import ACTS, conv64, exact_split, fixture, max_norm_err, tolerance  # noqa: F401  (re-exported)
from dicl_match_cases import PRODUCTS, bf16_round, relu64, split_bf16  # noqa: F401

EPS = 1e-5                              # nn.InstanceNorm2d's and nn.BatchNorm2d's default
NORMS = ("instance", "batch", "none")
FIXTURES = {norm: f"encoder_{norm}_b2_36x140" for norm in NORMS}
OPERATORS = ["conv2d_norm_act", "feature_encoder", "instance_norm_stats", "residual_join"]

# (B, C, Cout, k or (kh, kw), H, W, stride), and whether the case has the load transform and a residual.  The first
# six are the issue's; the others take the kernel's remaining paths
SHAPES = [
    ((1, 3, 64, 7, 13, 70, 2), False),      # the stem: Cin below one k-step, the 2-row tile, odd H
    ((2, 64, 96, 3, 9, 67, 2), False),      # a stride-2 3 x 3: two 32-wide output tiles, odd sides, two images
    ((1, 64, 96, 1, 9, 67, 2), False),      # the projection
    ((1, 96, 128, 3, 6, 8, 2), False),      # even sides, a map under one tile
    ((1, 16, 32, 3, 1, 1, 2), False),       # every tap but the centre is padding
    ((1, 20, 40, 3, 4, 33, 1), True),       # stride 1, nothing aligned, transform and residual
    ((1, 24, 40, 5, 9, 40, 2), False),      # 5 x 5 at stride 2: the 2-row tile with more than one k-step per chunk loop
    ((1, 16, 32, (5, 3), 7, 37, 2), True),  # a non-square kernel at stride 2, transform and residual
    ((2, 16, 32, (1, 3), 6, 37, 2), False), # a 1-tall kernel: only every second row is staged, the columns in two planes
    ((1, 40, 32, (3, 1), 9, 70, 2), False), # a 1-wide kernel: only every second column is staged, one plane
]
SHAPE_IDS = ["x".join(map(str, s)).replace("(", "").replace(")", "").replace(", ", "by") + ("-norm-res" if t else "")
             for s, t in SHAPES]


def kernel_sides(k):
    return (k, k) if isinstance(k, int) else tuple(k)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def out_side(n, stride):
    return (n - 1) // stride + 1


# ---- the operators -------------------------------------------------------------------------------------

def planes(s):
    return np.asarray(s, np.float64)[:, :, None, None]


def norm_conv_ref(x, scale, shift, weight, bias, residual, stride, act, products=None):
    """conv2d_norm_act; products = None: exact float64, 1 or 3: the emulation of that compute mode."""
    x = np.asarray(x, np.float64)
    if scale is not None:
        with np.errstate(invalid="ignore"):
            x = relu64(x * planes(scale) + planes(shift))
    if not products:
        out = conv64([(weight, x)], bias, act)[:, :, ::stride, ::stride]
    else:
        wh, wl = split_bf16(weight)
        xh, xl = split_bf16(x.astype(np.float32))
        parts = [(wh, xh)] + ([(wh, xl), (wl, xh)] if products == 3 else [])
        out = conv64(parts, np.asarray(bias, np.float32), act)[:, :, ::stride, ::stride]
    if residual is not None:
        with np.errstate(invalid="ignore"):
            out = relu64(out + np.asarray(residual, np.float64))
    return f32(out) if products else out


def stats_ref(x, eps=EPS, emulate=False):
    """instance_norm_stats: (scale, shift), both (B, C)."""
    x = np.asarray(x, np.float64)
    mean, var = x.mean(axis=(2, 3)), x.var(axis=(2, 3))
    scale = 1.0 / np.sqrt(var + eps)
    shift = -mean * scale
    return (f32(scale), f32(shift)) if emulate else (scale, shift)


def instance_norm64(x, eps=EPS):
    x = np.asarray(x, np.float64)
    mean, var = x.mean(axis=(2, 3), keepdims=True), x.var(axis=(2, 3), keepdims=True)
    return (x - mean) / np.sqrt(var + eps)


def join_ref(y, y_stats, x, x_stats, emulate=False):
    """residual_join: relu(xs + relu(ys))."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        if y_stats is not None:
            y = y * planes(y_stats[0]) + planes(y_stats[1])
        if x_stats is not None:
            x = x * planes(x_stats[0]) + planes(x_stats[1])
        out = relu64(x + relu64(y))
    return f32(out) if emulate else out


# ---- the encoder ---------------------------------------------------------------------------------------

# (block prefix, stride) in module order
BLOCKS = (("layer1.0", 1), ("layer1.1", 1), ("layer2.0", 2), ("layer2.1", 1), ("layer3.0", 2), ("layer3.1", 1))


def conv_norm_names():
    """(convolution, norm or None) state-dict prefixes of the 16 convolutions in the operator's order."""
    names = [("conv1", "norm1")]
    for prefix, stride in BLOCKS:
        names += [(f"{prefix}.conv1", f"{prefix}.norm1"), (f"{prefix}.conv2", f"{prefix}.norm2")]
        if stride == 2:
            names.append((f"{prefix}.downsample.0", f"{prefix}.norm3"))
    return names + [("conv2", None)]


def block_names(stride):
    """conv_norm_names of a ResidualBlock on its own."""
    return [("conv1", "norm1"), ("conv2", "norm2")] + ([("downsample.0", "norm3")] if stride == 2 else [])


def folded_params(module, names=None):
    """weights, biases of the convolutions `names` (default: the encoder's 16) as the operators take them, from the
    module's state dict: an eval-mode batch norm folded in float64 (W' = s W, b' = (b - mean) s + beta, s = gamma /
    sqrt(var + eps)), rounded to fp32."""
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in module.state_dict().items()
          if v.is_floating_point()}
    weights, biases = [], []
    for conv, norm in names or conv_norm_names():
        w, b = sd[f"{conv}.weight"], sd[f"{conv}.bias"]
        if norm is not None and f"{norm}.running_var" in sd:
            s = sd[f"{norm}.weight"] / np.sqrt(sd[f"{norm}.running_var"] + EPS)
            w, b = w * s[:, None, None, None], (b - sd[f"{norm}.running_mean"]) * s + sd[f"{norm}.bias"]
        weights.append(w.astype(np.float32))
        biases.append(b.astype(np.float32))
    return weights, biases


def block_ref(x, weights, biases, stride, instance, products=None):
    """One ResidualBlock on the operators' schedule; weights / biases: conv1, conv2 and (stride 2) the projection."""
    em = bool(products)
    if instance:
        y = norm_conv_ref(x, None, None, weights[0], biases[0], None, stride, "none", products)
        a, d = stats_ref(y, emulate=em)
        y = norm_conv_ref(y, a, d, weights[1], biases[1], None, 1, "none", products)
        y_stats = stats_ref(y, emulate=em)
        if stride == 1:
            return join_ref(y, y_stats, x, None, em)
        p = norm_conv_ref(x, None, None, weights[2], biases[2], None, stride, "none", products)
        return join_ref(y, y_stats, p, stats_ref(p, emulate=em), em)
    res = x if stride == 1 else norm_conv_ref(x, None, None, weights[2], biases[2], None, stride, "none", products)
    y = norm_conv_ref(x, None, None, weights[0], biases[0], None, stride, "relu", products)
    return norm_conv_ref(y, None, None, weights[1], biases[1], res, 1, "relu", products)


def encoder_ref(x, weights, biases, instance, products=None):
    """FeatureEncoder.forward on the operator's schedule, parameters as folded_params gives them."""
    em = bool(products)
    if instance:
        y = norm_conv_ref(x, None, None, weights[0], biases[0], None, 2, "none", products)
        x = join_ref(y, stats_ref(y, emulate=em), np.zeros_like(y), None, em)         # relu(norm(y))
    else:
        x = norm_conv_ref(x, None, None, weights[0], biases[0], None, 2, "relu", products)
    g = 1
    for _, stride in BLOCKS:
        n = 3 if stride == 2 else 2
        x = block_ref(x, weights[g:g + n], biases[g:g + n], stride, instance, products)
        g += n
    return norm_conv_ref(x, None, None, weights[15], biases[15], None, 1, "none", products)


def build_encoder(norm, **kwargs):
    """rmd.encoders.FeatureEncoder(256, norm) in eval mode with the generator's parameters."""
    import rmd.encoders
    from detinit import det_init_fanin
    return det_init_fanin(rmd.encoders.FeatureEncoder(256, norm, **kwargs)).eval()


@functools.lru_cache(maxsize=None)
def encoder_case(norm):
    """The fixture of one norm type with the operator's parameters, and per mode the emulation error e of the whole
    chain against the fixture's float64 output and the tolerance.  Shared; never modified."""
    g = fixture(FIXTURES[norm])
    weights, biases = folded_params(build_encoder(norm))
    case = {"x": g["x"], "ref": g["out64"], "out": g["out"], "keys": g["keys"], "ref_err": float(g["ref_err"]),
            "weights": weights, "biases": biases, "e": {}, "tol": {}}
    for precision, products in PRODUCTS.items():
        case["e"][precision], case["tol"][precision] = tolerance(
            encoder_ref(g["x"], weights, biases, norm == "instance", products), g["out64"])
    return case


# ---- single convolutions -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shape_case(shape, transformed):
    """Seeded inputs of one shape — an N(0, 1) map, He-scaled weights, N(0, 0.1^2) biases and, where `transformed`,
    statistics (scale in 0.5 .. 1.5, shift N(0, 0.5^2)) and an N(0, 1) residual — with, per activation, the float64
    result and per mode the emulation error e and the tolerance.  Shared; never modified."""
    b, c, cout, k, ht, wd, stride = shape
    kh, kw = kernel_sides(k)
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    x = rng.standard_normal((b, c, ht, wd)).astype(np.float32)
    weight = (rng.standard_normal((cout, c, kh, kw)) * np.sqrt(2.0 / (kh * kw * c))).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    scale = shift = residual = None
    if transformed:
        scale = rng.uniform(0.5, 1.5, (b, c)).astype(np.float32)
        shift = (0.5 * rng.standard_normal((b, c))).astype(np.float32)
        residual = rng.standard_normal((b, cout, out_side(ht, stride), out_side(wd, stride))).astype(np.float32)
    case = {"args": (x, scale, shift, weight, bias, residual), "stride": stride, "ref": {}, "e": {}, "tol": {}}
    for act in ACTS:
        case["ref"][act] = norm_conv_ref(x, scale, shift, weight, bias, residual, stride, act)
        for precision, products in PRODUCTS.items():
            case["e"][act, precision], case["tol"][act, precision] = tolerance(
                norm_conv_ref(x, scale, shift, weight, bias, residual, stride, act, products), case["ref"][act])
    return case


# ---- one-hot weights at stride 2 -----------------------------------------------------------------------

# (B, C, Cout, H, W): k-step boundaries at channels 16 and 32 with a padded tail after channel 32, 32-row tile
# boundaries at 32 and 64 with a padded tail after row 69; an odd and an even side, two 32-wide output tiles
ONEHOT_SHAPE = (1, 33, 70, 7, 70)
ONEHOT_CIN = (0, 15, 16, 31, 32)
ONEHOT_COUT = (0, 31, 32, 63, 64, 69)


def onehot_cases():
    """(k, out channel, in channel, tap row, tap column): every tap of a 3 x 3 and of a 7 x 7 kernel, the input and
    output channels in turn."""
    cases, n = [], 0
    for k in (3, 7):
        for i in range(k):
            for j in range(k):
                cases.append((k, ONEHOT_COUT[n % len(ONEHOT_COUT)], ONEHOT_CIN[n % len(ONEHOT_CIN)], i, j))
                n += 1
    return cases


def onehot_expected(x, k, cin, i, j, stride=2):
    """The one non-zero output channel: input channel cin read at (s y + i - k/2, s x + j - k/2), zero outside."""
    p = k // 2
    ht, wd = x.shape[2:]
    padded = np.pad(x[:, cin], ((0, 0), (p, p + stride), (p, p + stride)))
    return padded[:, i::stride, j::stride][:, :out_side(ht, stride), :out_side(wd, stride)]
