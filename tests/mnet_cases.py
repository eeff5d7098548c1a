"""Shared helpers of test_mnet.py / test_gpu_mnet.py: the tests' own float64 restatement of the k x k MatchingNet
(csrc/mnet.hip; blocks/dicl.py:93-118), a float64 emulation of the kernels' two compute modes, the tolerance rule,
the shapes, the one-hot cases and the fixtures of tests/golden/gen_golden_mnet.py.

Restatement: layers 1-4 are conv_cases.conv64 read at every stride-th position (encoder_cases.norm_conv_ref at
stride 1 and 2); the transposed convolution is written from its formula — tap (ky, kx) of input position (iy, ix)
adds W5'[c, o, ky, kx] x[c, iy, ix] to output (2 iy - 1 + ky, 2 ix - 1 + kx), what falls outside the map dropped —
as 16 float64 matrix products scattered at stride 2; it is not F.conv_transpose2d (test_mnet.py checks it against
that to 1e-12).  The last layer is conv64 over the zero-padded u.  ReLUs keep NaN.

Emulation of a compute mode (the project's rule): the operands of layers 1-5 rounded to fp32 and split with
split_bf16, the kept products (hi.hi, and for three products hi.lo and lo.hi) summed in float64, every stored tensor
— the four maps and u — rounded to fp32, the last layer in float64 from the fp32 u.

Tolerance (dicl_match_cases.FLOOR / FACTOR): e = max|emulation - float64| / max|float64| on the CPU, the kernels are
gated at max(1e-5, 3 e) max-normalised against float64.  Nothing here comes from a kernel.
"""

import functools
import zlib

import numpy as np

from conv_cases import conv64, max_norm_err, tolerance  # noqa: F401  (re-exported)
from dicl_match_cases import PRODUCTS, relu64, split_bf16
from encoder_cases import f32, norm_conv_ref

STRIDES = (1, 2, 1, 1)
FIXTURES = ["mnet_bn_b2_c16_r2_8x12", "mnet_none_b1_c8_r3_6x10_s05", "mnet_emb_b1_c16_r2_4x6",
            "mnet_nan_b1_c16_r2_8x12"]
NAN_FIXTURE = "mnet_nan_b1_c16_r2_8x12"
OPERATORS = ["matching_net", "mnet_tail"]

# The tail kernel's tile: a workgroup owns 3 x 31 input positions = 6 x 62 cost pixels.
# (N, c3, c4, h2, w2)
TAIL_SHAPES = [
    (1, 64, 32, 1, 1),          # a 2 x 2 output that is nearly all padding
    (2, 64, 32, 3, 5),
    (1, 24, 12, 2, 3),          # nothing a multiple of 16
    (1, 32, 16, 4, 6),          # mnet_scale 0.5
    (1, 64, 32, 5, 35),         # horizontally a 31-position tile plus a remainder of 4 (62 + 8 cost columns)
    (1, 64, 32, 19, 3),         # vertically six 3-position tiles plus a remainder of 1 (36 + 2 cost rows)
    (3, 64, 32, 4, 17),         # sample independence
]
BATCH_TAIL = TAIL_SHAPES[6]
TAIL_IDS = ["x".join(map(str, s)) for s in TAIL_SHAPES]

# (B, du, dv, c_in, scale, h, w)
NET_SHAPES = [
    (1, 3, 3, 32, 1, 8, 12),
    (2, 1, 1, 34, 1, 2, 2),
    (1, 5, 5, 16, 0.5, 6, 10),
    (1, 7, 7, 32, 1, 4, 6),     # 49 images: group 4 leaves a last group of 1
]
GROUP_SHAPE = NET_SHAPES[3]
NET_IDS = ["x".join(map(str, s)) for s in NET_SHAPES]


def widths(c_in, scale):
    return c_in, int(scale * 96), int(scale * 128), int(scale * 64), int(scale * 32)


# ---- the restatement -----------------------------------------------------------------------------------

def tconv64(x, w5):
    """ConvTranspose2d(c3, c4, 4, stride 2, padding 1) without bias from its formula: x (N, c3, h2, w2), w5
    (c3, c4, 4, 4) -> (N, c4, 2 h2, 2 w2), float64."""
    x, w5 = np.asarray(x, np.float64), np.asarray(w5, np.float64)
    n, c3, h2, w2 = x.shape
    c4 = w5.shape[1]
    out = np.zeros((n, c4, 2 * h2 + 2, 2 * w2 + 2))        # row Y + 1: Y = 2 iy - 1 + ky runs over -1 .. 2 h2
    cols = x.reshape(n, c3, h2 * w2)
    with np.errstate(all="ignore"):
        for ky in range(4):
            for kx in range(4):
                part = np.matmul(w5[:, :, ky, kx].T, cols).reshape(n, c4, h2, w2)
                out[:, :, ky:ky + 2 * h2:2, kx:kx + 2 * w2:2] += part
    return out[:, :, 1:-1, 1:-1]


def tail_ref(x, w5, t5, w6, b6, products=None):
    """mnet_tail; products = None: exact float64, 1 or 3: the emulation of that compute mode."""
    c4 = np.asarray(w5).shape[1]
    with np.errstate(all="ignore"):
        if not products:
            u = relu64(tconv64(x, w5) + np.asarray(t5, np.float64).reshape(1, -1, 1, 1))
        else:
            wh, wl = split_bf16(w5)
            xh, xl = split_bf16(np.asarray(x, np.float32))
            acc = tconv64(xh, wh)
            if products == 3:
                acc = acc + tconv64(xl, wh) + tconv64(xh, wl)
            u = f32(relu64(acc + f32(t5).reshape(1, -1, 1, 1)))
            w6, b6 = f32(w6), f32(b6)
        return conv64([(np.asarray(w6, np.float64).reshape(1, c4, 3, 3), u)], np.asarray(b6).reshape(-1)[:1], "none")[:, 0]


def net_ref(mvol, weights, biases, products=None):
    """matching_net on (N, c_in, h, w) images -> (N, h, w)."""
    x = np.asarray(mvol, np.float64)
    for i, stride in enumerate(STRIDES):
        x = norm_conv_ref(x, None, None, weights[i], biases[i], None, stride, "relu", products)
    return tail_ref(x, weights[4], biases[4], weights[5], biases[5], products)


def _he(rng, shape, fan_in):
    return (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)


def _bias(rng, n):
    return (rng.standard_normal(n) * 0.1).astype(np.float32)


def _with_tolerances(case, ref_fn):
    case["ref"] = ref_fn(*case["args"])
    case["e"], case["tol"] = {}, {}
    for precision, products in PRODUCTS.items():
        case["e"][precision], case["tol"][precision] = tolerance(ref_fn(*case["args"], products), case["ref"])
    return case


@functools.lru_cache(maxsize=None)
def tail_case(shape):
    """Seeded inputs of one tail shape — an N(0, 1) map clipped at zero like a ReLU's output, He-scaled weights,
    N(0, 0.1^2) biases — with the float64 result and per mode e and the tolerance.  Shared; never modified."""
    n, c3, c4, h2, w2 = shape
    rng = np.random.default_rng(zlib.crc32(repr(("tail",) + shape).encode()))
    x = np.maximum(rng.standard_normal((n, c3, h2, w2)), 0.0).astype(np.float32)
    args = (x, _he(rng, (c3, c4, 4, 4), 4 * c3), _bias(rng, c4), _he(rng, (c4, 3, 3), 9 * c4), _bias(rng, 1))
    return _with_tolerances({"args": args}, tail_ref)


def net_params(rng, c_in, scale):
    _, c1, c2, c3, c4 = widths(c_in, scale)
    chans = [(c1, c_in), (c2, c1), (c2, c2), (c3, c2)]
    weights = [_he(rng, (co, ci, 3, 3), 9 * ci) for co, ci in chans]
    biases = [_bias(rng, co) for co, _ in chans]
    weights += [_he(rng, (c3, c4, 4, 4), 4 * c3), _he(rng, (c4, 3, 3), 9 * c4)]
    biases += [_bias(rng, c4), _bias(rng, 1)]
    return weights, biases


@functools.lru_cache(maxsize=None)
def net_case(shape):
    """Seeded inputs of one whole-network shape with the float64 result (B, du, dv, h, w), e and the tolerance of
    the emulated chain.  Shared; never modified."""
    b, du, dv, c_in, scale, h, w = shape
    rng = np.random.default_rng(zlib.crc32(repr(("net",) + shape).encode()))
    mvol = rng.standard_normal((b, du, dv, c_in, h, w)).astype(np.float32)
    weights, biases = net_params(rng, c_in, scale)

    def ref(mvol, weights, biases, products=None):
        return net_ref(mvol.reshape(-1, c_in, h, w), weights, biases, products).reshape(b, du, dv, h, w)
    return _with_tolerances({"args": (mvol, weights, biases)}, ref)


# ---- one-hot cases on dyadic data ------------------------------------------------------------------------

ONEHOT_SHAPE = (1, 24, 12, 4, 35)           # (N, c3, c4, h2, w2): two tiles in each direction, nothing aligned
ONEHOT_POSITIONS = ((2, 17), (0, 0), (0, 34), (3, 0), (3, 34), (1, 0), (3, 31))    # interior, corners, edges, a seam


def dyadic(rng, shape):
    """Multiples of 1/8 in -2 .. 2: exact in bfloat16, and so are their sums with 0.5 and b6."""
    return (rng.integers(-16, 17, shape) / 8.0).astype(np.float32)


def w5_onehot_expected(x, c, ky, kx):
    """Channel c of relu(x) scattered at stride 2 by tap (ky, kx): u[Y, X] = relu(x[c, iy, ix]) at Y = 2 iy - 1 + ky,
    X = 2 ix - 1 + kx inside the map, zero elsewhere."""
    n, _, h2, w2 = x.shape
    out = np.zeros((n, 2 * h2 + 2, 2 * w2 + 2), np.float64)
    out[:, ky:ky + 2 * h2:2, kx:kx + 2 * w2:2] = np.maximum(x[:, c].astype(np.float64), 0.0)
    return out[:, 1:-1, 1:-1]


def w6_onehot_expected(shape, i, j, b6, t5=0.5):
    """W5' = 0: u = relu(t5) = t5 inside the map and zero outside, so tap (i, j) gives b6 + t5 where (Y + i - 1,
    X + j - 1) lies inside the map and b6 where it does not."""
    n, _, _, h2, w2 = shape
    ho, wo = 2 * h2, 2 * w2
    ys, xs = np.meshgrid(np.arange(ho) + i - 1, np.arange(wo) + j - 1, indexing="ij")
    inside = (ys >= 0) & (ys < ho) & (xs >= 0) & (xs < wo)
    return np.broadcast_to(np.where(inside, np.float64(b6) + t5, np.float64(b6)), (n, ho, wo))


# ---- the fixtures ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture(name):
    from conftest import load_golden
    return load_golden(name)


def build_module(name, device="cpu", **kwargs):
    """The drop-in correlation module of a fixture in eval mode: det_init weights, then the stored norm state."""
    import torch
    import rmd
    from detinit import det_init
    g = fixture(name)
    c = g["fmap1"].shape[1]
    extra = {} if str(g["cmod"]) == "dicl-emb" else {"mnet_scale": float(g["mnet_scale"])}
    mod = det_init(rmd.corr.make_cmod(str(g["cmod"]), c, int(g["radius"]), dap_init="standard",
                                      norm_type=str(g["norm_type"]), **extra, **kwargs))
    stored = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.") and k != "sd.keys"}
    mod.load_state_dict(stored, strict=False)
    return mod.eval().to(device)


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """A fixture's stack (the drop-in's own rmd.ops.dicl_stack on the CPU) with its module's folded parameters, the
    float64 cost, e and the tolerance."""
    import torch
    from rmd import ops
    g = fixture(name)
    mod = build_module(name)
    with torch.no_grad():
        weights, biases = mod.mnet.folded()
        stack = ops.dicl_stack(torch.from_numpy(g["fmap1"]), torch.from_numpy(g["fmap2"]), torch.from_numpy(g["coords"]),
                               int(g["radius"]), extra_delta=str(g["cmod"]) == "dicl-emb").numpy()
    weights, biases = [t.detach().numpy().copy() for t in weights], [t.detach().numpy().copy() for t in biases]
    b, du, dv, c_in, h, w = stack.shape

    def ref(stack, weights, biases, products=None):
        return net_ref(stack.reshape(-1, c_in, h, w), weights, biases, products).reshape(b, du, dv, h, w)
    return _with_tolerances({"args": (stack, weights, biases)}, ref)
