"""Shared helpers of test_dicl_match.py / test_gpu_dicl_match.py: the fixtures of
tests/golden/gen_golden_dicl_match.py (loaded once per process, never modified), the tests' own float64
restatement of the fused dicl-1x1 cost, a float64 emulation of the kernel's two compute modes, the
tolerance rule and the shape sweep.

Restatement: oracle.dicl.dicl_stack as it is, then the folded MLP in float64 numpy with a ReLU that keeps
NaN.  Emulation of a compute mode: every layer's operands rounded to fp32, split into the bfloat16 hi part
and the bfloat16 of the residual, the products the mode keeps (hi.hi, and for three products hi.lo and
lo.hi) summed in float64, activations rounded to fp32 between layers; the last layer in float64 from the
fp32 activations.

Tolerance: for each case and mode, e = max|emulation - float64| / max|float64| (CPU only), and the kernel
is gated at max(1e-5, 3 e) max-normalised against float64.  The factor 3 covers the fp32 accumulation
order and the spread of a maximum over a few thousand samples; 1e-5 is the project's gate for its
fp32-accumulating kernels.  Nothing here comes from the kernel.
"""

import functools
import zlib

import numpy as np

from conftest import load_golden

FLOOR = 1e-5
FACTOR = 3.0
PRODUCTS = {"fp32": 3, "bf16": 1}

FIXTURES = ["match_bn_b2_c16_8x12", "match_none_b1_c32_6x10", "match_nan_b2_c16_8x12"]
NAN_FIXTURE = "match_nan_b2_c16_8x12"
NAN_PIXELS = ((0, 2, 5), (1, 6, 3))      # (batch, y, x) of the two poisoned coordinates

# (B, C, h, w, r, widths)
SWEEP = [
    (1, 16, 3, 5, 1, (32, 32, 32)),
    (2, 16, 5, 7, 2, (96, 128, 64)),
    (1, 32, 9, 19, 4, (96, 128, 64)),       # the models' sizes: a strip remainder and more than one workgroup
    (2, 64, 4, 33, 3, (96, 128, 64)),       # 2C = 128
    (1, 32, 7, 6, 4, (48, 64, 32)),         # mnet scale 0.5: padded to 64, 64, 32
    (3, 48, 2, 2, 1, (64, 96, 32)),
]
# not in the issue's list: the widest supported network, whose weight fragments do not fit LDS in the
# three-product mode (the kernel's global-memory weight route)
WIDEST = (1, 64, 3, 11, 2, (128, 128, 128))


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_golden(name)


def relu64(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, 0.0, x)          # NaN < 0 is False: NaN stays, as torch.relu


def _columns(f1, f2, coords, radius):
    """(B, d, d, 2C, h, w) float64 stack of the oracle -> columns (2C, B*d*d*h*w) and the output shape."""
    from oracle.dicl import dicl_stack
    with np.errstate(all="ignore"):
        st = dicl_stack(np.asarray(f1, np.float64), np.asarray(f2, np.float64), np.asarray(coords, np.float64), radius)
    b, d, _, c2, h, w = st.shape
    return st.transpose(3, 0, 1, 2, 4, 5).reshape(c2, -1), (b, d, d, h, w)


def reference64(f1, f2, coords, radius, weights, biases):
    """The float64 restatement -> cost (B, d, d, h, w)."""
    x, shape = _columns(f1, f2, coords, radius)
    with np.errstate(all="ignore"):
        for wt, t in zip(weights[:3], biases[:3]):
            x = relu64(np.asarray(wt, np.float64).reshape(wt.shape[0], -1) @ x + np.asarray(t, np.float64).reshape(-1, 1))
        out = np.asarray(weights[3], np.float64).reshape(1, -1) @ x + np.float64(np.asarray(biases[3]).reshape(-1)[0])
    return out.reshape(shape)


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even) as float32; NaN and inf stay."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isfinite(x), r, x)


def split_bf16(x):
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_round(x)
    with np.errstate(invalid="ignore"):
        lo = bf16_round(x - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def emulate(f1, f2, coords, radius, weights, biases, products):
    """The float64 emulation of a compute mode (1 or 3 bf16 products per layer) -> cost (B, d, d, h, w)."""
    x, shape = _columns(f1, f2, coords, radius)
    with np.errstate(all="ignore"):
        for wt, t in zip(weights[:3], biases[:3]):
            wh, wl = split_bf16(np.asarray(wt).reshape(wt.shape[0], -1))
            xh, xl = split_bf16(x.astype(np.float32))
            acc = wh @ xh
            if products == 3:
                acc = acc + wh @ xl + wl @ xh
            x = relu64(acc + np.asarray(t, np.float32).astype(np.float64).reshape(-1, 1)).astype(np.float32)
        out = (np.asarray(weights[3], np.float32).astype(np.float64).reshape(1, -1) @ x.astype(np.float64)
               + np.float64(np.asarray(biases[3], np.float32).reshape(-1)[0]))
    return out.reshape(shape)


def dap_emulate(cost, weight):
    """rmd_dap's arithmetic on an emulated cost (B, d, d, h, w): the cost rounded to fp32, weight (D, D, 1, 1)
    and cost split into bfloat16 hi and residual, hi.hi + hi.lo + lo.hi summed in float64."""
    b, d, _, h, w = cost.shape
    wh, wl = split_bf16(np.asarray(weight).reshape(d * d, d * d))
    xh, xl = split_bf16(cost.reshape(b, d * d, h * w).astype(np.float32))
    with np.errstate(all="ignore"):
        return (wh @ xh + wh @ xl + wl @ xh).reshape(cost.shape)


def max_norm_err(got, ref):
    """max|got - ref| / max|ref| over the finite reference entries; NaN positions must be identical."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions differ"
    fin = np.isfinite(ref)
    return float(np.abs(got[fin] - ref[fin]).max() / np.abs(ref[fin]).max())


def _with_tolerances(case):
    ref = reference64(*case["args"])
    case["ref"] = ref
    case["e"], case["tol"] = {}, {}
    for precision, products in PRODUCTS.items():
        e = max_norm_err(emulate(*case["args"], products), ref)
        case["e"][precision] = e
        case["tol"][precision] = max(FLOOR, FACTOR * e)
    return case


def grid_coords(rng, b, h, w, sigma):
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return np.stack([xs, ys])[None] + rng.normal(0.0, sigma, size=(b, 2, h, w))


@functools.lru_cache(maxsize=None)
def sweep_case(shape):
    """Seeded inputs of one sweep shape — He-initialised layers, coordinates grid + N(0, 2^2) with a tenth
    of the pixels thrown far outside the map — with the float64 result, the per-mode emulation error e and
    the tolerance.  Shared; never modified."""
    b, c, h, w, r, widths = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    f1 = rng.standard_normal((b, c, h, w), dtype=np.float32)
    f2 = rng.standard_normal((b, c, h, w), dtype=np.float32)
    co = grid_coords(rng, b, h, w, 2.0)
    far = rng.random((b, h, w)) < 0.1
    co = np.where(far[:, None], co + rng.choice([-1.0, 1.0], size=(b, 2, h, w)) * rng.uniform(40, 400, (b, 2, h, w)), co)
    weights, biases, cin = [], [], 2 * c
    for cout in widths + (1,):
        weights.append((rng.standard_normal((cout, cin)) * np.sqrt(2.0 / cin)).astype(np.float32))
        biases.append((rng.standard_normal(cout) * 0.1).astype(np.float32))
        cin = cout
    weights[3] = weights[3].reshape(-1)
    return _with_tolerances({"args": (f1, f2, co.astype(np.float32), r, weights, biases)})


def build_module(name, device="cpu", **kwargs):
    """The drop-in module of a fixture in eval mode: det_init weights, then the stored norm state."""
    import torch
    import rmd
    from detinit import det_init
    g = fixture(name)
    c = g["fmap1"].shape[1]
    mod = det_init(rmd.corr.make_cmod("dicl-1x1", c, int(g["radius"]), dap_init="standard",
                                      norm_type=str(g["norm_type"]), mnet_scale=float(g["mnet_scale"]), **kwargs))
    stored = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.") and k != "sd.keys"}
    mod.load_state_dict(stored, strict=False)
    return mod.eval().to(device)


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """A fixture's inputs with its module's folded parameters, the float64 result, e and the tolerance."""
    import torch
    g = fixture(name)
    with torch.no_grad():
        weights, biases = build_module(name).mnet.folded()
    weights, biases = [t.detach().numpy().copy() for t in weights], [t.detach().numpy().copy() for t in biases]
    return _with_tolerances({"args": (g["fmap1"], g["fmap2"], g["coords"], int(g["radius"]), weights, biases)})


def all_cases():
    """(label, case getter) of the three fixtures, the sweep and the widest network."""
    return ([(n, functools.partial(fixture_case, n)) for n in FIXTURES]
            + [(repr(s), functools.partial(sweep_case, s)) for s in SWEEP + [WIDEST]])
