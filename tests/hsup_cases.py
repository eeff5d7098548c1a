"""Shared helpers of test_hsup.py / test_gpu_hsup.py: the fixtures of tests/golden/gen_golden_hsup.py
(loaded once per process and never modified), the tests' own numpy float64 restatement of the local
cross-attention of HUpCrossAttn (forward and analytic backward), the gate and the shape sweep.

Gate: conftest.rel_max_err (max |got - ref| / max |ref|, NaN positions identical) <= 1e-5 for out,
grad_q, grad_k and grad_v — the project's gate for its fp32 softmax kernels (dicl_head_cases.GATE).
reference_fp32_errors() evaluates the reference's own fp32 composition (the CPU kernels of the
operators, rmd/cpu.py: hsup.py:71-92 op for op) against the float64 restatement on every sweep case;
test_hsup.py asserts that it stays within a quarter of the gate, which makes the gate a condition on the
inputs: a case on which fp32 itself is less accurate than that must be changed, not the gate.

Sweep inputs: q and k are scaled so that the logits have a standard deviation of 3 (within about +-10);
PEAKED scales them to a standard deviation of 12, where one logit of most pixels is far above the rest.
"""

import functools
import zlib

import numpy as np

from conftest import load_golden

GATE = 1e-5
REFERENCE_SHARE = 0.25      # of the gate: the most the reference's own fp32 composition may use up

MODULE_FIXTURES = ["hsup_crossattn_b2_c8_3x5_f2x2", "hsup_crossattn_b1_c6_3x2_f1x4"]
BILINEAR_FIXTURE = "hsup_bilinear_b2_c5_3x4_f2x2"
CORE_FIXTURE = "hsup_core_nonfinite_b1_6x9_f2x2"
CROSSATTN_KEYS = ["conv_k", "conv_out", "conv_q", "conv_v_init", "conv_v_prev"]

# the kernels' tile (csrc/hsup.hip): a block covers TILE_COLS fine columns and TILE_ROWS fine rows (the generic
# route) or TILE_ROWS coarse rows (the 3x3 / 2x2 route), and stages CHUNK or CHUNK / 2 channels at a time; a gather
# thread owns GROUP channels
TILE_COLS, TILE_ROWS, CHUNK, GROUP = 64, 4, 16, 8

# (b, ck, cv, h2, w2, fy, fx, wy, wx)
SWEEP = [
    (1, 5, 7, 1, 1, 1, 1, 3, 3),            # one cell, eight padded neighbours
    (2, 8, 6, 3, 5, 2, 2, 3, 3),            # fast route, odd coarse sizes, every border
    (1, 64, 128, 4, 3, 2, 2, 3, 3),         # the models' channel counts
    (1, 4, 3, 2, 3, 3, 1, 3, 3),            # generic route, unequal factors
    (1, 3, 2, 1, 4, 2, 4, 3, 3),            # generic route, unequal factors
    (1, 16, 8, 2, 70, 2, 2, 3, 3),          # fine row of 140: longer than a wave, with a tail
    # past the tile in both directions with a remainder, channels past a chunk and a group with a remainder:
    (1, CHUNK + 3, CHUNK + 5, TILE_ROWS + 1, TILE_COLS // 2 + 3, 2, 2, 3, 3),       # fast: 10 x 70 fine pixels
    (1, 3, GROUP + 1, TILE_ROWS + 2, TILE_COLS + 3, 1, 1, 5, 5),                    # generic, its widest halo
    (1, 2, 2, 2, 2, 8, 8, 3, 3),            # factor 8
    (1, 4, 3, 3, 4, 2, 2, 1, 1),            # the other window sizes
    (1, 4, 3, 3, 4, 2, 2, 5, 3),
    (1, 4, 3, 3, 4, 2, 2, 1, 5),
]
PEAKED = (2, 8, 6, 3, 5, 2, 2, 3, 3)
FAST, GENERIC = "w3x3_f2x2", "generic"


def route(shape):
    """The route the C ABI's query names for a sweep shape."""
    from rmd import _lib
    b, ck, cv, h2, w2, fy, fx, wy, wx = shape
    return _lib.lib().rmd_local_cross_attn_kernel(b, ck, cv, h2 * fy, w2 * fx, h2, w2, wy, wx).decode()


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_golden(name)


def _windows(t, h, w, wy, wx):
    """(B, c, h2, w2) float64 -> (B, c, wy*wx, h, w): entry j of a fine pixel is the cell
    (Y + jy - wy/2, X + jx - wx/2) around its parent cell, zero outside the map."""
    b, c, h2, w2 = t.shape
    fy, fx = h // h2, w // w2
    py, px = wy // 2, wx // 2
    tp = np.pad(t, ((0, 0), (0, 0), (py, py), (px, px)))
    planes = [np.repeat(np.repeat(tp[:, :, jy:jy + h2, jx:jx + w2], fy, axis=2), fx, axis=3)
              for jy in range(wy) for jx in range(wx)]
    return np.stack(planes, axis=2)


def _softmax64(s):
    with np.errstate(all="ignore"):
        e = np.exp(s - s.max(axis=1, keepdims=True))        # a NaN logit: NaN for the whole pixel
        return e / e.sum(axis=1, keepdims=True)


def forward64(q, k, v, window=(3, 3)):
    """float64: out (B, cv, h, w) and the attention weights a (B, wy*wx, h, w)."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    _, _, h, w = q.shape
    with np.errstate(all="ignore"):
        s = (q[:, :, None] * _windows(k, h, w, *window)).sum(axis=1)
        a = _softmax64(s)
        return (a[:, None] * _windows(v, h, w, *window)).sum(axis=2), a


def _scatter(t, h2, w2, wy, wx):
    """(B, c, wy*wx, h, w) per-entry terms -> (B, c, h2, w2): every term added to the cell it read."""
    b, c, _, h, w = t.shape
    fy, fx = h // h2, w // w2
    py, px = wy // 2, wx // 2
    acc = np.zeros((b, c, h2 + 2 * py, w2 + 2 * px))
    cells = t.reshape(b, c, wy * wx, h2, fy, w2, fx).sum(axis=(4, 6))
    for jy in range(wy):
        for jx in range(wx):
            acc[:, :, jy:jy + h2, jx:jx + w2] += cells[:, :, jy * wx + jx]
    return acc[:, :, py:py + h2, px:px + w2]


def backward64(grad, q, k, v, window=(3, 3)):
    """float64 analytic gradients (grad_q, grad_k, grad_v): da_j = sum_c g[c] v[c, cell_j],
    ds_j = a_j (da_j - sum_i a_i da_i), grad_q = sum_j ds_j k_j, grad_k[cell] = sum ds q, grad_v[cell] = sum a g."""
    grad, q, k, v = (np.asarray(t, dtype=np.float64) for t in (grad, q, k, v))
    _, _, h, w = q.shape
    _, _, h2, w2 = k.shape
    with np.errstate(all="ignore"):
        kw, vw = _windows(k, h, w, *window), _windows(v, h, w, *window)
        a = _softmax64((q[:, :, None] * kw).sum(axis=1))
        da = (grad[:, :, None] * vw).sum(axis=1)
        ds = a * (da - (a * da).sum(axis=1, keepdims=True))
        grad_q = (ds[:, None] * kw).sum(axis=2)
        grad_k = _scatter(ds[:, None] * q[:, :, None], h2, w2, *window)
        grad_v = _scatter(a[:, None] * grad[:, :, None], h2, w2, *window)
    return grad_q, grad_k, grad_v


def _case(shape, logit_std, seed):
    b, ck, cv, h2, w2, fy, fx, wy, wx = shape
    h, w = h2 * fy, w2 * fx
    rng = np.random.default_rng(seed)
    scale = np.float32(np.sqrt(logit_std) / ck ** 0.25)         # std of a logit: scale^2 sqrt(ck)
    q = rng.standard_normal((b, ck, h, w), dtype=np.float32) * scale
    k = rng.standard_normal((b, ck, h2, w2), dtype=np.float32) * scale
    v = rng.standard_normal((b, cv, h2, w2), dtype=np.float32)
    grad = rng.standard_normal((b, cv, h, w), dtype=np.float32)
    out, _ = forward64(q, k, v, (wy, wx))
    grad_q, grad_k, grad_v = backward64(grad, q, k, v, (wy, wx))
    return dict(q=q, k=k, v=v, grad=grad, window=(wy, wx), out=out, grad_q=grad_q, grad_k=grad_k, grad_v=grad_v)


@functools.lru_cache(maxsize=None)
def sweep_case(shape):
    """Seeded inputs of one SWEEP shape with their float64 results.  Shared; never modified."""
    return _case(shape, 3.0, zlib.crc32(repr(shape).encode()))


@functools.lru_cache(maxsize=None)
def peaked_case():
    return _case(PEAKED, 12.0, 77)


def all_cases():
    return [(f"{s}", sweep_case(s)) for s in SWEEP] + [("peaked", peaked_case())]


RESULTS = ("out", "grad_q", "grad_k", "grad_v")


@functools.lru_cache(maxsize=None)
def reference_fp32_errors():
    """{case label: {result: rel_max_err}} of the reference's fp32 composition on the CPU (the operators' CPU
    kernels) against the float64 restatement.  Printed; test_hsup.py holds it to REFERENCE_SHARE * GATE."""
    import torch
    import rmd  # noqa: F401
    from conftest import rel_max_err
    errors = {}
    for label, c in all_cases():
        t = [torch.from_numpy(c[n]) for n in ("q", "k", "v")]
        out = torch.ops.rmd.local_cross_attn(*t, *c["window"])
        grads = torch.ops.rmd.local_cross_attn_backward(torch.from_numpy(c["grad"]), *t, *c["window"])
        errors[label] = {n: rel_max_err(g.numpy(), c[n]) for n, g in zip(RESULTS, (out,) + tuple(grads))}
        print(f"reference fp32 vs float64 {label}: " + " ".join(f"{n} {e:.2e}" for n, e in errors[label].items()))
    return errors


def run_module(name, device):
    """A module fixture through rmd.hsup on `device` -> ({name: numpy result}, sorted state-dict keys)."""
    import torch
    import rmd
    from detinit import det_init
    g = fixture(name)
    cls = rmd.hsup.HUpBilinear if name == BILINEAR_FIXTURE else rmd.hsup.HUpCrossAttn
    m = det_init(cls(int(g["channels"]))).to(device)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    h_prev, h_init = t(g["h_prev"]).requires_grad_(True), t(g["h_init"]).requires_grad_(True)
    out = m(h_prev, h_init)
    names, params = zip(*m.named_parameters())
    grads = torch.autograd.grad(out, (h_prev, h_init) + params, t(g["grad"]))
    res = {"out": out, "grad_h_prev": grads[0], "grad_h_init": grads[1],
           **{"grad_" + n: gr for n, gr in zip(names, grads[2:])}}
    return {n: r.detach().cpu().numpy() for n, r in res.items()}, sorted(m.state_dict().keys())
