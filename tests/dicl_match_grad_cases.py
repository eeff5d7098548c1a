"""Shared helpers of test_dicl_match_grad.py / test_gpu_dicl_match_grad.py: the float64 oracle of the fused
dicl-1x1 cost's backward, a float64 emulation of the kernel's roundings, the ReLU guard, the tolerance rule
and the cases.  Inputs, weights and the forward restatement are dicl_match_cases' (never modified).

Oracle: dicl_match_cases._columns (oracle.dicl.dicl_stack), the MLP and its backward in float64 numpy

    a0 = x; z_l = W_l a_{l-1} + t_l; a_l = relu(z_l)  (l = 1..3); cost = w4 . a3 + b4
    dz3 = (z3 > 0) ? w4 g : 0        gw4 += a3 g        gb4 += g
    da_{l-1} = W_l^T dz_l            dz_{l-1} = (z_{l-1} > 0) ? da_{l-1} : 0
    gW_l += dz_l a_{l-1}^T           gt_l += dz_l

and oracle.dicl.dicl_stack_backward for the adjoint of the gather (grad_fmap1, grad_fmap2).

Emulation: the same formulas with the kernel's roundings — every operand of a matrix product rounded to
fp32 and split into the bfloat16 hi part and the bfloat16 of the residual, each product hi.hi + hi.lo +
lo.hi summed in float64, activations and dz_l rounded to fp32 between layers, masks from the emulated
forward; dz3, gw4, gb4 and gt_l from fp32 values in float64.

ReLU guard (a condition on the inputs, not a tolerance): the derivative is discontinuous at z = 0, so any
fp32 implementation differs from float64 by whole units there.  band_l = 4 max|z_l(emulation) -
z_l(float64)|; a column is guarded if any float64 pre-activation lies within its layer's band, and the
cases' grad_cost (seeded normal) is ZERO on guarded columns, so they contribute nothing on either side.
At most GUARD_CAP of a case's columns may be guarded (asserted in the CPU test).

Tolerance: per case and per output, e = max|emulation - float64| / max|float64| (CPU only) and the gate is
max(1e-5, 3 e) — dicl_match_cases' rule; the CPU test also asserts e <= E_MAX so that a wrong emulation
cannot widen the gate.  Nothing here comes from the kernel.
"""

import functools
import zlib

import numpy as np

import dicl_match_cases as fwd
from conftest import load_golden

FLOOR, FACTOR = fwd.FLOOR, fwd.FACTOR
GUARD_CAP = 0.10
E_MAX = 2e-5
BAND = 4.0

OUTPUTS = ("grad_fmap1", "grad_fmap2", "gW1", "gW2", "gW3", "gw4", "gt1", "gt2", "gt3", "gb4")
DETERMINISTIC = tuple(n for n in OUTPUTS if n != "grad_fmap2")     # grad_fmap2: float atomics (include/rmd.h)

FIXTURES = ["match_grad_bn_b2_c16_8x12", "match_grad_none_b1_c32_6x10", "match_grad_nan_b2_c16_8x12"]
NAN_FIXTURE = "match_grad_nan_b2_c16_8x12"
FORWARD_FIXTURE = dict(zip(FIXTURES, fwd.FIXTURES))

# more work items (2 x 144 strips) than the kernel's grid (one workgroup per CU): the persistent loop
MORE_THAN_GRID = (2, 16, 48, 96, 1, (32, 32, 32))
SWEEP = fwd.SWEEP + [fwd.WIDEST, MORE_THAN_GRID]


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_golden(name)


def _mats(weights, biases, dtype):
    ws = [np.asarray(w, dtype).reshape(w.shape[0], -1) for w in weights[:3]] + [np.asarray(weights[3], dtype).reshape(-1)]
    ts = [np.asarray(t, dtype).reshape(-1) for t in biases]
    return ws, ts


def forward64(x, weights, biases):
    """Pre-activations [z1, z2, z3] and activations [x, a1, a2, a3] of the float64 restatement."""
    ws, ts = _mats(weights, biases, np.float64)
    zs, acts = [], [x]
    with np.errstate(all="ignore"):
        for wt, t in zip(ws[:3], ts[:3]):
            zs.append(wt @ acts[-1] + t[:, None])
            acts.append(fwd.relu64(zs[-1]))
    return zs, acts


def _prod3(a, b):
    """a @ b as the kernel's three products: operands rounded to fp32 and split, hi.hi + hi.lo + lo.hi."""
    ah, al = fwd.split_bf16(np.asarray(a, np.float32))
    bh, bl = fwd.split_bf16(np.asarray(b, np.float32))
    with np.errstate(all="ignore"):
        return ah @ bh + ah @ bl + al @ bh


def forward_emulated(x, weights, biases):
    ws, ts = _mats(weights, biases, np.float32)
    zs, acts = [], [x.astype(np.float32)]
    with np.errstate(all="ignore"):
        for wt, t in zip(ws[:3], ts[:3]):
            zs.append((_prod3(wt, acts[-1]) + t.astype(np.float64)[:, None]).astype(np.float32))
            acts.append(fwd.relu64(zs[-1]).astype(np.float32))
    return zs, acts


def _backward(zs, acts, weights, g, emulated):
    """(dx, [gW1, gW2, gW3], gw4, [gt1, gt2, gt3], gb4) of the formulas above; `emulated` rounds as the
    kernel does, else everything is float64."""
    ws, _ = _mats(weights, [np.zeros(1)] * 4, np.float32 if emulated else np.float64)
    rnd = (lambda v: v.astype(np.float32)) if emulated else (lambda v: v)
    mm = _prod3 if emulated else (lambda a, b: a @ b)
    g = rnd(np.asarray(g, np.float64))
    with np.errstate(all="ignore"):
        w4g = ws[3][:, None] * g[None, :] if emulated else ws[3].astype(np.float64)[:, None] * g[None, :]
        dz = rnd(np.where(zs[2] > 0, w4g, 0.0))
        gw4 = acts[3].astype(np.float64) @ g.astype(np.float64)
        gb4 = g.astype(np.float64).sum()
        gws, gts = [None] * 3, [None] * 3
        for l in (2, 1, 0):
            gws[l] = mm(dz, acts[l].T)
            gts[l] = dz.astype(np.float64).sum(axis=1)
            da = rnd(mm(ws[l].T, dz))
            if l > 0:
                dz = rnd(np.where(zs[l - 1] > 0, da, 0.0))
    return da.astype(np.float64), gws, gw4, gts, gb4


def _outputs(args, g, emulated):
    f1, f2, coords, radius, weights, biases = args
    from oracle.dicl import dicl_stack_backward
    x, shape = fwd._columns(f1, f2, coords, radius)
    zs, acts = (forward_emulated if emulated else forward64)(x, weights, biases)
    dx, gws, gw4, gts, gb4 = _backward(zs, acts, weights, g.reshape(-1), emulated)
    b, d, _, h, w = shape
    gstack = dx.reshape(dx.shape[0], b, d, d, h, w).transpose(1, 2, 3, 0, 4, 5)
    with np.errstate(all="ignore"):
        gf1, gf2 = dicl_stack_backward(np.asarray(f2).shape, np.asarray(coords, np.float64), radius,
                                       np.ascontiguousarray(gstack))
    vals = [gf1, gf2, *gws, gw4, *gts, np.asarray([gb4])]
    return dict(zip(OUTPUTS, vals))


def guard(args):
    """Boolean (B, d, d, h, w): columns with a float64 pre-activation inside its layer's band."""
    f1, f2, coords, radius, weights, biases = args
    x, shape = fwd._columns(f1, f2, coords, radius)
    z64, _ = forward64(x, weights, biases)
    zem, _ = forward_emulated(x, weights, biases)
    hit = np.zeros(x.shape[1], dtype=bool)
    with np.errstate(all="ignore"):
        for a, e in zip(z64, zem):
            diff = np.abs(e.astype(np.float64) - a)
            band = BAND * diff[np.isfinite(diff)].max()
            hit |= (np.abs(a) <= band).any(axis=0)
    return hit.reshape(shape)


def guarded_grad(args, seed):
    """(grad_cost float32, guarded fraction): seeded normal, zero on guarded columns."""
    hit = guard(args)
    g = np.random.default_rng(seed).standard_normal(hit.shape).astype(np.float32)
    g[hit] = 0.0
    return g, float(hit.mean())


def max_norm_err(got, ref):
    """dicl_match_cases.max_norm_err; an all-NaN or all-zero reference pins positions / exact zeros only."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions differ"
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    scale = np.abs(ref[fin]).max()
    err = np.abs(got[fin] - ref[fin]).max()
    return float(err / scale) if scale > 0 else float(err)


def _with_tolerances(case, seed):
    g, frac = guarded_grad(case["args"], seed)
    case.update(grad=g, guarded=frac, ref=_outputs(case["args"], g, False))
    emu = _outputs(case["args"], g, True)
    case["e"] = {k: max_norm_err(emu[k], case["ref"][k]) for k in OUTPUTS}
    case["tol"] = {k: max(FLOOR, FACTOR * e) for k, e in case["e"].items()}
    return case


@functools.lru_cache(maxsize=None)
def sweep_case(shape):
    """dicl_match_cases.sweep_case's inputs with the guarded grad_cost, the float64 gradients, e and tol."""
    return _with_tolerances({"args": fwd.sweep_case(shape)["args"]}, zlib.crc32(("grad" + repr(shape)).encode()))


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """A gradient fixture's case: the forward fixture's inputs and folded parameters, the STORED grad_cost."""
    case = _with_tolerances({"args": fwd.fixture_case(FORWARD_FIXTURE[name])["args"]}, fixture_seed(name))
    assert np.array_equal(case["grad"], fixture(name)["nodap.grad_out"].reshape(case["grad"].shape)), \
        "the stored grad_out is not this module's guarded gradient: regenerate the fixture"
    return case


def fixture_seed(name):
    return zlib.crc32(("grad" + name).encode())


def all_cases():
    return ([(n, functools.partial(fixture_case, n)) for n in FIXTURES]
            + [(repr(s), functools.partial(sweep_case, s)) for s in SWEEP])


def build_module(name, device="cpu", **kwargs):
    """dicl_match_cases.build_module of the forward fixture a gradient fixture belongs to."""
    return fwd.build_module(FORWARD_FIXTURE[name], device, **kwargs)


def module_gradients(mod, g, dap, device="cpu"):
    """Gradients of a drop-in module as the fixtures store them: the module's output (dap on or off) is
    driven by the stored grad_out and the gradient entering the mnet's cost is multiplied by the stored
    `keep` mask (a tensor hook on the cost, installed by a forward hook on *.mnet), so guarded columns
    contribute nothing.  Returns ({"fmap1", "fmap2", parameter name: gradient as numpy}, hook calls)."""
    import torch
    tag = "dap" if dap else "nodap"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    f1, f2 = t(g["fmap1"]).requires_grad_(True), t(g["fmap2"]).requires_grad_(True)
    keep = t(g["keep"])
    calls = []

    def hook(_m, _i, out):
        calls.append(tuple(out.shape))
        out.register_hook(lambda grad: grad * keep.reshape(grad.shape))

    for p in mod.parameters():
        p.grad = None
    handle = mod.mnet.register_forward_hook(hook)
    try:
        out = mod(f1, f2, t(g["coords"]), dap=dap)
    finally:
        handle.remove()
    out.backward(t(g[f"{tag}.grad_out"]))
    grads = {"fmap1": f1.grad, "fmap2": f2.grad}
    grads.update({k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
    return {k: v.detach().cpu().numpy() for k, v in grads.items()}, calls
