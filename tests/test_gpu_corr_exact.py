"""The RAFT correlation forward against exact expectations, in every compute mode (tests/corr_exact_cases.py).

Inputs are integers over powers of two and every scale a power of two, so no rounding happens before the
storage conversion: a GEMM must store the float64 pyramid rounded once (fp16 RNE, RMD_S24, or nothing),
and the pyramid tests assert BIT EQUALITY of every element of every level — in the default bf16 mode too,
whose Gaussian-input tests allow 1e-2.  The lookups (rmd_corr_lookup on the stored pyramid,
rmd_corr_otf_lookup on its virtual one) are compared per element with the float64 lookup of those exact
values within K * 2^-24 * M, K = 8 derived from the kernels' operation sequence (corr_exact_cases
docstring), M the largest |value| of the query's own level map; non-finite expectations by NaN position.
Every test prints a `corr-exact:` line (route, worst err / bound, elements compared).

Routes (rmd_corr_gemm_kernel is asserted per case): w8, x3 (S24 and f32) and tiled (bf16 and f32 operands,
f32 and fp16 storage).  Not reachable at these sizes and left with their own tests: the stationary GEMM
(a 4K map, test_stationary_path_4k_sampled_vs_oracle), the x3 balanced-schedule splits (batch 8 at 48 x 96,
test_x3_balanced_schedule_whole_pyramid_vs_exact in test_gpu_corr.py) and the lookup's non-buffer
path (level slabs of 2 GiB per image: the 4K test).  The on-the-fly cases reach the compiled and the
runtime channel loops, the MFMA box path, the per-query path and the 16 x 4 query blocks of wide bf16 maps
(tests/test_corr_exact.py::test_otf_cases_reach_every_lookup_path states which case reaches which).
"""
import numpy as np
import pytest
import torch

import corr_exact_cases as ce
import lookup_digest_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"
_DIGEST_KIND = {case.name: key for key, case in ce.DIGEST_PYRAMID.items()}
_PYR = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _report(line):
    print(f"corr-exact: {line}")


def _pyramid(case):
    """The case's pyramid on the GPU (built once): the digest cases' through their own builder."""
    from rmd import ops
    if case.name not in _PYR:
        ft = case.features()
        if case.name in _DIGEST_KIND:
            kind, shape = _DIGEST_KIND[case.name]
            pyr = lc.build_pyramid(kind, shape, torch.device("cuda:0"))
        else:
            pyr = ops.corr_pyramid(_t(ft.fmap1), _t(ft.fmap2), ce.LEVELS, case.precision, scale=case.scale)
        assert pyr.scale == case.scale and pyr.channels == case.gemm_channels
        _PYR[case.name] = pyr
    return _PYR[case.name]


@pytest.mark.parametrize("case", ce.PYRAMID_CASES, ids=[c.name for c in ce.PYRAMID_CASES])
def test_pyramid_is_bit_exact(case):
    """Every element of every level equals the float64 pyramid rounded once by the storage rule."""
    from rmd import _lib
    name, storage, d = ce.library_route(case)
    assert (name, storage) == (case.route, case.storage)
    want = case.stored()
    pyr = _pyramid(case)
    assert (pyr.desc.storage, pyr.desc.layout) == (d.storage, d.layout)
    assert (pyr.desc.layout == _lib.RMD_LAYOUT_TILES) == (name == "w8")
    torch.cuda.synchronize()
    n, bad = 0, []
    for l in range(ce.LEVELS):
        got = pyr.unpack(l).cpu().numpy().reshape(want[l].shape)
        miss = ce.pyramid_mismatches(got, want[l])
        n += got.size
        if miss:
            k = tuple(np.argwhere(got.view(np.int32) != want[l].view(np.int32))[0])
            bad.append(f"level {l}: {miss} of {got.size} differ, first at (b, query, y, x) = {k}: "
                       f"got {got[k]!r} ({got.view(np.uint32)[k]:#010x}) want {want[l][k]!r} ({want[l].view(np.uint32)[k]:#010x})")
    _report(f"pyramid {case.name}: route {name}, storage {storage}, {n} elements, {len(bad)} levels differ")
    assert not bad, "; ".join(bad)


_LOOKUP_CASES = [(k, s, r) for k in lc.KINDS for s in lc.SHAPES for r in ce.ALL_RADII]


@pytest.mark.parametrize("kind,shape,radius", _LOOKUP_CASES, ids=[lc.case_id(k, r, s) for k, s, r in _LOOKUP_CASES])
def test_lookup_vs_float64_on_the_stored_pyramid(kind, shape, radius):
    """The outputs the lookup digests pin (hand-placed queries included), and the radii between them,
    against the float64 lookup of the exact stored pyramid: unmasked, and with level 1 masked."""
    from rmd import ops
    case = ce.DIGEST_PYRAMID[kind, shape]
    stored = case.stored()
    pyr = _pyramid(case)
    assert str(pyr.data.dtype) == "torch." + lc.EXPECT[kind][0]
    h, w = shape
    co = lc.coords(shape)
    bound = ce.lookup_bound(stored, radius, h, w)
    worst, n = 0.0, 0
    for mask in ce.lookup_masks():
        got = ops.corr_lookup(pyr, _t(co), radius, mask_costs=list(mask)).cpu().numpy()
        ref = ce.lookup_reference(stored, co, radius, mask)
        assert got.dtype == np.float32
        try:
            wm, nm = ce.check_lookup(got, ref, bound)
        except AssertionError as e:
            raise AssertionError(f"{lc.case_id(kind, radius, shape)} mask {mask}: {e}") from None
        worst, n = max(worst, wm), n + nm
    _report(f"lookup {lc.case_id(kind, radius, shape)}: pyramid {case.route}/{case.storage}, worst err/bound "
            f"{worst:.3f}, {n} elements")


_OTF = [(c, p) for c in ce.OTF_CASES for p in c.precisions]


@pytest.mark.parametrize("case,precision", _OTF, ids=[f"{c.name}-{p}" for c, p in _OTF])
def test_otf_lookup_vs_float64_on_the_virtual_pyramid(case, precision):
    """rmd_corr_otf_prepare + rmd_corr_otf_lookup against the float64 lookup of the virtual pyramid
    (fmap1 * scale)^T P_l, P_l rounded to bf16 in the bf16 mode; sampled queries where the volume of all
    of them would not fit."""
    from rmd import ops
    ft = case.features()
    b, h, w = case.b, case.h, case.w
    co = case.coords()
    st = ops.otf_prepare(_t(ft.fmap1), _t(ft.fmap2), case.levels, precision, scale=case.scale)
    got = ops.otf_lookup(st, _t(co), case.radius, mask_costs=list(case.mask)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (b, case.levels * (2 * case.radius + 1) ** 2, h, w)
    q = None
    if case.sample is not None:
        q = case.queries()
        got = got.reshape(b, -1, h * w)[:, :, q].reshape(b, -1, 1, len(q))
        co = np.ascontiguousarray(co.reshape(b, 2, h * w)[:, :, q].reshape(b, 2, 1, len(q)))
    levels = ce.otf_levels(case, precision, q)
    ref = ce.lookup_reference(levels, co, case.radius, case.mask)
    bound = ce.lookup_bound(levels, case.radius, co.shape[2], co.shape[3])
    worst, n = ce.check_lookup(got, ref, bound)
    paths = sorted({p for _, p in ce.otf_box_paths(case, precision)})
    _report(f"otf {case.name} [{precision}]: channels {ce.otf_channel_path(case, precision)}, blocks "
            f"{'x'.join(map(str, ce.otf_block_shape(case, precision)))}, boxes {'+'.join(paths)}, worst err/bound "
            f"{worst:.3f}, {n} elements")
