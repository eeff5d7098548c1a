"""The lookup's outputs, bit for bit: sha256 of corr_lookup's result bytes against digests recorded from
the build before the lookup's instruction stream was reworked (tests/golden/lookup_digests.json,
tools/lookup_digests.py --record).  Cases and inputs: tests/lookup_digest_cases.py."""
import json
import os

import pytest

import lookup_digest_cases as lc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookup_digests.json")


def test_cases_cover_every_phase_and_have_a_digest():
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(lc.case_id(*c) for c in lc.all_cases())
    for shape in lc.SHAPES:
        for radius in lc.RADII:
            seen = lc.phase_coverage(shape, radius)
            assert seen == {(lvl, sh, par) for lvl in (0, 1) for sh in range(4) for par in range(2)}, (shape, radius)


_PYR = {}


def _pyramid(kind, shape):
    import torch

    from rmd import _lib, library
    if (kind, shape) not in _PYR:
        pyr = lc.build_pyramid(kind, shape, torch.device("cuda:0"))
        dtype, tiles = lc.EXPECT[kind]
        assert str(pyr.data.dtype) == "torch." + dtype
        assert (library.pyramid_layout(pyr.data) == _lib.RMD_LAYOUT_TILES) == tiles
        _PYR[kind, shape] = pyr
    return _PYR[kind, shape]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,radius,shape", lc.all_cases(), ids=[lc.case_id(*c) for c in lc.all_cases()])
def test_lookup_output_digest(kind, radius, shape):
    import torch
    want = json.load(open(GOLDEN))[lc.case_id(kind, radius, shape)]
    assert lc.digest(_pyramid(kind, shape), shape, radius, torch.device("cuda:0")) == want
