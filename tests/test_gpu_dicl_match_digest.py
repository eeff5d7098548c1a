"""The dicl-1x1 match kernels' outputs, bit for bit: sha256 of the result bytes of the fused cost (both
computes), the training forward and every deterministic backward output against digests recorded from the
build before the two kernels came to share csrc/dicl_match_common.h (tests/golden/match_digests.json,
tools/dicl_match_digests.py --record).  Cases and inputs: tests/dicl_match_digest_cases.py.

Every case holds a NaN coordinate, so bwd.gW2, bwd.gW3 and bwd.gw4 are all-NaN tensors (and half of bwd.gW1):
those digests pin the NaN pattern only.  The values of the parameter gradients are pinned by the bwd_finite.*
digests, taken with the two non-finite positions moved onto the map."""
import json
import os

import pytest

import dicl_match_digest_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_digests.json")
IDS = [dc.case_id(s) for s in dc.CASES]


def test_every_case_has_every_digest_and_masks_few_units():
    want = json.load(open(GOLDEN))
    assert len(want["source_hash"]) == 16
    assert sorted(want["digests"]) == sorted(IDS)
    for shape in dc.CASES:
        assert sorted(want["digests"][dc.case_id(shape)]) == sorted(dc.OUTPUT_NAMES), shape
        masked = dc.masked_fraction(shape)
        print(f"{dc.case_id(shape)}: {masked:.4f} of the hidden units masked")
        assert masked <= dc.MASKED_CAP, (shape, masked)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", dc.CASES, ids=IDS)
def test_match_output_digests(shape):
    import torch
    want = json.load(open(GOLDEN))["digests"][dc.case_id(shape)]
    got = dc.digests(shape, torch.device("cuda:0"))
    assert [n for n in dc.OUTPUT_NAMES if got[n] != want[n]] == []
