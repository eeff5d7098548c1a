"""Hybrid-model parity with the fused k x k MatchingNet: the ctf_l3_fwd_384x512 fixture (tests/golden/gen_ctf_l3.py,
the reference's own run) through tests/e2e CtfL3Net whose three correlation modules are built with fused="on", at
the gate of test_gpu_ctf_l3.py: |EPE - EPE_ref| <= 1e-3 px for every 1/8-level output.  The fp32 mode is asserted;
the bf16 mode is measured and reported, not asserted."""

import json

import pytest
import torch

from conftest import load_golden
from detinit import det_init_fanin
from e2e.ctf_l3_net import CtfL3Net
from synth import epe, frame_pair

pytestmark = pytest.mark.gpu

HEAD_GAIN = 0.02
FIXTURE = "ctf_l3_fwd_384x512"


def _net(**fused):
    import rmd
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def make_cmod(*args, **kwargs):
        return rmd.corr.make_cmod(*args, **kwargs, **fused)

    net = CtfL3Net(make_cmod, rmd.corr.make_flow_regression, upnet_cls=rmd.raft.Up8Network)
    return det_init_fanin(net, head_gain=HEAD_GAIN).cuda().eval()


def _epe_diffs(net, g):
    h, w, pad = int(g["height"]), int(g["width"]), int(g["pad"])
    iters = tuple(int(i) for i in g["iterations"])
    img1, img2, gt = frame_pair(h, w, pad=pad)
    calls = []
    hooks = [m.mnet.register_forward_hook(lambda mod, i, o: calls.append(mod.fused))
             for m in (net.corr_3, net.corr_4, net.corr_5)]
    with torch.no_grad():
        out3 = net(torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda(), iters)[2]
    for hook in hooks:
        hook.remove()
    assert len(calls) == sum(iters) and set(calls) == {"on"}          # every cost came from the fused path, once per iteration
    return [abs(epe(f.cpu().numpy(), gt) - float(r)) for f, r in zip(out3, g["epe3"])]


def test_ctf_l3_forward_with_the_fused_matching_net():
    g = load_golden(FIXTURE)
    net = _net(fused="on")
    assert sorted(net.state_dict().keys()) == sorted(g["keys"].tolist())
    d32 = _epe_diffs(net, g)
    d16 = _epe_diffs(_net(fused="on", precision="bf16"), g)
    rep = {"fixture": FIXTURE, "max_abs_epe_diff_fp32": max(d32), "max_abs_epe_diff_bf16_not_asserted": max(d16),
           "epe_ref": g["epe3"].tolist()}
    print(json.dumps(rep))
    assert max(d32) <= 1e-3, rep
