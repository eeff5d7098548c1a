"""End to end without MIOpen: RAFT 12-iteration inference at 436x1024 as test_gpu_update_block_e2e.py runs it (fp32
correlation, the update block and the upsampler on the fused HIP operators), with the two encoders replaced as well:
net.fnet by rmd.encoders.FeatureEncoder(256, "instance", fused="on") and net.cnet by
rmd.encoders.FeatureEncoder(256, "batch", fused="on"), in their fp32 (split-bf16) mode.  The state-dict keys are the
same, so det_init_fanin gives them the fixture's weights.

Gates: that file's own fp32 ones — |EPE - EPE_ref| <= 1e-3 px after every iteration, sampled flow <= 1e-2 px.
The bf16 mode is measured by tools/encoder_probe.py and not asserted here.
"""

import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from detinit import det_init_fanin
from e2e.raft_net import RaftNet
from synth import epe, frame_pair

pytestmark = pytest.mark.gpu


def test_raft_12_iterations_with_the_fused_encoders_match_the_reference():
    import rmd.encoders
    import rmd.raft
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    g = load_golden("e2e_raft_436x1024")
    h, w, iters = int(g["height"]), int(g["width"]), int(g["iterations"])
    net = RaftNet(rmd.raft.CorrBlock, precision="fp32", upnet_cls=rmd.raft.Up8Network)
    net.fnet = rmd.encoders.FeatureEncoder(256, "instance", fused="on")
    net.cnet = rmd.encoders.FeatureEncoder(256, "batch", fused="on")
    net.update_block = rmd.raft.BasicUpdateBlock(324, gru_fused="on", fused="on")
    net.upnet = rmd.raft.Up8Network(128, fused="on")
    net = det_init_fanin(net).eval().cuda()
    assert sorted(net.state_dict().keys()) == sorted(g["keys"].tolist())
    img1, img2, gt = frame_pair(h, w)
    with torch.no_grad():
        flows = [f.cpu().numpy() for f in net(torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda(), iters)]
    d_epe = [abs(epe(f, gt) - float(r)) for f, r in zip(flows, g["epe"])]
    d_flow = {}
    for k in (1, 4, 12):
        f = flows[k - 1][0, :, :h, :w].reshape(2, -1)[:, g["pixels"]]
        d_flow[k] = float(np.abs(f - g[f"flow_it{k}"]).max())
    report = {"network": "encoders + gru + motion encoder + flow head + up8 fused fp32", "epe_ref_it12": float(g["epe"][-1]),
              "epe_it12": epe(flows[-1], gt), "max_abs_epe_diff": max(d_epe), "epe_diff_it12": d_epe[-1],
              "max_flow_diff_px": d_flow}
    print(json.dumps(report))
    assert max(d_epe) <= 1e-3, report
    assert max(d_flow.values()) <= 1e-2, report
