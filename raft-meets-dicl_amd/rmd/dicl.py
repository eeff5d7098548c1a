"""DICL baseline cost volume — drop-in for FlowLevel.compute_cost (src/models/impls/dicl.py:212-241)
and the feature warp in front of it (FlowLevel.forward, :171-184).

`compute_cost(mnet, feat1, feat2, maxdisp)` builds the masked integer-displacement volume with one
rmd_dicl_stack_int pass and runs the (unchanged) MatchingNet on it.  With `flow` given, feat2 is first
warped back by it (common/warp.py) inside the same kernel pair (rmd_dicl_stack_int_warped), so the
warped map never makes the reference's extra grid_sample/mask round trip.

`FlowLevelCostMixin` gives a reference FlowLevel the same methods:
    class FlowLevel(FlowLevelCostMixin, reference.FlowLevel)
Its forward reproduces FlowLevel.forward (coarse flow upsampled x2, detached) and hands the flow to
compute_cost instead of warping feat2 separately.

The flow head of a level — `FlowRegression` (dicl.py:53-85) and `FlowEntropy` (dicl.py:31-50), drop-ins
for the reference classes — is one rmd_dicl_flow_head pass over the cost (rmd.ops.dicl_flow_head).
`FlowLevelHeadMixin.compute_flow` reproduces FlowLevel.compute_flow (dicl.py:186-210) with ONE head
launch per level: the head's (B, 3, h, w) output is the flow (coarse flow added) and the entropy, in the
channel order the context network's input starts with.  `FlowLevelMixin` combines both mixins:
    class FlowLevel(FlowLevelMixin, reference.FlowLevel)
keeps the reference's sub-modules (mnet, dap, flow, entropy, ctxnet) and state-dict keys; forward hooks
on mnet, dap and ctxnet fire as before (the parameter-free `flow` and `entropy` children stay in place
but the fused head runs instead of them).
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


def cost_volume(feat1, feat2, maxdisp, flow=None):
    """(B,C,h,w) x2 [+ flow (B,2,h,w)] -> (B, 2ru+1, 2rv+1, 2C, h, w) masked matching volume."""
    ru, rv = (int(m) for m in maxdisp)
    if flow is not None:
        return ops.dicl_stack_int_warped(feat1, feat2, flow, ru, rv)
    return ops.dicl_stack_int(feat1, feat2, ru, rv)


def compute_cost(mnet, feat1, feat2, maxdisp, flow=None):
    return mnet(cost_volume(feat1, feat2, maxdisp, flow))


class FlowLevelCostMixin:
    _warp_flow = None

    def forward(self, img1, feat1, feat2, flow_coarse, raw=False, dap=True, ctx=True, scale=1.0):
        _, _, h, w = feat1.shape
        flow_up = None
        if flow_coarse is not None:
            flow_up = (2.0 * F.interpolate(flow_coarse, (h, w), mode="bilinear", align_corners=True)).detach()
        self._warp_flow = flow_up                  # consumed by compute_cost (fused warp)
        try:
            return self.compute_flow(img1, feat1, feat2, flow_up, raw, dap, ctx, scale)
        finally:
            self._warp_flow = None

    def compute_cost(self, feat1, feat2):
        return compute_cost(self.mnet, feat1, feat2, self.maxdisp, self._warp_flow)


class FlowRegression(nn.Module):
    """Soft-argmin flow regression: cost (B, du, dv, h, w) -> flow (B, 2, h, w) (dicl.py:53-85)."""

    def __init__(self):
        super().__init__()

    def forward(self, cost):
        return ops.dicl_flow_head(cost)[0]


class FlowEntropy(nn.Module):
    """Normalised entropy of the displacement softmax: (B, du, dv, h, w) -> (B, h, w) (dicl.py:31-50)."""

    def __init__(self, eps=1e-9):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        return ops.dicl_flow_head(x, None, self.eps)[1][:, 0]


class FlowLevelHeadMixin:
    def compute_flow(self, img1, feat1, feat2, flow_coarse, raw, dap, ctx, scale):
        _, _, h, w = feat1.shape

        cost = self.compute_cost(feat1, feat2)                      # dicl.py:190-191
        cost = self.dap(cost) if dap else cost

        # flow + flow_coarse and the entropy in one pass (dicl.py:194-195, 202)
        eps = getattr(getattr(self, "entropy", None), "eps", 1e-9)
        head = torch.ops.rmd.dicl_flow_head(cost, flow_coarse, float(eps))
        flow = head[:, :2]
        flow_raw = flow if raw else None

        if ctx:                                                     # dicl.py:199-208
            img1 = F.interpolate(img1, (h, w), mode="bilinear", align_corners=True)
            ctxf = torch.cat((head.detach(), feat1, img1), dim=1)   # flow, entropy, features, image
            flow = flow + self.ctxnet(ctxf) * scale

        return flow, flow_raw


class FlowLevelMixin(FlowLevelCostMixin, FlowLevelHeadMixin):
    pass
