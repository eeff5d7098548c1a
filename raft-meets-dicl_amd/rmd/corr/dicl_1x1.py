"""Drop-in for corr.dicl_1x1.CorrelationModule — src/models/common/corr/dicl_1x1.py:33-86."""

import torch
import torch.nn as nn

from .. import library, ops
from ..blocks.dicl import DisplacementAwareProjection, MatchingNet1x1
from .dicl import _delta


class CorrelationModule(nn.Module):
    """fused: "off" builds the stack and runs the mnet's convolutions (the default); "auto" computes the
    cost with the fused kernel (ops.dicl_match_1x1) where it applies — no gradient needed, a foldable mnet,
    a supported shape — and takes the "off" path elsewhere; "on" raises where "auto" would fall back.
    precision ("fp32" / "bf16") is the fused kernel's compute mode.  fused_backward=True (opt-in) lets the
    fused path serve calls that need a gradient too, through the differentiable operator
    (ops.dicl_match_1x1(differentiable=True)): its backward recomputes the MLP per column, so neither the
    stack nor a hidden activation is kept for it.  That needs precision "fp32", a foldable mnet (eval-mode
    or frozen batch norm, or no norm) and a supported shape."""

    FUSED = ("off", "auto", "on")

    def __init__(self, feature_dim, radius, dap_init="identity", norm_type="batch", relu_inplace=True,
                 mnet_scale=1, fused="off", precision="fp32", fused_backward=False):
        super().__init__()
        if fused not in self.FUSED:
            raise ValueError(f"unknown fused value '{fused}', expected one of {self.FUSED}")
        if precision not in ops.MATCH_PRECISIONS:
            raise ValueError(f"unknown precision '{precision}', expected one of {sorted(ops.MATCH_PRECISIONS)}")
        self.radius = radius
        self.fused = fused
        self.precision = precision
        self.fused_backward = bool(fused_backward)
        self.mnet = MatchingNet1x1(2 * feature_dim, norm_type=norm_type, relu_inplace=relu_inplace, scale=mnet_scale)
        self.dap = DisplacementAwareProjection((radius, radius), init=dap_init)
        self.register_buffer("delta", _delta(radius), persistent=False)
        self.output_dim = (2 * self.radius + 1) ** 2

    def needs_gradient(self, f1, f2, coords):
        """Whether autograd would record this call."""
        return torch.is_grad_enabled() and (any(t.requires_grad for t in (f1, f2, coords))
                                            or any(p.requires_grad for p in self.mnet.parameters()))

    def fused_fallback_reason(self, f1, f2, coords):
        """Why this call cannot take the fused path (None: it can)."""
        grad = self.needs_gradient(f1, f2, coords)
        if grad and not self.fused_backward:
            return "a gradient is needed (the fused operator is not differentiable)"
        if grad and self.precision != "fp32":
            return f"a gradient is needed and precision is '{self.precision}' (the one-product mode has no backward)"
        if not self.mnet.foldable():
            return "the mnet's norm layers need per-call statistics (group, instance or train-mode batch norm)"
        if f1.dim() != 4 or f1.shape != f2.shape:
            return f"fmap shapes {tuple(f1.shape)} / {tuple(f2.shape)}"
        if f1.device.type == "cuda":
            widths = ops.match_padded_widths([block[0].weight for block in list(self.mnet)[:3]])
            if not library.match_supported(f1.shape[1], *widths, self.radius):
                return (f"unsupported shape: {f1.shape[1]} channels, hidden widths {widths}, radius {self.radius} "
                        f"(rmd_dicl_match_1x1_supported)")
            if grad and not library.match_backward_supported(f1.shape[1], *widths, self.radius):
                return (f"unsupported shape for the backward: {f1.shape[1]} channels, hidden widths {widths}, radius "
                        f"{self.radius} (rmd_dicl_match_1x1_backward_supported)")
        return None

    def forward(self, f1, f2, coords, dap=True):
        batch, _, h, w = f1.shape
        reason = "fused is off" if self.fused == "off" else self.fused_fallback_reason(f1, f2, coords)
        if self.fused == "on" and reason is not None:
            raise RuntimeError(f"dicl_1x1.CorrelationModule(fused='on'): {reason}")
        if reason is None:
            cost = self.mnet(ops.StackSpec(f1, f2, coords, self.radius, self.precision,
                                           differentiable=self.needs_gradient(f1, f2, coords)))
        else:
            cost = self.mnet(ops.dicl_stack(f1, f2, coords, self.radius))
        if dap:
            cost = self.dap(cost)
        return cost.reshape(batch, -1, h, w)


# single-level soft-argmax regressions of this module (reference classes of the same names)
from ..heads import CorrSoftArgMaxFlowRegression as SoftArgMaxFlowRegression  # noqa: E402,F401
from ..heads import CorrSoftArgMaxFlowRegressionWithDap as SoftArgMaxFlowRegressionWithDap  # noqa: E402,F401
