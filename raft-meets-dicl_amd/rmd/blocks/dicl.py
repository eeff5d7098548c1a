"""DICL building blocks — drop-in for src/models/common/blocks/dicl.py (qzed/raft-meets-dicl v2).

MatchingNet is a plain nn.Sequential of MIOpen convolutions with the reference's module names, so
checkpoints load unchanged (`mnet.0.0.weight`, ...) and forward hooks on `*.mnet` keep working; with
fused="auto" / "on" its inference forward is the rmd_matching_net operator on the folded parameters.
MatchingNet1x1 is the same nn.Sequential, and given an ops.StackSpec instead of the stack it returns
the fused rmd_dicl_match_1x1 cost of its folded parameters.
DisplacementAwareProjection keeps its `conv1` parameter ((D, D, 1, 1), identity init) but runs the
projection through rmd_dap.
"""

import numpy as np
import torch
import torch.nn as nn

from .. import library, ops


def make_norm2d(ty, num_channels, num_groups):
    """src/models/common/norm.py:4-15."""
    if ty == "group":
        return nn.GroupNorm(num_groups=num_groups, num_channels=num_channels)
    if ty == "batch":
        return nn.BatchNorm2d(num_channels)
    if ty == "instance":
        return nn.InstanceNorm2d(num_channels)
    if ty == "none":
        return nn.Sequential()
    raise ValueError(f"unknown norm type '{ty}'")


class ConvBlock(nn.Sequential):
    """conv (no bias) -> norm -> ReLU (blocks/dicl.py:15-23)."""

    def __init__(self, c_in, c_out, norm_type="batch", relu_inplace=True, num_groups=8, **kwargs):
        super().__init__(nn.Conv2d(c_in, c_out, bias=False, **kwargs),
                         make_norm2d(norm_type, c_out, num_groups),
                         nn.ReLU(inplace=relu_inplace))


class ConvBlockTransposed(nn.Sequential):
    """transposed conv (no bias) -> norm -> ReLU (blocks/dicl.py:26-34)."""

    def __init__(self, c_in, c_out, norm_type="batch", relu_inplace=True, num_groups=8, **kwargs):
        super().__init__(nn.ConvTranspose2d(c_in, c_out, bias=False, **kwargs),
                         make_norm2d(norm_type, c_out, num_groups),
                         nn.ReLU(inplace=relu_inplace))


FUSED_MODES = ("off", "auto", "on")       # rmd.update's


def norm_foldable(norm):
    """Eval-mode batch norm with running statistics, or no norm at all: a per-channel affine map that does not
    depend on the input.  Group, instance and train-mode batch norm need per-call statistics."""
    if isinstance(norm, nn.BatchNorm2d):
        return not norm.training and norm.track_running_stats and norm.running_mean is not None
    return isinstance(norm, nn.Sequential) and len(norm) == 0


def norm_affine(norm, like):
    """(s, t) with norm(y) = s y + t per channel for a foldable norm: s = gamma / sqrt(var + eps), t = beta - mean s
    (s = 1, t = 0 without a norm).  Torch ops on the module's device, no host read."""
    if not isinstance(norm, nn.BatchNorm2d):
        return None, torch.zeros_like(like)
    s = torch.rsqrt(norm.running_var + norm.eps)
    if norm.affine:
        s = s * norm.weight
    t = -norm.running_mean * s
    if norm.affine:
        t = t + norm.bias
    return s, t


class MatchingNet(nn.Sequential):
    """Stacked feature pairs (B, du, dv, 2C, h, w) -> cost (B, du, dv, h, w) (blocks/dicl.py:93-118).

    ``fused="off"`` (the default) is the reference's nn.Sequential of MIOpen convolutions.  In inference the whole
    network can run as one operator, torch.ops.rmd.matching_net (csrc/mnet.hip): the norms folded into the weights
    on the device, four MFMA implicit-GEMM convolutions and one kernel for the transposed convolution and the
    last layer, walked over the B du dv images in groups that share one workspace.  "auto" falls back to the
    sequential path when a gradient is needed, autocast is on, a tensor is not float32 or not on the GPU, a norm is
    group, instance or train-mode batch norm, a side of the map is odd or the widths are unsupported; "on" raises a
    RuntimeError naming the reason.  ``precision`` "fp32" (three split-bf16 products) or "bf16" (one).  State-dict
    keys and forward hooks on the module are the same on both paths; hooks on the inner blocks do not fire on the
    fused path."""

    def __init__(self, input_channels, norm_type="batch", relu_inplace=True, scale=1, fused="off", precision="fp32"):
        if fused not in FUSED_MODES:
            raise ValueError(f"MatchingNet: unknown fused mode '{fused}', expected one of {FUSED_MODES}")
        if precision not in ops.MNET_PRECISIONS:
            raise ValueError(f"MatchingNet: unknown precision '{precision}', expected one of "
                             f"{sorted(ops.MNET_PRECISIONS)}")
        c1, c2, c3, c4 = int(scale * 96), int(scale * 128), int(scale * 64), int(scale * 32)
        kw = dict(norm_type=norm_type, relu_inplace=relu_inplace)
        super().__init__(
            ConvBlock(input_channels, c1, kernel_size=3, padding=1, **kw),
            ConvBlock(c1, c2, kernel_size=3, padding=1, stride=2, **kw),
            ConvBlock(c2, c2, kernel_size=3, padding=1, **kw),
            ConvBlock(c2, c3, kernel_size=3, padding=1, **kw),
            ConvBlockTransposed(c3, c4, kernel_size=4, padding=1, stride=2, num_groups=4, **kw),
            nn.Conv2d(c4, 1, kernel_size=3, padding=1),
        )
        self.fused = fused
        self.precision = precision

    def widths(self):
        """(c_in, c1, c2, c3, c4)."""
        return (self[0][0].in_channels, self[0][0].out_channels, self[1][0].out_channels, self[3][0].out_channels,
                self[4][0].out_channels)

    def _foldable(self):
        """Whether folded() can state every block as relu(W' x + t)."""
        return all(norm_foldable(block[1]) for block in list(self)[:5])

    def _folded(self):
        """([W1', W2', W3', W4', W5', w6], [t1, .., t5, b6]): each block as relu(W' x + t) with its norm folded in,
        norm(W x) = s (W x) + t, W' = s W along the output channels — dim 0 of a Conv2d weight, dim 1 of the
        ConvTranspose2d's (c3, c4, 4, 4) —; then the last layer's (c4, 3, 3) weight and its bias.  Torch ops on the
        module's device, no host read."""
        if not self._foldable():
            raise RuntimeError("MatchingNet.folded: group, instance and train-mode batch norm need per-call statistics "
                               "and cannot be folded into the weights")
        weights, biases = [], []
        for i, block in enumerate(list(self)[:5]):
            w = block[0].weight
            s, t = norm_affine(block[1], w[0, :, 0, 0] if i == 4 else w[:, 0, 0, 0])
            if s is not None:
                w = w * (s[None, :, None, None] if i == 4 else s[:, None, None, None])
            weights.append(w)
            biases.append(t)
        weights.append(self[5].weight[0])
        biases.append(self[5].bias)
        return weights, biases

    def __getattr__(self, name):
        # net.foldable() and net.folded(), as MatchingNet1x1's.  They are looked up per instance: the class itself
        # carries no attribute of these names, which tests/test_dicl_match.py pins (it tells the two networks apart
        # by them)
        if name == "foldable":
            return self._foldable
        if name == "folded":
            return self._folded
        return super().__getattr__(name)

    def fallback_reason(self, mvol):
        """Why the fused operator cannot serve this call (None if it can)."""
        if not self._foldable():
            return "a norm is group, instance or train-mode batch norm (per-call statistics cannot be folded)"
        tensors = [mvol] + [t for t in self.state_dict(keep_vars=True).values() if t.is_floating_point()]
        if any(t.dtype != torch.float32 for t in tensors):
            return "the tensors are not all float32"
        if torch.is_autocast_enabled() or (mvol.device.type == "cpu" and torch.is_autocast_enabled("cpu")):
            return "autocast is on"
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return "a gradient is needed (the fused MatchingNet is inference only)"
        if mvol.dim() != 6:
            return f"the input must be 6-D, got {tuple(mvol.shape)}"
        if any(t.device != mvol.device for t in tensors):
            return "the input and the parameters are on different devices"
        ht, wd = mvol.shape[-2:]
        if ht % 2 or wd % 2:
            return f"a side of the {ht} x {wd} map is odd"
        widths = self.widths()
        if mvol.shape[3] != widths[0] or not library.mnet_supported(*widths, ht, wd):
            return f"unsupported widths {widths} on a {ht} x {wd} map ({library.MNET_RANGE})"
        if not mvol.is_cuda:
            return "the tensors are not on the GPU"
        return None

    def forward(self, mvol):
        reason = self.fallback_reason(mvol) if self.fused != "off" else "off"
        if reason is None:
            weights, biases = self.folded()
            return ops.matching_net(mvol, weights, biases, precision=self.precision)
        if self.fused == "on":
            raise RuntimeError(f"MatchingNet(fused='on'): {reason}")
        b, du, dv, c2, h, w = mvol.shape
        cost = super().forward(mvol.view(b * du * dv, c2, h, w))
        return cost.view(b, du, dv, h, w)


class MatchingNet1x1(nn.Sequential):
    """1x1-conv matching network (src/models/common/corr/dicl_1x1.py:8-30)."""

    def __init__(self, input_channels, norm_type="batch", relu_inplace=True, scale=1):
        c1, c2, c3 = int(scale * 96), int(scale * 128), int(scale * 64)
        kw = dict(norm_type=norm_type, relu_inplace=relu_inplace)
        super().__init__(
            ConvBlock(input_channels, c1, kernel_size=1, **kw),
            ConvBlock(c1, c2, kernel_size=1, **kw),
            ConvBlock(c2, c3, kernel_size=1, **kw),
            nn.Conv2d(c3, 1, kernel_size=1),
        )

    _norm_foldable = staticmethod(norm_foldable)

    def foldable(self):
        """Whether folded() can state every ConvBlock as relu(W' x + t)."""
        return all(self._norm_foldable(block[1]) for block in list(self)[:3])

    def folded(self):
        """([W1', W2', W3', w4], [t1, t2, t3, b4]): each ConvBlock as relu(W' x + t) with its norm folded in,
        norm(W x) = s (W x) + t, s = gamma / sqrt(var + eps), t = beta - mean s (s = 1, t = 0 without a
        norm), W' = s[:, None] W; then the last layer's weight row and bias.  Torch ops on the module's
        device, no host read."""
        if not self.foldable():
            raise RuntimeError("MatchingNet1x1.folded: group, instance and train-mode batch norm need per-call "
                               "statistics and cannot be folded into the weights")
        weights, biases = [], []
        for block in list(self)[:3]:
            conv, norm = block[0], block[1]
            w = conv.weight[:, :, 0, 0]
            if isinstance(norm, nn.BatchNorm2d):
                s = torch.rsqrt(norm.running_var + norm.eps)
                if norm.affine:
                    s = s * norm.weight
                t = -norm.running_mean * s
                if norm.affine:
                    t = t + norm.bias
                w = s[:, None] * w
            else:
                t = torch.zeros_like(w[:, 0])
            weights.append(w)
            biases.append(t)
        weights.append(self[3].weight[0, :, 0, 0])
        biases.append(self[3].bias)
        return weights, biases

    def forward(self, mvol):
        if isinstance(mvol, ops.StackSpec):       # fused path: the stack is never built
            weights, biases = self.folded()
            return ops.dicl_match_1x1(mvol.fmap1, mvol.fmap2, mvol.coords, mvol.radius, weights, biases,
                                      precision=mvol.precision, differentiable=mvol.differentiable)
        b, du, dv, c2, h, w = mvol.shape
        cost = super().forward(mvol.view(b * du * dv, c2, h, w))
        return cost.view(b, du, dv, h, w)


class DisplacementAwareProjection(nn.Module):
    """1x1 conv over the (2u+1)(2v+1) displacement channels, no bias (blocks/dicl.py:121-150)."""

    def __init__(self, disp_range, init="identity"):
        super().__init__()
        if init not in ("identity", "standard"):
            raise ValueError(f"unknown init value '{init}'")
        disp_range = np.asarray(disp_range)
        assert disp_range.shape == (2,)
        n = int(np.prod(2 * disp_range + 1))
        self.conv1 = nn.Conv2d(n, n, bias=False, kernel_size=1)
        if init == "identity":
            nn.init.eye_(self.conv1.weight[:, :, 0, 0])

    def forward(self, x):
        return ops.dap(x, self.conv1.weight)
