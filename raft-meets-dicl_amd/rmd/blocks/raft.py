"""RAFT building blocks — drop-in for src/models/common/blocks/raft.py (qzed/raft-meets-dicl v2).

ResidualBlock with the reference's constructor arguments, attribute names and state-dict keys (`norm3` is shared
with `downsample.1`, as in the reference).  It keeps the reference's composition as its default (``fused="off"``)
and, in inference, can run on the fused HIP operators of csrc/encoder.hip: torch.ops.rmd.conv2d_norm_act (an MFMA
implicit-GEMM convolution of stride 1 or 2 that normalises its input while staging it and adds the residual in
its epilogue), torch.ops.rmd.instance_norm_stats and torch.ops.rmd.residual_join.

  norm 'none', eval-mode 'batch' (folded into the weights on the device): the projection if present, conv1 with
      ReLU, conv2 with relu3(x + relu2(.)) in its store — no norm, ReLU or add pass.
  norm 'instance': conv1 raw -> statistics -> conv2 normalising on load -> statistics -> the same two steps for
      the projection -> the join.  The normalised map between conv1 and conv2 is never written; the block's result
      is (the join writes it).

``fused`` and ``precision`` are rmd.update's: "off" | "auto" | "on" and "fp32" | "bf16".  "auto" falls back to the
composition when a gradient is needed, autocast is on, the tensors are not fp32 GPU tensors, the norm is 'group', a
batch norm is in training mode or keeps no running statistics, an instance norm has affine parameters or running
statistics, or a shape is unsupported; "on" raises a RuntimeError naming the reason instead.  Forward hooks on the
inner modules do not fire on the fused path; hooks on the block do.
"""

import torch
import torch.nn as nn

from .. import library, ops
from ..update import check_fused_arguments
from .dicl import make_norm2d


def norm_kind(norm):
    """("none" | "instance" | "batch", None) for a norm module the fused operators serve, (None, reason) otherwise."""
    if isinstance(norm, nn.Sequential) and len(norm) == 0:
        return "none", None
    if isinstance(norm, nn.GroupNorm):
        return None, "group norm is not fused"
    if isinstance(norm, nn.InstanceNorm2d):
        if norm.affine or norm.track_running_stats:
            return None, "the instance norm has affine parameters or running statistics"
        return "instance", None
    if isinstance(norm, nn.BatchNorm2d):
        if norm.training:
            return None, "the batch norm is in training mode (batch statistics cannot be folded into the weights)"
        if norm.running_mean is None or norm.running_var is None:
            return None, "the batch norm keeps no running statistics"
        return "batch", None
    return None, f"unknown norm module {type(norm).__name__}"


def norms_kind(norms):
    """The one kind of all `norms`, or (None, reason)."""
    kinds = [norm_kind(n) for n in norms]
    for kind, reason in kinds:
        if reason:
            return None, reason
    if len({k for k, _ in kinds}) != 1:
        return None, f"mixed norm types {sorted({k for k, _ in kinds})}"
    return kinds[0][0], None


def folded(conv, norm):
    """(weight, bias) of the convolution with an eval-mode batch norm folded in: norm(W x + b) = s (W x + b) + t, s =
    gamma / sqrt(var + eps), t = beta - mean s.  Other norms leave the parameters as they are.  Torch ops on the
    module's device, no host read."""
    if not isinstance(norm, nn.BatchNorm2d):
        return conv.weight, conv.bias
    s = torch.rsqrt(norm.running_var + norm.eps)
    if norm.affine:
        s = s * norm.weight
    t = (conv.bias - norm.running_mean) * s
    if norm.affine:
        t = t + norm.bias
    return conv.weight * s[:, None, None, None], t


def norm_tensors(norm):
    """The tensors of a norm module that the fused path reads: its parameters and, for a batch norm, the running
    statistics that folded() uses."""
    stats = [norm.running_mean, norm.running_var] if isinstance(norm, nn.BatchNorm2d) else []
    return list(norm.parameters()) + [t for t in stats if t is not None]


def fused_fallback_reason(x, params, kind_reason):
    """The conditions shared by ResidualBlock and FeatureEncoder (None if the fused operators can run)."""
    if kind_reason:
        return kind_reason
    tensors = [x] + list(params)
    if any(t.dtype != torch.float32 for t in tensors):
        return "the tensors are not all float32"
    if torch.is_autocast_enabled() or (x.device.type == "cpu" and torch.is_autocast_enabled("cpu")):
        return "autocast is on"
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return "a gradient is needed (the fused encoder is inference only)"
    if x.dim() != 4:
        return f"the input must be 4-D, got {tuple(x.shape)}"
    if any(t.device != x.device for t in tensors):
        return "the input and the parameters are on different devices"
    if not x.is_cuda:
        return "the tensors are not on the GPU"
    return None


class ResidualBlock(nn.Module):
    """Residual block for feature / context encoder"""

    def __init__(self, in_planes, out_planes, norm_type='group', stride=1, relu_inplace=True, fused="off",
                 precision="fp32"):
        super().__init__()
        check_fused_arguments("ResidualBlock", fused, precision)
        self.fused = fused
        self.precision = precision

        self.conv1 = nn.Conv2d(in_planes, out_planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(out_planes, out_planes, kernel_size=3, padding=1)

        self.relu1 = nn.ReLU(inplace=relu_inplace)
        self.relu2 = nn.ReLU(inplace=relu_inplace)
        self.relu3 = nn.ReLU(inplace=relu_inplace)

        self.norm1 = make_norm2d(norm_type, num_channels=out_planes, num_groups=out_planes//8)
        self.norm2 = make_norm2d(norm_type, num_channels=out_planes, num_groups=out_planes//8)
        if stride > 1:
            self.norm3 = make_norm2d(norm_type, num_channels=out_planes, num_groups=out_planes//8)

        self.downsample = None
        if stride > 1:
            self.downsample = nn.Sequential(
                nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride),
                self.norm3,
            )

    def conv_norms(self):
        """(conv, norm) pairs in the operator's order: conv1, conv2 and, where present, downsample.0."""
        pairs = [(self.conv1, self.norm1), (self.conv2, self.norm2)]
        if self.downsample is not None:
            pairs.append((self.downsample[0], self.downsample[1]))
        return pairs

    def fallback_reason(self, x):
        """Why the fused operators cannot serve this call (None if they can)."""
        pairs = self.conv_norms()
        kind, reason = norms_kind([n for _, n in pairs])
        params = [p for c, n in pairs for p in (c.weight, c.bias, *norm_tensors(n))]
        reason = fused_fallback_reason(x, params, reason)
        if reason:
            return reason
        stride = self.conv1.stride[0]
        ht, wd = x.shape[2:]
        ho, wo = library.out_side(ht, stride), library.out_side(wd, stride)
        for conv, _ in pairs:
            if conv.stride[0] != conv.stride[1] or conv.padding != (conv.kernel_size[0] // 2, conv.kernel_size[1] // 2):
                return f"unsupported convolution: stride {conv.stride}, padding {conv.padding}"
            # conv1 and the projection read the block's input, conv2 reads conv1's result
            size = (ho, wo) if conv is self.conv2 else (ht, wd)
            reason = library.norm_conv_unsupported_reason(*conv.kernel_size, conv.stride[0], conv.in_channels,
                                                          conv.out_channels, *size)
            if reason:
                return reason
        if kind == "instance" and ho * wo < 2:
            return "the instance norm needs more than one pixel per plane"
        return None

    def _fused(self, x):
        pairs = self.conv_norms()
        stride, p = self.conv1.stride[0], self.precision
        (w1, b1), (w2, b2) = folded(*pairs[0]), folded(*pairs[1])
        if isinstance(self.norm1, nn.InstanceNorm2d):
            y = ops.conv2d_norm_act(x, w1, b1, stride=stride, precision=p)
            scale, shift = ops.instance_norm_stats(y, self.norm1.eps)
            y = ops.conv2d_norm_act(y, w2, b2, scale=scale, shift=shift, precision=p)
            y_stats = ops.instance_norm_stats(y, self.norm2.eps)
            if self.downsample is None:
                return ops.residual_join(y, x, y_stats)
            x = ops.conv2d_norm_act(x, *folded(*pairs[2]), stride=stride, precision=p)
            return ops.residual_join(y, x, y_stats, ops.instance_norm_stats(x, self.norm3.eps))
        res = x
        if self.downsample is not None:
            res = ops.conv2d_norm_act(x, *folded(*pairs[2]), stride=stride, precision=p)
        y = ops.conv2d_norm_act(x, w1, b1, stride=stride, act="relu", precision=p)
        return ops.conv2d_norm_act(y, w2, b2, residual=res, act="relu", precision=p)

    def forward(self, x):
        if self.fused != "off":
            reason = self.fallback_reason(x)
            if reason is None:
                return self._fused(x)
            if self.fused == "on":
                raise RuntimeError(f"ResidualBlock(fused='on'): {reason}")

        y = x
        y = self.relu1(self.norm1(self.conv1(y)))
        y = self.relu2(self.norm2(self.conv2(y)))

        if self.downsample is not None:
            x = self.downsample(x)

        return self.relu3(x + y)
