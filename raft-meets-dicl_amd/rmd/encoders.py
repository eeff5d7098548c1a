"""RAFT's feature / context encoder — drop-in for src/models/common/encoders (qzed/raft-meets-dicl v2), type 'raft'
at stride 8 (encoders/raft/s3.py:8-72).

FeatureEncoder with the reference's constructor arguments, attribute names and state-dict keys.  ``fused="off"``
(the default) is the reference's forward line for line; in inference the whole forward can run as one operator,
torch.ops.rmd.feature_encoder (csrc/encoder.hip): 16 MFMA implicit-GEMM convolutions over one workspace, the
instance norm as per-plane statistics applied while the next convolution stages its input, eval-mode batch norm
folded into the weights on the device, and the blocks' residual joins in a convolution's epilogue ('none',
'batch') or one elementwise pass ('instance').  No MIOpen call, no host synchronisation.

``fused`` and ``precision`` are rmd.update's.  "auto" falls back to the composition under the conditions
rmd.blocks.raft documents, and when dropout is active; "on" raises a RuntimeError naming the reason.  Forward hooks
on the encoder fire on both paths; hooks on its inner modules do not fire on the fused path.
"""

import torch
import torch.nn as nn

from . import library, ops
from .blocks.dicl import make_norm2d
from .blocks.raft import ResidualBlock, folded, fused_fallback_reason, norm_tensors, norms_kind
from .update import check_fused_arguments


class FeatureEncoder(nn.Module):
    """Feature / context encoder network"""

    def __init__(self, output_dim=128, norm_type='batch', dropout=0.0, init_mode='fan_out', relu_inplace=True,
                 fused="off", precision="fp32"):
        super().__init__()
        check_fused_arguments("FeatureEncoder", fused, precision)
        self.fused = fused
        self.precision = precision

        # input convolution             # (H, W, 3) -> (H/2, W/2, 64)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.norm1 = make_norm2d(norm_type, num_channels=64, num_groups=8)
        self.relu1 = nn.ReLU(inplace=relu_inplace)

        # residual blocks
        self.layer1 = nn.Sequential(    # (H/2, W/2, 64) -> (H/2, W/2, 64)
            ResidualBlock(64, 64, norm_type, stride=1, relu_inplace=relu_inplace),
            ResidualBlock(64, 64, norm_type, stride=1, relu_inplace=relu_inplace),
        )

        self.layer2 = nn.Sequential(    # (H/2, W/2, 64) -> (H/4, W/4, 96)
            ResidualBlock(64, 96, norm_type, stride=2, relu_inplace=relu_inplace),
            ResidualBlock(96, 96, norm_type, stride=1, relu_inplace=relu_inplace),
        )

        self.layer3 = nn.Sequential(    # (H/4, W/4, 96) -> (H/8, W/8, 128)
            ResidualBlock(96, 128, norm_type, stride=2, relu_inplace=relu_inplace),
            ResidualBlock(128, 128, norm_type, stride=1, relu_inplace=relu_inplace),
        )

        # output convolution            # (H/8, W/8, 128) -> (H/8, W/8, output_dim)
        self.conv2 = nn.Conv2d(128, output_dim, kernel_size=1)

        # dropout
        self.dropout = nn.Dropout2d(p=dropout)

        # initialize weights
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode=init_mode, nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def conv_norms(self):
        """(conv, norm or None) pairs of the 16 convolutions in the operator's order: conv1; per block conv1, conv2
        and, where present, downsample.0; conv2."""
        pairs = [(self.conv1, self.norm1)]
        for layer in (self.layer1, self.layer2, self.layer3):
            for block in layer:
                pairs += block.conv_norms()
        return pairs + [(self.conv2, None)]

    def fallback_reason(self, x):
        """Why the fused operator cannot serve this call (None if it can); x is the batch after concatenation."""
        pairs = self.conv_norms()
        norms = [n for _, n in pairs if n is not None]
        kind, reason = norms_kind(norms)
        params = [p for c, _ in pairs for p in (c.weight, c.bias)] + [t for n in norms for t in norm_tensors(n)]
        if reason is None and self.training and self.dropout.p > 0:
            reason = "dropout is active"
        reason = fused_fallback_reason(x, params, reason)
        if reason:
            return reason
        if kind == "instance" and any(n.eps != library.INSTANCE_NORM_EPS for n in norms):
            return f"an instance norm's eps is not {library.INSTANCE_NORM_EPS}"
        want = library.feature_encoder_convs(self.conv2.out_channels)
        have = [(c.out_channels, c.in_channels, c.kernel_size[0], c.stride[0]) for c, _ in pairs]
        if len(pairs) != 16 or have != want or x.shape[1] != 3:
            return "the modules are not the s3 encoder's 16 convolutions over a 3-channel image"
        ht, wd = x.shape[2:]
        if kind == "instance" and library.out_side(ht, 8) * library.out_side(wd, 8) < 2:     # three halvings, rounded up
            return "the instance norm needs more than one pixel per plane at 1/8 resolution"
        return library.feature_encoder_unsupported_reason(self.conv2.out_channels, ht, wd)

    def _fused(self, x):
        pairs = self.conv_norms()
        params = [folded(c, n) for c, n in pairs]
        norm = "instance" if isinstance(self.norm1, nn.InstanceNorm2d) else "none"
        return ops.feature_encoder(x, [w for w, _ in params], [b for _, b in params], norm, self.precision)

    def forward(self, x):
        # input may be tuple/list for flow network (img1, img2), combine this into single batch
        is_list = isinstance(x, tuple) or isinstance(x, list)
        if is_list:
            batch_dim = x[0].shape[0]
            x = torch.cat(x, dim=0)

        reason = self.fallback_reason(x) if self.fused != "off" else "off"
        if reason is None:
            x = self._fused(x)              # dropout is the identity here: fallback_reason saw it inactive
        else:
            if self.fused == "on":
                raise RuntimeError(f"FeatureEncoder(fused='on'): {reason}")

            # input layer
            x = self.relu1(self.norm1(self.conv1(x)))

            # residual blocks
            x = self.layer1(x)
            x = self.layer2(x)
            x = self.layer3(x)

            # output layer
            x = self.dropout(self.conv2(x))

        if is_list:
            x = torch.split(x, (batch_dim, batch_dim), dim=0)

        return x


def make_encoder_s3(encoder_type, output_dim, norm_type, dropout, relu_inplace=True, **kwargs):
    """encoders/__init__.py:52-60 for the type this package mirrors."""
    if encoder_type == 'raft':
        return FeatureEncoder(output_dim=output_dim, norm_type=norm_type, dropout=dropout, relu_inplace=relu_inplace,
                              **kwargs)
    if encoder_type in ('dicl', 'rfpm-raft'):
        raise ValueError(f"feature encoder type '{encoder_type}' is not mirrored here (only 'raft' is)")
    raise ValueError(f"unsupported feature encoder type: '{encoder_type}'")
