"""Hidden-state upsamplers of the coarse-to-fine models — drop-ins for src/models/common/hsup.py.

The coarse-to-fine models (raft+dicl/ctf-l2..4, raft/sl-ctf-l2..4) build one upsampler per level
transition from their `upsample-hidden` parameter (e.g. raft_dicl_ctf_l3.py:64, 74-75) and call it as
`h = upsampler(h_prev, h_init)` with the coarse level's final hidden state and the fine level's
initial one (:173, :210).

  HUpNone        hsup.py:8-13    returns h_init
  HUpBilinear    hsup.py:16-33   h_init + bilinear(conv1(h_prev)); conv1 starts as the identity.  The
                                 reference's torch composition (the convolution stays with MIOpen)
  HUpCrossAttn   hsup.py:36-97   1x1 convolutions (MIOpen), then ONE rmd.ops.local_cross_attn pass
                                 for hsup.py:66-92 — the reference unfolds K and V and expands both to
                                 (B, c, 9, h, w) —, then the residual and conv_out

Constructor arguments, state-dict keys (conv1; conv_q, conv_v_init, conv_k, conv_v_prev, conv_out) and
initialisation are the reference's.  Sizes that are no integer multiple of the coarse ones raise a
RuntimeError (the reference fails in its reshape).
"""

import torch.nn as nn
import torch.nn.functional as F

from . import ops


class HUpNone(nn.Module):
    def __init__(self, recurrent_channels) -> None:
        super().__init__()

    def forward(self, h_prev, h_init):
        return h_init


class HUpBilinear(nn.Module):
    def __init__(self, recurrent_channels) -> None:
        super().__init__()
        # per-pixel linear map between the levels, the identity at first (hsup.py:20-25)
        self.conv1 = nn.Conv2d(recurrent_channels, recurrent_channels, 1)
        nn.init.eye_(self.conv1.weight[:, :, 0, 0])

    def forward(self, h_prev, h_init):
        _, _, h, w = h_init.shape
        h_prev = F.interpolate(self.conv1(h_prev), (h, w), mode="bilinear", align_corners=True)     # hsup.py:30-31
        return h_init + h_prev


class HUpCrossAttn(nn.Module):
    def __init__(self, recurrent_channels) -> None:
        super().__init__()
        value_channels = recurrent_channels
        key_channels = 64

        self.window_size = (3, 3)
        self.window_padding = (self.window_size[0] // 2, self.window_size[1] // 2)

        self.conv_q = nn.Conv2d(recurrent_channels, key_channels, 1)            # fine level
        self.conv_v_init = nn.Conv2d(recurrent_channels, value_channels, 1)
        self.conv_k = nn.Conv2d(recurrent_channels, key_channels, 1)            # coarse level
        self.conv_v_prev = nn.Conv2d(recurrent_channels, value_channels, 1)
        self.conv_out = nn.Conv2d(value_channels, recurrent_channels, 1)

    def forward(self, h_prev, h_init):
        _, _, h, w = h_init.shape
        _, _, h2, w2 = h_prev.shape
        if h % h2 or w % w2:
            raise RuntimeError(f"HUpCrossAttn: h_init {tuple(h_init.shape)} is not an integer multiple of h_prev "
                               f"{tuple(h_prev.shape)}")
        q = self.conv_q(h_init)                                                 # hsup.py:62-64
        k = self.conv_k(h_prev)
        v = self.conv_v_prev(h_prev)
        x = ops.local_cross_attn(q, k, v, self.window_size)                     # hsup.py:66-92
        return self.conv_out(self.conv_v_init(h_init) + x)                      # hsup.py:95-97


def make_hidden_state_upsampler(type, recurrent_channels):
    if type == "none":
        return HUpNone(recurrent_channels)
    elif type == "bilinear":
        return HUpBilinear(recurrent_channels)
    elif type == "crossattn":
        return HUpCrossAttn(recurrent_channels)
    else:
        raise ValueError(f"unknown hidden state upsampler type '{type}'")
