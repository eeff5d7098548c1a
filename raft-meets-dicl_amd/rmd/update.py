"""Drop-ins for RAFT's update block — qzed/raft-meets-dicl src/models/impls/raft.py:193-296.

BasicMotionEncoder, SepConvGru, FlowHead and BasicUpdateBlock with the reference's constructor arguments,
attribute names and state-dict keys.  Each keeps the reference's composition as its default (``fused="off"``)
and, in inference, can run on the fused HIP operators.  SepConvGru: torch.ops.rmd.sepconv_gru (csrc/gru.hip),
six MFMA implicit-GEMM convolutions with the sigmoid / tanh / gating in their epilogues, no cat, no
pre-activation in memory.  BasicMotionEncoder: torch.ops.rmd.motion_encoder (csrc/conv.hip), its five
convolutions with ReLU epilogues writing channel slices, no cat.  FlowHead: two torch.ops.rmd.conv2d_act.

``fused``:
  "off"   the reference's composition line for line (bitwise the reference's on the CPU); trains.
  "auto"  the operator iff the tensors are fp32 GPU tensors, autocast is off, no gradient is needed (grad
          mode off, or neither h, x nor a parameter requires grad) and the widths are supported; the
          composition otherwise.  CPU tensors run the operator's CPU kernel under the same conditions.
  "on"    as "auto", but a RuntimeError naming the reason where "auto" would fall back.
``fused_backward`` (BasicMotionEncoder, FlowHead, BasicUpdateBlock; default False): with "auto" / "on", a call that
needs a gradient runs on torch.ops.rmd.conv2d_act_train (csrc/conv_backward.hip: data, weight and bias gradients
in HIP) under the same conditions, in the fp32 mode only.  The recurrent unit keeps its eager training path.
``precision`` is the operator's: "fp32" (three split-bf16 products, the parity mode) or "bf16" (one).

Forward hooks on the inner convolutions (and FlowHead's relu) do not fire on the fused paths (they are never
called); hooks on the modules themselves and on the update block do.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import library, ops

FUSED_MODES = ("off", "auto", "on")


def check_fused_arguments(name, fused, precision):
    if fused not in FUSED_MODES:
        raise ValueError(f"{name}: unknown fused mode '{fused}', expected one of {FUSED_MODES}")
    if precision not in ops.CONV_PRECISIONS:
        raise ValueError(f"{name}: unknown precision '{precision}', expected one of {sorted(ops.CONV_PRECISIONS)}")


def conv_needs_grad(inputs, convs):
    """Whether a call on `inputs` through the Conv2d modules `convs` records a graph."""
    tensors = list(inputs) + [p for c in convs for p in (c.weight, c.bias)]
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def conv_fallback_reason(inputs, convs, fused_backward=False, precision="fp32"):
    """Why the fused convolution operators cannot serve `inputs` (4-D maps of one size) through the Conv2d modules
    `convs` (None if they can): the conditions SepConvGru.fallback_reason documents.  With fused_backward a call
    that needs a gradient is served too (torch.ops.rmd.conv2d_act_train), in the fp32 mode only."""
    tensors = list(inputs) + [p for c in convs for p in (c.weight, c.bias)]
    first = inputs[0]
    if any(t.device != first.device for t in tensors):
        return "the inputs and the parameters are on different devices"
    if any(t.dtype != torch.float32 for t in tensors):
        return "the tensors are not all float32"
    if torch.is_autocast_enabled() or (first.device.type == "cpu" and torch.is_autocast_enabled("cpu")):
        return "autocast is on"
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        if not fused_backward:
            return "a gradient is needed (the fused convolutions are inference only)"
        if precision != "fp32":
            return "a gradient is needed and the fused backward is fp32 only (precision='bf16' has no backward)"
    if any(t.dim() != 4 for t in inputs):
        return f"the inputs must be 4-D, got {[tuple(t.shape) for t in inputs]}"
    if first.is_cuda:
        for c in convs:
            kh, kw = c.kernel_size
            reason = library.conv_unsupported_reason(kh, kw, c.in_channels, 0, c.out_channels, first.shape[2],
                                                     first.shape[3])
            if reason:
                return reason
    return None


class BasicMotionEncoder(nn.Module):
    """Encoder to combine correlation and flow for GRU input (raft.py:193-225)"""

    def __init__(self, corr_planes, fused="off", precision="fp32", fused_backward=False):
        super().__init__()
        check_fused_arguments("BasicMotionEncoder", fused, precision)
        self.fused = fused
        self.precision = precision
        self.fused_backward = bool(fused_backward)

        self.convc1 = nn.Conv2d(corr_planes, 256, 1, padding=0)
        self.convc2 = nn.Conv2d(256, 192, 3, padding=1)

        self.convf1 = nn.Conv2d(2, 128, 7, padding=3)
        self.convf2 = nn.Conv2d(128, 64, 3, padding=1)

        self.conv = nn.Conv2d(192 + 64, 128 - 2, 3, padding=1)

        self.output_dim = 128                           # (128 - 2) + 2

    def _convs(self):
        return (self.convc1, self.convc2, self.convf1, self.convf2, self.conv)

    def fallback_reason(self, flow, corr):
        """Why the fused operator cannot serve this call (None if it can)."""
        return conv_fallback_reason([flow, corr], self._convs(), self.fused_backward, self.precision)

    def _train(self, flow, corr):
        """The five convolutions as differentiable operators; `conv` reads (cor, flo) as its two sources."""
        def conv(x0, x1, m):
            return ops.conv2d_act(x0, x1, m.weight, m.bias, "relu", "fp32", differentiable=True)
        cor = conv(conv(corr, None, self.convc1), None, self.convc2)
        flo = conv(conv(flow, None, self.convf1), None, self.convf2)
        return torch.cat([conv(cor, flo, self.conv), flow], dim=1)

    def forward(self, flow, corr):
        if self.fused != "off":
            reason = self.fallback_reason(flow, corr)
            if reason is None:
                convs = self._convs()
                if conv_needs_grad([flow, corr], convs):
                    return self._train(flow, corr)
                return ops.motion_encoder(flow, corr, [c.weight for c in convs], [c.bias for c in convs],
                                          self.precision)
            if self.fused == "on":
                raise RuntimeError(f"BasicMotionEncoder(fused='on'): {reason}")

        cor = F.relu(self.convc1(corr))
        cor = F.relu(self.convc2(cor))

        flo = F.relu(self.convf1(flow))
        flo = F.relu(self.convf2(flo))

        combined = torch.cat([cor, flo], dim=1)
        combined = F.relu(self.conv(combined))

        return torch.cat([combined, flow], dim=1)


class SepConvGru(nn.Module):
    """Convolutional 2-part (horizontal/vertical) GRU for flow updates (raft.py:228-259)"""

    def __init__(self, hidden_dim=128, input_dim=128+128, fused="off", precision="fp32"):
        super().__init__()
        if fused not in FUSED_MODES:
            raise ValueError(f"SepConvGru: unknown fused mode '{fused}', expected one of {FUSED_MODES}")
        if precision not in ops.GRU_PRECISIONS:
            raise ValueError(f"SepConvGru: unknown precision '{precision}', expected one of {sorted(ops.GRU_PRECISIONS)}")
        self.fused = fused
        self.precision = precision

        # horizontal GRU
        self.convz1 = nn.Conv2d(hidden_dim + input_dim, hidden_dim, (1, 5), padding=(0, 2))
        self.convr1 = nn.Conv2d(hidden_dim + input_dim, hidden_dim, (1, 5), padding=(0, 2))
        self.convq1 = nn.Conv2d(hidden_dim + input_dim, hidden_dim, (1, 5), padding=(0, 2))

        # vertical GRU
        self.convz2 = nn.Conv2d(hidden_dim + input_dim, hidden_dim, (5, 1), padding=(2, 0))
        self.convr2 = nn.Conv2d(hidden_dim + input_dim, hidden_dim, (5, 1), padding=(2, 0))
        self.convq2 = nn.Conv2d(hidden_dim + input_dim, hidden_dim, (5, 1), padding=(2, 0))

    def _convs(self):
        return (self.convz1, self.convr1, self.convq1, self.convz2, self.convr2, self.convq2)

    def fallback_reason(self, h, x):
        """Why the fused operator cannot serve this call (None if it can)."""
        params = [p for c in self._convs() for p in (c.weight, c.bias)]
        tensors = [h, x] + params
        if any(t.device != h.device for t in tensors):
            return "h, x and the parameters are on different devices"
        if any(t.dtype != torch.float32 for t in tensors):
            return "the tensors are not all float32"
        if torch.is_autocast_enabled() or (h.device.type == "cpu" and torch.is_autocast_enabled("cpu")):
            return "autocast is on"
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return "a gradient is needed (the fused unit is inference only)"
        if h.dim() != 4 or x.dim() != 4:
            return f"h and x must be 4-D, got {tuple(h.shape)} / {tuple(x.shape)}"
        if h.is_cuda:
            hd, xd = h.shape[1], x.shape[1]
            if not library.gru_supported(hd, xd):
                return (f"unsupported widths: hidden {hd} (a multiple of 32 in 32..128), input {xd} (a multiple of "
                        f"16), hidden + input <= 512")
            if (hd + xd) * h.shape[2] * h.shape[3] >= library.GRU_MAX_IMAGE:
                return f"unsupported size: (hidden + input) H W = {(hd + xd) * h.shape[2] * h.shape[3]} >= 2^30"
        return None

    def forward(self, h, x):
        if self.fused != "off":
            reason = self.fallback_reason(h, x)
            if reason is None:
                convs = self._convs()
                return ops.sepconv_gru(h, x, [c.weight for c in convs], [c.bias for c in convs], self.precision)
            if self.fused == "on":
                raise RuntimeError(f"SepConvGru(fused='on'): {reason}")

        # horizontal GRU
        hx = torch.cat([h, x], dim=1)                               # input vector
        z = torch.sigmoid(self.convz1(hx))                          # update gate vector
        r = torch.sigmoid(self.convr1(hx))                          # reset gate vector
        q = torch.tanh(self.convq1(torch.cat((r * h, x), dim=1)))   # candidate activation
        h = (1.0 - z) * h + z * q                                   # output vector

        # vertical GRU
        hx = torch.cat([h, x], dim=1)                               # input vector
        z = torch.sigmoid(self.convz2(hx))                          # update gate vector
        r = torch.sigmoid(self.convr2(hx))                          # reset gate vector
        q = torch.tanh(self.convq2(torch.cat((r * h, x), dim=1)))   # candidate activation
        h = (1.0 - z) * h + z * q                                   # output vector

        return h


class FlowHead(nn.Module):
    """Head to compute delta-flow from GRU hidden-state (raft.py:262-273)"""

    def __init__(self, input_dim=128, hidden_dim=256, relu_inplace=True, fused="off", precision="fp32",
                 fused_backward=False):
        super().__init__()
        check_fused_arguments("FlowHead", fused, precision)
        self.fused = fused
        self.precision = precision
        self.fused_backward = bool(fused_backward)

        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, 2, 3, padding=1)
        self.relu = nn.ReLU(inplace=relu_inplace)

    def fallback_reason(self, x):
        """Why the fused operator cannot serve this call (None if it can)."""
        return conv_fallback_reason([x], (self.conv1, self.conv2), self.fused_backward, self.precision)

    def forward(self, x):
        if self.fused != "off":
            reason = self.fallback_reason(x)
            if reason is None:
                train = conv_needs_grad([x], (self.conv1, self.conv2))
                y = ops.conv2d_act(x, None, self.conv1.weight, self.conv1.bias, "relu", self.precision, train)
                return ops.conv2d_act(y, None, self.conv2.weight, self.conv2.bias, "none", self.precision, train)
            if self.fused == "on":
                raise RuntimeError(f"FlowHead(fused='on'): {reason}")

        return self.conv2(self.relu(self.conv1(x)))


class BasicUpdateBlock(nn.Module):
    """Network to compute single flow update delta (raft.py:276-296)"""

    def __init__(self, corr_planes, input_dim=128, hidden_dim=128, relu_inplace=True, *, gru_fused="off",
                 gru_precision="fp32", fused="off", precision="fp32", fused_backward=False):
        super().__init__()

        self.enc = BasicMotionEncoder(corr_planes, fused=fused, precision=precision, fused_backward=fused_backward)
        self.gru = SepConvGru(hidden_dim=hidden_dim, input_dim=input_dim+self.enc.output_dim, fused=gru_fused,
                              precision=gru_precision)
        self.flow = FlowHead(input_dim=hidden_dim, hidden_dim=256, relu_inplace=relu_inplace, fused=fused,
                             precision=precision, fused_backward=fused_backward)

    def forward(self, h, x, corr, flow):
        m = self.enc(flow, corr)            # motion features
        x = torch.cat((x, m), dim=1)        # input for GRU

        h = self.gru(h, x)                  # update hidden state (N, hidden, h/8, w/8)
        d = self.flow(h)                    # compute flow delta from hidden state (N, 2, h/8, w/8)

        return h, d
