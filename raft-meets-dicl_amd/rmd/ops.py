"""Torch-facing wrappers over the C ABI (include/rmd.h): device checks, allocation, streams.

Outputs and workspaces come from torch's caching allocator; the C launchers only enqueue kernels
on torch's current HIP stream.  GPU tensors run the HIP kernels (and raise if librmd.so is missing);
CPU tensors dispatch to the operators' CPU kernels (rmd/cpu.py, the reference's ATen algorithm).
The token-linked autograd functions of the RAFT correlation and of the on-the-fly lookup are
GPU-only: on the CPU the operators' own ATen graph carries the gradient.
"""

import ctypes

import torch

from . import _lib, config, library
from ._lib import RMD_BF16, RMD_BF16X3, RMD_F16, RMD_F32, RMD_S24
from .library import _f32

# precision modes: (GEMM compute type, pyramid storage type)
PRECISIONS = {
    "fp32": (RMD_BF16X3, RMD_S24),    # fp32-accurate split-bf16 MFMA (3 products), 24-bit pyramid: parity mode (default)
    "fp32-f32": (RMD_BF16X3, RMD_F32),# the same GEMM, f32 pyramid
    "fp32-s24": (RMD_BF16X3, RMD_S24),# the same GEMM, 24-bit pyramid
    "fp32-exact": (RMD_F32, RMD_F32), # exact f32 MFMA (v_mfma_f32_32x32x2_f32), f32 pyramid
    "bf16": (RMD_BF16, RMD_F16),      # bf16 MFMA operands, f32 accumulate, fp16 pyramid: perf mode
    "bf16-f32": (RMD_BF16, RMD_F32),  # bf16 operands, f32 pyramid
    "fp32-f16": (RMD_F32, RMD_F16),   # exact f32 GEMM, fp16 pyramid
}


def set_default_precision(name):
    """Process-wide precision of blocks built with precision=None (rmd.config 'corr-precision')."""
    if name not in PRECISIONS:
        raise ValueError(f"unknown precision '{name}', expected one of {sorted(PRECISIONS)}")
    config.configure(precision=name)


def get_default_precision():
    return config.current().precision


def _require_gpu(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("rmd: HIP kernels need GPU tensors")


def _same_device(*tensors):
    """All inputs on one device: GPU tensors run the HIP kernels, CPU tensors the CPU kernels."""
    dev = None
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"rmd: expected a tensor, got {type(t).__name__}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"rmd: tensors on different devices ({dev} / {t.device})")


class Pyramid:
    """Correlation pyramid in the tiled, query-minor HBM layout of include/rmd.h.  ``data`` is 1-D in the
    row layout, (n, 8) in the tiles layout (rmd.library.pyramid_view) and uint8 (n, 3) with RMD_S24 storage."""

    def __init__(self, data, desc, channels, scale):
        self.data = data
        self.desc = desc
        self.channels = channels
        self.scale = scale

    @property
    def levels(self):
        return self.desc.levels

    def level_shape(self, i):
        return self.desc.level_h[i], self.desc.level_w[i]

    def unpack(self, i):
        """Level i in the reference layout (B, H, W, 1, H_i, W_i) as float32 — for tests/debugging."""
        d = self.desc
        b, h, w = d.batch, d.height, d.width
        th, tw, ty, tx = d.tile_h[i], d.tile_w[i], d.tiles_y[i], d.tiles_x[i]
        hl, wl = d.level_h[i], d.level_w[i]
        s = d.query_slots
        off = d.level_offset[i]
        flat = library.s24_decode(self.data) if d.storage == RMD_S24 else self.data.reshape(-1)
        x = flat[off: off + b * ty * tx * s * th * tw].view(b, ty, tx, s, th, tw)
        x = x.permute(0, 3, 1, 4, 2, 5).reshape(b, s, ty * th, tx * tw)[..., :hl, :wl]
        if d.layout == _lib.RMD_LAYOUT_TILES:
            x = x.index_select(1, torch.as_tensor(tiles_slots(h, w), device=x.device))
        return x.float().reshape(b, h, w, 1, hl, wl)


def tiles_slots(h, w):
    """Query slot of every pixel (raster order) in the tiles layout (include/rmd.h RMD_LAYOUT_TILES)."""
    y1, x1 = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    qx, hp = (w + 15) // 16, h // 2
    s = ((y1 // 2) * qx + x1 // 16) * 32 + ((x1 % 16) // 4) * 8 + (y1 % 2) * 4 + x1 % 4
    s = torch.where(y1 < 2 * hp, s, hp * qx * 32 + x1)
    return s.reshape(-1)


def corr_pyramid(fmap1, fmap2, levels=4, precision=None, events=None, scale=None):
    """raft.CorrBlock.__init__ (raft.py:18-47) on the GPU -> Pyramid (torch.ops.rmd.corr_pyramid).

    ``scale`` multiplies the products: None = 1/sqrt(C) (raft.py:33), 1.0 = raft_fs.CorrBlock.

    ``events`` (optional list) receives (start, end) HIP events bracketing the GEMM launch alone
    (the operand prep runs before the start event) — bench.py's roofline timing; that call runs the
    two C-ABI halves of what the operator runs directly: rmd_corr_prepare_queries + rmd_corr_pyramid_staged
    on the w8 GEMM (whose launch then includes staging fmap2 from fp32), rmd_corr_prepare +
    rmd_corr_pyramid_prepared on every other.
    """
    _same_device(fmap1, fmap2)
    if fmap1.shape != fmap2.shape or fmap1.dim() != 4:
        raise ValueError(f"fmap1/fmap2 must be equal (B,C,H,W) shapes, got {tuple(fmap1.shape)} / {tuple(fmap2.shape)}")
    compute, storage = PRECISIONS[precision or get_default_precision()]
    b, c, h, w = fmap1.shape
    scale = 1.0 / float(c) ** 0.5 if scale is None else float(scale)
    if events is None:
        data = torch.ops.rmd.corr_pyramid(fmap1, fmap2, levels, compute, storage, scale)
        # the storage the GEMM wrote (S24 is the x3 GEMM's alone: other GEMMs of the call store F32)
        d = library.describe(b, h, w, levels, library.pyramid_storage(data), library.pyramid_layout(data))
        return Pyramid(data, d, c, scale)
    _require_gpu(fmap1, fmap2)
    f1, f2 = _f32(fmap1), _f32(fmap2)
    d, data, ws = library.pyramid_buffers(f1, levels, compute, storage)
    staged = _lib.lib().rmd_corr_gemm_kernel(ctypes.byref(d), c, compute) == b"w8"
    with torch.cuda.device(f1.device):                  # the events record on this device's current stream
        if staged:
            _lib.launch("rmd_corr_prepare_queries", f1, f1, c, ctypes.byref(d), compute, ws)
        else:
            _lib.launch("rmd_corr_prepare", f1, f1, f2, c, scale, ctypes.byref(d), compute, ws)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if staged:
            _lib.launch("rmd_corr_pyramid_staged", f1, f2, c, scale, ctypes.byref(d), compute, data, ws)
        else:
            _lib.launch("rmd_corr_pyramid_prepared", f1, c, scale, ctypes.byref(d), compute, data, ws)
        e1.record()
        events.append((e0, e1))
    return Pyramid(data, d, c, scale)


def corr_lookup(pyr, coords, radius, mask_costs=()):
    """raft.CorrBlock.__call__ (raft.py:49-95) -> (B, L*(2r+1)^2, H, W) float32."""
    _same_device(pyr.data, coords)
    d = pyr.desc
    if tuple(coords.shape) != (d.batch, 2, d.height, d.width):
        raise ValueError(f"coords must be (B,2,H,W)=({d.batch},2,{d.height},{d.width}), got {tuple(coords.shape)}")
    return torch.ops.rmd.corr_lookup(pyr.data, coords, d.levels, radius, _mask_bits(mask_costs, d.levels))


# ---- on-the-fly lookup (raft_fs semantics without the volume) -------------------------------------

class OtfState:
    """Operand rows of rmd_corr_otf_prepare (query rows * scale, pooled target rows of every level)."""

    def __init__(self, ws, b, c, h, w, levels, compute):
        self.ws, self.b, self.c, self.h, self.w, self.levels, self.compute = ws, b, c, h, w, levels, compute


def otf_prepare(fmap1, fmap2, levels, precision=None, scale=1.0):
    _same_device(fmap1, fmap2)
    if fmap1.shape != fmap2.shape or fmap1.dim() != 4:
        raise ValueError(f"fmap1/fmap2 must be equal (B,C,H,W) shapes, got {tuple(fmap1.shape)} / {tuple(fmap2.shape)}")
    compute = PRECISIONS[precision or get_default_precision()][0]     # fp32: split bf16, fp32-exact: f32
    b, c, h, w = fmap1.shape
    ws = torch.ops.rmd.corr_otf_prepare(fmap1, fmap2, levels, compute, float(scale))
    return OtfState(ws, b, c, h, w, levels, compute)


def otf_lookup(st, coords, radius, mask_costs=()):
    _same_device(st.ws, coords)
    if tuple(coords.shape) != (st.b, 2, st.h, st.w):
        raise ValueError(f"coords must be (B,2,H,W)=({st.b},2,{st.h},{st.w}), got {tuple(coords.shape)}")
    return torch.ops.rmd.corr_otf_lookup(st.ws, coords, st.c, st.levels, st.compute, radius,
                                         _mask_bits(mask_costs, st.levels))


# ---- on-the-fly lookup autograd (training without the volume) ----------------------------------
#
# Same token scheme as the volume path below: every lookup's backward turns its grad_out into a record
# of patch weights (rmd_corr_otf_record, O(L*N*(2r+2)^2) floats, no volume), and the prepare's
# backward — which autograd runs after all of them — computes d fmap1 / d fmap2 from all records in one
# pass (rmd_corr_otf_backward: the union target box of a query tile swept once for every iteration).

class _OtfState:
    def __init__(self, otf, f1, f2, scale):
        self.otf = otf
        self.f1 = f1
        self.f2 = f2
        self.scale = scale
        self.records = []
        self.radius = None


class _OtfPrepareFn(torch.autograd.Function):
    """Autograd node of raft_fs.CorrBlock.__init__ (raft_fs.py:16-31) on the on-the-fly path."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, state):
        ctx.state = state
        return fmap1.new_zeros(())

    @staticmethod
    def backward(ctx, _gtoken):
        st = ctx.state
        o = st.otf
        if not st.records:
            return torch.zeros_like(st.f1), torch.zeros_like(st.f2), None
        ws = _lib.workspace("corr_otf_backward", st.f1, o.b, o.c, o.h, o.w, o.levels, o.compute)
        if ws.numel() == 0:
            raise ValueError(f"otf backward: unsupported sizes (C={o.c} must be <= 256)")
        g1 = torch.empty_like(st.f1)
        g2 = torch.empty_like(st.f2)
        recs = (ctypes.c_void_p * len(st.records))(*[r.data_ptr() for r in st.records])
        _lib.launch("rmd_corr_otf_backward", st.f1, st.f1, st.f2, o.ws, o.b, o.c, o.h, o.w, o.levels, float(st.scale),
                    o.compute, st.radius, len(st.records), recs, g1, g2, ws)
        st.records = []
        return g1, g2, None


class _OtfLookupFn(torch.autograd.Function):
    """Autograd node of raft_fs.CorrBlock.__call__ (raft_fs.py:33-87) on the on-the-fly path; coords carry
    no gradient (raft.py:402)."""

    @staticmethod
    def forward(ctx, token, coords, state, radius, mask_costs):
        out = otf_lookup(state.otf, coords, radius, mask_costs)
        ctx.state = state
        ctx.radius = radius
        ctx.mask = _mask_bits(mask_costs, state.otf.levels)
        ctx.save_for_backward(_f32(coords))
        return out

    @staticmethod
    def backward(ctx, gout):
        (co,) = ctx.saved_tensors
        st = ctx.state
        o = st.otf
        if st.radius is not None and st.radius != ctx.radius:
            raise ValueError("otf backward: all lookups of one block must use the same radius")
        st.radius = ctx.radius
        nbytes = _lib.lib().rmd_corr_otf_record_bytes(o.b, o.h, o.w, o.levels, ctx.radius)
        rec = co.new_empty(nbytes, dtype=torch.uint8)
        g = _f32(gout)
        _lib.launch("rmd_corr_otf_record", co, g, co, o.b, o.h, o.w, o.levels, ctx.radius, ctx.mask, rec)
        st.records.append(rec)
        return gout.new_zeros(()), None, None, None, None


def otf_block_autograd(fmap1, fmap2, levels, precision, scale=1.0):
    """On-the-fly operands + autograd token for a block whose feature maps require gradients."""
    _require_gpu(fmap1, fmap2)
    otf = otf_prepare(fmap1, fmap2, levels, precision, scale=scale)
    st = _OtfState(otf, _f32(fmap1), _f32(fmap2), scale)
    token = _OtfPrepareFn.apply(fmap1, fmap2, st)
    return otf, st, token


def otf_lookup_autograd(token, state, coords, radius, mask_costs=()):
    return _OtfLookupFn.apply(token, coords, state, radius, tuple(mask_costs))


# ---- RAFT correlation autograd (training) -------------------------------------------------------
#
# The pyramid Function returns a scalar "token" that every lookup of the same CorrBlock takes as an
# input, so autograd runs all lookup backwards before the pyramid backward.  Each lookup backward
# only hands its grad_out and coordinates to the shared _CorrState; the pyramid backward writes ONE
# dense fp32 gradient G over the T' padded targets, in the pyramid's chunked query-minor order
# (8-target chunks, include/rmd.h), from all of them in one pass (rmd_corr_grad_build: the sums of
# one rmd_corr_lookup_backward per lookup into a zeroed G, in the same order, without the zero fill
# and the per-lookup read-modify-write passes), then turns G into d fmap1 / d fmap2 with two MFMA
# GEMMs that read G in its blocked order (rmd_corr_grad_gemm layouts 3 / 2, no transpose pass;
# split-bf16 products in the fp32 modes, bf16 products with fp32 accumulation in the bf16 modes) and
# the native pool / unpool kernels (G, pool and unpool in fp32 in every mode).

# False: one rmd_corr_lookup_backward per lookup into a zeroed G (the round-4 path; A/B only)
GRAD_BUILD = True
# bf16 modes: G written as bfloat16 by the build and read by the bf16-B grad GEMMs (bit-identical to
# the fp32 G, whose GEMM rounds it to bfloat16 on load; half the G traffic).  False: fp32 G (A/B only)
GRAD_BF16 = True
# The pending lookup gradients are fp32 (B, L (2r+1)^2, H, W) tensors kept alive until the pyramid
# backward (cfg2 b8, r = 4: 73 MB each, 0.88 GB for 12 lookups).  Past this many bytes they are folded
# into an fp32 G early (the build accumulates in lookup order, so G is the same sums) and released.
GRAD_PENDING_BYTES = 1 << 30


class _CorrState:
    def __init__(self, pyr, f1, f2, precision):
        self.pyr = pyr
        self.f1 = f1
        self.f2 = f2
        self.precision = precision
        self.grad = None          # dense G (GRAD_BUILD False: allocated by the first lookup backward)
        self.pending = []         # (grad_out, coords, radius, level mask) per lookup backward, in order


def _mask_bits(mask_costs, levels):
    mask = 0
    for m in mask_costs:
        if 0 <= m - 3 < levels:
            mask |= 1 << (m - 3)
    return mask


def _build_grad(st, bf16=False):
    """G from the pending lookup gradients (rmd_corr_grad_build), consecutive equal radii per launch,
    added to the fp32 G of an earlier flush if there is one; bf16: one launch writes a bfloat16 G (the
    caller checked one radius, <= 16 lookups, no earlier flush)."""
    d = st.pyr.desc
    lib = _lib.lib()
    t = lib.rmd_corr_grad_targets(d.height, d.width, d.levels)
    pend, st.pending = st.pending, []
    dev = pend[0][0].device
    G = st.grad
    if G is None:
        G = torch.empty(d.batch * d.height * d.width * t, dtype=torch.bfloat16 if bf16 else torch.float32,
                        device=dev)
    i = 0
    acc0 = 1 if st.grad is not None else 0
    while i < len(pend):
        j = i
        while j < len(pend) and pend[j][2] == pend[i][2]:
            j += 1
        grp = pend[i:j]
        gouts = (ctypes.c_void_p * len(grp))(*[x[0].data_ptr() for x in grp])
        cos = (ctypes.c_void_p * len(grp))(*[x[1].data_ptr() for x in grp])
        masks = (ctypes.c_uint * len(grp))(*[x[3] for x in grp])
        _lib.launch("rmd_corr_grad_build_ex", G, gouts, cos, masks, len(grp), ctypes.byref(d), grp[0][2],
                    1 if i > 0 else acc0, 1 if bf16 else 0, G)
        i = j
    return G


class _CorrPyramidFn(torch.autograd.Function):
    """Autograd node of raft.CorrBlock.__init__ (raft.py:18-47)."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, state):
        ctx.state = state
        return fmap1.new_zeros(())

    @staticmethod
    def backward(ctx, _gtoken):
        st = ctx.state
        f1, f2 = st.f1, st.f2
        b, c, h, w = f1.shape
        n = h * w
        levels = st.pyr.levels
        bf16_mode = PRECISIONS[st.precision][0] == RMD_BF16
        if st.pending:
            one_launch = len(st.pending) <= 16 and len({x[2] for x in st.pending}) == 1 and st.grad is None
            st.grad = _build_grad(st, bf16=GRAD_BF16 and bf16_mode and one_launch)
        if st.grad is None:
            return torch.zeros_like(f1), torch.zeros_like(f2), None
        lib = _lib.lib()
        t = lib.rmd_corr_grad_targets(h, w, levels)
        scale = st.pyr.scale
        pooled = torch.empty((b, c, t), dtype=torch.float32, device=f1.device)
        g2 = torch.empty_like(f2)
        _lib.launch("rmd_corr_pool_targets", f1, f2, b, c, h, w, levels, scale, pooled)
        G = st.grad                 # (B, T'/8, N, 8): element (t', p) at ((t'/8) N + p) 8 + t' % 8
        g1 = torch.empty((b, c, n), dtype=torch.float32, device=f1.device)
        dpool = torch.empty((b, c, t), dtype=torch.float32, device=f1.device)
        ws = torch.empty(max(lib.rmd_corr_grad_gemm_workspace_bytes(b, c, t, n),
                             lib.rmd_corr_grad_gemm_workspace_bytes(b, c, n, t), 1),
                         dtype=torch.uint8, device=f1.device)
        # grad_fmap1 = P G (K = T', layout 3: G blocked along k), dP = fmap1 G^T (K = N, layout 2: G
        # blocked along n): MFMA GEMMs (corr_grad.hip) in the block's compute — split-bf16 (fp32
        # accuracy) for the fp32 modes, one bf16 product for the bf16 modes
        gc = RMD_BF16 if bf16_mode else RMD_BF16X3
        if G.dtype == torch.bfloat16:
            # bfloat16 G (bf16 modes): the same products as the fp32-G GEMM, half the bytes
            _lib.launch("rmd_corr_grad_gemm_bf16g", f1, pooled, t, G, n, b, c, t, n, 3, g1, ws)
            _lib.launch("rmd_corr_grad_gemm_bf16g", f1, f1, n, G, n, b, c, n, t, 2, dpool, ws)
        else:
            _lib.launch("rmd_corr_grad_gemm", f1, pooled, t, G, n, b, c, t, n, 3, gc, g1, ws)
            _lib.launch("rmd_corr_grad_gemm", f1, f1, n, G, n, b, c, n, t, 2, gc, dpool, ws)
        _lib.launch("rmd_corr_unpool_targets", f1, dpool, b, c, h, w, levels, scale, g2)
        st.grad = None
        return g1.view(b, c, h, w), g2, None


class _CorrLookupFn(torch.autograd.Function):
    """Autograd node of raft.CorrBlock.__call__ (raft.py:49-95); coords carry no gradient (raft.py:402)."""

    @staticmethod
    def forward(ctx, token, coords, state, radius, mask_costs):
        out = corr_lookup(state.pyr, coords, radius, mask_costs)
        ctx.state = state
        ctx.radius = radius
        ctx.mask = _mask_bits(mask_costs, state.pyr.levels)
        ctx.save_for_backward(_f32(coords))
        return out

    @staticmethod
    def backward(ctx, gout):
        (co,) = ctx.saved_tensors
        st = ctx.state
        g = _f32(gout)
        if GRAD_BUILD:
            # G is written from every lookup's gradient at once by the pyramid backward
            st.pending.append((g, co, ctx.radius, ctx.mask))
            if sum(x[0].numel() for x in st.pending) * 4 > GRAD_PENDING_BYTES:
                st.grad = _build_grad(st)         # fp32 G, accumulated from here on
            return gout.new_zeros(()), None, None, None, None
        d = st.pyr.desc
        lib = _lib.lib()
        if st.grad is None:
            t = lib.rmd_corr_grad_targets(d.height, d.width, d.levels)
            st.grad = torch.zeros(d.batch * d.height * d.width * t, dtype=torch.float32, device=co.device)
        _lib.launch("rmd_corr_lookup_backward", co, g, ctypes.byref(d), co, ctx.radius, ctx.mask, st.grad)
        return gout.new_zeros(()), None, None, None, None


def corr_block_autograd(fmap1, fmap2, levels, precision, scale=None):
    """Pyramid + autograd token for a CorrBlock whose feature maps require gradients."""
    _require_gpu(fmap1, fmap2)
    precision = precision or get_default_precision()
    pyr = corr_pyramid(fmap1, fmap2, levels, precision, scale=scale)
    st = _CorrState(pyr, _f32(fmap1), _f32(fmap2), precision)
    token = _CorrPyramidFn.apply(fmap1, fmap2, st)
    return pyr, st, token


def corr_lookup_autograd(token, state, coords, radius, mask_costs=()):
    return _CorrLookupFn.apply(token, coords, state, radius, tuple(mask_costs))


# ---- DICL cost volumes and DAP ------------------------------------------------------------------

def dicl_stack(fmap1, fmap2, coords, radius, level=0, norm_hw=None, extra_delta=False):
    """(B,C,h,w), (B,C,hl,wl), (B,2,h,w) -> (B, 2r+1, 2r+1, 2C[+2], h, w) MatchingNet input
    (torch.ops.rmd.dicl_stack; corr/dicl.py:26-54)."""
    _same_device(fmap1, fmap2, coords)
    nh, nw = norm_hw if norm_hw is not None else fmap1.shape[-2:]
    return torch.ops.rmd.dicl_stack(fmap1, fmap2, coords, radius, level, int(nh), int(nw), bool(extra_delta))


MATCH_PRECISIONS = {"fp32": RMD_BF16X3, "bf16": RMD_BF16}
MATCH_WIDTH_STEP = 32      # the HIP kernel's hidden widths: whole 32-row MFMA tiles


class StackSpec:
    """What ops.dicl_stack would be called with, handed to MatchingNet1x1 instead of the stack itself: the
    fused path computes the cost from it (dicl_match_1x1) and the stack is never built."""

    __slots__ = ("fmap1", "fmap2", "coords", "radius", "precision", "differentiable")

    def __init__(self, fmap1, fmap2, coords, radius, precision="fp32", differentiable=False):
        self.fmap1, self.fmap2, self.coords, self.radius, self.precision = fmap1, fmap2, coords, radius, precision
        self.differentiable = differentiable


def match_padded_widths(weights):
    """Hidden widths of folded MatchingNet1x1 weights after padding to whole MFMA tiles."""
    return tuple(-(-w.shape[0] // MATCH_WIDTH_STEP) * MATCH_WIDTH_STEP for w in weights[:3])


def _pad_match(weights, biases):
    """Zero rows (and the matching zero columns of the next layer) up to the next multiple of 32: a padded
    channel is relu(0 x + 0) = 0 and multiplies zero weights, so it adds nothing."""
    ws, ts = [w.reshape(w.shape[0], -1) for w in weights[:3]] + [weights[3].reshape(1, -1)], list(biases)
    for i, wide in enumerate(match_padded_widths(ws)):
        extra = wide - ws[i].shape[0]
        if extra:
            ws[i] = torch.nn.functional.pad(ws[i], (0, 0, 0, extra))
            ts[i] = torch.nn.functional.pad(ts[i].reshape(-1), (0, extra))
            ws[i + 1] = torch.nn.functional.pad(ws[i + 1], (0, extra))
    return ws[:3] + [ws[3].reshape(-1)], ts


def dicl_match_1x1(fmap1, fmap2, coords, radius, weights, biases, precision="fp32", differentiable=False):
    """Fused dicl-1x1 cost (torch.ops.rmd.dicl_match_1x1; corr/dicl_1x1.py:8-30, 51-79): fmap1, fmap2
    (B, C, h, w), coords (B, 2, h, w) -> (B, 2r+1, 2r+1, h, w), the displacement gather of ops.dicl_stack and
    the folded MatchingNet1x1 (weights [W1', W2', W3', w4], biases [t1, t2, t3, b4] from
    MatchingNet1x1.folded()) in one kernel.  precision "fp32": three split-bf16 products per layer (parity
    mode); "bf16": one.  Not differentiable unless differentiable=True, which routes to
    torch.ops.rmd.dicl_match_1x1_train: the same cost bit for bit (fp32 only), whose backward recomputes the
    MLP per column (rmd_dicl_match_1x1_backward) and reaches fmap1, fmap2 and, through the padding here and
    MatchingNet1x1.folded(), the raw parameters."""
    if precision not in MATCH_PRECISIONS:
        raise ValueError(f"dicl_match_1x1: unknown precision '{precision}', expected one of {sorted(MATCH_PRECISIONS)}")
    if differentiable and precision != "fp32":
        raise ValueError("dicl_match_1x1: the one-product mode has no backward (differentiable=True needs precision='fp32')")
    weights, biases = list(weights), list(biases)
    _same_device(fmap1, fmap2, coords, *weights, *biases)
    if len(weights) == 4 and len(biases) == 4 and fmap1.device.type == "cuda":
        weights, biases = _pad_match(weights, biases)
    if differentiable:
        return torch.ops.rmd.dicl_match_1x1_train(fmap1, fmap2, coords, int(radius), weights, biases)
    return torch.ops.rmd.dicl_match_1x1(fmap1, fmap2, coords, int(radius), weights, biases, MATCH_PRECISIONS[precision])


GRU_PRECISIONS = MATCH_PRECISIONS


def sepconv_gru(h, x, weights, biases, precision="fp32"):
    """Fused SepConvGRU (torch.ops.rmd.sepconv_gru; raft.py:228-259), inference only: h (B, Hd, H, W),
    x (B, Xd, H, W), weights [z1, r1, q1, z2, r2, q2] and their biases -> the new h.  precision "fp32": three
    split-bf16 products per convolution (parity mode); "bf16": one.  Not differentiable."""
    if precision not in GRU_PRECISIONS:
        raise ValueError(f"sepconv_gru: unknown precision '{precision}', expected one of {sorted(GRU_PRECISIONS)}")
    weights, biases = list(weights), list(biases)
    _same_device(h, x, *weights, *biases)
    return torch.ops.rmd.sepconv_gru(h, x, weights, biases, GRU_PRECISIONS[precision])


CONV_PRECISIONS = MATCH_PRECISIONS
CONV_ACTS = {"none": 0, "relu": 1}


def conv2d_act(x0, x1, weight, bias, act="none", precision="fp32", differentiable=False):
    """Fused convolution (torch.ops.rmd.conv2d_act; raft.py:193-225, 262-273, 299-331): a stride-1,
    "same"-padded convolution over cat(x0 (B, C0, H, W), x1 (B, C1, H, W) or None) with weight (Cout, C0 + C1,
    kh, kw), kh and kw odd, bias (Cout,) and act "none" or "relu" -> (B, Cout, H, W).  precision "fp32": three
    split-bf16 products (parity mode); "bf16": one.  Not differentiable unless differentiable=True, which routes to
    torch.ops.rmd.conv2d_act_train: the same result bit for bit (fp32 only), whose backward (rmd_conv2d_backward)
    reaches x0, x1, weight and bias."""
    if precision not in CONV_PRECISIONS:
        raise ValueError(f"conv2d_act: unknown precision '{precision}', expected one of {sorted(CONV_PRECISIONS)}")
    if act not in CONV_ACTS:
        raise ValueError(f"conv2d_act: unknown activation '{act}', expected one of {sorted(CONV_ACTS)}")
    if differentiable and precision != "fp32":
        raise ValueError("conv2d_act: the one-product mode has no backward (differentiable=True needs precision='fp32')")
    _same_device(x0, *([] if x1 is None else [x1]), weight, bias)
    if differentiable:
        return torch.ops.rmd.conv2d_act_train(x0, x1, weight, bias, CONV_ACTS[act])
    return torch.ops.rmd.conv2d_act(x0, x1, weight, bias, CONV_ACTS[act], CONV_PRECISIONS[precision])


def motion_encoder(flow, corr, weights, biases, precision="fp32"):
    """Fused BasicMotionEncoder (torch.ops.rmd.motion_encoder; raft.py:193-225), inference only: flow (B, 2, H, W),
    corr (B, planes, H, W), weights and biases of convc1, convc2, convf1, convf2, conv -> (B, 128, H, W) whose
    last two channels are flow.  Five convolutions with ReLU epilogues; no cat.  Not differentiable."""
    if precision not in CONV_PRECISIONS:
        raise ValueError(f"motion_encoder: unknown precision '{precision}', expected one of {sorted(CONV_PRECISIONS)}")
    weights, biases = list(weights), list(biases)
    _same_device(flow, corr, *weights, *biases)
    return torch.ops.rmd.motion_encoder(flow, corr, weights, biases, CONV_PRECISIONS[precision])


ENCODER_NORMS = {"none": _lib.RMD_NORM_NONE, "instance": _lib.RMD_NORM_INSTANCE}


def _given(*tensors):
    return [t for t in tensors if t is not None]


def conv2d_norm_act(x, weight, bias, scale=None, shift=None, residual=None, stride=1, act="none", precision="fp32"):
    """Strided, normalising convolution (torch.ops.rmd.conv2d_norm_act; blocks/raft.py:13-46), inference only: a
    convolution of stride 1 or 2 and padding k / 2 over relu(x scale + shift) (the (B, C) statistics of
    instance_norm_stats; x itself without them), bias, act "none" or "relu" and, with a residual of the output's
    shape, relu(. + residual) -> (B, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1).  Not differentiable."""
    if precision not in CONV_PRECISIONS:
        raise ValueError(f"conv2d_norm_act: unknown precision '{precision}', expected one of {sorted(CONV_PRECISIONS)}")
    if act not in CONV_ACTS:
        raise ValueError(f"conv2d_norm_act: unknown activation '{act}', expected one of {sorted(CONV_ACTS)}")
    _same_device(x, weight, bias, *_given(scale, shift, residual))
    return torch.ops.rmd.conv2d_norm_act(x, scale, shift, weight, bias, residual, stride, CONV_ACTS[act],
                                         CONV_PRECISIONS[precision])


def instance_norm_stats(x, eps=1e-5):
    """nn.InstanceNorm2d at its defaults in scale / shift form (torch.ops.rmd.instance_norm_stats): x (B, C, H, W)
    -> (scale, shift), both (B, C), with norm(x) = x scale + shift.  Not differentiable."""
    _same_device(x)
    return torch.ops.rmd.instance_norm_stats(x, float(eps))


def residual_join(y, x, y_stats=None, x_stats=None):
    """relu(xs + relu(ys)) (torch.ops.rmd.residual_join; blocks/raft.py:38-46): ys = y scale + shift for y_stats =
    (scale, shift), xs likewise (the projection's norm); each as given without statistics.  Not differentiable."""
    ya, yd = y_stats or (None, None)
    xa, xd = x_stats or (None, None)
    _same_device(y, x, *_given(ya, yd, xa, xd))
    return torch.ops.rmd.residual_join(y, ya, yd, x, xa, xd)


def feature_encoder(x, weights, biases, norm="none", precision="fp32"):
    """Fused FeatureEncoder (torch.ops.rmd.feature_encoder; encoders/raft/s3.py:8-72), inference only: x (B, 3, H, W),
    the 16 convolutions' weights and biases in module order (batch norm folded in), norm "none" or "instance"
    -> (B, output_dim, H / 8, W / 8).  Not differentiable."""
    if precision not in CONV_PRECISIONS:
        raise ValueError(f"feature_encoder: unknown precision '{precision}', expected one of {sorted(CONV_PRECISIONS)}")
    if norm not in ENCODER_NORMS:
        raise ValueError(f"feature_encoder: unknown norm '{norm}', expected one of {sorted(ENCODER_NORMS)}")
    weights, biases = list(weights), list(biases)
    _same_device(x, *weights, *biases)
    return torch.ops.rmd.feature_encoder(x, weights, biases, ENCODER_NORMS[norm], CONV_PRECISIONS[precision])


MNET_PRECISIONS = MATCH_PRECISIONS
# Default budget of matching_net's workspace (the packed weights and one group's four intermediate maps).
# Provenance: tools/mnet_probe.py, profiles/mnet_r18.json "budgets" — the whole network at the cfg4 1/8 level on b8
# (648 images of 64 x 48 x 160; MIOpen 18.5 ms), median of 20, fp32 / bf16 mode:
#    64 MiB (groups of 12)  20.13 / 11.78 ms
#   128 MiB (24)            12.84 /  7.86 ms
#   256 MiB (49)            12.88 /  5.82 ms
#   512 MiB (98)            13.04 /  5.15 ms
# The fp32 mode is flat from 128 MiB on (within 1.6 %), the bf16 mode keeps gaining; 512 MiB has the smallest sum of
# the two and is the default.  No knee at the 256 MiB Infinity Cache shows in either mode.
MNET_WORKSPACE_BYTES = 512 << 20


def mnet_group(images, widths, height, width, workspace_bytes=None):
    """Images per pass of matching_net: the largest count whose workspace (rmd_matching_net_workspace_bytes) fits
    `workspace_bytes` (default MNET_WORKSPACE_BYTES), at least 1 and at most `images`.  Host arithmetic only."""
    budget = MNET_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    one = library.mnet_workspace_bytes(1, *widths, height, width)
    if one == 0:
        raise ValueError(f"matching_net: unsupported sizes: channels {tuple(widths)} on {height} x {width} "
                         f"({library.MNET_RANGE})")
    per = library.mnet_workspace_bytes(2, *widths, height, width) - one     # the maps are linear in the group
    group = max(1, min(images, 1 + (budget - one) // per if budget > one else 1))
    while group > 1 and library.mnet_workspace_bytes(group, *widths, height, width) > budget:
        group -= 1                                                          # each map is rounded up to 256 bytes
    return group


def matching_net(mvol, weights, biases, precision="fp32", workspace_bytes=None):
    """Fused k x k MatchingNet (torch.ops.rmd.matching_net; blocks/dicl.py:93-118), inference only: mvol (B, du, dv,
    c_in, h, w), h and w even, with the folded parameters of MatchingNet.folded() -> cost (B, du, dv, h, w).  The
    B du dv images are walked in groups whose workspace fits `workspace_bytes` (default MNET_WORKSPACE_BYTES); the
    result does not depend on it, bit for bit.  precision "fp32": three split-bf16 products per layer (parity mode);
    "bf16": one; the last layer is fp32 in both.  Not differentiable."""
    if precision not in MNET_PRECISIONS:
        raise ValueError(f"matching_net: unknown precision '{precision}', expected one of {sorted(MNET_PRECISIONS)}")
    weights, biases = list(weights), list(biases)
    _same_device(mvol, *weights, *biases)
    group = 1
    if mvol.device.type == "cuda":
        widths = library.check_mnet_args(mvol, weights, biases, 1, MNET_PRECISIONS[precision])
        b, du, dv, _, ht, wd = mvol.shape
        group = mnet_group(b * du * dv, widths, ht, wd, workspace_bytes)
    return torch.ops.rmd.matching_net(mvol, weights, biases, group, MNET_PRECISIONS[precision])


def mnet_tail(x, weight5, bias5, weight6, bias6, precision="fp32"):
    """The last two layers of MatchingNet in one kernel (torch.ops.rmd.mnet_tail; blocks/dicl.py:107-108), inference
    only: x (N, c3, h2, w2), weight5 (c3, c4, 4, 4) and bias5 (c4,) of the transposed convolution (norm folded in),
    weight6 (c4, 3, 3) and bias6 (1,) -> cost (N, 2 h2, 2 w2).  Not differentiable."""
    if precision not in MNET_PRECISIONS:
        raise ValueError(f"mnet_tail: unknown precision '{precision}', expected one of {sorted(MNET_PRECISIONS)}")
    _same_device(x, weight5, bias5, weight6, bias6)
    return torch.ops.rmd.mnet_tail(x, weight5, bias5, weight6, bias6, MNET_PRECISIONS[precision])


def dicl_stack_int(fmap1, fmap2, ru, rv):
    """Integer-displacement matching volume with occlusion mask (torch.ops.rmd.dicl_stack_int;
    impls/dicl.py:212-238)."""
    _same_device(fmap1, fmap2)
    return torch.ops.rmd.dicl_stack_int(fmap1, fmap2, ru, rv)


def dicl_stack_int_warped(fmap1, fmap2, flow, ru, rv):
    """Masked integer volume of (fmap1, warp_backwards(fmap2, flow)) in one fused pass pair
    (torch.ops.rmd.dicl_stack_int_warped; impls/dicl.py:178-181 + 212-238)."""
    _same_device(fmap1, fmap2, flow)
    return torch.ops.rmd.dicl_stack_int_warped(fmap1, fmap2, flow, ru, rv)


def dap(x, weight):
    """x (B, D, ...) -> W x over the displacement dim; weight (D, D[, 1, 1]) (torch.ops.rmd.dap;
    blocks/dicl.py:143-150)."""
    _same_device(x, weight)
    return torch.ops.rmd.dap(x, weight)


def up8(mask, flow, temperature=4.0):
    """mask (B, 576, h, w) logits, flow (B, 2, h, w) -> convex-upsampled flow (B, 2, 8h, 8w)
    (torch.ops.rmd.up8; raft.py:319-331)."""
    _same_device(mask, flow)
    return torch.ops.rmd.up8(mask, flow, float(temperature))


def softargmax(cost, levels, radius, temperature=1.0):
    """cost (B, >= L*(2r+1)^2, h, w) -> list of L flows (B, 2, h, w), level l scaled by 2^l
    (torch.ops.rmd.softargmax; raft.py:112-135, corr/dot.py:83-90)."""
    _same_device(cost)
    return list(torch.ops.rmd.softargmax(cost, levels, radius, float(temperature)).unbind(0))


def dicl_flow_head(cost, flow_coarse=None, eps=1e-9):
    """cost (B, du, dv, h, w) [+ flow_coarse (B, 2, h, w)] -> (flow (B, 2, h, w), entropy (B, 1, h, w)): the
    soft-argmin flow (plus the coarse flow) and the normalised entropy of the same softmax, two views of
    the one (B, 3, h, w) output of torch.ops.rmd.dicl_flow_head (impls/dicl.py:31-85, 194-195, 202)."""
    if flow_coarse is None:
        _same_device(cost)
    else:
        _same_device(cost, flow_coarse)
    out = torch.ops.rmd.dicl_flow_head(cost, flow_coarse, float(eps))
    return out[:, :2], out[:, 2:]


def local_cross_attn(q, k, v, window=(3, 3)):
    """q (B, ck, h, w), k (B, ck, h2, w2), v (B, cv, h2, w2) -> (B, cv, h, w): every fine pixel attends over
    the `window` of coarse cells around its parent cell, zero-padded at the border (the attention of
    HUpCrossAttn.forward, common/hsup.py:71-92), in one pass without the expanded K / V."""
    _same_device(q, k, v)
    win_y, win_x = (int(s) for s in window)
    return torch.ops.rmd.local_cross_attn(q, k, v, win_y, win_x)


# ---- sequence losses -----------------------------------------------------------------------------

LOSS_ORDS = {1: _lib.RMD_LOSS_L1, 2: _lib.RMD_LOSS_L2, "absmean": _lib.RMD_LOSS_ABSMEAN,
             "robust": _lib.RMD_LOSS_ROBUST}
LOSS_MODES = ("bilinear",)


class _SequenceLossFn(torch.autograd.Function):
    """Autograd node of one rmd_sequence_loss call (a list-valued formula, like _CorrPyramidFn).  The
    backward recomputes from the inputs: only the K pixel counts are kept besides them."""

    @staticmethod
    def forward(ctx, target, valid, masks, mask_index, weights, norm, include_invalid, skip_empty, scale, *flows):
        loss, counts = torch.ops.rmd.sequence_loss(list(flows), target, valid, masks, mask_index, weights, norm,
                                                   include_invalid, skip_empty, scale)
        ctx.save_for_backward(target, valid, counts, *masks, *flows)
        ctx.meta = (len(masks), mask_index, weights, norm, include_invalid, scale)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        nmask, mask_index, weights, norm, include_invalid, scale = ctx.meta
        target, valid, counts = ctx.saved_tensors[:3]
        masks = list(ctx.saved_tensors[3:3 + nmask])
        flows = list(ctx.saved_tensors[3 + nmask:])
        needs = [bool(n) for n in ctx.needs_input_grad[9:]]
        grads = torch.ops.rmd.sequence_loss_backward(gloss, flows, target, valid, masks, mask_index, weights, counts,
                                                     needs, norm, include_invalid, scale)
        return (None,) * 9 + tuple(g.to(f.dtype) if n else None for g, f, n in zip(grads, flows, needs))


def sequence_loss(flows, target, valid, weights, ord=1, masks=None, include_invalid=False, skip_empty=False,
                  scale=1.0, mode="bilinear"):
    """scale * sum_k weights[k] * mean over the set pixels of dist_ord(up(flows[k]) - target) — the loop of
    raft.py:616-644, loss/mlseq.py:34-57, raft_dicl_ctf_l3.py:430-463 and dicl.py:436-462 in one fused pass
    (torch.ops.rmd.sequence_loss).  flows: (B, 2, h_k, w_k) each, upsampled bilinearly (align_corners, scaled
    by the size ratios) where smaller than target (B, 2, H, W); valid (B, H, W) bool or uint8; masks: None or
    one entry per prediction, a (B, H, W) mask that replaces `valid` or None.  GPU tensors run the HIP
    kernels and never fall back: ord must be 1, 2, 'absmean' or 'robust' and mode 'bilinear'."""
    flows = list(flows)
    masks = [None] * len(flows) if masks is None else list(masks)
    weights = [float(w) for w in weights]
    if len(masks) != len(flows) or len(weights) != len(flows):
        raise ValueError(f"sequence_loss: {len(flows)} flows, {len(weights)} weights, {len(masks)} masks")
    _same_device(target, valid, *flows, *[m for m in masks if m is not None])
    try:
        norm = LOSS_ORDS.get(ord)
    except TypeError:
        norm = None
    if norm is None or mode not in LOSS_MODES:
        if target.device.type != "cpu":
            raise ValueError(f"sequence_loss: ord={ord!r}, mode={mode!r} has no HIP kernel (supported: ord 1, 2, "
                             f"'absmean', 'robust'; mode 'bilinear'); GPU tensors do not fall back")
        from . import cpu
        return cpu.sequence_loss_eager(flows, target, valid, masks, weights, ord, include_invalid, skip_empty,
                                       scale, mode)[0]
    total = None
    step = _lib.LOSS_MAX_PREDICTIONS
    for i in range(0, len(flows), step):
        own, index = [], []
        for m in masks[i:i + step]:
            if m is None:
                index.append(-1)
            else:
                hit = next((j for j, o in enumerate(own) if o is m), None)
                if hit is None:
                    hit = len(own)
                    own.append(m)
                index.append(hit)
        if target.device.type == "cpu":        # the CPU kernel's own ATen graph carries the gradient
            part = torch.ops.rmd.sequence_loss(flows[i:i + step], target, valid, own, index, weights[i:i + step],
                                               norm, include_invalid, skip_empty, float(scale))[0]
        else:
            part = _SequenceLossFn.apply(target, valid, own, index, weights[i:i + step], norm, bool(include_invalid),
                                         bool(skip_empty), float(scale), *flows[i:i + step])
        total = part if total is None else total + part
    return target.new_zeros((), dtype=torch.float32) if total is None else total


# ---- flow metrics --------------------------------------------------------------------------------

_SLOT_PIXELS, _SLOT_VALID, _SLOT_EPE, _SLOT_FL, _SLOT_ANGLE, _SLOT_ANGLE_VALID, _SLOT_MAG, _SLOT_BAD, _SLOT_NEAR = range(9)


class FlowMetricsResult:
    """Raw statistics of one rmd.ops.flow_metrics call: `stats` (estimates, samples, 8 + len(distances))
    float64 on the inputs' device, slots as in include/rmd.h (the 8 fixed ones, then one count per
    distance).  per_sample() / batch() derive the metrics as tensors on that device; nothing is read
    back before host(), which copies everything to the CPU in one transfer."""

    def __init__(self, stats, distances, ord, extra=None):
        self.stats = stats
        self.distances = tuple(distances)
        self.ord = ord
        self.extra = extra
        self._derived = {}              # per_sample() / batch() are derived once; `stats` is not modified

    def _derive(self, s):
        n_px, n_valid = s[..., _SLOT_PIXELS], s[..., _SLOT_VALID]
        return {
            "n_pixels": n_px, "n_valid": n_valid, "nonfinite": s[..., _SLOT_BAD],
            "epe": s[..., _SLOT_EPE] / n_valid,                                     # epe.py:50
            "within": s[..., _SLOT_NEAR:] / n_valid.unsqueeze(-1),                  # epe.py:51, one per distance
            "fl_all": s[..., _SLOT_FL] / n_valid,                                   # fl_all.py:44
            "aae": torch.rad2deg(s[..., _SLOT_ANGLE] / n_px),                       # aae.py:44, all pixels
            "aae_valid": torch.rad2deg(s[..., _SLOT_ANGLE_VALID] / n_valid),
            "magnitude": s[..., _SLOT_MAG] / n_px,                                  # flow.py:34
        }

    def per_sample(self):
        """Every sample on its own: tensors (estimates, samples), `within` (estimates, samples, distances)."""
        if "per_sample" not in self._derived:
            self._derived["per_sample"] = self._derive(self.stats)
        return self._derived["per_sample"]

    def batch_stats(self):
        """The sample rows added in index order (estimates, slots)."""
        total = self.stats[:, 0]
        for b in range(1, self.stats.shape[1]):
            total = total + self.stats[:, b]
        return total

    def batch(self):
        """The whole batch as one set of pixels: tensors (estimates,), `within` (estimates, distances)."""
        if "batch" not in self._derived:
            self._derived["batch"] = self._derive(self.batch_stats())
        return self._derived["batch"]

    def host(self):
        """The same result on the CPU: ONE device-to-host copy carries the statistics and `extra` (a
        tensor that rides along, e.g. the loss; returned as float64 in `.extra`)."""
        if self.stats.device.type == "cpu":
            extra = None if self.extra is None else self.extra.detach().double()
            return FlowMetricsResult(self.stats, self.distances, self.ord, extra)
        if self.extra is None:
            return FlowMetricsResult(self.stats.cpu(), self.distances, self.ord)
        extra = self.extra.detach()
        packed = torch.cat([self.stats.reshape(-1), extra.double().reshape(-1)]).cpu()
        n = self.stats.numel()
        return FlowMetricsResult(packed[:n].view(self.stats.shape), self.distances, self.ord,
                                 packed[n:].view(extra.shape))


def flow_metrics(estimates, target, valid, distances=(1, 3, 5), fl=(3, 0.05), ord=2, extra=None):
    """The flow metrics of src/metrics (epe.py, fl_all.py, aae.py, flow.py) for every estimate and every
    sample in one fused pass (torch.ops.rmd.flow_metrics) -> FlowMetricsResult.  estimates: one tensor or
    a sequence, each shaped like target: (B, 2, H, W) or a single instance (2, H, W) (then valid is
    (H, W) and B = 1); valid bool or uint8.  distances: the epe thresholds (`<=`), fl: (absolute,
    relative) outlier thresholds, ord: the magnitude's norm (1, 2, inf or any other p > 0).  More than 8
    distances or 32 estimates are chunked into several launches.  Nothing synchronises with the host:
    read the result with .host().  Not differentiable."""
    estimates = [estimates] if isinstance(estimates, torch.Tensor) else list(estimates)
    if not estimates:
        raise ValueError("flow_metrics: no estimate")
    _same_device(target, valid, *estimates)
    if target.dim() == 3:
        target, valid = target.unsqueeze(0), valid.unsqueeze(0)
        estimates = [e.unsqueeze(0) if e.dim() == 3 else e for e in estimates]
    if valid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"flow_metrics: valid must be bool or uint8, got {valid.dtype}")
    ord = float(ord)
    if not ord > 0:
        raise ValueError(f"flow_metrics: bad ord {ord} (1, 2, inf or any other p > 0)")
    distances = [float(d) for d in distances]
    es, tg, va = [_f32(e) for e in estimates], _f32(target), valid.detach().contiguous()
    dstep, estep = _lib.METRICS_MAX_DISTANCES, _lib.METRICS_MAX_ESTIMATES
    rows = []
    for i in range(0, len(es), estep):
        parts = []
        for j in range(0, max(len(distances), 1), dstep):
            chunk = distances[j:j + dstep]
            st = torch.ops.rmd.flow_metrics(es[i:i + estep], tg, va, chunk, float(fl[0]), float(fl[1]), ord)
            parts.append(st[..., :_SLOT_NEAR + len(chunk)] if j == 0 else st[..., _SLOT_NEAR:_SLOT_NEAR + len(chunk)])
        rows.append(parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1))
    stats = rows[0] if len(rows) == 1 else torch.cat(rows, dim=0)
    return FlowMetricsResult(stats, distances, ord, extra)
