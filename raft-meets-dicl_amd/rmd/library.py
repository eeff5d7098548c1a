"""torch.library registration of the rmd operators: `torch.ops.rmd.*` over the C ABI of librmd.so.

One table (_OPS: name -> family, schema) defines every operator.  Each has a HIP kernel (CUDA dispatch
key, registered with @_hip: the device checks, then one _lib.launch of the C entry point on torch's
current stream), a fake (meta) kernel that only computes output shapes (torch.compile / torch.export /
FakeTensor tracing; where both allocate the same outputs they share the function that states the shapes),
a CPU kernel for CPU tensors (rmd/cpu.py: the reference's ATen algorithm, registered for CPU and
AutogradCPU — a dispatch by device, never a fallback for a GPU tensor), and, where the reference's
module is trained through it, an autograd formula whose backward is again an rmd operator.  A new
operator is one table entry here, its kernels, and one function of its name in rmd/cpu.py.  Schemas
follow SURVEY.md §8(b):

  corr_pyramid(fmap1, fmap2, levels, compute, storage, scale) -> pyramid     raft.py:18-47
  corr_lookup(pyramid, coords, levels, radius, level_mask) -> corr           raft.py:49-95
  corr_otf_prepare / corr_otf_lookup                                        raft_fs.py:13-87, corr/dot.py:25-57
  dicl_stack(fmap1, fmap2, coords, radius, level, norm_h, norm_w, extra) ->  corr/dicl.py:26-54,
        (B, 2r+1, 2r+1, 2C[+2], h, w)                                        dicl_emb.py:51-89, raft_dicl_ml.py:294-315
  dicl_stack_int(fmap1, fmap2, ru, rv), dicl_stack_int_warped(.., flow, ..) impls/dicl.py:178-238
  dap(x, weight)                                                             blocks/dicl.py:143-150
  up8(mask, flow, temperature), softargmax(cost, levels, radius, T)          raft.py:98-190, 319-331
  warp_backwards(img2, flow, eps) -> (est, mask)                             common/warp.py:5-33
  sequence_loss(flows[], target, valid, masks[], ...) -> (loss, counts)      raft.py:616-644, loss/mlseq.py:34-67,
                                                                             raft_dicl_ctf_l3.py:430-473, dicl.py:436-472
  flow_metrics(estimates[], target, valid, distances[], ...) -> stats        metrics/epe.py, fl_all.py, aae.py, flow.py
  dicl_flow_head(cost, flow_coarse?, eps) -> (B, 3, h, w) flow + entropy     impls/dicl.py:31-85, 194-195, 202
  local_cross_attn(q, k, v, win_y, win_x) -> (B, cv, h, w)                   common/hsup.py:71-92
  dicl_match_1x1(fmap1, fmap2, coords, radius, weights[], biases[],          corr/dicl_1x1.py:8-30, 51-79
        compute) -> (B, 2r+1, 2r+1, h, w) cost
  dicl_match_1x1_train(fmap1, fmap2, coords, radius, weights[], biases[])    the same cost (fp32 mode), differentiable:
        / dicl_match_1x1_backward(grad, ..., needs_grad) -> grads[]          its formula recomputes from the inputs
  sepconv_gru(h, x, weights[], biases[], compute) -> (B, Hd, H, W)           raft.py:228-259 (inference)
  conv2d_act(x0, x1?, weight, bias, act, compute) -> (B, Cout, H, W)         raft.py:193-225, 262-273, 299-331
  conv2d_act_train(x0, x1?, weight, bias, act) / conv2d_act_backward(...)    the same, differentiable (fp32 mode)
  motion_encoder(flow, corr, weights[], biases[], compute) -> (B, 128, H, W) raft.py:193-225 (both inference)
  conv2d_norm_act / instance_norm_stats / residual_join / feature_encoder     encoders/raft/s3.py:8-72,
                                                                              blocks/raft.py:13-46 (inference)
  matching_net(mvol, weights[], biases[], group, compute) -> (B, du, dv, h, w) blocks/dicl.py:93-118 (inference)
  mnet_tail(x, weight5, bias5, weight6, bias6, compute) -> (N, 2 h2, 2 w2)    its last two layers (:107-108)

The RAFT correlation's training path keeps rmd.ops' token-linked autograd functions: all lookups of
one CorrBlock accumulate into ONE dense pyramid gradient (query-minor, fp32) whose layout differs from
the pyramid tensor's own (chunked, fp16 in the perf mode), which a per-op autograd formula (gradient
shaped and typed like its input) cannot express.  corr_pyramid / corr_lookup here are the inference
operators.
"""

import ctypes

import torch

from . import _lib

LIB = torch.library.Library("rmd", "DEF")

# name -> (family, schema without the name).  Families: "model" is the SURVEY.md §8(b) model-operator
# set (operators()); "loss", "metric", "head", "attn", "match", "match_train", "update", "conv", "conv_train",
# "encoder" and "mnet" are listed by loss_operators(), metric_operators(), head_operators(), attn_operators(),
# match_operators(), match_train_operators(), update_operators(), conv_operators(), conv_train_operators(),
# encoder_operators() and mnet_operators().
_OPS = {
    "corr_pyramid": ("model", "(Tensor fmap1, Tensor fmap2, int levels, int compute, int storage, float scale) "
                              "-> Tensor"),
    "corr_lookup": ("model", "(Tensor pyramid, Tensor coords, int levels, int radius, int level_mask) -> Tensor"),
    "corr_otf_prepare": ("model", "(Tensor fmap1, Tensor fmap2, int levels, int compute, float scale) -> Tensor"),
    "corr_otf_lookup": ("model", "(Tensor workspace, Tensor coords, int channels, int levels, int compute, int radius, "
                                 "int level_mask) -> Tensor"),
    "dicl_stack": ("model", "(Tensor fmap1, Tensor fmap2, Tensor coords, int radius, int level, int norm_h, "
                            "int norm_w, bool extra_delta) -> Tensor"),
    "dicl_stack_backward": ("model", "(Tensor grad, Tensor coords, int channels, int level_h, int level_w, int radius, "
                                     "int level, int norm_h, int norm_w, bool extra_delta) -> (Tensor, Tensor)"),
    "dicl_stack_int": ("model", "(Tensor fmap1, Tensor fmap2, int ru, int rv) -> Tensor"),
    "dicl_stack_int_backward": ("model", "(Tensor grad, Tensor fmap2, int ru, int rv) -> (Tensor, Tensor)"),
    "dicl_stack_int_warped": ("model", "(Tensor fmap1, Tensor fmap2, Tensor flow, int ru, int rv) -> Tensor"),
    "dicl_stack_int_warped_backward": ("model", "(Tensor grad, Tensor fmap2, Tensor flow, int ru, int rv) "
                                                "-> (Tensor, Tensor)"),
    "dap": ("model", "(Tensor x, Tensor weight) -> Tensor"),
    "dap_transpose": ("model", "(Tensor grad, Tensor weight) -> Tensor"),
    "dap_weight_grad": ("model", "(Tensor grad, Tensor x, int disp) -> Tensor"),
    "up8": ("model", "(Tensor mask, Tensor flow, float temperature) -> Tensor"),
    "up8_backward": ("model", "(Tensor grad, Tensor mask, Tensor flow, float temperature) -> (Tensor, Tensor)"),
    "softargmax": ("model", "(Tensor cost, int levels, int radius, float temperature) -> Tensor"),
    "softargmax_backward": ("model", "(Tensor grad, Tensor cost, int levels, int radius, float temperature) -> Tensor"),
    "warp_backwards": ("model", "(Tensor img2, Tensor flow, float eps) -> (Tensor, Tensor)"),
    "warp_backwards_backward": ("model", "(Tensor grad, Tensor flow, float eps) -> Tensor"),
    "sequence_loss": ("loss", "(Tensor[] flows, Tensor target, Tensor valid, Tensor[] masks, int[] mask_index, "
                              "float[] weights, int norm, bool include_invalid, bool skip_empty, float scale) "
                              "-> (Tensor, Tensor)"),
    "sequence_loss_backward": ("loss", "(Tensor grad_loss, Tensor[] flows, Tensor target, Tensor valid, "
                                       "Tensor[] masks, int[] mask_index, float[] weights, Tensor counts, "
                                       "bool[] needs_grad, int norm, bool include_invalid, float scale) -> Tensor[]"),
    "flow_metrics": ("metric", "(Tensor[] estimates, Tensor target, Tensor valid, float[] distances, float fl_abs, "
                               "float fl_rel, float mag_ord) -> Tensor"),
    "dicl_flow_head": ("head", "(Tensor cost, Tensor? flow_coarse, float eps) -> Tensor"),
    "dicl_flow_head_backward": ("head", "(Tensor grad, Tensor cost, float eps) -> Tensor"),
    "local_cross_attn": ("attn", "(Tensor q, Tensor k, Tensor v, int win_y, int win_x) -> Tensor"),
    "local_cross_attn_backward": ("attn", "(Tensor grad, Tensor q, Tensor k, Tensor v, int win_y, int win_x) "
                                          "-> (Tensor, Tensor, Tensor)"),
    "dicl_match_1x1": ("match", "(Tensor fmap1, Tensor fmap2, Tensor coords, int radius, Tensor[] weights, "
                                "Tensor[] biases, int compute) -> Tensor"),
    "dicl_match_1x1_train": ("match_train", "(Tensor fmap1, Tensor fmap2, Tensor coords, int radius, "
                                            "Tensor[] weights, Tensor[] biases) -> Tensor"),
    "dicl_match_1x1_backward": ("match_train", "(Tensor grad, Tensor fmap1, Tensor fmap2, Tensor coords, int radius, "
                                               "Tensor[] weights, Tensor[] biases, bool[] needs_grad) -> Tensor[]"),
    "sepconv_gru": ("update", "(Tensor h, Tensor x, Tensor[] weights, Tensor[] biases, int compute) -> Tensor"),
    "conv2d_act": ("conv", "(Tensor x0, Tensor? x1, Tensor weight, Tensor bias, int act, int compute) -> Tensor"),
    "motion_encoder": ("conv", "(Tensor flow, Tensor corr, Tensor[] weights, Tensor[] biases, int compute) -> Tensor"),
    "conv2d_act_train": ("conv_train", "(Tensor x0, Tensor? x1, Tensor weight, Tensor bias, int act) -> Tensor"),
    "conv2d_act_backward": ("conv_train", "(Tensor grad, Tensor? y, Tensor x0, Tensor? x1, Tensor weight, int act, "
                                          "bool[] needs_grad) -> Tensor[]"),
    "conv2d_norm_act": ("encoder", "(Tensor x, Tensor? scale, Tensor? shift, Tensor weight, Tensor bias, "
                                   "Tensor? residual, int stride, int act, int compute) -> Tensor"),
    "instance_norm_stats": ("encoder", "(Tensor x, float eps) -> (Tensor, Tensor)"),
    "residual_join": ("encoder", "(Tensor y, Tensor? y_scale, Tensor? y_shift, Tensor x, Tensor? x_scale, "
                                 "Tensor? x_shift) -> Tensor"),
    "feature_encoder": ("encoder", "(Tensor x, Tensor[] weights, Tensor[] biases, int norm, int compute) -> Tensor"),
    "matching_net": ("mnet", "(Tensor mvol, Tensor[] weights, Tensor[] biases, int group, int compute) -> Tensor"),
    "mnet_tail": ("mnet", "(Tensor x, Tensor weight5, Tensor bias5, Tensor weight6, Tensor bias6, int compute) "
                          "-> Tensor"),
}
for _name, (_, _schema) in _OPS.items():
    LIB.define(_name + _schema)


def _family(family):
    return sorted(name for name, (f, _) in _OPS.items() if f == family)


def operators():
    """Names of the registered torch.ops.rmd model operators."""
    return _family("model")


def loss_operators():
    """Names of the registered torch.ops.rmd loss operators."""
    return _family("loss")


def metric_operators():
    """Names of the registered torch.ops.rmd metric operators."""
    return _family("metric")


def head_operators():
    """Names of the registered torch.ops.rmd DICL flow-head operators."""
    return _family("head")


def attn_operators():
    """Names of the registered torch.ops.rmd hidden-state upsampler (local cross-attention) operators."""
    return _family("attn")


def match_operators():
    """Names of the registered torch.ops.rmd fused matching-network operators."""
    return _family("match")


def match_train_operators():
    """Names of the registered torch.ops.rmd differentiable fused matching-network operators."""
    return _family("match_train")


def update_operators():
    """Names of the registered torch.ops.rmd update-block (recurrent unit) operators."""
    return _family("update")


def conv_operators():
    """Names of the registered torch.ops.rmd update-block convolution operators."""
    return _family("conv")


def conv_train_operators():
    """Names of the registered torch.ops.rmd differentiable update-block convolution operators."""
    return _family("conv_train")


def encoder_operators():
    """Names of the registered torch.ops.rmd feature / context encoder operators."""
    return _family("encoder")


def mnet_operators():
    """Names of the registered torch.ops.rmd k x k matching-network operators."""
    return _family("mnet")


def _hip(name):
    """Register the HIP kernel of an operator (CUDA dispatch key); its CPU kernel lives in rmd/cpu.py.
    The dispatcher picks this kernel when any one tensor argument is on a GPU, and the launch hands raw
    pointers to one device's stream: so every tensor argument — members of Tensor[] and non-None
    Tensor? arguments too — must be a GPU tensor, and all of them on the same device."""
    def deco(fn):
        def kernel(*args):
            dev = None
            for a in args:
                for t in a if isinstance(a, (list, tuple)) else (a,):
                    if not isinstance(t, torch.Tensor):
                        continue
                    if t.device.type != "cuda":
                        raise ValueError(f"rmd::{name}: all tensors must be on the GPU, got one on {t.device}")
                    if dev is None:
                        dev = t.device
                    elif t.device != dev:
                        raise ValueError(f"{name}: tensors on different devices ({dev} / {t.device})")
            return fn(*args)
        LIB.impl(name, kernel, "CUDA")
        return fn
    return deco


def _fake(name):
    return torch.library.register_fake(f"rmd::{name}")


def _f32(t):
    """fp32, contiguous, detached (no aten.to call for fp32 inputs: an operator below autograd must
    not hand back its own input)."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t.contiguous()


def _like(t, shape=None):
    """Uninitialised fp32 output on t's device, shaped `shape` or like t.  t.new_empty serves real and
    fake tensors alike, so a HIP kernel and its fake kernel allocate from the one statement of a shape."""
    return t.new_empty(t.shape if shape is None else shape, dtype=torch.float32)


_DESC = {}


def describe(batch, height, width, levels, storage, layout=_lib.RMD_LAYOUT_ROWS):
    """rmd_pyramid_describe_layout, cached per geometry (host-only)."""
    key = (batch, height, width, levels, storage, layout)
    d = _DESC.get(key)
    if d is None:
        d = _DESC[key] = _lib.describe(batch, height, width, levels, storage, layout)
    return d


def describe_for(batch, height, width, levels, storage, channels, compute):
    """rmd_pyramid_describe_for: the layout the GEMM of (channels, compute) writes, cached."""
    key = ("for", batch, height, width, levels, storage, channels, compute)
    d = _DESC.get(key)
    if d is None:
        d = _DESC[key] = _lib.describe_for(batch, height, width, levels, storage, channels, compute)
    return d


_STORAGE = {_lib.RMD_F32: torch.float32, _lib.RMD_F16: torch.float16, _lib.RMD_S24: torch.uint8}
_STORAGE_CODE = {torch.float32: _lib.RMD_F32, torch.float16: _lib.RMD_F16, torch.uint8: _lib.RMD_S24}

# The pyramid tensor carries its layout and storage in its shape and dtype, so corr_lookup never
# trusts a caller's word for them: RMD_LAYOUT_ROWS pyramids are 1-D (total_elements,) float32/float16,
# RMD_LAYOUT_TILES pyramids 2-D (total_elements / 8, 8) float16 — one row per 2 x 4 chunk (every tiles
# level holds a multiple of 64 elements) — and RMD_S24 pyramids (row layout) uint8 (total_elements, 3).
TILES_ROW = 8
S24_BYTES = 3


def pyramid_view(data, layout):
    """The flat pyramid allocation shaped for its layout (see TILES_ROW)."""
    return data.view(-1, TILES_ROW) if layout == _lib.RMD_LAYOUT_TILES else data


def pyramid_layout(pyramid):
    """Layout of a pyramid tensor from its shape; ValueError for any other shape."""
    if pyramid.dtype == torch.uint8:
        if pyramid.dim() == 2 and pyramid.shape[1] == S24_BYTES:
            return _lib.RMD_LAYOUT_ROWS
    elif pyramid.dim() == 1:
        return _lib.RMD_LAYOUT_ROWS
    elif pyramid.dim() == 2 and pyramid.shape[1] == TILES_ROW:
        return _lib.RMD_LAYOUT_TILES
    raise ValueError(f"corr_lookup: a pyramid is 1-D (row layout), (n, {TILES_ROW}) (tiles layout) or uint8 "
                     f"(n, {S24_BYTES}) (S24 storage), got {pyramid.dtype} {tuple(pyramid.shape)}")


def pyramid_storage(pyramid):
    """RMD_F32 / RMD_F16 / RMD_S24 of a pyramid tensor (its dtype)."""
    if pyramid.dtype not in _STORAGE_CODE:
        raise ValueError(f"corr_lookup: pyramid dtype must be float32, float16 or uint8 (S24), got {pyramid.dtype}")
    return _STORAGE_CODE[pyramid.dtype]


def pyramid_elements(pyramid):
    """Pyramid elements held by a pyramid tensor (S24: 3 bytes each)."""
    return pyramid.shape[0] if pyramid.dtype == torch.uint8 else pyramid.numel()


def new_pyramid(like, d):
    """Uninitialised pyramid tensor for desc d on like's device (like.new_empty: fake tensors too)."""
    if d.storage == _lib.RMD_S24:
        return like.new_empty((d.total_elements, S24_BYTES), dtype=torch.uint8)
    return pyramid_view(like.new_empty((d.total_elements,), dtype=_STORAGE[d.storage]), d.layout)


def pyramid_buffers(f1, levels, compute, storage):
    """What a pyramid GEMM over fmaps shaped like f1 (B, C, H, W) writes into: (desc, uninitialised
    pyramid, workspace) — d.storage is the GEMM's own (S24 falls back to F32 off the x3 GEMM)."""
    b, c, h, w = f1.shape
    d = describe_for(b, h, w, levels, storage, c, compute)
    ws = _lib.workspace("corr_pyramid", f1, ctypes.byref(d), c, compute)
    return d, new_pyramid(f1, d), ws


def s24_encode(x):
    """float tensor -> RMD_S24 bytes (n, 3): the top 24 bits of each fp32 word, rounded half away from
    zero on the magnitude; NaN stays a quiet NaN (include/rmd.h RMD_S24, the x3 GEMM's epilogue)."""
    u = _f32(x).reshape(-1).view(torch.int32)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = torch.where(nan, u | 0x00400000, u + 0x80)
    return r.view(torch.uint8).view(-1, 4)[:, 1:4].contiguous()


def s24_decode(b):
    """RMD_S24 bytes (n, 3) -> float32 (n,) (low mantissa byte zero)."""
    w = torch.zeros((b.shape[0], 4), dtype=torch.uint8, device=b.device)
    w[:, 1:4] = b
    return w.view(torch.float32).reshape(-1)


# ---- RAFT correlation pyramid + lookup (inference operators) -----------------------------------

def _check_fmaps(f1, f2):
    if f1.shape != f2.shape or f1.dim() != 4:
        raise ValueError(f"fmap1/fmap2 must be equal (B,C,H,W) shapes, got {tuple(f1.shape)} / {tuple(f2.shape)}")


@_hip("corr_pyramid")
def _corr_pyramid(fmap1, fmap2, levels, compute, storage, scale):
    _check_fmaps(fmap1, fmap2)
    f1, f2 = _f32(fmap1), _f32(fmap2)
    d, data, ws = pyramid_buffers(f1, levels, compute, storage)
    _lib.launch("rmd_corr_pyramid_fused", f1, f1, f2, f1.shape[1], float(scale), ctypes.byref(d), compute, data, ws)
    return data


@_fake("corr_pyramid")
def _(fmap1, fmap2, levels, compute, storage, scale):
    _check_fmaps(fmap1, fmap2)
    b, c, h, w = fmap1.shape
    if fmap1.device.type == "cpu":                  # rmd/cpu.py writes the row layout, S24 as F32
        d = describe(b, h, w, levels, _lib.RMD_F32 if storage == _lib.RMD_S24 else storage)
    else:
        d = describe_for(b, h, w, levels, storage, c, compute)
    return new_pyramid(fmap1, d)


def _lookup_out(coords, levels, radius):
    b, _, h, w = coords.shape
    return _like(coords, (b, levels * (2 * radius + 1) ** 2, h, w))


@_hip("corr_lookup")
def _corr_lookup(pyramid, coords, levels, radius, level_mask):
    b, two, h, w = coords.shape
    if pyramid.dtype not in _STORAGE_CODE or not pyramid.is_contiguous():
        raise ValueError(f"corr_lookup: pyramid must be a contiguous float32/float16/uint8 (S24) tensor, got "
                         f"{pyramid.dtype} {tuple(pyramid.shape)}")
    d = describe(b, h, w, levels, pyramid_storage(pyramid), pyramid_layout(pyramid))
    if two != 2 or pyramid_elements(pyramid) != d.total_elements:
        raise ValueError(f"corr_lookup: coords {tuple(coords.shape)} do not match the pyramid ({pyramid.numel()} elements)")
    co = _f32(coords)
    out = _lookup_out(co, levels, radius)
    _lib.launch("rmd_corr_lookup", co, pyramid, ctypes.byref(d), co, radius, level_mask, out)
    return out


@_fake("corr_lookup")
def _(pyramid, coords, levels, radius, level_mask):
    pyramid_layout(pyramid)
    return _lookup_out(coords, levels, radius)


@_hip("corr_otf_prepare")
def _corr_otf_prepare(fmap1, fmap2, levels, compute, scale):
    _check_fmaps(fmap1, fmap2)
    f1, f2 = _f32(fmap1), _f32(fmap2)
    b, c, h, w = f1.shape
    ws = _lib.workspace("corr_otf", f1, b, c, h, w, levels, compute)
    if ws.numel() == 0:
        raise ValueError(f"otf: unsupported sizes {tuple(f1.shape)} with {levels} levels")
    _lib.launch("rmd_corr_otf_prepare", f1, f1, f2, b, c, h, w, levels, float(scale), compute, ws)
    return ws


@_fake("corr_otf_prepare")
def _(fmap1, fmap2, levels, compute, scale):
    b, c, h, w = fmap1.shape
    if fmap1.device.type == "cpu":                  # rmd/cpu.py: fmap1 * scale + pooled levels, float32
        n = b * c * (h * w + sum((h >> i) * (w >> i) for i in range(levels)))
        return fmap1.new_empty((n,), dtype=torch.float32)
    return _lib.workspace("corr_otf", fmap1, b, c, h, w, levels, compute)


@_hip("corr_otf_lookup")
def _corr_otf_lookup(workspace, coords, channels, levels, compute, radius, level_mask):
    b, two, h, w = coords.shape
    # the workspace must be the one corr_otf_prepare built for these sizes and this compute mode: its
    # segment layout depends on all of them, and the kernel trusts it
    want = _lib.lib().rmd_corr_otf_workspace_bytes(b, channels, h, w, levels, compute)
    if (two != 2 or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
            or want == 0 or workspace.numel() != want):
        raise ValueError(f"corr_otf_lookup: workspace ({workspace.dtype}, {workspace.numel()} B) does not match "
                         f"coords {tuple(coords.shape)}, channels={channels}, levels={levels}, compute={compute} "
                         f"({want} B expected)")
    co = _f32(coords)
    out = _lookup_out(co, levels, radius)
    _lib.launch("rmd_corr_otf_lookup", co, workspace, b, channels, h, w, levels, compute, co, radius, level_mask, out)
    return out


@_fake("corr_otf_lookup")
def _(workspace, coords, channels, levels, compute, radius, level_mask):
    return _lookup_out(coords, levels, radius)


# ---- DICL displacement stacks -------------------------------------------------------------------

def _stack_out(f1, radius, extra):
    b, c, h, w = f1.shape
    d = 2 * radius + 1
    return _like(f1, (b, d, d, 2 * c + (2 if extra else 0), h, w))


@_hip("dicl_stack")
def _dicl_stack(fmap1, fmap2, coords, radius, level, norm_h, norm_w, extra_delta):
    f1, f2, co = _f32(fmap1), _f32(fmap2), _f32(coords)
    b, c, h, w = f1.shape
    hl, wl = f2.shape[-2:]
    if f2.shape[:2] != (b, c) or tuple(co.shape) != (b, 2, h, w):
        raise ValueError("dicl_stack: fmap2 must be (B,C,hl,wl) and coords (B,2,h,w) matching fmap1")
    out = _stack_out(f1, radius, extra_delta)
    _lib.launch("rmd_dicl_stack", f1, f1, f2, co, b, c, h, w, hl, wl, radius, level, norm_h, norm_w,
                int(extra_delta), out)
    return out


@_fake("dicl_stack")
def _(fmap1, fmap2, coords, radius, level, norm_h, norm_w, extra_delta):
    return _stack_out(fmap1, radius, extra_delta)


def _stack_grads(coords, channels, level_h, level_w):
    b, _, h, w = coords.shape
    return _like(coords, (b, channels, h, w)), _like(coords, (b, channels, level_h, level_w))


@_hip("dicl_stack_backward")
def _dicl_stack_backward(grad, coords, channels, level_h, level_w, radius, level, norm_h, norm_w, extra_delta):
    g, co = _f32(grad), _f32(coords)
    b, _, h, w = co.shape
    g1, g2 = _stack_grads(co, channels, level_h, level_w)
    _lib.launch("rmd_dicl_stack_backward", g, g, co, b, channels, h, w, level_h, level_w, radius, level, norm_h,
                norm_w, int(extra_delta), g1, g2)
    return g1, g2


@_fake("dicl_stack_backward")
def _(grad, coords, channels, level_h, level_w, radius, level, norm_h, norm_w, extra_delta):
    return _stack_grads(coords, channels, level_h, level_w)


def _dicl_stack_setup(ctx, inputs, output):
    fmap1, fmap2, coords, radius, level, norm_h, norm_w, extra = inputs
    ctx.save_for_backward(coords)
    ctx.meta = (fmap1.shape[1], fmap2.shape[-2], fmap2.shape[-1], radius, level, norm_h, norm_w, extra)


def _dicl_stack_bwd(ctx, grad):
    (coords,) = ctx.saved_tensors
    c, hl, wl, radius, level, nh, nw, extra = ctx.meta
    g1, g2 = torch.ops.rmd.dicl_stack_backward(grad, coords, c, hl, wl, radius, level, nh, nw, extra)
    return g1, g2, None, None, None, None, None, None


torch.library.register_autograd("rmd::dicl_stack", _dicl_stack_bwd, setup_context=_dicl_stack_setup)


def _int_out(f1, ru, rv):
    b, c, h, w = f1.shape
    return _like(f1, (b, 2 * ru + 1, 2 * rv + 1, 2 * c, h, w))


@_hip("dicl_stack_int")
def _dicl_stack_int(fmap1, fmap2, ru, rv):
    f1, f2 = _f32(fmap1), _f32(fmap2)
    b, c, h, w = f1.shape
    if tuple(f2.shape) != (b, c, h, w):
        raise ValueError("dicl_stack_int: fmap1 and fmap2 must have equal (B,C,h,w) shapes")
    ws = _lib.workspace("dicl_stack_int", f1, b, h, w)
    out = _int_out(f1, ru, rv)
    _lib.launch("rmd_dicl_stack_int", f1, f1, f2, b, c, h, w, ru, rv, out, ws)
    return out


@_fake("dicl_stack_int")
def _(fmap1, fmap2, ru, rv):
    return _int_out(fmap1, ru, rv)


@_hip("dicl_stack_int_backward")
def _dicl_stack_int_backward(grad, fmap2, ru, rv):
    g, f2 = _f32(grad), _f32(fmap2)
    b, c, h, w = f2.shape
    ws = _lib.workspace("dicl_stack_int", g, b, h, w)
    g1, g2 = _like(f2), _like(f2)
    _lib.launch("rmd_dicl_stack_int_backward", g, g, f2, b, c, h, w, ru, rv, g1, g2, ws)
    return g1, g2


@_fake("dicl_stack_int_backward")
def _(grad, fmap2, ru, rv):
    return _like(fmap2), _like(fmap2)


def _int_setup(ctx, inputs, output):
    _, fmap2, ru, rv = inputs
    ctx.save_for_backward(_f32(fmap2))
    ctx.meta = (ru, rv)


def _int_bwd(ctx, grad):
    (f2,) = ctx.saved_tensors
    g1, g2 = torch.ops.rmd.dicl_stack_int_backward(grad, f2, *ctx.meta)
    return g1, g2, None, None


torch.library.register_autograd("rmd::dicl_stack_int", _int_bwd, setup_context=_int_setup)


@_hip("dicl_stack_int_warped")
def _dicl_stack_int_warped(fmap1, fmap2, flow, ru, rv):
    f1, f2, fl = _f32(fmap1), _f32(fmap2), _f32(flow)
    b, c, h, w = f1.shape
    if tuple(f2.shape) != (b, c, h, w) or tuple(fl.shape) != (b, 2, h, w):
        raise ValueError("dicl_stack_int_warped: need fmap1, fmap2 (B,C,h,w) and flow (B,2,h,w)")
    ws = _lib.workspace("dicl_stack_int_warped", f1, b, c, h, w)
    out = _int_out(f1, ru, rv)
    _lib.launch("rmd_dicl_stack_int_warped", f1, f1, f2, fl, b, c, h, w, ru, rv, out, ws)
    return out


@_fake("dicl_stack_int_warped")
def _(fmap1, fmap2, flow, ru, rv):
    return _int_out(fmap1, ru, rv)


@_hip("dicl_stack_int_warped_backward")
def _dicl_stack_int_warped_backward(grad, fmap2, flow, ru, rv):
    g, f2, fl = _f32(grad), _f32(fmap2), _f32(flow)
    b, c, h, w = f2.shape
    ws = _lib.workspace("dicl_stack_int_warped", g, b, c, h, w)
    g1, g2 = _like(f2), _like(f2)
    _lib.launch("rmd_dicl_stack_int_warped_backward", g, g, f2, fl, b, c, h, w, ru, rv, g1, g2, ws)
    return g1, g2


@_fake("dicl_stack_int_warped_backward")
def _(grad, fmap2, flow, ru, rv):
    return _like(fmap2), _like(fmap2)


def _warped_setup(ctx, inputs, output):
    _, fmap2, flow, ru, rv = inputs
    ctx.save_for_backward(_f32(fmap2), _f32(flow))
    ctx.meta = (ru, rv)


def _warped_bwd(ctx, grad):
    f2, fl = ctx.saved_tensors
    g1, g2 = torch.ops.rmd.dicl_stack_int_warped_backward(grad, f2, fl, *ctx.meta)
    return g1, g2, None, None, None


torch.library.register_autograd("rmd::dicl_stack_int_warped", _warped_bwd, setup_context=_warped_setup)


# ---- displacement-aware projection ---------------------------------------------------------------

def _dap_launch(x, weight, transpose):
    b, dd = x.shape[0], weight.shape[0]
    if x.numel() % (b * dd) or weight.numel() != dd * dd:
        raise ValueError(f"dap: x {tuple(x.shape)} does not hold {dd} displacement channels per batch")
    xc = _f32(x)
    wc = _f32(weight).reshape(dd, dd)
    out = _like(xc)
    _lib.launch("rmd_dap", xc, xc, wc, b, dd, xc.numel() // (b * dd), transpose, out)
    return out


@_hip("dap")
def _dap(x, weight):
    return _dap_launch(x, weight, 0)


@_fake("dap")
def _(x, weight):
    return _like(x)


@_hip("dap_transpose")
def _dap_transpose(grad, weight):
    return _dap_launch(grad, weight, 1)


@_fake("dap_transpose")
def _(grad, weight):
    return _like(grad)


@_hip("dap_weight_grad")
def _dap_weight_grad(grad, x, disp):
    """dW = sum_b g_b x_b^T (rmd_dap_weight_grad: split-bf16 MFMA, deterministic split-K)."""
    b = x.shape[0]
    if grad.shape != x.shape or x.numel() % (b * disp):
        raise ValueError(f"dap_weight_grad: grad {tuple(grad.shape)} / x {tuple(x.shape)} with {disp} displacements")
    gc, xc = _f32(grad), _f32(x)
    n = xc.numel() // (b * disp)
    ws = _lib.workspace("dap_weight_grad", xc, b, disp, n)
    out = _like(xc, (disp, disp))
    _lib.launch("rmd_dap_weight_grad", xc, gc, xc, b, disp, n, out, ws)
    return out


@_fake("dap_weight_grad")
def _(grad, x, disp):
    return _like(x, (disp, disp))


def _dap_setup(ctx, inputs, output):
    x, weight = inputs
    ctx.save_for_backward(x, weight)


def _dap_bwd(ctx, grad):
    x, weight = ctx.saved_tensors
    b, dd = x.shape[0], weight.shape[0]
    gx = torch.ops.rmd.dap_transpose(grad, weight) if ctx.needs_input_grad[0] else None
    gw = None
    if ctx.needs_input_grad[1]:
        gw = torch.ops.rmd.dap_weight_grad(grad, x, dd).reshape(weight.shape).to(weight.dtype)
    return gx, gw


torch.library.register_autograd("rmd::dap", _dap_bwd, setup_context=_dap_setup)


# ---- flow heads ----------------------------------------------------------------------------------

def _up8_out(flow):
    b, _, h, w = flow.shape
    return _like(flow, (b, 2, 8 * h, 8 * w))


@_hip("up8")
def _up8(mask, flow, temperature):
    b, c, h, w = flow.shape
    if c != 2 or tuple(mask.shape) != (b, 576, h, w):
        raise ValueError(f"up8: need flow (B,2,h,w) and mask (B,576,h,w), got {tuple(flow.shape)}, {tuple(mask.shape)}")
    mc, fc = _f32(mask), _f32(flow)
    out = _up8_out(fc)
    _lib.launch("rmd_up8", fc, mc, fc, b, h, w, float(temperature), out)
    return out


@_fake("up8")
def _(mask, flow, temperature):
    return _up8_out(flow)


@_hip("up8_backward")
def _up8_backward(grad, mask, flow, temperature):
    g, mc, fc = _f32(grad), _f32(mask), _f32(flow)
    b, _, h, w = fc.shape
    ws = _lib.workspace("up8", g, b, h, w)
    gm, gf = _like(mc), _like(fc)
    _lib.launch("rmd_up8_backward", g, mc, fc, g, b, h, w, float(temperature), gm, gf, ws)
    return gm, gf


@_fake("up8_backward")
def _(grad, mask, flow, temperature):
    return _like(mask), _like(flow)


def _up8_setup(ctx, inputs, output):
    mask, flow, temperature = inputs
    ctx.save_for_backward(mask, flow)
    ctx.temperature = temperature


def _up8_bwd(ctx, grad):
    mask, flow = ctx.saved_tensors
    gm, gf = torch.ops.rmd.up8_backward(grad, mask, flow, ctx.temperature)
    return gm.to(mask.dtype), gf.to(flow.dtype), None


torch.library.register_autograd("rmd::up8", _up8_bwd, setup_context=_up8_setup)


def _sam_out(cost, levels):
    return _like(cost, (levels, cost.shape[0], 2) + tuple(cost.shape[2:]))


@_hip("softargmax")
def _softargmax(cost, levels, radius, temperature):
    b, ctot = cost.shape[:2]
    n = cost[0, 0].numel()
    if ctot < levels * (2 * radius + 1) ** 2:
        raise ValueError(f"softargmax: {ctot} channels < {levels} levels x {(2 * radius + 1) ** 2} displacements")
    cc = _f32(cost)
    flows = _sam_out(cc, levels)
    _lib.launch("rmd_softargmax", cc, cc, b, ctot, n, levels, radius, float(temperature), flows)
    return flows


@_fake("softargmax")
def _(cost, levels, radius, temperature):
    return _sam_out(cost, levels)


@_hip("softargmax_backward")
def _softargmax_backward(grad, cost, levels, radius, temperature):
    cc, g = _f32(cost), _f32(grad)
    b, ctot = cc.shape[:2]
    n = cc[0, 0].numel()
    gc = torch.zeros_like(cc) if ctot > levels * (2 * radius + 1) ** 2 else torch.empty_like(cc)
    _lib.launch("rmd_softargmax_backward", g, cc, g, b, ctot, n, levels, radius, float(temperature), gc)
    return gc


@_fake("softargmax_backward")
def _(grad, cost, levels, radius, temperature):
    return _like(cost)


def _sam_setup(ctx, inputs, output):
    cost, levels, radius, temperature = inputs
    ctx.save_for_backward(cost)
    ctx.meta = (levels, radius, temperature)


def _sam_bwd(ctx, grad):
    (cost,) = ctx.saved_tensors
    gc = torch.ops.rmd.softargmax_backward(grad, cost, *ctx.meta)
    return gc.to(cost.dtype), None, None, None


torch.library.register_autograd("rmd::softargmax", _sam_bwd, setup_context=_sam_setup)


# ---- backward warp -------------------------------------------------------------------------------

@_hip("warp_backwards")
def _warp_backwards(img2, flow, eps):
    b, c, h, w = img2.shape
    if tuple(flow.shape) != (b, 2, h, w):
        raise ValueError(f"warp_backwards: flow {tuple(flow.shape)} must be (B, 2, h, w) for img2 {tuple(img2.shape)}")
    ic, fc = _f32(img2), _f32(flow)
    out = _like(ic)
    mask = ic.new_empty((b, 1, h, w), dtype=torch.uint8)        # the kernel writes bytes; the fake says bool
    _lib.launch("rmd_warp_backwards", ic, ic, fc, b, c, h, w, float(eps), out, mask)
    return out, mask.bool()


@_fake("warp_backwards")
def _(img2, flow, eps):
    b, c, h, w = img2.shape
    return _like(img2), img2.new_empty((b, 1, h, w), dtype=torch.bool)


@_hip("warp_backwards_backward")
def _warp_backwards_backward(grad, flow, eps):
    g, fc = _f32(grad), _f32(flow)
    b, c, h, w = g.shape
    gi = _like(g)
    _lib.launch("rmd_warp_backwards_backward", g, g, fc, b, c, h, w, float(eps), gi)
    return gi


@_fake("warp_backwards_backward")
def _(grad, flow, eps):
    return _like(grad)


def _warp_setup(ctx, inputs, output):
    img2, flow, eps = inputs
    ctx.save_for_backward(flow)
    ctx.eps = eps
    ctx.dtype = img2.dtype
    ctx.mark_non_differentiable(output[1])


def _warp_bwd(ctx, grad, _gmask):
    (flow,) = ctx.saved_tensors
    return torch.ops.rmd.warp_backwards_backward(grad, flow, ctx.eps).to(ctx.dtype), None, None


torch.library.register_autograd("rmd::warp_backwards", _warp_bwd, setup_context=_warp_setup)


# ---- sequence losses -----------------------------------------------------------------------------
#
# The loss operators take tensor lists (one entry per prediction).  `masks` holds the distinct
# per-prediction masks and mask_index[k] the entry prediction k uses (-1: the shared `valid`).  The
# list-valued autograd formula lives in rmd.ops (_SequenceLossFn).

LOSS_NORMS = (_lib.RMD_LOSS_L1, _lib.RMD_LOSS_L2, _lib.RMD_LOSS_ABSMEAN, _lib.RMD_LOSS_ROBUST)


def _u8(t):
    """A (B, H, W) mask as contiguous bytes (bool is reinterpreted, not copied)."""
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise ValueError(f"sequence_loss: masks must be bool or uint8, got {t.dtype}")
    return t


def check_loss_args(flows, target, valid, masks, mask_index, weights, norm):
    """Shape and argument checks shared by the GPU, CPU and fake kernels of the loss operators."""
    if target.dim() != 4 or target.shape[1] != 2:
        raise ValueError(f"sequence_loss: target must be (B, 2, H, W), got {tuple(target.shape)}")
    b, _, h, w = target.shape
    if tuple(valid.shape) != (b, h, w):
        raise ValueError(f"sequence_loss: valid must be (B, H, W) = ({b}, {h}, {w}), got {tuple(valid.shape)}")
    if not flows or len(weights) != len(flows) or len(mask_index) != len(flows):
        raise ValueError(f"sequence_loss: {len(flows)} flows, {len(weights)} weights, {len(mask_index)} mask indices")
    if norm not in LOSS_NORMS:
        raise ValueError(f"sequence_loss: norm {norm} (supported: RMD_LOSS_L1 = 1, RMD_LOSS_L2 = 2, "
                         f"RMD_LOSS_ABSMEAN = 3, RMD_LOSS_ROBUST = 4)")
    for f in flows:
        if f.dim() != 4 or f.shape[0] != b or f.shape[1] != 2 or f.shape[2] < 1 or f.shape[3] < 1:
            raise ValueError(f"sequence_loss: a prediction must be ({b}, 2, h, w), got {tuple(f.shape)}")
    for m in masks:
        if tuple(m.shape) != (b, h, w):
            raise ValueError(f"sequence_loss: a mask must be ({b}, {h}, {w}), got {tuple(m.shape)}")
    for i in mask_index:
        if not -1 <= i < len(masks):
            raise ValueError(f"sequence_loss: mask index {i} with {len(masks)} masks")


def _loss_table(flows, masks, mask_index, weights, grads=None):
    table = (_lib.LossPrediction * len(flows))()
    for k, f in enumerate(flows):
        e = table[k]
        e.flow = f.data_ptr()
        e.mask = masks[mask_index[k]].data_ptr() if mask_index[k] >= 0 else None
        e.grad = grads[k].data_ptr() if grads is not None and grads[k].numel() else None
        e.height, e.width = f.shape[2], f.shape[3]
        e.weight = float(weights[k])
    return table


def _loss_out(target, n):
    return target.new_empty((), dtype=torch.float32), target.new_empty((n,), dtype=torch.int64)


@_hip("sequence_loss")
def _sequence_loss(flows, target, valid, masks, mask_index, weights, norm, include_invalid, skip_empty, scale):
    check_loss_args(flows, target, valid, masks, mask_index, weights, norm)
    fl, tg, va, ms = [_f32(f) for f in flows], _f32(target), _u8(valid), [_u8(m) for m in masks]
    b, _, h, w = tg.shape
    n = len(fl)
    ws = _lib.workspace("sequence_loss", tg, b, h, w, min(n, _lib.LOSS_MAX_PREDICTIONS))
    loss, counts = _loss_out(tg, n)
    _lib.launch("rmd_sequence_loss", tg, _loss_table(fl, ms, mask_index, weights), n, tg, va, b, h, w, norm,
                int(include_invalid), int(skip_empty), float(scale), loss, counts, ws)
    return loss, counts


@_fake("sequence_loss")
def _(flows, target, valid, masks, mask_index, weights, norm, include_invalid, skip_empty, scale):
    check_loss_args(flows, target, valid, masks, mask_index, weights, norm)
    return _loss_out(target, len(flows))


def _loss_grads(flows, needs_grad):
    """One gradient per prediction; a prediction that needs none gets an empty tensor (and the kernel a
    null pointer for it, _loss_table)."""
    return [_like(f, f.shape if need else (0,)) for f, need in zip(flows, needs_grad)]


@_hip("sequence_loss_backward")
def _sequence_loss_backward(grad_loss, flows, target, valid, masks, mask_index, weights, counts, needs_grad, norm,
                            include_invalid, scale):
    check_loss_args(flows, target, valid, masks, mask_index, weights, norm)
    if len(needs_grad) != len(flows) or counts.dtype != torch.int64 or counts.numel() != len(flows):
        raise ValueError("sequence_loss_backward: needs_grad and counts (int64) must have one entry per prediction")
    fl, tg, va, ms = [_f32(f) for f in flows], _f32(target), _u8(valid), [_u8(m) for m in masks]
    g, cn = _f32(grad_loss).reshape(()), counts.contiguous()
    b, _, h, w = tg.shape
    grads = _loss_grads(fl, needs_grad)
    if any(needs_grad):
        _lib.launch("rmd_sequence_loss_backward", tg, _loss_table(fl, ms, mask_index, weights, grads), len(fl), tg, va,
                    b, h, w, norm, int(include_invalid), float(scale), g, cn)
    return grads


@_fake("sequence_loss_backward")
def _(grad_loss, flows, target, valid, masks, mask_index, weights, counts, needs_grad, norm, include_invalid, scale):
    return _loss_grads(flows, needs_grad)


# ---- flow metrics --------------------------------------------------------------------------------
#
# The operator returns the raw statistics of include/rmd.h (estimates, samples, RMD_METRICS_SLOTS)
# float64; rmd.ops.flow_metrics derives the metrics from them.  It is not differentiable: its Autograd
# kernel runs the backend kernel below autograd, so the result never carries a graph.

def check_metric_args(estimates, target, valid, distances, mag_ord):
    """Shape and argument checks shared by the GPU, CPU and fake kernels of flow_metrics."""
    if target.dim() != 4 or target.shape[1] != 2:
        raise ValueError(f"flow_metrics: target must be (B, 2, H, W), got {tuple(target.shape)}")
    b, _, h, w = target.shape
    if tuple(valid.shape) != (b, h, w):
        raise ValueError(f"flow_metrics: valid must be (B, H, W) = ({b}, {h}, {w}), got {tuple(valid.shape)}")
    if not 1 <= len(estimates) <= _lib.METRICS_MAX_ESTIMATES:
        raise ValueError(f"flow_metrics: {len(estimates)} estimates (1..{_lib.METRICS_MAX_ESTIMATES} per call; "
                         f"rmd.ops.flow_metrics chunks longer lists)")
    if len(distances) > _lib.METRICS_MAX_DISTANCES:
        raise ValueError(f"flow_metrics: {len(distances)} distances (0..{_lib.METRICS_MAX_DISTANCES} per call; "
                         f"rmd.ops.flow_metrics chunks longer lists)")
    if not mag_ord > 0:
        raise ValueError(f"flow_metrics: bad mag_ord {mag_ord} (1, 2, inf or any other p > 0)")
    for e in estimates:
        if tuple(e.shape) != tuple(target.shape):
            raise ValueError(f"flow_metrics: an estimate must be {tuple(target.shape)}, got {tuple(e.shape)}")


def _metrics_out(estimates, target):
    return target.new_empty((len(estimates), target.shape[0], _lib.METRICS_SLOTS), dtype=torch.float64)


@_hip("flow_metrics")
def _flow_metrics(estimates, target, valid, distances, fl_abs, fl_rel, mag_ord):
    check_metric_args(estimates, target, valid, distances, mag_ord)
    es, tg, va = [_f32(e) for e in estimates], _f32(target), _u8(valid)
    b, _, h, w = tg.shape
    n, nd = len(es), len(distances)
    ws = _lib.workspace("flow_metrics", tg, b, h, w, n)
    stats = _metrics_out(es, tg)
    table = (ctypes.c_void_p * n)(*[e.data_ptr() for e in es])
    dist = (ctypes.c_float * max(nd, 1))(*[float(d) for d in distances])
    _lib.launch("rmd_flow_metrics", tg, table, n, tg, va, b, h, w, dist, nd, float(fl_abs), float(fl_rel),
                float(mag_ord), stats, ws)
    return stats


@_fake("flow_metrics")
def _(estimates, target, valid, distances, fl_abs, fl_rel, mag_ord):
    check_metric_args(estimates, target, valid, distances, mag_ord)
    return _metrics_out(estimates, target)


def _flow_metrics_below_autograd(estimates, target, valid, distances, fl_abs, fl_rel, mag_ord):
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.rmd.flow_metrics(estimates, target, valid, distances, fl_abs, fl_rel, mag_ord)


LIB.impl("flow_metrics", _flow_metrics_below_autograd, "Autograd")


# ---- DICL flow head ------------------------------------------------------------------------------
#
# One operator serves FlowRegression, FlowEntropy and the coarse-flow addition of a DICL level
# (impls/dicl.py:31-85, :195): out (B, 3, h, w) holds the flow in channels 0-1 and the normalised
# entropy in channel 2.  Its autograd formula recomputes the softmax from the cost
# (dicl_flow_head_backward); the gradient of flow_coarse is the first two channels of the upstream one.

HEAD_MAX_RANGE = 8


def check_head_args(cost, flow_coarse, eps, grad=None):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of the head operators."""
    if cost.dim() != 5:
        raise ValueError(f"dicl_flow_head: cost must be (B, du, dv, h, w), got {tuple(cost.shape)}")
    b, du, dv, h, w = cost.shape
    if du % 2 != 1 or dv % 2 != 1 or du > 2 * HEAD_MAX_RANGE + 1 or dv > 2 * HEAD_MAX_RANGE + 1:
        raise ValueError(f"dicl_flow_head: du = {du}, dv = {dv} must be odd (2r + 1) with ranges 0..{HEAD_MAX_RANGE}")
    if b < 1 or h < 1 or w < 1:
        raise ValueError(f"dicl_flow_head: empty cost {tuple(cost.shape)}")
    if not 0.0 <= eps < 0.5:
        raise ValueError(f"dicl_flow_head: eps {eps} not in [0, 0.5)")
    for name, t, ch in (("flow_coarse", flow_coarse, 2), ("grad", grad, 3)):
        if t is None:
            continue
        if tuple(t.shape) != (b, ch, h, w):
            raise ValueError(f"dicl_flow_head: {name} must be ({b}, {ch}, {h}, {w}), got {tuple(t.shape)}")
    for name, t in (("cost", cost), ("flow_coarse", flow_coarse), ("grad", grad)):
        if t is not None and not t.is_floating_point():
            raise ValueError(f"dicl_flow_head: {name} must be a floating-point tensor, got {t.dtype}")


def _head_out(cost):
    b, _, _, h, w = cost.shape
    return _like(cost, (b, 3, h, w))


@_hip("dicl_flow_head")
def _dicl_flow_head(cost, flow_coarse, eps):
    check_head_args(cost, flow_coarse, eps)
    cc = _f32(cost)
    fc = None if flow_coarse is None else _f32(flow_coarse)
    b, du, dv, h, w = cc.shape
    out = _head_out(cc)
    _lib.launch("rmd_dicl_flow_head", cc, cc, fc, b, du, dv, h * w, float(eps), out)
    return out


@_fake("dicl_flow_head")
def _(cost, flow_coarse, eps):
    check_head_args(cost, flow_coarse, eps)
    return _head_out(cost)


@_hip("dicl_flow_head_backward")
def _dicl_flow_head_backward(grad, cost, eps):
    check_head_args(cost, None, eps, grad)
    g, cc = _f32(grad), _f32(cost)
    b, du, dv, h, w = cc.shape
    gc = _like(cc)
    _lib.launch("rmd_dicl_flow_head_backward", cc, cc, g, b, du, dv, h * w, float(eps), gc)
    return gc


@_fake("dicl_flow_head_backward")
def _(grad, cost, eps):
    check_head_args(cost, None, eps, grad)
    return _like(cost)


def _head_setup(ctx, inputs, output):
    cost, flow_coarse, eps = inputs
    ctx.save_for_backward(cost)
    ctx.eps = eps
    ctx.coarse_dtype = None if flow_coarse is None else flow_coarse.dtype


def _head_bwd(ctx, grad):
    (cost,) = ctx.saved_tensors
    gc = gf = None
    if ctx.needs_input_grad[0]:
        gc = torch.ops.rmd.dicl_flow_head_backward(grad, cost, ctx.eps).to(cost.dtype)
    if ctx.coarse_dtype is not None and ctx.needs_input_grad[1]:
        gf = grad[:, :2].to(ctx.coarse_dtype)
    return gc, gf, None


torch.library.register_autograd("rmd::dicl_flow_head", _head_bwd, setup_context=_head_setup)


# ---- hidden-state upsampler: local cross-attention -----------------------------------------------
#
# local_cross_attn is the attention of HUpCrossAttn.forward (common/hsup.py:71-92) without the
# expanded K / V; its autograd formula is local_cross_attn_backward, which recomputes the softmax from
# q, k and v (nothing else is saved).

ATTN_WINDOWS = (1, 3, 5)
ATTN_MAX_FACTOR = 64


def check_attn_args(q, k, v, win_y, win_x, grad=None):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of the attention operators."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"local_cross_attn: q, k, v must be (B, c, h, w), got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    b, ck, h, w = q.shape
    _, cv, h2, w2 = v.shape
    if min(b, ck, h, w, cv, h2, w2) < 1:
        raise ValueError(f"local_cross_attn: empty tensor (q {tuple(q.shape)}, v {tuple(v.shape)})")
    if tuple(k.shape) != (b, ck, h2, w2) or v.shape[0] != b:
        raise ValueError(f"local_cross_attn: k must be ({b}, {ck}, {h2}, {w2}) for q {tuple(q.shape)} and "
                         f"v {tuple(v.shape)}, got {tuple(k.shape)}")
    if win_y not in ATTN_WINDOWS or win_x not in ATTN_WINDOWS:
        raise ValueError(f"local_cross_attn: window {win_y}x{win_x}: sizes must be in {ATTN_WINDOWS}")
    if h % h2 or w % w2:
        raise RuntimeError(f"local_cross_attn: the fine size of q {tuple(q.shape)} is not an integer multiple of the "
                           f"coarse size of k {tuple(k.shape)}")
    if h // h2 > ATTN_MAX_FACTOR or w // w2 > ATTN_MAX_FACTOR:
        raise ValueError(f"local_cross_attn: factors {h // h2}x{w // w2} above {ATTN_MAX_FACTOR} are not supported")
    if grad is not None and tuple(grad.shape) != (b, cv, h, w):
        raise ValueError(f"local_cross_attn: grad must be ({b}, {cv}, {h}, {w}), got {tuple(grad.shape)}")
    for name, t in (("q", q), ("k", k), ("v", v), ("grad", grad)):
        if t is not None and not t.is_floating_point():
            raise ValueError(f"local_cross_attn: {name} must be a floating-point tensor, got {t.dtype}")


def _attn_out(q, v):
    return _like(q, (q.shape[0], v.shape[1], q.shape[2], q.shape[3]))


@_hip("local_cross_attn")
def _local_cross_attn(q, k, v, win_y, win_x):
    check_attn_args(q, k, v, win_y, win_x)
    qc, kc, vc = _f32(q), _f32(k), _f32(v)
    b, ck, h, w = qc.shape
    _, cv, h2, w2 = vc.shape
    out = _attn_out(qc, vc)
    _lib.launch("rmd_local_cross_attn", qc, qc, kc, vc, b, ck, cv, h, w, h2, w2, win_y, win_x, out)
    return out


@_fake("local_cross_attn")
def _(q, k, v, win_y, win_x):
    check_attn_args(q, k, v, win_y, win_x)
    return _attn_out(q, v)


@_hip("local_cross_attn_backward")
def _local_cross_attn_backward(grad, q, k, v, win_y, win_x):
    check_attn_args(q, k, v, win_y, win_x, grad)
    g, qc, kc, vc = _f32(grad), _f32(q), _f32(k), _f32(v)
    b, ck, h, w = qc.shape
    _, cv, h2, w2 = vc.shape
    gq, gk, gv = _like(qc), _like(kc), _like(vc)
    ws = _lib.workspace("local_cross_attn", qc, b, h, w, win_y, win_x)
    _lib.launch("rmd_local_cross_attn_backward", qc, g, qc, kc, vc, b, ck, cv, h, w, h2, w2, win_y, win_x, gq, gk, gv,
                ws)
    return gq, gk, gv


@_fake("local_cross_attn_backward")
def _(grad, q, k, v, win_y, win_x):
    check_attn_args(q, k, v, win_y, win_x, grad)
    return _like(q), _like(k), _like(v)


def _attn_setup(ctx, inputs, output):
    q, k, v, ctx.win_y, ctx.win_x = inputs
    ctx.save_for_backward(q, k, v)


def _attn_bwd(ctx, grad):
    q, k, v = ctx.saved_tensors
    if not any(ctx.needs_input_grad[:3]):
        return None, None, None, None, None
    grads = torch.ops.rmd.local_cross_attn_backward(grad, q, k, v, ctx.win_y, ctx.win_x)
    return tuple(g.to(t.dtype) if need else None
                 for g, t, need in zip(grads, (q, k, v), ctx.needs_input_grad[:3])) + (None, None)


torch.library.register_autograd("rmd::local_cross_attn", _attn_bwd, setup_context=_attn_setup)


# ---- fused dicl-1x1 cost: gather + folded 1x1 MatchingNet ------------------------------------------
#
# weights = [W1' (c1, 2C), W2' (c2, c1), W3' (c3, c2), w4 (c3 elements)], biases = [t1, t2, t3, b4 (1)]:
# MatchingNet1x1 with its norm layers folded (rmd.blocks.dicl.MatchingNet1x1.folded()).  The HIP kernel
# wants hidden widths that are multiples of 32 (rmd.ops.dicl_match_1x1 zero-pads); the CPU kernel takes
# any.  Not differentiable: like flow_metrics, its Autograd kernel runs the backend kernel below autograd.

MATCH_COMPUTE = (_lib.RMD_BF16X3, _lib.RMD_BF16)


def check_match_args(fmap1, fmap2, coords, radius, weights, biases, compute):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of dicl_match_1x1;
    returns the hidden widths (c1, c2, c3)."""
    _check_fmaps(fmap1, fmap2)
    b, c, h, w = fmap1.shape
    if tuple(coords.shape) != (b, 2, h, w):
        raise ValueError(f"dicl_match_1x1: coords must be ({b}, 2, {h}, {w}), got {tuple(coords.shape)}")
    if min(b, c, h, w) < 1 or radius < 0:
        raise ValueError(f"dicl_match_1x1: empty fmap {tuple(fmap1.shape)} or negative radius {radius}")
    if len(weights) != 4 or len(biases) != 4:
        raise ValueError(f"dicl_match_1x1: need 4 weights and 4 biases, got {len(weights)} and {len(biases)}")
    if compute not in MATCH_COMPUTE:
        raise ValueError(f"dicl_match_1x1: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    cin = 2 * c
    for i in range(3):
        if weights[i].dim() != 2 or weights[i].shape[1] != cin:
            raise ValueError(f"dicl_match_1x1: weights[{i}] must be (c{i + 1}, {cin}), got {tuple(weights[i].shape)}")
        cin = weights[i].shape[0]
    widths = tuple(wt.shape[0] for wt in weights[:3])
    for i, want in enumerate(widths + (1,)):
        if biases[i].numel() != want:
            raise ValueError(f"dicl_match_1x1: biases[{i}] must hold {want} elements, got {tuple(biases[i].shape)}")
    if weights[3].numel() != cin:
        raise ValueError(f"dicl_match_1x1: weights[3] must hold {cin} elements, got {tuple(weights[3].shape)}")
    for t in (fmap1, fmap2, coords, *weights, *biases):
        if not t.is_floating_point():
            raise ValueError(f"dicl_match_1x1: tensors must be floating point, got {t.dtype}")
    return widths


def match_supported(channels, c1, c2, c3, radius):
    """rmd_dicl_match_1x1_supported: whether the HIP kernel serves these sizes (host only)."""
    return bool(_lib.lib().rmd_dicl_match_1x1_supported(channels, c1, c2, c3, radius))


def _match_out(fmap1, radius):
    b, _, h, w = fmap1.shape
    d = 2 * radius + 1
    return _like(fmap1, (b, d, d, h, w))


@_hip("dicl_match_1x1")
def _dicl_match_1x1(fmap1, fmap2, coords, radius, weights, biases, compute):
    c1, c2, c3 = check_match_args(fmap1, fmap2, coords, radius, weights, biases, compute)
    b, c, h, w = fmap1.shape
    if not match_supported(c, c1, c2, c3, radius):
        raise ValueError(f"dicl_match_1x1: unsupported on the GPU: channels {c} (a multiple of 16 up to 64), hidden "
                         f"widths {c1}, {c2}, {c3} (multiples of 32 up to 128), radius {radius} (1..4)")
    f1, f2, co = _f32(fmap1), _f32(fmap2), _f32(coords)
    ws, ts = [_f32(t) for t in weights], [_f32(t) for t in biases]
    work = _lib.workspace("dicl_match_1x1", f1, c, c1, c2, c3, compute)
    out = _match_out(f1, radius)
    _lib.launch("rmd_dicl_match_1x1", f1, f1, f2, co, b, c, h, w, radius, ws[0], ts[0], ws[1], ts[1], ws[2], ts[2],
                ws[3], ts[3], c1, c2, c3, compute, out, work)
    return out


@_fake("dicl_match_1x1")
def _(fmap1, fmap2, coords, radius, weights, biases, compute):
    check_match_args(fmap1, fmap2, coords, radius, weights, biases, compute)
    return _match_out(fmap1, radius)


def _dicl_match_1x1_below_autograd(fmap1, fmap2, coords, radius, weights, biases, compute):
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.rmd.dicl_match_1x1(fmap1, fmap2, coords, radius, weights, biases, compute)


LIB.impl("dicl_match_1x1", _dicl_match_1x1_below_autograd, "Autograd")


# ---- fused dicl-1x1 cost for training ---------------------------------------------------------------
#
# dicl_match_1x1_train is dicl_match_1x1 in its fp32 mode (the same HIP kernel, RMD_BF16X3: bitwise the same
# cost) with an autograd formula that saves only its inputs; dicl_match_1x1_backward recomputes the MLP per
# column (rmd_dicl_match_1x1_backward) and returns [grad_fmap1, grad_fmap2, gW1, gW2, gW3, gw4, gt1, gt2,
# gt3, gb4], an empty tensor for every member of a group that needs_grad = [fmap1, fmap2, parameters]
# switches off.  The one-product mode has no backward.  Coordinates carry no gradient.

def match_backward_supported(channels, c1, c2, c3, radius):
    """rmd_dicl_match_1x1_backward_supported: whether the HIP backward serves these sizes (host only)."""
    return bool(_lib.lib().rmd_dicl_match_1x1_backward_supported(channels, c1, c2, c3, radius))


def check_match_backward_args(grad, fmap1, fmap2, coords, radius, weights, biases, needs_grad):
    """check_match_args plus the gradient's shape and the three needs_grad flags; returns the widths."""
    widths = check_match_args(fmap1, fmap2, coords, radius, weights, biases, _lib.RMD_BF16X3)
    b, _, h, w = fmap1.shape
    d = 2 * radius + 1
    if tuple(grad.shape) != (b, d, d, h, w) or not grad.is_floating_point():
        raise ValueError(f"dicl_match_1x1_backward: grad must be a floating-point ({b}, {d}, {d}, {h}, {w}) tensor, "
                         f"got {grad.dtype} {tuple(grad.shape)}")
    if len(needs_grad) != 3:
        raise ValueError(f"dicl_match_1x1_backward: needs_grad is [fmap1, fmap2, parameters], got {len(needs_grad)} flags")
    return widths


def _match_grads(fmap1, weights, biases, needs_grad):
    """The ten gradients, shaped like what they belong to; (0,) for the members of a skipped group."""
    shapes = [fmap1.shape, fmap1.shape] + [t.shape for t in weights] + [t.shape for t in biases]
    needs = [needs_grad[0], needs_grad[1]] + [needs_grad[2]] * 8
    return [_like(fmap1, tuple(s) if need else (0,)) for s, need in zip(shapes, needs)]


def _match_unsupported(name, c, widths, radius):
    return ValueError(f"{name}: unsupported on the GPU: channels {c} (a multiple of 16 up to 64), hidden widths "
                      f"{widths[0]}, {widths[1]}, {widths[2]} (multiples of 32 up to 128), radius {radius} (1..4)")


@_hip("dicl_match_1x1_train")
def _dicl_match_1x1_train(fmap1, fmap2, coords, radius, weights, biases):
    return _dicl_match_1x1(fmap1, fmap2, coords, radius, weights, biases, _lib.RMD_BF16X3)


@_fake("dicl_match_1x1_train")
def _(fmap1, fmap2, coords, radius, weights, biases):
    check_match_args(fmap1, fmap2, coords, radius, weights, biases, _lib.RMD_BF16X3)
    return _match_out(fmap1, radius)


@_hip("dicl_match_1x1_backward")
def _dicl_match_1x1_backward(grad, fmap1, fmap2, coords, radius, weights, biases, needs_grad):
    widths = check_match_backward_args(grad, fmap1, fmap2, coords, radius, weights, biases, needs_grad)
    b, c, h, w = fmap1.shape
    if not match_backward_supported(c, *widths, radius):
        raise _match_unsupported("dicl_match_1x1_backward", c, widths, radius)
    g, f1, f2, co = _f32(grad), _f32(fmap1), _f32(fmap2), _f32(coords)
    ws, ts = [_f32(t) for t in weights], [_f32(t) for t in biases]
    grads = _match_grads(f1, ws, ts, needs_grad)
    if any(needs_grad):
        work = _lib.workspace("dicl_match_1x1_backward", f1, b, c, h, w, radius, *widths)
        gf1, gf2, gw1, gw2, gw3, gw4, gt1, gt2, gt3, gb4 = [t if t.numel() else None for t in grads]
        _lib.launch("rmd_dicl_match_1x1_backward", f1, g, f1, f2, co, b, c, h, w, radius, ws[0], ts[0], ws[1], ts[1],
                    ws[2], ts[2], ws[3], *widths, _lib.RMD_BF16X3, gf1, gf2, gw1, gt1, gw2, gt2, gw3, gt3, gw4, gb4,
                    work)
    return grads


@_fake("dicl_match_1x1_backward")
def _(grad, fmap1, fmap2, coords, radius, weights, biases, needs_grad):
    check_match_backward_args(grad, fmap1, fmap2, coords, radius, weights, biases, needs_grad)
    return _match_grads(fmap1, weights, biases, needs_grad)


def _match_train_setup(ctx, inputs, output):
    fmap1, fmap2, coords, radius, weights, biases = inputs
    ctx.save_for_backward(fmap1, fmap2, coords, *weights, *biases)
    ctx.radius = radius
    ctx.param_needs = [t.requires_grad for t in (*weights, *biases)]
    ctx.needs = [fmap1.requires_grad, fmap2.requires_grad, any(ctx.param_needs)]


def _match_train_bwd(ctx, grad):
    fmap1, fmap2, coords = ctx.saved_tensors[:3]
    weights, biases = list(ctx.saved_tensors[3:7]), list(ctx.saved_tensors[7:11])
    if not any(ctx.needs):
        return None, None, None, None, [None] * 4, [None] * 4
    grads = torch.ops.rmd.dicl_match_1x1_backward(grad, fmap1, fmap2, coords, ctx.radius, weights, biases, ctx.needs)
    like = [fmap1, fmap2] + weights + biases
    needs = ctx.needs[:2] + ctx.param_needs
    out = [g.to(t.dtype) if need else None for g, t, need in zip(grads, like, needs)]
    return out[0], out[1], None, None, out[2:6], out[6:10]


torch.library.register_autograd("rmd::dicl_match_1x1_train", _match_train_bwd, setup_context=_match_train_setup)


# ---- fused SepConvGRU (raft.py:228-259), inference --------------------------------------------------
#
# weights = [z1, r1, q1 (Hd, Hd + Xd, 1, 5), z2, r2, q2 (Hd, Hd + Xd, 5, 1)], biases = six (Hd,) vectors: the
# parameters of SepConvGru in the order its forward uses them.  Not differentiable: like dicl_match_1x1, its
# Autograd kernel runs the backend kernel below autograd (training keeps the module's eager path).

GRU_COMPUTE = (_lib.RMD_BF16X3, _lib.RMD_BF16)


def check_gru_args(h, x, weights, biases, compute):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of sepconv_gru; returns
    (hidden, input) widths."""
    if h.dim() != 4 or x.dim() != 4 or h.shape[0] != x.shape[0] or h.shape[2:] != x.shape[2:]:
        raise ValueError(f"sepconv_gru: h (B, Hd, H, W) and x (B, Xd, H, W) expected, got {tuple(h.shape)} / "
                         f"{tuple(x.shape)}")
    if min(h.shape) < 1 or x.shape[1] < 1:
        raise ValueError(f"sepconv_gru: empty h {tuple(h.shape)} or x {tuple(x.shape)}")
    if len(weights) != 6 or len(biases) != 6:
        raise ValueError(f"sepconv_gru: need 6 weights and 6 biases, got {len(weights)} and {len(biases)}")
    if compute not in GRU_COMPUTE:
        raise ValueError(f"sepconv_gru: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    hd, xd = h.shape[1], x.shape[1]
    for i, (wt, bs) in enumerate(zip(weights, biases)):
        want = (hd, hd + xd, 1, 5) if i < 3 else (hd, hd + xd, 5, 1)
        if tuple(wt.shape) != want:
            raise ValueError(f"sepconv_gru: weights[{i}] must be {want}, got {tuple(wt.shape)}")
        if bs.numel() != hd:
            raise ValueError(f"sepconv_gru: biases[{i}] must hold {hd} elements, got {tuple(bs.shape)}")
    for t in (h, x, *weights, *biases):
        if not t.is_floating_point():
            raise ValueError(f"sepconv_gru: tensors must be floating point, got {t.dtype}")
    return hd, xd


def gru_supported(hidden, input):
    """rmd_sepconv_gru_supported: whether the HIP kernel serves these widths (host only)."""
    return bool(_lib.lib().rmd_sepconv_gru_supported(hidden, input))


GRU_MAX_IMAGE = 1 << 30     # (Hd + Xd) H W per image: 32-bit lane offsets inside an image


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


@_hip("sepconv_gru")
def _sepconv_gru(h, x, weights, biases, compute):
    hd, xd = check_gru_args(h, x, weights, biases, compute)
    b, _, ht, wd = h.shape
    if not gru_supported(hd, xd) or (hd + xd) * ht * wd >= GRU_MAX_IMAGE:
        raise ValueError(f"sepconv_gru: unsupported on the GPU: hidden {hd} (a multiple of 32 in 32..128), input {xd} "
                         f"(a multiple of 16), hidden + input <= 512, (hidden + input) H W < 2^30")
    hh, xx = _f32(h), _f32(x)
    ws, ts = [_f32(t) for t in weights], [_f32(t) for t in biases]
    work = _lib.workspace("sepconv_gru", hh, b, hd, xd, ht, wd)
    out = _like(hh)
    _lib.launch("rmd_sepconv_gru", hh, hh, xx, _pointers(ws), _pointers(ts), out, work, b, hd, xd, ht, wd, compute)
    return out


@_fake("sepconv_gru")
def _(h, x, weights, biases, compute):
    check_gru_args(h, x, weights, biases, compute)
    return _like(h)


def _sepconv_gru_below_autograd(h, x, weights, biases, compute):
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.rmd.sepconv_gru(h, x, weights, biases, compute)


LIB.impl("sepconv_gru", _sepconv_gru_below_autograd, "Autograd")


# ---- fused k x k convolutions (raft.py:193-225, 262-273, 299-331), inference -------------------------
#
# conv2d_act: a stride-1, "same"-padded convolution over cat(x0, x1) with bias and activation (act 0: none,
# 1: ReLU).  motion_encoder: BasicMotionEncoder.forward, parameters in the order convc1, convc2, convf1, convf2,
# conv.  Not differentiable, like sepconv_gru: training keeps the modules' eager paths.

CONV_COMPUTE = GRU_COMPUTE
CONV_ACTS = (0, 1)
CONV_MAX_IMAGE = 1 << 30    # channels H W per image, inputs and destination: 32-bit lane offsets inside an image
# (Cout, Cin (None: corr_planes), k) of the encoder's five convolutions
ENCODER_CONVS = ((256, None, 1), (192, 256, 3), (128, 2, 7), (64, 128, 3), (126, 256, 3))


def check_conv_args(x0, x1, weight, bias, act, compute):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of conv2d_act; returns
    (C0, C1, Cout, kh, kw)."""
    if x0.dim() != 4 or min(x0.shape) < 1:
        raise ValueError(f"conv2d_act: x0 (B, C0, H, W), not empty, expected, got {tuple(x0.shape)}")
    c0, c1 = x0.shape[1], 0
    if x1 is not None:
        if x1.dim() != 4 or x1.shape[0] != x0.shape[0] or x1.shape[2:] != x0.shape[2:] or x1.shape[1] < 1:
            raise ValueError(f"conv2d_act: x1 must be (B, C1 >= 1, H, W) like x0 {tuple(x0.shape)}, got "
                             f"{tuple(x1.shape)}")
        c1 = x1.shape[1]
    if compute not in CONV_COMPUTE:
        raise ValueError(f"conv2d_act: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    if act not in CONV_ACTS:
        raise ValueError(f"conv2d_act: act {act} (supported: 0 = none, 1 = ReLU)")
    if weight.dim() != 4 or weight.shape[1] != c0 + c1 or weight.shape[0] < 1:
        raise ValueError(f"conv2d_act: weight must be (Cout, {c0 + c1}, kh, kw) for inputs of {c0} + {c1} channels, "
                         f"got {tuple(weight.shape)}")
    cout, _, kh, kw = weight.shape
    if kh % 2 != 1 or kw % 2 != 1:
        raise ValueError(f"conv2d_act: kernel sides must be odd ('same' padding), got {kh} x {kw}")
    if bias.numel() != cout:
        raise ValueError(f"conv2d_act: bias must hold {cout} elements, got {tuple(bias.shape)}")
    for t in (x0, x1, weight, bias):
        if t is not None and not t.is_floating_point():
            raise ValueError(f"conv2d_act: tensors must be floating point, got {t.dtype}")
    return c0, c1, cout, kh, kw


def conv_supported(kh, kw, c0, c1, cout):
    """rmd_conv2d_supported: whether the HIP kernel serves this convolution (host only)."""
    return bool(_lib.lib().rmd_conv2d_supported(kh, kw, c0, c1, cout))


CONV_RANGE = "kernel sides odd in 1..7, C0 + C1 <= 512, Cout <= 1024, channels x H x W < 2^30"


def conv_unsupported_reason(kh, kw, c0, c1, cout, ht, wd, out_channels=None):
    """Why the HIP kernel cannot serve this convolution on an (ht, wd) map (None if it can)."""
    # the documented range first: what it refuses is refused without the library
    if kh % 2 != 1 or kw % 2 != 1 or max(kh, kw) > 7 or c0 + c1 > 512 or cout > 1024 \
            or not conv_supported(kh, kw, c0, c1, cout):
        return f"unsupported convolution {kh}x{kw}, {c0} + {c1} -> {cout} channels ({CONV_RANGE})"
    if max(c0 + c1, out_channels or cout) * ht * wd >= CONV_MAX_IMAGE:
        return f"unsupported size: channels x H x W = {max(c0 + c1, out_channels or cout) * ht * wd} >= 2^30"
    return None


@_hip("conv2d_act")
def _conv2d_act(x0, x1, weight, bias, act, compute):
    c0, c1, cout, kh, kw = check_conv_args(x0, x1, weight, bias, act, compute)
    b, _, ht, wd = x0.shape
    reason = conv_unsupported_reason(kh, kw, c0, c1, cout, ht, wd)
    if reason:
        raise ValueError(f"conv2d_act: unsupported on the GPU: {reason}")
    a0, a1 = _f32(x0), (None if x1 is None else _f32(x1))
    wt, bs = _f32(weight), _f32(bias)
    work = _lib.workspace("conv2d", a0, c0, c1, cout, kh, kw)
    out = _like(a0, (b, cout, ht, wd))
    _lib.launch("rmd_conv2d", a0, a0, a1, wt, bs, out, work, b, c0, c1, cout, kh, kw, ht, wd, cout, 0, act, compute)
    return out


@_fake("conv2d_act")
def _(x0, x1, weight, bias, act, compute):
    _, _, cout, _, _ = check_conv_args(x0, x1, weight, bias, act, compute)
    return _like(x0, (x0.shape[0], cout, x0.shape[2], x0.shape[3]))


def check_encoder_args(flow, corr, weights, biases, compute):
    """The shared checks of motion_encoder; returns corr_planes."""
    if flow.dim() != 4 or corr.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] != corr.shape[0] \
            or flow.shape[2:] != corr.shape[2:] or min(flow.shape) < 1 or corr.shape[1] < 1:
        raise ValueError(f"motion_encoder: flow (B, 2, H, W) and corr (B, planes, H, W) expected, got "
                         f"{tuple(flow.shape)} / {tuple(corr.shape)}")
    if len(weights) != 5 or len(biases) != 5:
        raise ValueError(f"motion_encoder: need 5 weights and 5 biases, got {len(weights)} and {len(biases)}")
    if compute not in CONV_COMPUTE:
        raise ValueError(f"motion_encoder: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    planes = corr.shape[1]
    for i, ((cout, cin, k), wt, bs) in enumerate(zip(ENCODER_CONVS, weights, biases)):
        want = (cout, planes if cin is None else cin, k, k)
        if tuple(wt.shape) != want:
            raise ValueError(f"motion_encoder: weights[{i}] must be {want}, got {tuple(wt.shape)}")
        if bs.numel() != cout:
            raise ValueError(f"motion_encoder: biases[{i}] must hold {cout} elements, got {tuple(bs.shape)}")
    for t in (flow, corr, *weights, *biases):
        if not t.is_floating_point():
            raise ValueError(f"motion_encoder: tensors must be floating point, got {t.dtype}")
    return planes


def encoder_unsupported_reason(planes, ht, wd):
    """Why the HIP kernels cannot serve the encoder on an (ht, wd) map (None if they can)."""
    return conv_unsupported_reason(1, 1, planes, 0, 256, ht, wd)


@_hip("motion_encoder")
def _motion_encoder(flow, corr, weights, biases, compute):
    planes = check_encoder_args(flow, corr, weights, biases, compute)
    b, _, ht, wd = flow.shape
    reason = encoder_unsupported_reason(planes, ht, wd)
    if reason:
        raise ValueError(f"motion_encoder: unsupported on the GPU: {reason}")
    fl, co = _f32(flow), _f32(corr)
    ws, ts = [_f32(t) for t in weights], [_f32(t) for t in biases]
    work = _lib.workspace("motion_encoder", fl, b, planes, ht, wd)
    out = _like(fl, (b, 128, ht, wd))
    _lib.launch("rmd_motion_encoder", fl, fl, co, _pointers(ws), _pointers(ts), out, work, b, planes, ht, wd, compute)
    return out


@_fake("motion_encoder")
def _(flow, corr, weights, biases, compute):
    check_encoder_args(flow, corr, weights, biases, compute)
    return _like(flow, (flow.shape[0], 128, flow.shape[2], flow.shape[3]))


def _conv2d_act_below_autograd(x0, x1, weight, bias, act, compute):
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.rmd.conv2d_act(x0, x1, weight, bias, act, compute)


def _motion_encoder_below_autograd(flow, corr, weights, biases, compute):
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.rmd.motion_encoder(flow, corr, weights, biases, compute)


LIB.impl("conv2d_act", _conv2d_act_below_autograd, "Autograd")
LIB.impl("motion_encoder", _motion_encoder_below_autograd, "Autograd")


# ---- fused k x k convolutions, training (csrc/conv_backward.hip) ------------------------------------
#
# conv2d_act_train: conv2d_act's kernel in the parity mode (bit for bit its result) with an autograd formula that
# saves x0, x1, weight and the output.  conv2d_act_backward(grad, y, x0, x1, weight, act, needs_grad) returns
# [gx0, gx1, gweight, gbias], an empty tensor for what needs_grad = [x0, x1, weight, bias] switches off (and for
# gx1 without an x1); y is the forward's output, given exactly when act is 1.  The one-product mode has no backward.

def check_conv_backward_args(grad, y, x0, x1, weight, act, needs_grad):
    """check_conv_args plus the shapes of grad and y and the four needs_grad flags; returns (C0, C1, Cout, kh, kw)."""
    name = "conv2d_act_backward"
    if weight.dim() != 4:
        raise ValueError(f"{name}: weight must be 4-D, got {tuple(weight.shape)}")
    dims = check_conv_args(x0, x1, weight, weight.new_empty(weight.shape[0]), act, _lib.RMD_BF16X3)
    want = (x0.shape[0], dims[2], x0.shape[2], x0.shape[3])
    if tuple(grad.shape) != want or not grad.is_floating_point():
        raise ValueError(f"{name}: grad must be a floating-point {want} tensor, got {grad.dtype} {tuple(grad.shape)}")
    if (y is None) != (act == 0):
        raise ValueError(f"{name}: y (the forward's output) must be given exactly when act is 1 (ReLU)")
    if y is not None and (tuple(y.shape) != want or not y.is_floating_point()):
        raise ValueError(f"{name}: y must be a floating-point {want} tensor, got {y.dtype} {tuple(y.shape)}")
    if len(needs_grad) != 4:
        raise ValueError(f"{name}: needs_grad is [x0, x1, weight, bias], got {len(needs_grad)} flags")
    return dims


def conv_backward_supported(kh, kw, c0, c1, cout):
    """rmd_conv2d_backward_supported: whether the HIP backward serves this convolution (host only)."""
    return bool(_lib.lib().rmd_conv2d_backward_supported(kh, kw, c0, c1, cout))


def conv_backward_kernels(needs_grad, act, has_x1=True):
    """rmd_conv2d_backward_kernels: the names of the kernels conv2d_act_backward launches for these needs_grad flags
    [x0, x1, weight, bias], in order (host only)."""
    n0, n1, nw, nb = (int(bool(v)) for v in needs_grad)
    return _lib.lib().rmd_conv2d_backward_kernels(n0, n1 if has_x1 else 0, nw, nb, act).decode().split()


def _conv_grads(x0, x1, weight, needs_grad):
    """The four gradients, shaped like what they belong to; (0,) for a skipped one and for gx1 without an x1."""
    shapes = [x0.shape, None if x1 is None else x1.shape, weight.shape, (weight.shape[0],)]
    return [_like(x0, tuple(s) if need and s is not None else (0,)) for s, need in zip(shapes, needs_grad)]


@_hip("conv2d_act_train")
def _conv2d_act_train(x0, x1, weight, bias, act):
    return _conv2d_act(x0, x1, weight, bias, act, _lib.RMD_BF16X3)


@_fake("conv2d_act_train")
def _(x0, x1, weight, bias, act):
    _, _, cout, _, _ = check_conv_args(x0, x1, weight, bias, act, _lib.RMD_BF16X3)
    return _like(x0, (x0.shape[0], cout, x0.shape[2], x0.shape[3]))


@_hip("conv2d_act_backward")
def _conv2d_act_backward(grad, y, x0, x1, weight, act, needs_grad):
    c0, c1, cout, kh, kw = check_conv_backward_args(grad, y, x0, x1, weight, act, needs_grad)
    b, _, ht, wd = x0.shape
    reason = conv_unsupported_reason(kh, kw, c0, c1, cout, ht, wd)
    if reason or not conv_backward_supported(kh, kw, c0, c1, cout):
        raise ValueError(f"conv2d_act_backward: unsupported on the GPU: {reason or 'unsupported convolution'}")
    g, yy = _f32(grad), (None if y is None else _f32(y))
    a0, a1, wt = _f32(x0), (None if x1 is None else _f32(x1)), _f32(weight)
    grads = _conv_grads(a0, a1, wt, needs_grad)
    if any(t.numel() for t in grads):
        work = _lib.workspace("conv2d_backward", a0, b, c0, c1, cout, kh, kw, ht, wd)
        gx0, gx1, gw, gb = [t if t.numel() else None for t in grads]
        _lib.launch("rmd_conv2d_backward", a0, g, yy, a0, a1, wt, gx0, gx1, gw, gb, work, b, c0, c1, cout, kh, kw, ht,
                    wd, act)
    return grads


@_fake("conv2d_act_backward")
def _(grad, y, x0, x1, weight, act, needs_grad):
    check_conv_backward_args(grad, y, x0, x1, weight, act, needs_grad)
    return _conv_grads(x0, x1, weight, needs_grad)


def _conv_train_setup(ctx, inputs, output):
    x0, x1, weight, bias, act = inputs
    ctx.save_for_backward(x0, x1, weight, output if act else None)
    ctx.act = act
    ctx.bias_dtype = bias.dtype
    ctx.needs = [x0.requires_grad, x1 is not None and x1.requires_grad, weight.requires_grad, bias.requires_grad]


def _conv_train_bwd(ctx, grad):
    x0, x1, weight, y = ctx.saved_tensors
    if not any(ctx.needs):
        return None, None, None, None, None
    grads = torch.ops.rmd.conv2d_act_backward(grad, y, x0, x1, weight, ctx.act, ctx.needs)
    dtypes = [x0.dtype, None if x1 is None else x1.dtype, weight.dtype, ctx.bias_dtype]
    out = [g.to(d) if need else None for g, d, need in zip(grads, dtypes, ctx.needs)]
    return out[0], out[1], out[2], out[3], None


torch.library.register_autograd("rmd::conv2d_act_train", _conv_train_bwd, setup_context=_conv_train_setup)


# ---- the feature / context encoder (encoders/raft/s3.py:8-72, blocks/raft.py:13-46), inference ------------
#
# conv2d_norm_act: a convolution of stride 1 or 2 with padding k / 2 over relu(x scale + shift) (x itself without the
# statistics), bias, activation and, with a residual, relu(. + residual).  instance_norm_stats: nn.InstanceNorm2d at
# its defaults as (scale, shift), norm(x) = x scale + shift.  residual_join: relu(xs + relu(ys)).  feature_encoder:
# FeatureEncoder.forward, the 16 convolutions' parameters in module order, norm 0 (none; batch norm folded) or 1
# (instance).  Not differentiable, like conv2d_act.

ENCODER_STRIDES = (1, 2)
ENCODER_NORMS = (_lib.RMD_NORM_NONE, _lib.RMD_NORM_INSTANCE)
INSTANCE_NORM_EPS = 1e-5            # nn.InstanceNorm2d's default, the one feature_encoder uses
ENCODER_RANGE = "kernel sides odd in 1..7, stride 1 or 2, C <= 512, Cout <= 1024, channels x H x W < 2^30"


def out_side(n, stride):
    """Output side of a convolution of padding k / 2 and this stride over n positions."""
    return (n - 1) // stride + 1


def feature_encoder_convs(output_dim):
    """(Cout, Cin, k, stride) of FeatureEncoder's 16 convolutions in module order: conv1; per block conv1, conv2
    and (stride 2) downsample.0; conv2."""
    convs, cin = [(64, 3, 7, 2)], 64
    for width, stride in ((64, 1), (96, 2), (128, 2)):
        convs += [(width, cin, 3, stride), (width, width, 3, 1)]
        if stride == 2:
            convs.append((width, cin, 1, 2))
        convs += [(width, width, 3, 1), (width, width, 3, 1)]
        cin = width
    return convs + [(output_dim, 128, 1, 1)]


def _check_stats(name, scale, shift, like, what):
    if (scale is None) != (shift is None):
        raise ValueError(f"{name}: {what}_scale and {what}_shift are given together")
    for t in (scale, shift):
        if t is not None and (tuple(t.shape) != tuple(like.shape[:2]) or not t.is_floating_point()):
            raise ValueError(f"{name}: the statistics of {what} must be floating point (B, C) = "
                             f"{tuple(like.shape[:2])}, got {tuple(t.shape)} {t.dtype}")


def check_norm_conv_args(x, scale, shift, weight, bias, residual, stride, act, compute):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of conv2d_norm_act; returns the
    output's shape."""
    name = "conv2d_norm_act"
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{name}: x (B, C, H, W), not empty, expected, got {tuple(x.shape)}")
    if compute not in CONV_COMPUTE:
        raise ValueError(f"{name}: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    if act not in CONV_ACTS:
        raise ValueError(f"{name}: act {act} (supported: 0 = none, 1 = ReLU)")
    if stride not in ENCODER_STRIDES:
        raise ValueError(f"{name}: stride {stride} (supported: 1, 2)")
    b, c, ht, wd = x.shape
    if weight.dim() != 4 or weight.shape[1] != c or weight.shape[0] < 1:
        raise ValueError(f"{name}: weight must be (Cout, {c}, kh, kw), got {tuple(weight.shape)}")
    cout, _, kh, kw = weight.shape
    if kh % 2 != 1 or kw % 2 != 1:
        raise ValueError(f"{name}: kernel sides must be odd (padding k / 2), got {kh} x {kw}")
    if bias.numel() != cout:
        raise ValueError(f"{name}: bias must hold {cout} elements, got {tuple(bias.shape)}")
    _check_stats(name, scale, shift, x, "x")
    shape = (b, cout, out_side(ht, stride), out_side(wd, stride))
    if residual is not None and tuple(residual.shape) != shape:
        raise ValueError(f"{name}: residual must be {shape}, got {tuple(residual.shape)}")
    for t in (x, weight, bias, residual):
        if t is not None and not t.is_floating_point():
            raise ValueError(f"{name}: tensors must be floating point, got {t.dtype}")
    return shape


def norm_conv_unsupported_reason(kh, kw, stride, c, cout, ht, wd):
    """Why the HIP kernel cannot serve this convolution on an (ht, wd) map (None if it can)."""
    # the documented range first: what it refuses is refused without the library
    if kh % 2 != 1 or kw % 2 != 1 or max(kh, kw) > 7 or stride not in ENCODER_STRIDES or c > 512 or cout > 1024 \
            or not _lib.lib().rmd_conv2d_strided_supported(kh, kw, stride, c, cout):
        return f"unsupported convolution {kh}x{kw} stride {stride}, {c} -> {cout} channels ({ENCODER_RANGE})"
    size = max(c * ht * wd, cout * out_side(ht, stride) * out_side(wd, stride))
    if size >= CONV_MAX_IMAGE:
        return f"unsupported size: channels x H x W = {size} >= 2^30"
    return None


def _opt(t):
    return None if t is None else _f32(t)


@_hip("conv2d_norm_act")
def _conv2d_norm_act(x, scale, shift, weight, bias, residual, stride, act, compute):
    shape = check_norm_conv_args(x, scale, shift, weight, bias, residual, stride, act, compute)
    b, c, ht, wd = x.shape
    cout, _, kh, kw = weight.shape
    reason = norm_conv_unsupported_reason(kh, kw, stride, c, cout, ht, wd)
    if reason:
        raise ValueError(f"conv2d_norm_act: unsupported on the GPU: {reason}")
    xx, wt, bs = _f32(x), _f32(weight), _f32(bias)
    work = _lib.workspace("conv2d_strided", xx, c, cout, kh, kw)
    out = _like(xx, shape)
    _lib.launch("rmd_conv2d_strided", xx, xx, _opt(scale), _opt(shift), wt, bs, _opt(residual), out, work, b, c, cout,
                kh, kw, ht, wd, stride, act, compute)
    return out


@_fake("conv2d_norm_act")
def _(x, scale, shift, weight, bias, residual, stride, act, compute):
    return _like(x, check_norm_conv_args(x, scale, shift, weight, bias, residual, stride, act, compute))


def check_stats_args(x, eps):
    """The shared checks of instance_norm_stats."""
    if x.dim() != 4 or min(x.shape) < 1 or not x.is_floating_point():
        raise ValueError(f"instance_norm_stats: floating point x (B, C, H, W), not empty, expected, got "
                         f"{tuple(x.shape)} {x.dtype}")
    if x.shape[2] * x.shape[3] < 2:
        raise ValueError(f"instance_norm_stats: a plane of one pixel has no variance, got {tuple(x.shape)}")
    if not eps >= 0:
        raise ValueError(f"instance_norm_stats: eps must not be negative, got {eps}")


@_hip("instance_norm_stats")
def _instance_norm_stats(x, eps):
    check_stats_args(x, eps)
    b, c, ht, wd = x.shape
    if ht * wd >= CONV_MAX_IMAGE:
        raise ValueError(f"instance_norm_stats: unsupported on the GPU: H x W = {ht * wd} >= 2^30")
    xx = _f32(x)
    scale, shift = _like(xx, (b, c)), _like(xx, (b, c))
    _lib.launch("rmd_instance_stats", xx, xx, scale, shift, b, c, ht, wd, ctypes.c_float(eps))
    return scale, shift


@_fake("instance_norm_stats")
def _(x, eps):
    check_stats_args(x, eps)
    return _like(x, x.shape[:2]), _like(x, x.shape[:2])


def check_join_args(y, y_scale, y_shift, x, x_scale, x_shift):
    """The shared checks of residual_join."""
    if y.dim() != 4 or min(y.shape) < 1 or x.shape != y.shape:
        raise ValueError(f"residual_join: y and x (B, C, H, W), not empty, of one shape expected, got "
                         f"{tuple(y.shape)} / {tuple(x.shape)}")
    if not (y.is_floating_point() and x.is_floating_point()):
        raise ValueError(f"residual_join: tensors must be floating point, got {y.dtype} / {x.dtype}")
    _check_stats("residual_join", y_scale, y_shift, y, "y")
    _check_stats("residual_join", x_scale, x_shift, x, "x")


@_hip("residual_join")
def _residual_join(y, y_scale, y_shift, x, x_scale, x_shift):
    check_join_args(y, y_scale, y_shift, x, x_scale, x_shift)
    b, c, ht, wd = y.shape
    if ht * wd >= CONV_MAX_IMAGE:
        raise ValueError(f"residual_join: unsupported on the GPU: H x W = {ht * wd} >= 2^30")
    yy, xx = _f32(y), _f32(x)
    out = _like(yy)
    _lib.launch("rmd_residual_join", yy, yy, _opt(y_scale), _opt(y_shift), xx, _opt(x_scale), _opt(x_shift), out, b, c,
                ht, wd)
    return out


@_fake("residual_join")
def _(y, y_scale, y_shift, x, x_scale, x_shift):
    check_join_args(y, y_scale, y_shift, x, x_scale, x_shift)
    return _like(y)


def check_feature_encoder_args(x, weights, biases, norm, compute):
    """The shared checks of feature_encoder; returns the output's shape."""
    name = "feature_encoder"
    if x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1:
        raise ValueError(f"{name}: x (B, 3, H, W), not empty, expected, got {tuple(x.shape)}")
    if len(weights) != 16 or len(biases) != 16:
        raise ValueError(f"{name}: need 16 weights and 16 biases, got {len(weights)} and {len(biases)}")
    if compute not in CONV_COMPUTE:
        raise ValueError(f"{name}: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    if norm not in ENCODER_NORMS:
        raise ValueError(f"{name}: norm {norm} (supported: RMD_NORM_NONE = 0, RMD_NORM_INSTANCE = 1)")
    if weights[15].dim() != 4 or weights[15].shape[0] < 1:
        raise ValueError(f"{name}: weights[15] must be (output_dim, 128, 1, 1), got {tuple(weights[15].shape)}")
    output_dim = weights[15].shape[0]
    for i, ((cout, cin, k, _), wt, bs) in enumerate(zip(feature_encoder_convs(output_dim), weights, biases)):
        if tuple(wt.shape) != (cout, cin, k, k):
            raise ValueError(f"{name}: weights[{i}] must be {(cout, cin, k, k)}, got {tuple(wt.shape)}")
        if bs.numel() != cout:
            raise ValueError(f"{name}: biases[{i}] must hold {cout} elements, got {tuple(bs.shape)}")
    for t in (x, *weights, *biases):
        if not t.is_floating_point():
            raise ValueError(f"{name}: tensors must be floating point, got {t.dtype}")
    ht, wd = x.shape[2:]
    for _ in range(3):
        ht, wd = out_side(ht, 2), out_side(wd, 2)
    if norm == _lib.RMD_NORM_INSTANCE and ht * wd < 2:
        raise ValueError(f"{name}: the instance norm needs more than one pixel at 1/8 resolution, got an input of "
                         f"{tuple(x.shape[2:])}")
    return (x.shape[0], output_dim, ht, wd)


def feature_encoder_unsupported_reason(output_dim, ht, wd):
    """Why the HIP kernels cannot serve the encoder on an (ht, wd) image (None if they can)."""
    if output_dim > 1024:
        return f"unsupported output_dim {output_dim} (at most 1024)"
    size, h, w = 0, ht, wd
    for width in (64, 96, 128):         # a side of 1 stays 1 while the channels grow: the largest map is not always the first
        h, w = out_side(h, 2), out_side(w, 2)
        size = max(size, width * h * w)
    if max(size, 3 * ht * wd, output_dim * h * w) >= CONV_MAX_IMAGE:
        return f"unsupported size: channels x H x W = {max(size, 3 * ht * wd, output_dim * h * w)} >= 2^30"
    return None


@_hip("feature_encoder")
def _feature_encoder(x, weights, biases, norm, compute):
    shape = check_feature_encoder_args(x, weights, biases, norm, compute)
    b, _, ht, wd = x.shape
    reason = feature_encoder_unsupported_reason(shape[1], ht, wd)
    if reason:
        raise ValueError(f"feature_encoder: unsupported on the GPU: {reason}")
    xx = _f32(x)
    ws, ts = [_f32(t) for t in weights], [_f32(t) for t in biases]
    work = _lib.workspace("feature_encoder", xx, b, ht, wd, shape[1])
    out = _like(xx, shape)
    _lib.launch("rmd_feature_encoder", xx, xx, _pointers(ws), _pointers(ts), out, work, b, ht, wd, shape[1], norm,
                ctypes.c_float(INSTANCE_NORM_EPS), compute)
    return out


@_fake("feature_encoder")
def _(x, weights, biases, norm, compute):
    return _like(x, check_feature_encoder_args(x, weights, biases, norm, compute))


def _below_autograd(name):
    op = getattr(torch.ops.rmd, name)

    def kernel(*args):
        with torch._C._AutoDispatchBelowAutograd():
            return op(*args)
    LIB.impl(name, kernel, "Autograd")


for _name in _family("encoder"):
    _below_autograd(_name)


# ---- the k x k MatchingNet (blocks/dicl.py:93-118), inference ---------------------------------------------
#
# matching_net: MatchingNet.forward on folded parameters (MatchingNet.folded()): weights [W1' .. W4' (Cout, Cin, 3, 3),
# W5' (c3, c4, 4, 4) in nn.ConvTranspose2d's layout, w6 (c4, 3, 3)], biases [t1 .. t5, b6 (one element)]; `group` is
# the number of images (of the B du dv) per pass over the workspace.  mnet_tail: its last two layers on x (N, c3, h2,
# w2).  Not differentiable, like conv2d_act.

MNET_MAX_IMAGE = CONV_MAX_IMAGE
MNET_RANGE = ("h and w even, layer inputs of at most 512 channels, c3 <= 64, c4 <= 32, channels x H x W < 2^30 for every "
              "map")


def check_tail_args(x, weight5, bias5, weight6, bias6, compute):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of mnet_tail; returns (c3, c4)."""
    name = "mnet_tail"
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{name}: x (N, c3, h2, w2), not empty, expected, got {tuple(x.shape)}")
    if compute not in CONV_COMPUTE:
        raise ValueError(f"{name}: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    c3 = x.shape[1]
    if weight5.dim() != 4 or weight5.shape[0] != c3 or weight5.shape[1] < 1 or tuple(weight5.shape[2:]) != (4, 4):
        raise ValueError(f"{name}: weight5 must be ({c3}, c4, 4, 4), got {tuple(weight5.shape)}")
    c4 = weight5.shape[1]
    if bias5.numel() != c4:
        raise ValueError(f"{name}: bias5 must hold {c4} elements, got {tuple(bias5.shape)}")
    if tuple(weight6.shape) != (c4, 3, 3):
        raise ValueError(f"{name}: weight6 must be ({c4}, 3, 3), got {tuple(weight6.shape)}")
    if bias6.numel() != 1:
        raise ValueError(f"{name}: bias6 must hold one element, got {tuple(bias6.shape)}")
    for t in (x, weight5, bias5, weight6, bias6):
        if not t.is_floating_point():
            raise ValueError(f"{name}: tensors must be floating point, got {t.dtype}")
    return c3, c4


def tail_supported(c3, c4, h2, w2):
    """rmd_mnet_tail_supported: whether the HIP kernel serves these sizes (host only)."""
    return c3 * h2 * w2 < MNET_MAX_IMAGE and bool(_lib.lib().rmd_mnet_tail_supported(c3, c4, h2, w2))


@_hip("mnet_tail")
def _mnet_tail(x, weight5, bias5, weight6, bias6, compute):
    c3, c4 = check_tail_args(x, weight5, bias5, weight6, bias6, compute)
    n, _, h2, w2 = x.shape
    if not tail_supported(c3, c4, h2, w2):
        raise ValueError(f"mnet_tail: unsupported on the GPU: channels {c3} -> {c4} on {h2} x {w2} (c3 <= 64, c4 <= 32, "
                         f"c3 h2 w2 < 2^30)")
    xx, w5, b5, w6, b6 = (_f32(t) for t in (x, weight5, bias5, weight6, bias6))
    work = _lib.workspace("mnet_tail", xx, c3, c4)
    out = _like(xx, (n, 2 * h2, 2 * w2))
    _lib.launch("rmd_mnet_tail", xx, xx, w5, b5, w6, b6, out, work, n, c3, c4, h2, w2, compute)
    return out


@_fake("mnet_tail")
def _(x, weight5, bias5, weight6, bias6, compute):
    check_tail_args(x, weight5, bias5, weight6, bias6, compute)
    return _like(x, (x.shape[0], 2 * x.shape[2], 2 * x.shape[3]))


def check_mnet_args(mvol, weights, biases, group, compute):
    """Shape, dtype and argument checks shared by the GPU, CPU and fake kernels of matching_net; returns the widths
    (c_in, c1, c2, c3, c4)."""
    name = "matching_net"
    if mvol.dim() != 6 or min(mvol.shape) < 1:
        raise ValueError(f"{name}: mvol (B, du, dv, c_in, h, w), not empty, expected, got {tuple(mvol.shape)}")
    if len(weights) != 6 or len(biases) != 6:
        raise ValueError(f"{name}: need 6 weights and 6 biases, got {len(weights)} and {len(biases)}")
    if compute not in CONV_COMPUTE:
        raise ValueError(f"{name}: compute {compute} (supported: RMD_BF16X3 = 3, RMD_BF16 = 2)")
    if group < 1:
        raise ValueError(f"{name}: group must be at least 1, got {group}")
    c_in, ht, wd = mvol.shape[3:]
    if ht % 2 or wd % 2:
        raise ValueError(f"{name}: h and w must be even (the reference's view fails on odd sides), got {ht} x {wd}")
    for i in (0, 1, 2, 3):
        if weights[i].dim() != 4 or weights[i].shape[0] < 1:
            raise ValueError(f"{name}: weights[{i}] must be (Cout, Cin, 3, 3), got {tuple(weights[i].shape)}")
    c1, c2, c3 = weights[0].shape[0], weights[1].shape[0], weights[3].shape[0]
    if weights[4].dim() != 4 or weights[4].shape[1] < 1:
        raise ValueError(f"{name}: weights[4] must be ({c3}, c4, 4, 4), got {tuple(weights[4].shape)}")
    c4 = weights[4].shape[1]
    want = [(c1, c_in, 3, 3), (c2, c1, 3, 3), (c2, c2, 3, 3), (c3, c2, 3, 3), (c3, c4, 4, 4), (c4, 3, 3)]
    for i, (wt, bs, shape) in enumerate(zip(weights, biases, want)):
        if tuple(wt.shape) != shape:
            raise ValueError(f"{name}: weights[{i}] must be {shape}, got {tuple(wt.shape)}")
        n = 1 if i == 5 else (c4 if i == 4 else shape[0])
        if bs.numel() != n:
            raise ValueError(f"{name}: biases[{i}] must hold {n} elements, got {tuple(bs.shape)}")
    for t in (mvol, *weights, *biases):
        if not t.is_floating_point():
            raise ValueError(f"{name}: tensors must be floating point, got {t.dtype}")
    return c_in, c1, c2, c3, c4


def mnet_supported(c_in, c1, c2, c3, c4, ht, wd):
    """rmd_matching_net_supported: whether the HIP kernels serve these sizes (host only)."""
    if max(c_in, c1) * ht * wd >= MNET_MAX_IMAGE:      # the documented range first: ints that fit the C call
        return False
    return bool(_lib.lib().rmd_matching_net_supported(c_in, c1, c2, c3, c4, ht, wd))


def mnet_workspace_bytes(group, c_in, c1, c2, c3, c4, ht, wd):
    """rmd_matching_net_workspace_bytes (host only; 0: unsupported arguments)."""
    return _lib.lib().rmd_matching_net_workspace_bytes(group, c_in, c1, c2, c3, c4, ht, wd)


@_hip("matching_net")
def _matching_net(mvol, weights, biases, group, compute):
    widths = check_mnet_args(mvol, weights, biases, group, compute)
    b, du, dv, _, ht, wd = mvol.shape
    if not mnet_supported(*widths, ht, wd):
        raise ValueError(f"matching_net: unsupported on the GPU: channels {widths} on {ht} x {wd} ({MNET_RANGE})")
    n = b * du * dv
    group = min(group, n)
    xx = _f32(mvol)
    ws, ts = [_f32(t) for t in weights], [_f32(t) for t in biases]
    work = _lib.workspace("matching_net", xx, group, *widths, ht, wd)
    out = _like(xx, (b, du, dv, ht, wd))
    _lib.launch("rmd_matching_net", xx, xx, _pointers(ws), _pointers(ts), out, work, n, group, *widths, ht, wd, compute)
    return out


@_fake("matching_net")
def _(mvol, weights, biases, group, compute):
    check_mnet_args(mvol, weights, biases, group, compute)
    b, du, dv, _, ht, wd = mvol.shape
    return _like(mvol, (b, du, dv, ht, wd))


for _name in _family("mnet"):
    _below_autograd(_name)
