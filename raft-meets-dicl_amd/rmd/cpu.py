"""CPU kernels of the torch.ops.rmd operators: ATen composites of the reference's own algorithms.

The reference's modules run on any device (src/models/impls/raft.py:15-95 is plain torch), so a user
who evaluates on the CPU keeps the drop-ins: every rmd operator has a kernel here, registered for the
CPU and AutogradCPU dispatch keys (SURVEY.md §7 "CPU dispatch").

Dispatch, not fallback: a CUDA tensor always reaches the HIP kernel of rmd/library.py (which raises if
librmd.so is missing); only CPU tensors come here.  Each kernel restates the reference lines it names
with the same ATen calls (matmul, avg_pool2d, grid_sample, ...), in fp32 whatever the compute mode
(the storage dtype of a pyramid is honoured), so CPU results follow the reference op for op.
Registered at AutogradCPU, the kernels record their ATen graph: the modules train on CPU through
ordinary autograd (the alias-key formulas of rmd/library.py serve the CUDA kernels).

CPU-side formats:
  * corr_pyramid returns the row layout (1-D, include/rmd.h RMD_LAYOUT_ROWS) for every precision;
  * corr_otf_prepare returns a float32 "workspace" holding fmap1 * scale and the pooled fmap2 levels
    (the HIP workspace is an opaque byte buffer in the kernel's operand order).
"""

import math

import torch
import torch.nn.functional as F

from . import _lib
from .library import (INSTANCE_NORM_EPS, LIB, _OPS, _STORAGE, check_attn_args, check_conv_args, check_conv_backward_args,
                      check_encoder_args,
                      check_feature_encoder_args, check_gru_args, check_join_args, check_mnet_args,
                      check_norm_conv_args, check_stats_args, check_tail_args,
                      check_head_args, check_loss_args, check_match_args, check_match_backward_args, check_metric_args,
                      pyramid_elements, pyramid_layout, pyramid_storage, s24_decode)


def _delta(r, device):
    """(2r+1, 2r+1, 2) displacement grid, meshgrid(dx, dy, indexing='ij') (raft.py:55-59)."""
    d = torch.linspace(-r, r, 2 * r + 1, device=device)
    return torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)


def _normalise(cen, w_den, h_den):
    """grid_sample coordinates as the reference computes them in place (raft.py:69-70)."""
    x = 2 * cen[..., 0] / w_den - 1
    y = 2 * cen[..., 1] / h_den - 1
    return torch.stack((x, y), dim=-1)


# ---- RAFT correlation pyramid + lookup (raft.py:18-95) ------------------------------------------

def _corr_levels(f1, f2, levels, scale):
    """raft.py:26-47: corr = fmap1^T fmap2 (B, H, W, 1, H, W) normalised, then 2x2 average pools."""
    b, c, h, w = f1.shape
    corr = torch.matmul(f1.reshape(b, c, h * w).transpose(1, 2), f2.reshape(b, c, h * w))
    if abs(scale * (c ** 0.5) - 1.0) < 1e-6:
        corr = corr / torch.tensor(c).float().sqrt()        # raft.CorrBlock's normalisation, op for op
    elif scale != 1.0:
        corr = corr * scale
    lv = [corr.reshape(b * h * w, 1, h, w)]
    for _ in range(1, levels):
        lv.append(F.avg_pool2d(lv[-1], kernel_size=2, stride=2))
    return lv


def _pack_rows(lv, desc, dtype):
    """Levels (B*N, 1, H_l, W_l) -> the row-layout pyramid (include/rmd.h element formula)."""
    b, n = desc.batch, desc.height * desc.width
    parts, at = [], 0
    for i, x in enumerate(lv):
        hl, wl, cw, tx = desc.level_h[i], desc.level_w[i], desc.tile_w[i], desc.tiles_x[i]
        if desc.level_offset[i] != at:
            parts.append(x.new_zeros(desc.level_offset[i] - at))
        x = F.pad(x.reshape(b, n, hl, wl), (0, tx * cw - wl))
        parts.append(x.reshape(b, n, hl, tx, cw).permute(0, 2, 3, 1, 4).reshape(-1))
        at = desc.level_offset[i] + parts[-1].numel()
    if desc.total_elements != at:
        parts.append(lv[0].new_zeros(desc.total_elements - at))
    return torch.cat(parts).to(dtype)


def _unpack(pyramid, desc, i):
    """Level i of a pyramid tensor (either layout) as (B*N, 1, H_i, W_i) float32."""
    b, h, w = desc.batch, desc.height, desc.width
    th, tw, ty, tx = desc.tile_h[i], desc.tile_w[i], desc.tiles_y[i], desc.tiles_x[i]
    s, off = desc.query_slots, desc.level_offset[i]
    x = pyramid.reshape(-1)[off: off + b * ty * tx * s * th * tw].view(b, ty, tx, s, th, tw)
    x = x.permute(0, 3, 1, 4, 2, 5).reshape(b, s, ty * th, tx * tw)[..., :desc.level_h[i], :desc.level_w[i]]
    if desc.layout == _lib.RMD_LAYOUT_TILES:
        from .ops import tiles_slots
        x = x.index_select(1, tiles_slots(h, w).to(x.device))
    return x.float().reshape(b * h * w, 1, desc.level_h[i], desc.level_w[i])


def corr_pyramid(fmap1, fmap2, levels, compute, storage, scale):
    f1, f2 = fmap1.float(), fmap2.float()
    b, c, h, w = f1.shape
    if storage == _lib.RMD_S24:
        # S24 is the x3 GEMM's output format; every other GEMM (this one too) stores F32, as
        # rmd_pyramid_describe_for resolves it — which also keeps the ATen graph differentiable
        storage = _lib.RMD_F32
    desc = _lib.describe(b, h, w, levels, storage, _lib.RMD_LAYOUT_ROWS)
    return _pack_rows(_corr_levels(f1, f2, levels, float(scale)), desc, _STORAGE[storage])


def corr_lookup(pyramid, coords, levels, radius, level_mask):
    """raft.py:49-95 over the levels stored in `pyramid`."""
    b, _, h, w = coords.shape
    desc = _lib.describe(b, h, w, levels, pyramid_storage(pyramid), pyramid_layout(pyramid))
    if pyramid_elements(pyramid) != desc.total_elements:
        raise ValueError(f"corr_lookup: coords {tuple(coords.shape)} do not match the pyramid "
                         f"({pyramid_elements(pyramid)} elements)")
    if desc.storage == _lib.RMD_S24:
        pyramid = s24_decode(pyramid)
    r = radius
    co = coords.float().permute(0, 2, 3, 1)
    delta = _delta(r, coords.device)
    out = []
    for i in range(levels):
        corr = _unpack(pyramid, desc, i)
        h2, w2 = corr.shape[-2:]
        cen = co.reshape(b, h, w, 1, 1, 2) / 2 ** i + delta
        cen = _normalise(cen, w2 - 1, h2 - 1).reshape(b * h * w, 2 * r + 1, 2 * r + 1, 2)
        corr = F.grid_sample(corr, cen, align_corners=True).view(b, h, w, -1)
        if (level_mask >> i) & 1:
            corr = torch.zeros_like(corr)
        out.append(corr)
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous().float()


# ---- on-the-fly lookup (raft_fs.py:13-87) -------------------------------------------------------

def _otf_split(workspace, b, c, h, w, levels):
    sizes = [(h >> i, w >> i) for i in range(levels)]
    n1 = b * c * h * w
    f1 = workspace[:n1].view(b, c, h, w)
    pyr, at = [], n1
    for hl, wl in sizes:
        k = b * c * hl * wl
        pyr.append(workspace[at: at + k].view(b, c, hl, wl))
        at += k
    if at != workspace.numel():
        raise ValueError(f"corr_otf_lookup: workspace of {workspace.numel()} floats does not match "
                         f"({b}, {c}, {h}, {w}) with {levels} levels")
    return f1, pyr


def corr_otf_prepare(fmap1, fmap2, levels, compute, scale):
    """raft_fs.py:16-31: fmap2 and its avg-pooled levels, kept with fmap1 * scale."""
    f2 = fmap2.float()
    parts = [(fmap1.float() * float(scale)).reshape(-1), f2.reshape(-1)]
    for _ in range(1, levels):
        f2 = F.avg_pool2d(f2, kernel_size=2, stride=2)
        parts.append(f2.reshape(-1))
    return torch.cat(parts)


def corr_otf_lookup(workspace, coords, channels, levels, compute, radius, level_mask):
    """raft_fs.py:33-87: grid-sample each pooled level at the window and dot it with fmap1."""
    b, _, h, w = coords.shape
    if workspace.dtype != torch.float32:
        raise ValueError("corr_otf_lookup: a CPU workspace comes from the CPU corr_otf_prepare (float32)")
    f1, pyr = _otf_split(workspace, b, channels, h, w, levels)
    c, r = channels, radius
    f1 = f1.permute(0, 2, 3, 1).reshape(b, h, w, c, 1)
    delta = _delta(r, coords.device).view(1, 2 * r + 1, 1, 2 * r + 1, 1, 2)
    co = coords.float().permute(0, 2, 3, 1).reshape(b, 1, h, 1, w, 2)
    out = []
    for i, f2 in enumerate(pyr):
        h2, w2 = f2.shape[-2:]
        cen = _normalise(co / 2 ** i + delta, w2 - 1, h2 - 1).reshape(b, (2 * r + 1) * h, (2 * r + 1) * w, 2)
        s = F.grid_sample(f2, cen, align_corners=True).view(b, c, 2 * r + 1, h, 2 * r + 1, w)
        s = s.permute(0, 3, 5, 2, 4, 1).reshape(b, h, w, (2 * r + 1) ** 2, c)
        corr = torch.matmul(s, f1).view(b, h, w, (2 * r + 1) ** 2)
        if (level_mask >> i) & 1:
            corr = torch.zeros_like(corr)
        out.append(corr)
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous().float()


# ---- DICL displacement stacks (corr/dicl.py:26-54, dicl_emb.py:51-89, raft_dicl_ml.py:294-315) ----

def _stack_f2(f2, coords, h, w, radius, level, norm_h, norm_w):
    b, c = f2.shape[:2]
    r = radius
    delta = _delta(r, coords.device).view(1, 2 * r + 1, 1, 2 * r + 1, 1, 2)
    co = coords.float().permute(0, 2, 3, 1).reshape(b, 1, h, 1, w, 2)
    cen = (co / 2 ** level if level else co) + delta
    cen = _normalise(cen, norm_w - 1, norm_h - 1).reshape(b, (2 * r + 1) * h, (2 * r + 1) * w, 2)
    s = F.grid_sample(f2, cen, align_corners=True).view(b, c, 2 * r + 1, h, 2 * r + 1, w)
    return s.permute(0, 2, 4, 1, 3, 5)                      # (B, 2r+1, 2r+1, C, h, w)


def dicl_stack(fmap1, fmap2, coords, radius, level, norm_h, norm_w, extra_delta):
    f1, f2 = fmap1.float(), fmap2.float()
    b, c, h, w = f1.shape
    d = 2 * radius + 1
    parts = [f1.view(b, 1, 1, c, h, w).expand(-1, d, d, -1, -1, -1),
             _stack_f2(f2, coords, h, w, radius, level, norm_h, norm_w)]
    if extra_delta:                                          # dicl_emb.py:82-86: delta as positional encoding
        parts.append(_delta(radius, f1.device).view(1, d, d, 2, 1, 1).expand(b, -1, -1, -1, h, w))
    return torch.cat(parts, dim=-3)


def dicl_stack_backward(grad, coords, channels, level_h, level_w, radius, level, norm_h, norm_w, extra_delta):
    b, _, h, w = coords.shape
    g = grad.float()
    g1 = g[:, :, :, :channels].sum(dim=(1, 2))
    with torch.enable_grad():
        f2 = torch.zeros(b, channels, level_h, level_w, device=grad.device, requires_grad=True)
        s = _stack_f2(f2, coords.detach(), h, w, radius, level, norm_h, norm_w)
        (g2,) = torch.autograd.grad(s, f2, g[:, :, :, channels:2 * channels])
    return g1, g2


def dicl_stack_int(fmap1, fmap2, ru, rv):
    """impls/dicl.py:212-238: integer-displacement volume, zeroed where the f2 half sums to 0."""
    f1, f2 = fmap1.float(), fmap2.float()
    b, c, h, w = f1.shape
    du, dv = 2 * ru + 1, 2 * rv + 1
    rows = []
    for i in range(du):
        cols = []
        for j in range(dv):
            di, dj = i - ru, j - rv
            w0, w1, h0, h1 = max(0, -di), min(w, w - di), max(0, -dj), min(h, h - dj)
            dw0, dw1, dh0, dh1 = max(0, di), min(w, w + di), max(0, dj), min(h, h + dj)
            a = F.pad(f1[:, :, h0:h1, w0:w1], (w0, w - w1, h0, h - h1))
            z = F.pad(f2[:, :, dh0:dh1, dw0:dw1], (w0, w - w1, h0, h - h1))
            cols.append(torch.cat((a, z), dim=1))
        rows.append(torch.stack(cols, dim=1))
    mvol = torch.stack(rows, dim=1)                          # (B, du, dv, 2C, h, w)
    valid = mvol[:, :, :, c:].detach().sum(dim=-3) != 0
    return mvol * valid.unsqueeze(3)


def _int_grads(grad, fmap1_like, fmap2, fn):
    with torch.enable_grad():
        f1 = torch.zeros_like(fmap1_like, dtype=torch.float32, requires_grad=True)
        f2 = fmap2.detach().float().requires_grad_(True)
        out = fn(f1, f2)
        return torch.autograd.grad(out, (f1, f2), grad.float())


def dicl_stack_int_backward(grad, fmap2, ru, rv):
    return _int_grads(grad, fmap2, fmap2, lambda a, z: dicl_stack_int(a, z, ru, rv))


# ---- backward warp (common/warp.py:5-33) --------------------------------------------------------

def _warp_grid(flow, h, w):
    cx = torch.arange(0, w, device=flow.device).view(1, w).expand(h, -1)
    cy = torch.arange(0, h, device=flow.device).view(h, 1).expand(-1, w)
    fpos = (torch.stack((cx, cy), dim=0).float() + flow.float()).permute(0, 2, 3, 1)
    return _normalise(fpos, max(w - 1, 0), max(h - 1, 0))


def warp_backwards(img2, flow, eps):
    b, c, h, w = img2.shape
    fpos = _warp_grid(flow, h, w)
    est = F.grid_sample(img2.float(), fpos, align_corners=True)
    mask = F.grid_sample(torch.ones(b, 1, h, w, device=img2.device), fpos, align_corners=True) > (1.0 - eps)
    return est * mask, mask


def warp_backwards_backward(grad, flow, eps):
    with torch.enable_grad():
        img = torch.zeros(grad.shape, device=grad.device, requires_grad=True)
        est, _ = warp_backwards(img, flow.detach(), eps)
        return torch.autograd.grad(est, img, grad.float())[0]


def dicl_stack_int_warped(fmap1, fmap2, flow, ru, rv):
    """impls/dicl.py:178-181 (warp_backwards of feat2 by the coarse flow, eps 1e-5) + :212-238."""
    warped, _ = warp_backwards(fmap2, flow.detach(), 1e-5)
    return dicl_stack_int(fmap1, warped, ru, rv)


def dicl_stack_int_warped_backward(grad, fmap2, flow, ru, rv):
    return _int_grads(grad, fmap2, fmap2, lambda a, z: dicl_stack_int_warped(a, z, flow, ru, rv))


# ---- displacement-aware projection (blocks/dicl.py:143-150) -------------------------------------

def _dap_view(x, weight):
    b, dd = x.shape[0], weight.shape[0]
    if x.numel() % (b * dd) or weight.numel() != dd * dd:
        raise ValueError(f"dap: x {tuple(x.shape)} does not hold {dd} displacement channels per batch")
    return x.float().reshape(b, dd, -1, 1), weight.float().reshape(dd, dd, 1, 1)


def dap(x, weight):
    xv, wv = _dap_view(x, weight)
    return F.conv2d(xv, wv).reshape(x.shape)                 # the reference's 1x1 nn.Conv2d, no bias


def dap_transpose(grad, weight):
    gv, wv = _dap_view(grad, weight)
    return F.conv2d(gv, wv.reshape(wv.shape[0], -1).t().reshape(wv.shape)).reshape(grad.shape)


def dap_weight_grad(grad, x, disp):
    b = x.shape[0]
    g, xx = grad.float().reshape(b, disp, -1), x.float().reshape(b, disp, -1)
    return torch.einsum("bop,bip->oi", g, xx)


# ---- flow heads (raft.py:98-190, 319-331) -------------------------------------------------------

def up8(mask, flow, temperature):
    b, c, h, w = flow.shape
    m = torch.softmax(mask.float().view(b, 1, 9, 8, 8, h, w) / temperature, dim=2)
    up = F.unfold(8 * flow.float(), (3, 3), padding=1).view(b, c, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(b, 2, h * 8, w * 8)


def up8_backward(grad, mask, flow, temperature):
    with torch.enable_grad():
        m = mask.detach().float().requires_grad_(True)
        f = flow.detach().float().requires_grad_(True)
        return torch.autograd.grad(up8(m, f, temperature), (m, f), grad.float())


def softargmax(cost, levels, radius, temperature):
    b = cost.shape[0]
    dd = (2 * radius + 1) ** 2
    if cost.shape[1] < levels * dd:
        raise ValueError(f"softargmax: {cost.shape[1]} channels < {levels} levels x {dd} displacements")
    rest = tuple(cost.shape[2:])
    c = cost.float().reshape(b, cost.shape[1], 1, -1)
    delta = _delta(radius, cost.device).view(1, dd, 2, 1)
    flows = []
    for lvl in range(levels):
        score = F.softmax(c[:, lvl * dd:(lvl + 1) * dd] / temperature, dim=1)
        flows.append(torch.sum(delta * 2 ** lvl * score, dim=1).reshape((b, 2) + rest))
    return torch.stack(flows)


def softargmax_backward(grad, cost, levels, radius, temperature):
    with torch.enable_grad():
        c = cost.detach().float().requires_grad_(True)
        return torch.autograd.grad(softargmax(c, levels, radius, temperature), c, grad.float())[0]


# ---- sequence losses (raft.py:616-644, loss/mlseq.py:34-67, raft_dicl_ctf_l3.py:430-473, dicl.py:436-472) ----

def loss_upsample(flow, shape, mode="bilinear"):
    """mlseq.py:59-67 / raft_dicl_ctf_l3.py:465-473: interpolate, then scale each component by its ratio."""
    _b, _c, fh, fw = flow.shape
    th, tw = shape[-2:]
    flow = F.interpolate(flow, (th, tw), mode=mode, align_corners=None if mode == "nearest" else True)
    flow[:, 0, :, :] = flow[:, 0, :, :] * (tw / fw)
    flow[:, 1, :, :] = flow[:, 1, :, :] * (th / fh)
    return flow


def sequence_loss_eager(flows, target, valid, masks, weights, ord, include_invalid, skip_empty, scale,
                        mode="bilinear"):
    """The reference's loop for any `ord` / upsampling mode -> (loss, per-prediction pixel counts)."""
    target = target.float()
    loss = target.new_zeros(())
    counts = []
    for flow, mask, weight in zip(flows, masks, weights):
        flow = flow.float()
        if flow.shape != target.shape:
            flow = loss_upsample(flow, target.shape, mode)              # mlseq.py:45-46
        if ord == "absmean":
            dist = (flow - target).abs().mean(dim=-3)                   # raft.py:627-628
        elif ord == "robust":
            dist = ((flow - target).abs().sum(dim=-3) + 1e-8) ** 0.4    # dicl.py:450-451
        else:
            dist = torch.linalg.vector_norm(flow - target, ord=ord, dim=-3)     # raft.py:630, mlseq.py:49
        mask = (valid if mask is None else mask).bool()
        if include_invalid:
            dist = dist * mask                                          # raft.py:633
        else:
            dist = dist[mask]                                           # raft.py:639, mlseq.py:52
        counts.append(dist.numel())
        if skip_empty and dist.numel() == 0:                            # raft_dicl_ctf_l3.py:453
            continue
        loss = loss + weight * dist.mean()                              # raft.py:642, mlseq.py:55
    return loss * scale, torch.tensor(counts, dtype=torch.int64)        # mlseq.py:57


_LOSS_ORD = {_lib.RMD_LOSS_L1: 1, _lib.RMD_LOSS_L2: 2, _lib.RMD_LOSS_ABSMEAN: "absmean", _lib.RMD_LOSS_ROBUST: "robust"}


def sequence_loss(flows, target, valid, masks, mask_index, weights, norm, include_invalid, skip_empty, scale):
    check_loss_args(flows, target, valid, masks, mask_index, weights, norm)
    own = [masks[i] if i >= 0 else None for i in mask_index]
    return sequence_loss_eager(flows, target, valid, own, weights, _LOSS_ORD[norm], include_invalid, skip_empty, scale)


def sequence_loss_backward(grad_loss, flows, target, valid, masks, mask_index, weights, counts, needs_grad, norm,
                           include_invalid, scale):
    with torch.enable_grad():
        fl = [f.detach().float().requires_grad_(bool(need)) for f, need in zip(flows, needs_grad)]
        # an empty selection contributes NaN to the loss but nothing to any gradient: skip it here
        loss, _ = sequence_loss(fl, target.detach(), valid, masks, mask_index, weights, norm, include_invalid, True,
                                scale)
        wanted = [f for f, need in zip(fl, needs_grad) if need]
        got = iter(torch.autograd.grad(loss, wanted, grad_loss.float().reshape(()), allow_unused=True)
                   if wanted and loss.requires_grad else [None] * len(wanted))
    out = []
    for f, need in zip(fl, needs_grad):
        if not need:
            out.append(target.new_empty((0,)))
            continue
        g = next(got)
        out.append(torch.zeros_like(f) if g is None else g)
    return out


# ---- flow metrics (metrics/epe.py:35-53, fl_all.py:29-44, aae.py:30-44, flow.py:32-36) ------------

def metric_angle(estimate, target):
    """aae.py:32-44 per pixel in radians, on the CHANNEL axis (dim -3) and in float64 from the inputs as
    they are: what the reference evaluates when it is handed channel-last views."""
    u_est, v_est = estimate.double().unbind(-3)
    u_tgt, v_tgt = target.double().unbind(-3)
    n_est = torch.sqrt(torch.square(u_est) + torch.square(v_est))
    n_tgt = torch.sqrt(torch.square(u_tgt) + torch.square(v_tgt))
    cos = (u_est * u_tgt + v_est * v_tgt + 1) / (n_est * n_tgt + 1)
    return torch.arccos(torch.clamp(cos, -1.0, 1.0))


def flow_metrics_eager(estimate, target, valid, distances=(1, 3, 5), fl=(3, 0.05), ord=2):
    """The reference's expressions one metric after the other, boolean indexing included (each
    `epe[valid]` launches nonzero and waits for the host on a GPU) -> dict of 0-dim tensors.  A batch
    or a single instance, like the reference's classes."""
    out = {}
    epe = torch.linalg.vector_norm(estimate - target, ord=2, dim=-3)[valid]         # epe.py:39-42
    out["epe/mean"] = epe.mean()
    for d in distances:
        out[f"epe/{d}px"] = (epe <= d).float().mean()                               # epe.py:51
    epe = torch.linalg.vector_norm(estimate - target, ord=2, dim=-3)[valid]         # fl_all.py:33-38
    tgt = torch.linalg.vector_norm(target, ord=2, dim=-3)[valid]
    out["fl-all"] = torch.logical_and(epe > fl[0], epe > fl[1] * tgt).float().mean()     # fl_all.py:41-44
    out["aae"] = torch.rad2deg(metric_angle(estimate, target).mean())               # aae.py:44
    out["flow-magnitude"] = torch.linalg.vector_norm(estimate, ord=ord, dim=-3).mean()   # flow.py:34
    return out


def flow_metrics(estimates, target, valid, distances, fl_abs, fl_rel, mag_ord):
    """The slot table of include/rmd.h from the same expressions, every sample on its own: selections
    (`where`), never products, so a NaN outside the mask stays out of the masked sums."""
    check_metric_args(estimates, target, valid, distances, mag_ord)
    target = target.detach().float()
    mask = valid.detach() != 0
    b, _, h, w = target.shape
    tgt = torch.linalg.vector_norm(target, ord=2, dim=-3)
    zero = target.new_zeros((), dtype=torch.float64)

    def total(x, where=None):
        x = x.double()
        return (x if where is None else torch.where(where, x, zero)).sum(dim=(-2, -1))

    rows = []
    for est in estimates:
        est = est.detach().float()
        epe = torch.linalg.vector_norm(est - target, ord=2, dim=-3)
        ang = metric_angle(est, target)
        slots = [torch.full((b,), float(h * w), dtype=torch.float64, device=target.device), total(mask),
                 total(epe, mask), total((epe > fl_abs) & (epe > fl_rel * tgt) & mask), total(ang), total(ang, mask),
                 total(torch.linalg.vector_norm(est, ord=mag_ord, dim=-3)), total((~torch.isfinite(est)).any(dim=-3))]
        slots += [total((epe <= d) & mask) for d in distances]
        slots += [zero.expand(b)] * (_lib.METRICS_SLOTS - len(slots))
        rows.append(torch.stack(slots, dim=-1))
    return torch.stack(rows)


# ---- DICL flow head (impls/dicl.py:31-85, 194-195, 202) --------------------------------------------

def flow_regression(cost):
    """FlowRegression.forward, dicl.py:59-85 -> (B, 2, h, w)."""
    batch, du, dv, h, w = cost.shape
    ru, rv = (du - 1) // 2, (dv - 1) // 2
    disp_u = torch.arange(-ru, ru + 1, device=cost.device, dtype=torch.float32)     # dicl.py:64-66
    disp_u = disp_u.view(du, 1).expand(-1, dv)
    disp_v = torch.arange(-rv, rv + 1, device=cost.device, dtype=torch.float32)     # dicl.py:69-71
    disp_v = disp_v.view(1, dv).expand(du, -1)
    disp = torch.stack((disp_u, disp_v), dim=0).view(1, 2, du, dv, 1, 1)            # dicl.py:74-75
    prob = F.softmax(cost.reshape(batch, du * dv, h, w), dim=1)                     # dicl.py:78-79
    prob = prob.view(batch, 1, du, dv, h, w)
    return (prob * disp).sum(dim=(2, 3))                                            # dicl.py:83


def flow_entropy(cost, eps=1e-9):
    """FlowEntropy.forward, dicl.py:39-50 -> (B, h, w)."""
    batch, du, dv, h, w = cost.shape
    x = F.softmax(cost.reshape(batch, du * dv, h, w), dim=1).view(batch, du, dv, h, w)     # dicl.py:43-45
    entropy = (-x * torch.clamp(x, eps, 1.0 - eps).log()).sum(dim=(1, 2))           # dicl.py:48
    return entropy / math.log(du * dv)                                              # dicl.py:50


def dicl_flow_head_eager(cost, flow_coarse, eps):
    """The reference's two modules and its coarse-flow addition, one after the other (dicl.py:194-195,
    202) -> (flow, entropy (B, 1, h, w))."""
    batch, _, _, h, w = cost.shape
    flow = flow_regression(cost)
    flow = flow + flow_coarse if flow_coarse is not None else flow
    return flow, flow_entropy(cost, eps).view(batch, 1, h, w)


def dicl_flow_head(cost, flow_coarse, eps):
    check_head_args(cost, flow_coarse, eps)
    return torch.cat(dicl_flow_head_eager(cost.float(), None if flow_coarse is None else flow_coarse.float(), eps), 1)


def dicl_flow_head_backward(grad, cost, eps):
    check_head_args(cost, None, eps, grad)
    with torch.enable_grad():
        c = cost.detach().float().requires_grad_(True)
        return torch.autograd.grad(dicl_flow_head(c, None, eps), c, grad.float())[0]


# ---- hidden-state upsampler: local cross-attention (common/hsup.py:71-92) --------------------------

def _window_views(t, window, h, w):
    """(B, c, h2, w2) -> (B, c, wy*wx, h, w): the zero-padded window of every coarse cell, repeated over
    the fine pixels of the cell (hsup.py:71-74, :76-79)."""
    batch, c, h2, w2 = t.shape
    n = window[0] * window[1]
    t = F.unfold(t, kernel_size=window, padding=(window[0] // 2, window[1] // 2))
    t = t.view(batch, c, n, h2, 1, w2, 1).expand(-1, -1, -1, -1, h // h2, -1, w // w2)
    return t.reshape(batch, c, n, h, w)


def local_cross_attn_eager(q, k, v, window=(3, 3)):
    """The attention of HUpCrossAttn.forward, hsup.py:66-92, op for op -> (B, cv, h, w)."""
    batch, ck, h, w = q.shape
    n = window[0] * window[1]
    k = _window_views(k, window, h, w)
    v = _window_views(v, window, h, w)
    k = k.permute(0, 3, 4, 1, 2)                                        # hsup.py:82-83
    q = q.permute(0, 2, 3, 1).view(batch, h, w, 1, ck)
    a = F.softmax(torch.matmul(q, k).squeeze(3), dim=-1)                # hsup.py:85-86
    a = a.permute(0, 3, 1, 2).view(batch, 1, n, h, w)                   # hsup.py:89-90
    return (a * v).sum(dim=2)                                           # hsup.py:92


def local_cross_attn(q, k, v, win_y, win_x):
    check_attn_args(q, k, v, win_y, win_x)
    return local_cross_attn_eager(q.float(), k.float(), v.float(), (win_y, win_x))


def local_cross_attn_backward(grad, q, k, v, win_y, win_x):
    check_attn_args(q, k, v, win_y, win_x, grad)
    with torch.enable_grad():
        ins = [t.detach().float().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad(local_cross_attn(*ins, win_y, win_x), ins, grad.float())


# ---- fused dicl-1x1 cost (corr/dicl_1x1.py:8-30, 51-79) --------------------------------------------

def dicl_match_1x1(fmap1, fmap2, coords, radius, weights, biases, compute):
    """The stack, then the folded MatchingNet1x1 as 1x1 convolutions: fp32 whatever the compute mode."""
    check_match_args(fmap1, fmap2, coords, radius, weights, biases, compute)
    b, c, h, w = fmap1.shape
    d = 2 * radius + 1
    x = dicl_stack(fmap1.detach(), fmap2.detach(), coords.detach(), radius, 0, h, w, False).reshape(b * d * d, 2 * c, h, w)
    for wt, t in zip(weights[:3], biases[:3]):
        x = F.relu(F.conv2d(x, wt.detach().float()[:, :, None, None], t.detach().float().reshape(-1)))
    x = F.conv2d(x, weights[3].detach().float().reshape(1, -1, 1, 1), biases[3].detach().float().reshape(1))
    return x.view(b, d, d, h, w)


def dicl_match_1x1_train(fmap1, fmap2, coords, radius, weights, biases):
    """The same composite with its ATen graph recorded (AutogradCPU): the stack, then 1x1 convolutions."""
    check_match_args(fmap1, fmap2, coords, radius, weights, biases, _lib.RMD_BF16X3)
    b, c, h, w = fmap1.shape
    d = 2 * radius + 1
    x = dicl_stack(fmap1.float(), fmap2.float(), coords.detach(), radius, 0, h, w, False).reshape(b * d * d, 2 * c, h, w)
    for wt, t in zip(weights[:3], biases[:3]):
        x = F.relu(F.conv2d(x, wt.float()[:, :, None, None], t.float().reshape(-1)))
    x = F.conv2d(x, weights[3].float().reshape(1, -1, 1, 1), biases[3].float().reshape(1))
    return x.view(b, d, d, h, w)


def dicl_match_1x1_backward(grad, fmap1, fmap2, coords, radius, weights, biases, needs_grad):
    """torch.autograd.grad of dicl_match_1x1_train's composite; (0,) tensors for a skipped group."""
    check_match_backward_args(grad, fmap1, fmap2, coords, radius, weights, biases, needs_grad)
    needs = [needs_grad[0], needs_grad[1]] + [needs_grad[2]] * 8
    with torch.enable_grad():
        ins = [t.detach().float().requires_grad_(True) for t in (fmap1, fmap2, *weights, *biases)]
        out = dicl_match_1x1_train(ins[0], ins[1], coords.detach(), radius, ins[2:6], ins[6:10])
        wanted = [t for t, need in zip(ins, needs) if need]
        got = iter(torch.autograd.grad(out, wanted, grad.float()) if wanted else ())
    return [next(got) if need else t.new_empty((0,)) for t, need in zip(ins, needs)]


# ---- fused SepConvGRU (raft.py:228-259) -------------------------------------------------------------

def sepconv_gru(h, x, weights, biases, compute):
    """The reference's own composition, fp32 whatever the compute mode: the horizontal half (1x5, padding
    (0, 2)), then the vertical one (5x1, padding (2, 0))."""
    check_gru_args(h, x, weights, biases, compute)
    h, x = h.detach().float(), x.detach().float()
    ws, bs = [t.detach().float() for t in weights], [t.detach().float().reshape(-1) for t in biases]
    for i, pad in ((0, (0, 2)), (3, (2, 0))):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(F.conv2d(hx, ws[i], bs[i], padding=pad))
        r = torch.sigmoid(F.conv2d(hx, ws[i + 1], bs[i + 1], padding=pad))
        q = torch.tanh(F.conv2d(torch.cat((r * h, x), dim=1), ws[i + 2], bs[i + 2], padding=pad))
        h = (1.0 - z) * h + z * q
    return h


# ---- fused k x k convolutions (raft.py:193-225, 262-273, 299-331) ------------------------------------

def conv2d_act(x0, x1, weight, bias, act, compute):
    """F.conv2d over cat(x0, x1) with 'same' padding, then the activation; fp32 whatever the compute mode."""
    _, _, _, kh, kw = check_conv_args(x0, x1, weight, bias, act, compute)
    x = x0.detach().float() if x1 is None else torch.cat([x0.detach().float(), x1.detach().float()], dim=1)
    out = F.conv2d(x, weight.detach().float(), bias.detach().float().reshape(-1), padding=(kh // 2, kw // 2))
    return F.relu(out) if act else out


def conv2d_act_train(x0, x1, weight, bias, act):
    """The same composite with its ATen graph recorded (AutogradCPU)."""
    _, _, _, kh, kw = check_conv_args(x0, x1, weight, bias, act, _lib.RMD_BF16X3)
    x = x0.float() if x1 is None else torch.cat([x0.float(), x1.float()], dim=1)
    out = F.conv2d(x, weight.float(), bias.float().reshape(-1), padding=(kh // 2, kw // 2))
    return F.relu(out) if act else out


def conv2d_act_backward(grad, y, x0, x1, weight, act, needs_grad):
    """torch.autograd.grad of conv2d_act_train's composite, its ReLU masked by the y given; (0,) tensors for a
    skipped gradient."""
    _, _, cout, kh, kw = check_conv_backward_args(grad, y, x0, x1, weight, act, needs_grad)
    needs = [needs_grad[0], needs_grad[1] and x1 is not None, needs_grad[2], needs_grad[3]]
    g = grad.detach().float()
    if act:
        g = torch.where(y.detach() <= 0, torch.zeros_like(g), g)        # !(y <= 0) keeps the gradient: NaN too
    with torch.enable_grad():
        ins = [None if t is None else t.detach().float().requires_grad_(True)
               for t in (x0, x1, weight, weight.new_zeros(cout))]
        out = conv2d_act_train(ins[0], ins[1], ins[2], ins[3], 0)
        wanted = [t for t, need in zip(ins, needs) if need]
        got = iter(torch.autograd.grad(out, wanted, g) if wanted else ())
    return [next(got) if need else x0.new_empty((0,), dtype=torch.float32) for need in needs]


def motion_encoder(flow, corr, weights, biases, compute):
    """BasicMotionEncoder.forward (raft.py:214-225), the reference's own composition in fp32."""
    check_encoder_args(flow, corr, weights, biases, compute)
    flow, corr = flow.detach().float(), corr.detach().float()
    ws, bs = [t.detach().float() for t in weights], [t.detach().float().reshape(-1) for t in biases]
    cor = F.relu(F.conv2d(corr, ws[0], bs[0]))
    cor = F.relu(F.conv2d(cor, ws[1], bs[1], padding=1))
    flo = F.relu(F.conv2d(flow, ws[2], bs[2], padding=3))
    flo = F.relu(F.conv2d(flo, ws[3], bs[3], padding=1))
    combined = F.relu(F.conv2d(torch.cat([cor, flo], dim=1), ws[4], bs[4], padding=1))
    return torch.cat([combined, flow], dim=1)


# ---- the feature / context encoder (encoders/raft/s3.py:8-72, blocks/raft.py:13-46) -------------------

def _planes(t):
    return t.detach().float()[:, :, None, None]


def conv2d_norm_act(x, scale, shift, weight, bias, residual, stride, act, compute):
    """F.conv2d with padding k / 2 over relu(x scale + shift), the activation, then relu(. + residual); fp32
    whatever the compute mode."""
    check_norm_conv_args(x, scale, shift, weight, bias, residual, stride, act, compute)
    _, _, kh, kw = weight.shape
    x = x.detach().float()
    if scale is not None:
        x = F.relu(x * _planes(scale) + _planes(shift))
    out = F.conv2d(x, weight.detach().float(), bias.detach().float().reshape(-1), stride=stride,
                   padding=(kh // 2, kw // 2))
    out = F.relu(out) if act else out
    return out if residual is None else F.relu(out + residual.detach().float())


def instance_norm_stats(x, eps):
    """scale = 1 / sqrt(var + eps) (biased variance) and shift = -mean scale per (sample, channel); the moments in
    float64, as the HIP kernel accumulates them."""
    check_stats_args(x, eps)
    var, mean = torch.var_mean(x.detach().double(), dim=(2, 3), unbiased=False)
    scale = torch.rsqrt(var + eps)
    return scale.float(), (-mean * scale).float()


def residual_join(y, y_scale, y_shift, x, x_scale, x_shift):
    """relu(xs + relu(ys)), ys = y y_scale + y_shift, xs = x x_scale + x_shift (each as given without statistics)."""
    check_join_args(y, y_scale, y_shift, x, x_scale, x_shift)
    y, x = y.detach().float(), x.detach().float()
    if y_scale is not None:
        y = y * _planes(y_scale) + _planes(y_shift)
    if x_scale is not None:
        x = x * _planes(x_scale) + _planes(x_shift)
    return F.relu(x + F.relu(y))


def feature_encoder(x, weights, biases, norm, compute):
    """FeatureEncoder.forward (s3.py:51-72) with the norm type none or instance, the reference's own composition
    in fp32."""
    check_feature_encoder_args(x, weights, biases, norm, compute)
    ws, bs = [t.detach().float() for t in weights], [t.detach().float().reshape(-1) for t in biases]

    def nrm(t):
        return F.instance_norm(t, eps=INSTANCE_NORM_EPS) if norm else t

    x = F.relu(nrm(F.conv2d(x.detach().float(), ws[0], bs[0], stride=2, padding=3)))
    g = 1
    for stride in (1, 1, 2, 1, 2, 1):
        y = F.relu(nrm(F.conv2d(x, ws[g], bs[g], stride=stride, padding=1)))
        y = F.relu(nrm(F.conv2d(y, ws[g + 1], bs[g + 1], padding=1)))
        if stride == 2:
            x = nrm(F.conv2d(x, ws[g + 2], bs[g + 2], stride=2))
        x = F.relu(x + y)
        g += 3 if stride == 2 else 2
    return F.conv2d(x, ws[15], bs[15])


# ---- the k x k MatchingNet (blocks/dicl.py:93-118) ----------------------------------------------------

def mnet_tail(x, weight5, bias5, weight6, bias6, compute):
    """relu(conv_transpose2d(x, W5', t5, stride 2, padding 1)), then the 3 x 3 convolution to one channel; fp32
    whatever the compute mode."""
    c3, c4 = check_tail_args(x, weight5, bias5, weight6, bias6, compute)
    u = F.relu(F.conv_transpose2d(x.detach().float(), weight5.detach().float(), bias5.detach().float().reshape(-1),
                                  stride=2, padding=1))
    return F.conv2d(u, weight6.detach().float().reshape(1, c4, 3, 3), bias6.detach().float().reshape(-1), padding=1)[:, 0]


def matching_net(mvol, weights, biases, group, compute):
    """MatchingNet.forward (blocks/dicl.py:111-118) on the folded parameters, the reference's own composition in
    fp32; `group` only sizes the HIP workspace."""
    check_mnet_args(mvol, weights, biases, group, compute)
    b, du, dv, c_in, ht, wd = mvol.shape
    ws, bs = [t.detach().float() for t in weights], [t.detach().float().reshape(-1) for t in biases]
    x = mvol.detach().float().reshape(b * du * dv, c_in, ht, wd)
    for i, stride in enumerate((1, 2, 1, 1)):
        x = F.relu(F.conv2d(x, ws[i], bs[i], stride=stride, padding=1))
    return mnet_tail(x, ws[4], bs[4], ws[5], bs[5], compute).reshape(b, du, dv, ht, wd)


# ---- registration ------------------------------------------------------------------------------
#
# The CPU kernel of an operator is the function of its name in this module.

_KERNELS = {name: globals().get(name) for name in _OPS}
assert all(_KERNELS.values()), f"every rmd operator needs a CPU kernel: {[n for n, f in _KERNELS.items() if not f]}"

for _name, _fn in _KERNELS.items():
    LIB.impl(_name, _fn, "CPU")
    if _name not in ("flow_metrics", "dicl_match_1x1", "sepconv_gru", "conv2d_act", "motion_encoder",
                     "conv2d_norm_act", "instance_norm_stats", "residual_join", "feature_encoder", "matching_net",
                     "mnet_tail"):     # not differentiable: library.py's Autograd kernel serves every device
        LIB.impl(_name, _fn, "AutogradCPU")
