"""Oracle: RAFT all-pairs correlation, pooled pyramid and windowed bilinear lookup (numpy).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Arithmetic is carried out in the dtype of the
inputs (float64 for checking, float32 for the timed CPU baseline).

Reference semantics restated here (qzed/raft-meets-dicl v2):
  * corr0[b,p,q] = sum_c f1[b,c,p] f2[b,c,q] / sqrt(C)           src/models/impls/raft.py:26-33
  * level l = avg_pool2d(level l-1, 2, 2) over the target dims, floor sizes   raft.py:38-47
  * lookup: level i is sampled at (x/2^i + dx, y/2^i + dy), dx,dy in {-r..r}, bilinear,
    align_corners=True, zero padding per tap                        raft.py:57-80
  * output channel = i*(2r+1)^2 + a*(2r+1) + b with x-offset a-r, y-offset b-r
    (meshgrid(dx, dy, indexing='ij'))                                raft.py:57-59,83,92-95
  * levels listed in mask_costs (as index i+3) are zeroed            raft.py:86-87
  * a level with height or width 1 divides by zero in the [-1,1] normalisation
    (raft.py:73-74) and yields NaN for every query                   (fixture corr_b1_c16_12x20_nan)
  * raft/fs: fmap2 is avg-pooled instead of the volume, no 1/sqrt(C)  src/models/impls/raft_fs.py:13-87
  * backward (autograd of raft.py:18-95), in the stages of include/rmd.h: the pyramid gradient G per
    lookup (corr_lookup_grad_levels) in the chunked target order (corr_grad_pack / corr_grad_unpack),
    the pooled targets P (corr_pool_targets), the unpooling (corr_unpool_targets); corr_lookup_backward
    composes them.  A 1-pixel level carries no gradient.

The bilinear lookup is restated in pixel coordinates (no [-1,1] round trip) with one weight set
per query and level: all (2r+1)^2 offsets are integers, so every tap shares frac(x/2^i),
frac(y/2^i).
"""

import collections

import numpy as np


def pyramid_level_shapes(h, w, levels):
    """Floor-sized level shapes of the avg-pool pyramid (raft.py:38-47)."""
    shapes = [(h, w)]
    for _ in range(1, levels):
        h, w = h // 2, w // 2
        shapes.append((h, w))
    return shapes


def corr_volume(fmap1, fmap2):
    """(B,C,H,W) x2 -> (B, H*W, H, W): raft.py:26-33.

    fmap1 may hold any subset of query pixels (B,C,h1,w1); targets always follow fmap2's grid.
    """
    b, c, h1, w1 = fmap1.shape
    h, w = fmap2.shape[-2:]
    f1 = fmap1.reshape(b, c, h1 * w1)
    f2 = fmap2.reshape(b, c, h * w)
    corr = np.matmul(f1.transpose(0, 2, 1), f2)
    corr = corr / np.sqrt(np.asarray(c, dtype=fmap1.dtype))
    return corr.reshape(b, h1 * w1, h, w)


def _avg_pool2(x):
    """2x2/2 average pool over the last two dims, floor sizes (F.avg_pool2d, raft.py:42)."""
    h2, w2 = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., : 2 * h2, : 2 * w2]
    return 0.25 * (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2])


def corr_pyramid(fmap1, fmap2, levels):
    """List of levels, each (B, H*W, H_i, W_i): raft.py:18-47."""
    pyr = [corr_volume(fmap1, fmap2)]
    for _ in range(1, levels):
        pyr.append(_avg_pool2(pyr[-1]))
    return pyr


def _bilinear_window(maps, cx, cy, r):
    """Sample the (2r+1)^2 integer-offset window of each query's own map.

    maps: (B, P, Hl, Wl)   one target map per query
    cx, cy: (B, P)         centre in this level's pixel coordinates
    returns (B, P, 2r+1 [x-offset a], 2r+1 [y-offset b])
    """
    bsz, p, hl, wl = maps.shape
    x0 = np.floor(cx)
    y0 = np.floor(cy)
    fx = (cx - x0)[..., None, None]
    fy = (cy - y0)[..., None, None]
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    k = 2 * r + 2
    offs = np.arange(-r, r + 2)
    xs = x0[..., None] + offs                                  # (B,P,k) patch columns
    ys = y0[..., None] + offs                                  # (B,P,k) patch rows
    vx = (xs >= 0) & (xs < wl)
    vy = (ys >= 0) & (ys < hl)
    xs_c = np.clip(xs, 0, wl - 1)
    ys_c = np.clip(ys, 0, hl - 1)
    bi = np.arange(bsz)[:, None, None, None]
    pi = np.arange(p)[None, :, None, None]
    patch = maps[bi, pi, ys_c[..., :, None], xs_c[..., None, :]]          # (B,P,k rows,k cols)
    patch = patch * (vy[..., :, None] & vx[..., None, :])                 # zero padding per tap
    top = patch[..., :-1, :]                                              # rows y0-r .. y0+r
    bot = patch[..., 1:, :]
    # out[a, b] (a = x index, b = y index)
    v00 = top[..., :, :-1]
    v01 = top[..., :, 1:]
    v10 = bot[..., :, :-1]
    v11 = bot[..., :, 1:]
    one = np.asarray(1, dtype=maps.dtype)
    out_yx = ((one - fx) * (one - fy) * v00 + fx * (one - fy) * v01 +
              (one - fx) * fy * v10 + fx * fy * v11)                      # (B,P,b,a)
    del k
    return np.swapaxes(out_yx, -1, -2)                                    # (B,P,a,b)


def corr_lookup(pyramid, coords, radius, mask_costs=()):
    """Windowed bilinear lookup over the pyramid -> (B, L*(2r+1)^2, H, W): raft.py:49-95.

    pyramid: list of (B, H*W, H_i, W_i);  coords: (B,2,H,W), ch0 = x, ch1 = y (level-0 pixels).
    """
    b, _, h, w = coords.shape
    d = 2 * radius + 1
    cx = coords[:, 0].reshape(b, h * w)
    cy = coords[:, 1].reshape(b, h * w)
    out = []
    for i, lvl in enumerate(pyramid):
        hl, wl = lvl.shape[-2:]
        if i + 3 in mask_costs:
            o = np.zeros((b, h * w, d, d), dtype=lvl.dtype)
        elif hl < 2 or wl < 2:
            o = np.full((b, h * w, d, d), np.nan, dtype=lvl.dtype)
        else:
            s = np.asarray(2.0 ** i, dtype=lvl.dtype)
            o = _bilinear_window(lvl, cx / s, cy / s, radius)
        out.append(o.reshape(b, h * w, d * d))
    out = np.concatenate(out, axis=-1)                                    # (B, P, L*d*d)
    return np.ascontiguousarray(out.transpose(0, 2, 1).reshape(b, -1, h, w))


def _pool_fmap(f):
    return _avg_pool2(f)


def corr_lookup_fs(fmap1, fmap2, coords, levels, radius, mask_costs=(), scale=None):
    """On-the-fly lookup: dot(fmap1, bilinear(pooled fmap2)) — raft_fs.py:13-87.

    ``scale`` multiplies the result: None → 1 (raft_fs has no 1/sqrt(C)); corr/dot.py:55-57 uses
    1/sqrt(C), raft.CorrBlock equals this times 1/sqrt(C).
    """
    b, c, h, w = fmap1.shape
    d = 2 * radius + 1
    f2s = [fmap2]
    for _ in range(1, levels):
        f2s.append(_pool_fmap(f2s[-1]))
    cx = coords[:, 0].reshape(b, h * w)
    cy = coords[:, 1].reshape(b, h * w)
    f1 = fmap1.reshape(b, c, h * w)
    out = []
    for i, f2 in enumerate(f2s):
        hl, wl = f2.shape[-2:]
        if i + 3 in mask_costs:
            o = np.zeros((b, h * w, d * d), dtype=fmap1.dtype)
        elif hl < 2 or wl < 2:
            o = np.full((b, h * w, d * d), np.nan, dtype=fmap1.dtype)
        else:
            s = np.asarray(2.0 ** i, dtype=fmap1.dtype)
            samp = _sample_features(f2, cx / s, cy / s, radius)           # (B,C,P,a,b)
            o = np.einsum("bcp,bcpxy->bpxy", f1, samp).reshape(b, h * w, d * d)
        if scale is not None:
            o = o * np.asarray(scale, dtype=o.dtype)
        out.append(o)
    out = np.concatenate(out, axis=-1)
    return np.ascontiguousarray(out.transpose(0, 2, 1).reshape(b, -1, h, w))


def _sample_features(f, cx, cy, r, sx=1.0, sy=1.0):
    """Bilinear zero-padded samples of feature map f (B,C,Hl,Wl) at ((cx+a-r)*sx, (cy+b-r)*sy).

    returns (B, C, P, 2r+1 [a], 2r+1 [b]).  With sx = sy = 1 all taps share one weight set.
    """
    bsz, c, hl, wl = f.shape
    d = 2 * r + 1
    off = np.arange(-r, r + 1, dtype=f.dtype)
    px = (cx[..., :, None] + off) * np.asarray(sx, dtype=f.dtype)          # (B,P,a)
    py = (cy[..., :, None] + off) * np.asarray(sy, dtype=f.dtype)          # (B,P,b)
    px = np.broadcast_to(px[..., :, None], px.shape + (d,))                # (B,P,a,b)
    py = np.broadcast_to(py[..., None, :], py.shape[:-1] + (d, d))
    x0 = np.floor(px)
    y0 = np.floor(py)
    fx = px - x0
    fy = py - y0
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    bi = np.arange(bsz)[:, None, None, None]
    out = np.zeros((bsz, c) + px.shape[1:], dtype=f.dtype)
    one = np.asarray(1, dtype=f.dtype)
    for dy, wy in ((0, one - fy), (1, fy)):
        for dx, wx in ((0, one - fx), (1, fx)):
            xx = x0 + dx
            yy = y0 + dy
            v = (xx >= 0) & (xx < wl) & (yy >= 0) & (yy < hl)
            vals = f[bi, :, np.clip(yy, 0, hl - 1), np.clip(xx, 0, wl - 1)]   # (B,P,a,b,C)
            out += np.moveaxis(vals * (wx * wy * v)[..., None], -1, 1)
    return out


# ---- Backward of raft.CorrBlock, stage by stage (include/rmd.h, "Backward of the RAFT correlation") --
#
# G_l = d(sum(out * grad_out)) / d(pyramid level l) per lookup; all levels packed in the chunked order
# of rmd.h as a (T' x N) matrix G; P = pooled fmap2 / sqrt(C) in the same target order; then
#   grad_fmap1 = P G,   dP = fmap1 G^T,   grad_fmap2 = unpool(dP) / sqrt(C).

CorrGradGeometry = collections.namedtuple("CorrGradGeometry", "lh lw nch coff TC targets")

# beyond this level coordinate no (2r+2)^2 patch meets a level (H, W < 16384): the query adds nothing
_FAR = 30000.0


def corr_grad_geometry(h, w, levels):
    """Chunked target order of G (rmd.h): per level H_l, W_l, nch(l) = ceil(W_l / 8) chunks per target
    row and coff(l) = sum_{l' < l} H_l' nch(l'), the first chunk; TC chunks and T' = 8 TC padded targets."""
    lh = [h >> l for l in range(levels)]
    lw = [w >> l for l in range(levels)]
    nch = [-(-x // 8) for x in lw]
    coff = [sum(lh[k] * nch[k] for k in range(l)) for l in range(levels)]
    tc = sum(a * n for a, n in zip(lh, nch))
    return CorrGradGeometry(lh, lw, nch, coff, tc, 8 * tc)


def corr_lookup_grad_levels(coords, levels, radius, grad_out, mask_costs=(), dtype=None):
    """Gradient of sum(out * grad_out) with respect to each pyramid level, for one lookup: a list of
    (B, N, H_l, W_l) arrays (transpose of grid_sample at raft.py:80, zero padding per tap).

    coords (B, 2, H, W); grad_out (B, L (2r+1)^2, H, W) in the lookup's channel order.  A level in
    mask_costs (as l + 3, raft.py:86-87) and a level with H_l < 2 or W_l < 2 (NaN in the reference,
    raft.py:73-74) are all zero.  A query whose level coordinate is NaN, +-inf or beyond +-30000 adds
    nothing.  Arithmetic in ``dtype`` (default: grad_out's).
    """
    dtype = np.dtype(grad_out.dtype if dtype is None else dtype)
    b, _, h, w = coords.shape
    n = h * w
    d, k = 2 * radius + 1, 2 * radius + 2
    g = np.asarray(grad_out, dtype=dtype).reshape(b, levels, d, d, n)         # (B, L, a [x], b [y], N)
    cx = np.asarray(coords[:, 0], dtype=dtype).reshape(b, n)
    cy = np.asarray(coords[:, 1], dtype=dtype).reshape(b, n)
    one = np.asarray(1, dtype=dtype)
    bi = np.broadcast_to(np.arange(b)[:, None, None, None], (b, n, k, k))
    pi = np.broadcast_to(np.arange(n)[None, :, None, None], (b, n, k, k))
    out = []
    for l, (hl, wl) in enumerate(pyramid_level_shapes(h, w, levels)):
        gl = np.zeros((b, n, hl, wl), dtype=dtype)
        out.append(gl)
        if l + 3 in mask_costs or hl < 2 or wl < 2:
            continue
        s = np.asarray(2.0 ** l, dtype=dtype)
        lx, ly = cx / s, cy / s
        far = ~(np.isfinite(lx) & np.isfinite(ly))
        far |= (np.abs(np.where(far, 0, lx)) > _FAR) | (np.abs(np.where(far, 0, ly)) > _FAR)
        lx, ly = np.where(far, 0, lx).astype(dtype), np.where(far, 0, ly).astype(dtype)
        x0, y0 = np.floor(lx), np.floor(ly)
        fx, fy = (lx - x0)[..., None, None], (ly - y0)[..., None, None]
        # patch[j, i]: gradient at target (y0 - r + j, x0 - r + i), j, i = 0 .. 2r+1; tap (a, b) sits at
        # (y0 - r + b, x0 - r + a) and spreads over the four corners with the forward's weights
        gt = np.moveaxis(g[:, l], -1, 1).swapaxes(-1, -2)                     # (B, N, b [y], a [x])
        patch = np.zeros((b, n, k, k), dtype=dtype)
        patch[..., :-1, :-1] += (one - fy) * (one - fx) * gt
        patch[..., :-1, 1:] += (one - fy) * fx * gt
        patch[..., 1:, :-1] += fy * (one - fx) * gt
        patch[..., 1:, 1:] += fy * fx * gt
        offs = np.arange(k) - radius
        yy = np.broadcast_to((y0.astype(np.int64)[..., None] + offs)[..., :, None], (b, n, k, k))
        xx = np.broadcast_to((x0.astype(np.int64)[..., None] + offs)[..., None, :], (b, n, k, k))
        v = (yy >= 0) & (yy < hl) & (xx >= 0) & (xx < wl) & ~far[..., None, None]
        gl[bi[v], pi[v], yy[v], xx[v]] = patch[v]                             # one patch per query: no repeats
    return out


def corr_grad_pack(levels_list):
    """Per-level (B, N, H_l, W_l) arrays -> G (B, TC, N, 8) in the chunked order of rmd.h: element
    (b, target (l, y, x), query p) at ((b TC + coff(l) + y nch(l) + x / 8) N + p) 8 + x % 8; pad targets
    (x >= W_l in a row's last chunk) are zero."""
    parts = []
    for gl in levels_list:
        b, n, hl, wl = gl.shape
        nch = -(-wl // 8)
        pad = np.zeros((b, n, hl, nch * 8), dtype=gl.dtype)
        pad[..., :wl] = gl
        parts.append(pad.reshape(b, n, hl * nch, 8).transpose(0, 2, 1, 3))
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def corr_grad_unpack(G, b, h, w, levels):
    """Inverse of corr_grad_pack: G (any shape of B TC N 8 elements) -> list of (B, N, H_l, W_l); the pad
    slots are dropped (corr_grad_pad_slots names them)."""
    geo = corr_grad_geometry(h, w, levels)
    n = h * w
    G = np.asarray(G).reshape(b, geo.TC, n, 8)
    out = []
    for l in range(levels):
        hl, wl, nch = geo.lh[l], geo.lw[l], geo.nch[l]
        blk = G[:, geo.coff[l]: geo.coff[l] + hl * nch].transpose(0, 2, 1, 3).reshape(b, n, hl, nch * 8)
        out.append(np.ascontiguousarray(blk[..., :wl]))
    return out


def corr_grad_pad_slots(h, w, levels):
    """(TC, 8) bool: True at the pad targets of the chunked order."""
    geo = corr_grad_geometry(h, w, levels)
    pad = np.zeros((geo.TC, 8), dtype=bool)
    for l in range(levels):
        rows = pad[geo.coff[l]: geo.coff[l] + geo.lh[l] * geo.nch[l]].reshape(geo.lh[l], geo.nch[l] * 8)
        rows[:, geo.lw[l]:] = True
    return pad


def _target_rows(levels_list):
    """Per-level (..., H_l, W_l) arrays -> (..., T') in the padded target order, pads zero."""
    parts = []
    for x in levels_list:
        hl, wl = x.shape[-2:]
        nch = -(-wl // 8)
        pad = np.zeros(x.shape[:-1] + (nch * 8,), dtype=x.dtype)
        pad[..., :wl] = x
        parts.append(pad.reshape(x.shape[:-2] + (hl * nch * 8,)))
    return np.concatenate(parts, axis=-1)


def corr_pool_targets(fmap2, levels, scale):
    """P (B, C, T') = avg_pool_{2^l}(fmap2) * scale for every level (successive 2x2 averages, floor
    sizes: raft.py:35-47 applied to the feature map), in G's padded target order, pads zero."""
    lv = [fmap2]
    for _ in range(1, levels):
        lv.append(_avg_pool2(lv[-1]))
    s = np.asarray(scale, dtype=fmap2.dtype)
    return _target_rows([x * s for x in lv])


def corr_unpool_targets(dP, h, w, levels, scale):
    """(B, C, T') -> (B, C, H, W): scale * sum_l avg_pool_{2^l}^T(level l of dP): every target spreads
    1/4^l of its value over its 2^l x 2^l block of the floor-cropped map (avg_pool2d_backward)."""
    geo = corr_grad_geometry(h, w, levels)
    out = np.zeros(dP.shape[:-1] + (h, w), dtype=dP.dtype)
    for l in range(levels):
        hl, wl, nch = geo.lh[l], geo.lw[l], geo.nch[l]
        x = dP[..., 8 * geo.coff[l]: 8 * (geo.coff[l] + hl * nch)].reshape(dP.shape[:-1] + (hl, nch * 8))[..., :wl]
        k = 2 ** l
        out[..., : hl * k, : wl * k] += np.repeat(np.repeat(x, k, axis=-2), k, axis=-1) / np.asarray(k * k, dtype=dP.dtype)
    return out * np.asarray(scale, dtype=dP.dtype)


def corr_lookup_backward(fmap1, fmap2, coords, levels, radius, grad_out, mask_costs=()):
    """d(sum(out*grad_out))/d(fmap1, fmap2) for raft.CorrBlock, as the composition of the stages above:
    grad_fmap1 = P G, dP = fmap1 G^T, grad_fmap2 = unpool(dP), with P and the unpooling scaled by
    1/sqrt(C).  1-pixel levels (NaN in the reference's forward) carry no gradient.  Coordinates carry no
    gradient (raft.py:402).  Dense, small sizes."""
    b, c, h, w = fmap1.shape
    n = h * w
    dt = fmap1.dtype
    gl = corr_lookup_grad_levels(coords, levels, radius, grad_out, mask_costs, dtype=dt)
    G = corr_grad_pack(gl).transpose(0, 1, 3, 2).reshape(b, -1, n)              # (B, T', N)
    scale = np.asarray(1, dtype=dt) / np.sqrt(np.asarray(c, dtype=dt))
    P = corr_pool_targets(fmap2, levels, scale)                                  # (B, C, T')
    gf1 = np.matmul(P, G).reshape(b, c, h, w)
    dP = np.matmul(fmap1.reshape(b, c, n), G.transpose(0, 2, 1))                 # (B, C, T')
    return gf1, corr_unpool_targets(dP, h, w, levels, scale)


def corr_lookup_fs_backward(fmap1, fmap2, coords, levels, radius, grad_out, mask_costs=(), scale=None):
    """d(sum(out*grad_out))/d(fmap1, fmap2) for raft_fs.CorrBlock (raft_fs.py:13-87; autograd of its
    avg_pool2d chain, grid_sample and matmul), with corr_lookup_fs's ``scale`` (None -> 1).

    raft_fs's output equals raft.CorrBlock's times sqrt(C) (pooling fmap2
    commutes with the product), so its gradient is corr_lookup_backward's times sqrt(C) * scale.
    """
    c = fmap1.shape[1]
    k = np.sqrt(np.asarray(c, dtype=fmap1.dtype)) * np.asarray(1.0 if scale is None else scale, dtype=fmap1.dtype)
    g1, g2 = corr_lookup_backward(fmap1, fmap2, coords, levels, radius, grad_out, mask_costs)
    return g1 * k, g2 * k

