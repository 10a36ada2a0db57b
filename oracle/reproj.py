"""Oracle (plain PyTorch-CPU restatement, dtype-generic, differentiable by autograd) of the photometric multi-view term.

TEST INFRASTRUCTURE -- see ``oracle/__init__.py``.  Never imported by the product.

One text runs in fp32 (the reference's arithmetic) and in fp64 (the yardstick): every input is cast to the dtype of
``depth``, and nothing below names a dtype.

* ``manydepth/layers.py:383-413``   BackprojectDepth: depth * (inv_K[:3,:3] (x, y, 1)), a row of ones appended
* ``manydepth/layers.py:416-443``   Project3D: (K T)[:3,:] X, / (z + 1e-7), / (W-1 | H-1), (. - 0.5) * 2
* ``manydepth/trainer.py:1041-1044`` F.grid_sample(..., padding_mode="border", align_corners=True)
* ``manydepth/trainer.py:1069-1081`` compute_reprojection_loss: 0.85 * ssim.mean(1) + 0.15 * l1.mean(1) (no_ssim: the L1 mean)
* ``manydepth/trainer.py:1163-1215`` identity maps, minimum / mean over the frames, the noise on the identity value, the
  automask of compute_loss_masks (:1083-1098: the reprojection wins a tie), sum / (count + 1e-7)

The reference knows no missing frame; the ``valid`` [N,F] rule is the project's (include/polardepth.h, "photometric
multi-view term", and tests/reproj_ref.combine): an invalid frame takes part in neither the reprojection nor the identity
reduction, an item without a valid frame leaves both the sum and the count, and the mean of ``avg`` is over the valid frames.

``sel`` (uint8 [N,H,W], 255 = masked) replaces the oracle's own argmin and mask by a GIVEN selection: the reduction then
reads "the selected frame's map where kept" (``avg``: "the mean over the valid frames where sel != 255").  A comparison of
two arithmetics of this term is meaningful only on one selection: a pixel that picks another frame, or flips its mask, in
one of them is a different function, not a rounding error.  ``coords`` does the same for the term's other discrete choice,
the bilinear cell of every sampled pixel (``sample_in_cells``): the term is continuous there but its gradient is not, and a
coordinate within 1e-4 px of a cell boundary lands on either side of it at depths that differ by fp32 rounding.
"""
import torch
import torch.nn.functional as F

from oracle.losses import ssim

MASKED = 255


def backproject(depth, inv_K):
    """layers.py:408-413: [N,1,H,W], [N,4,4] -> homogeneous camera points [N,4,H*W]."""
    N, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=depth.dtype), torch.arange(W, dtype=depth.dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=depth.dtype)], 0)      # [3,H*W]
    rays = torch.matmul(inv_K[:, :3, :3], pix[None].expand(N, -1, -1))
    pts = depth.reshape(N, 1, -1) * rays
    return torch.cat([pts, torch.ones(N, 1, H * W, dtype=depth.dtype)], 1)


def project(points, K, T, H, W):
    """layers.py:428-443: the sampling grid [N,H,W,2] in grid_sample's normalised coordinates."""
    P = torch.matmul(K, T)[:, :3, :]
    cam = torch.matmul(P, points)
    pix = cam[:, :2, :] / (cam[:, 2:3, :] + 1e-7)
    pix = pix.reshape(-1, 2, H, W).permute(0, 2, 3, 1)
    pix = pix / torch.tensor([W - 1, H - 1], dtype=pix.dtype)
    return (pix - 0.5) * 2


def sample_in_cells(src, grid, coords):
    """grid_sample(bilinear, padding_mode="border", align_corners=True) with the discrete part GIVEN: ``coords`` [N,H,W,2]
    are source pixel coordinates (u, v) of another evaluation of the same warp, and they alone decide, per axis, the cell
    (floor of the clamped coordinate) and whether the axis is clamped (<= 0, >= size - 1 or not finite: no gradient, as
    PyTorch's border rule has it).  The weights come from ``grid``.  The interpolant is continuous across a cell boundary,
    so a coordinate that lies 1e-4 px on the other side of one than ``coords`` changes the value by 1e-4 x a second
    difference -- but it keeps the slope of the given cell, where grid_sample would take the neighbour's."""
    N, C, H, W = src.shape
    flat = src.reshape(N, C, H * W)
    parts = []
    for a, size in ((0, W), (1, H)):
        c = coords[..., a].to(grid.dtype)
        free = (c > 0) & (c < size - 1)
        c = torch.where(torch.isfinite(c), c, torch.zeros_like(c)).clamp(0, size - 1)
        i0 = torch.floor(c)
        own = (grid[..., a] + 1) / 2 * (size - 1)
        own = torch.where(free, own, torch.where(torch.isfinite(own), own, torch.zeros_like(own)).clamp(0, size - 1).detach())
        parts.append((i0.to(torch.int64), (i0 + 1).clamp(max=size - 1).to(torch.int64), own - i0))
    (x0, x1, wx), (y0, y1, wy) = parts
    tap = lambda y, x: flat.gather(2, (y * W + x).reshape(N, 1, H * W).expand(-1, C, -1)).reshape(N, C, H, W)
    wx, wy = wx[:, None], wy[:, None]
    return (tap(y0, x0) * (1 - wx) + tap(y0, x1) * wx) * (1 - wy) + (tap(y1, x0) * (1 - wx) + tap(y1, x1) * wx) * wy


def warp(depth, src, K, inv_K, T, coords=None):
    """trainer.py:1021-1044 for one neighbouring frame: ``src`` [N,C,H,W] seen through ``depth`` and the pose ``T``
    (current camera -> source camera).  Returns (warped, grid).  ``coords``: see ``sample_in_cells``."""
    dt = depth.dtype
    H, W = depth.shape[2:]
    grid = project(backproject(depth, inv_K.to(dt)), K.to(dt), T.to(dt), H, W)
    if coords is not None:
        return sample_in_cells(src.to(dt), grid, coords), grid
    return F.grid_sample(src.to(dt), grid, padding_mode="border", align_corners=True), grid


def reprojection_loss(pred, target, no_ssim=False):
    """trainer.py:1069-1081: [N,1,H,W]."""
    l1 = torch.abs(target - pred).mean(1, True)
    if no_ssim:
        return l1
    return 0.85 * ssim(pred, target).mean(1, True) + 0.15 * l1


def _over_frames(maps, valid, avg):
    """(value [N,1,H,W], frame [N,1,H,W] int64 with 255 where no frame is valid, number of valid frames [N,1,1,1]): the
    minimum of the valid frames in frame order, a later frame only when strictly smaller, or their mean."""
    m = torch.zeros_like(maps[0])
    arg = torch.full(maps[0].shape, MASKED, dtype=torch.int64)
    cnt = valid.sum(1).reshape(-1, 1, 1, 1)
    for f, r in enumerate(maps):
        v = valid[:, f].reshape(-1, 1, 1, 1)
        if avg:
            m = torch.where(v, m + r, m)
        else:
            take = v & ((arg == MASKED) | (r < m))
            m = torch.where(take, r, m)
            arg = torch.where(take, torch.full_like(arg, f), arg)
    if avg:
        m = torch.where(cnt > 0, m / cnt.clamp(min=1).to(m.dtype), m)
        arg = torch.where(cnt > 0, torch.zeros_like(arg), arg)
    return m, arg, cnt


def combine(reproj, identity=None, noise=None, valid=None, avg=False, sel=None):
    """trainer.py:1163-1215 on F maps [N,1,H,W] as given (identity None: no automasking).  Returns a dict: ``loss``
    (differentiable in the reproj maps), ``sel`` uint8 [N,H,W], ``arg`` (the frame of the minimum before masking), ``mask``,
    ``count``, ``value``."""
    N = reproj[0].shape[0]
    val = torch.ones(N, len(reproj), dtype=torch.bool) if valid is None else torch.as_tensor(valid) != 0
    m, arg, cnt = _over_frames(reproj, val, avg)
    if sel is None:
        keep = (cnt > 0).expand_as(m)
        if identity is not None:
            idm, _, _ = _over_frames([i.detach() for i in identity], val, avg)
            if noise is not None:
                idm = idm + noise.to(idm.dtype)
            keep = keep & (m.detach() <= idm)
        sel = torch.where(keep, arg, torch.full_like(arg, MASKED))[:, 0].to(torch.uint8)
    else:
        sel = torch.as_tensor(sel).to(torch.uint8)
        keep = (sel != MASKED)[:, None]
        if not avg:                                   # the selected frame's map where kept
            pick = sel[:, None].to(torch.int64)
            m = sum(torch.where(pick == f, r, torch.zeros_like(r)) for f, r in enumerate(reproj))
    mask = keep.to(m.dtype)
    count = mask.sum()
    loss = (torch.where(keep, m, torch.zeros_like(m))).sum() / (count + 1e-7)
    return {"loss": loss, "sel": sel, "arg": arg[:, 0], "mask": keep[:, 0], "count": count, "value": m}


def photometric_term(depth, target, sources, K, inv_K, poses, valid=None, noise=None, no_ssim=False, automask=True,
                     avg=False, sel=None, coords=None, details=False):
    """The term of one scale: ``depth`` [N,1,H,W] (its dtype is the dtype of everything), ``target`` = ("color", 0, 0),
    ``sources`` / ``poses`` the F neighbouring frames and their matrices, ``K`` / ``inv_K`` of scale 0, ``noise`` [N,1,H,W]
    added to the identity value (ignored without automasking).  Differentiable in ``depth``.  ``coords``: optional, per frame
    the pixel coordinates [N,H,W,2] that decide the sampling cells (``sample_in_cells``), the counterpart of ``sel`` for the
    other discrete choice of the term.  ``details``: the dict of ``combine`` plus the warped images and the reproj /
    identity maps."""
    dt = depth.dtype
    target = target.to(dt)
    sources = [s.to(dt) for s in sources]
    warped = [warp(depth, s, K, inv_K, T, None if coords is None else coords[f])[0]
              for f, (s, T) in enumerate(zip(sources, poses))]
    reproj = [reprojection_loss(w, target, no_ssim) for w in warped]
    identity = [reprojection_loss(s, target, no_ssim) for s in sources] if automask else None
    out = combine(reproj, identity, noise.to(dt) if (automask and noise is not None) else None, valid, avg, sel)
    if not details:
        return out["loss"]
    out.update(warped=warped, reproj=reproj, identity=identity)
    return out
