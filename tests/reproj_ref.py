"""fp64 NumPy statement of the three definitions of csrc/reproj.hip (include/polardepth.h, "photometric multi-view term"):
view synthesis (coordinates, clamp flags, warped image), its gradient w.r.t. depth, and the minimum / automask reduction
over the frames.  Test infrastructure only; nothing here is fast."""
import numpy as np

F64 = np.float64


def project(depth, K, inv_K, T):
    """(u, v) source pixel coordinates [N,H,W,2] fp64, h.z + 1e-7 [N,H,W] and q = (K T)[:3,:3] r [N,H,W,3]."""
    depth, K, inv_K, T = (np.asarray(a, F64) for a in (depth, K, inv_K, T))
    N, _, H, W = depth.shape
    P = np.einsum("nik,nkj->nij", K, T)[:, :3, :]
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    pix = np.stack([xx, yy, np.ones_like(xx)], -1)                                  # [H,W,3]
    r = np.einsum("nij,hwj->nhwi", inv_K[:, :3, :3], pix)
    p = depth[:, 0, :, :, None] * r
    h = np.einsum("nij,nhwj->nhwi", P[:, :, :3], p) + P[:, None, None, :, 3]
    q = np.einsum("nij,nhwj->nhwi", P[:, :, :3], r)
    hz = h[..., 2] + 1e-7
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = h[..., :2] / hz[..., None]
    return uv, hz, q


def _axis(c, size):
    """Border padding of one axis: (clamped coordinate, lower cell, upper cell, upper weight, free flag)."""
    c = np.asarray(c, F64)
    free = (c > 0) & (c < size - 1)                                                 # False for NaN / inf as well
    cc = np.where(np.isfinite(c), c, 0.0)
    cc = np.clip(cc, 0.0, size - 1.0)
    f = np.floor(cc)
    i0 = f.astype(np.int64)
    i1 = np.minimum(i0 + 1, size - 1)
    return cc, i0, i1, cc - f, free


def sample(src, coords):
    """Bilinear sampling with border padding at the GIVEN coordinates [N,H,W,2] (fp32 or fp64 values, used exactly):
    warped [N,C,H,W] fp64, free_x / free_y [N,H,W] (False where the axis was clamped or is not finite) and the taps."""
    src = np.asarray(src, F64)
    N, C, H, W = src.shape
    _, x0, x1, wx1, fx = _axis(np.asarray(coords)[..., 0], W)
    _, y0, y1, wy1, fy = _axis(np.asarray(coords)[..., 1], H)
    n = np.arange(N)[:, None, None, None]
    c = np.arange(C)[None, :, None, None]
    tap = lambda yi, xi: src[n, c, yi[:, None], xi[:, None]]
    v00, v10, v01, v11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    wx1, wy1 = wx1[:, None], wy1[:, None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    warped = ((v00 * (wx0 * wy0) + v10 * (wx1 * wy0)) + v01 * (wx0 * wy1)) + v11 * (wx1 * wy1)
    return {"warped": warped, "free_x": fx, "free_y": fy, "taps": (v00, v10, v01, v11), "w": (wx0, wx1, wy0, wy1)}


def view_synth(depth, src, K, inv_K, T, coords=None):
    """pd_view_synth_fwd: coords (fp64 unless given), clamp flags and the warped image."""
    uv, _, _ = project(depth, K, inv_K, T)
    out = sample(src, uv if coords is None else coords)
    out["coords"] = uv
    return out


def view_synth_grad(gwarped, src, coords, depth, K, inv_K, T, magnitude=False):
    """pd_view_synth_bwd: d sum(gwarped * warped) / d depth [N,1,H,W] fp64, cells and weights from ``coords``.
    magnitude: the same expression with the absolute value of every term that is added (tap differences, channel terms,
    the two axes) -- what relative rounding errors of the summands are relative to."""
    s = sample(src, coords)
    v00, v10, v01, v11 = s["taps"]
    wx0, wx1, wy0, wy1 = s["w"]
    gw = np.asarray(gwarped, F64)
    m = np.abs if magnitude else (lambda a: a)
    gu = (m(gw) * (m(v10 - v00) * wy0 + m(v11 - v01) * wy1)).sum(1)
    gv = (m(gw) * (m(v01 - v00) * wx0 + m(v11 - v10) * wx1)).sum(1)
    uv, hz, q = project(depth, K, inv_K, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        du = np.where(s["free_x"], m((q[..., 0] - uv[..., 0] * q[..., 2]) / hz), 0.0)
        dv = np.where(s["free_y"], m((q[..., 1] - uv[..., 1] * q[..., 2]) / hz), 0.0)
    g = np.where(s["free_x"], gu * du, 0.0) + np.where(s["free_y"], gv * dv, 0.0)
    return g[:, None]


def near_boundary(coords, H, W, tol=1e-3):
    """[N,H,W] bool: a coordinate within ``tol`` px of a cell boundary or of the border (where the gradient jumps)."""
    out = np.zeros(np.asarray(coords).shape[:3], bool)
    for a, size in ((0, W), (1, H)):
        c = np.asarray(coords, F64)[..., a]
        ok = np.isfinite(c)
        cz = np.where(ok, c, -10.0)
        out |= ok & (cz > -tol) & (cz < size - 1 + tol) & (np.abs(cz - np.rint(cz)) < tol)
    return out


def combine(reproj, identity=None, noise=None, valid=None, avg=False):
    """pd_reproj_combine_fwd on maps GIVEN as they are (their values are used exactly; the per-pixel arithmetic -- the mean
    of ``avg`` and the noise addition -- is done in the maps' own dtype, the sums in fp64): sel [N,H,W] uint8, value
    [N,H,W], mask, sum, count, loss."""
    reproj = [np.asarray(r) for r in reproj]
    dt = reproj[0].dtype
    F = len(reproj)
    N, _, H, W = reproj[0].shape
    val = np.ones((N, F), bool) if valid is None else np.asarray(valid) != 0

    def over(maps):
        m = np.zeros((N, H, W), dt)
        arg = np.full((N, H, W), 255, np.int64)
        cnt = np.zeros((N, 1, 1), np.int64)
        for f in range(F):
            r = np.asarray(maps[f])[:, 0].astype(dt)
            v = val[:, f][:, None, None]
            cnt = cnt + v
            if avg:
                m = np.where(v, m + r, m).astype(dt)
            else:
                take = v & ((arg == 255) | (r < m))
                m = np.where(take, r, m)
                arg = np.where(take, f, arg)
        if avg:
            m = np.where(cnt > 0, m / np.maximum(cnt, 1).astype(dt), m).astype(dt)
            arg = np.where(cnt > 0, 0, 255) * np.ones((N, H, W), np.int64)
        return m, arg, cnt

    m, arg, cnt = over(reproj)
    keep = np.broadcast_to(cnt > 0, (N, H, W)).copy()
    if identity is not None:
        idm, _, _ = over(identity)
        if noise is not None:
            idm = (idm + np.asarray(noise)[:, 0].astype(dt)).astype(dt)
        keep &= m <= idm
    sel = np.where(keep, arg, 255).astype(np.uint8)
    terms = np.where(keep, m.astype(F64), 0.0)
    total, count = terms.sum(dtype=F64), float(keep.sum())
    return {"sel": sel, "value": m, "mask": keep, "sum": total, "count": count, "loss": total / (count + 1e-7),
            "abs_sum": np.abs(terms).sum(dtype=F64), "nvalid": cnt}


def combine_grad(gloss, sel, count, valid, F, avg=False):
    """pd_reproj_combine_bwd: F maps [N,1,H,W] fp64."""
    sel = np.asarray(sel)
    N = sel.shape[0]
    g = float(gloss) / (count + 1e-7)
    val = np.ones((N, F), bool) if valid is None else np.asarray(valid) != 0
    out = []
    for f in range(F):
        if avg:
            nv = val.sum(1)[:, None, None]
            out.append(np.where((sel != 255) & val[:, f][:, None, None], g / np.maximum(nv, 1), 0.0)[:, None])
        else:
            out.append(np.where(sel == f, g, 0.0)[:, None])
    return out
