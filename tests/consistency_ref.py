"""The NumPy statement of pd_depth_consistency (include/polardepth.h, "multi-view depth consistency"), written in the
header's order of operations so that the device can match it bit for bit: the five reasons, the forward leg, the four taps
and their fp32 blend, the rigid inverse and the return leg in fp64, the levels, the records (math.fsum: the exactly rounded
sum, which no order changes) and the per-pixel outputs.  Test infrastructure only; nothing here is fast."""
import math

import numpy as np

F64, F32 = np.float64, np.float32
BINS = 256
DEFAULT_TAUS = ((4.0, 0.04), (2.0, 0.02), (1.0, 0.01))
COUNTERS = ("loose", "mid", "tight", "invalid", "absent", "filtered", "outside", "hole")
INVALID, ABSENT, FILTERED, OUTSIDE, HOLE, COMPARED = 3, 4, 5, 6, 7, 8      # outcome codes: the counter's index, or 8


def in_class(mask, lo, hi):
    return np.ones(mask.shape, bool) if lo > hi else (mask >= lo) & (mask <= hi)


def in_range(d, lo, hi):
    with np.errstate(invalid="ignore"):
        return (d >= F32(lo)) & (d <= F32(hi))                     # fp32, NaN fails


def cam_P(K, T):
    """[..., 3, 4] fp64: entry (i, j) = ((K[i][0] T[0][j] + K[i][1] T[1][j]) + K[i][2] T[2][j]) + K[i][3] T[3][j]"""
    K, T = np.asarray(K, F64), np.asarray(T, F64)
    k = lambda c: K[..., :3, c, None]
    t = lambda r: T[..., None, r, :]
    return ((k(0) * t(0) + k(1) * t(1)) + k(2) * t(2)) + k(3) * t(3)


def rigid_inverse(T):
    """[..., 4, 4] fp64: [R^T | -(R^T t)], (R^T t)[i] = (R[0][i] t0 + R[1][i] t1) + R[2][i] t2, last row (0, 0, 0, 1)"""
    T = np.asarray(T, F64)
    R, t = T[..., :3, :3], T[..., :3, 3]
    Ti = np.zeros(T.shape, F64)
    Ti[..., :3, :3] = np.swapaxes(R, -1, -2)
    Ti[..., :3, 3] = -((R[..., 0, :] * t[..., 0, None] + R[..., 1, :] * t[..., 1, None]) + R[..., 2, :] * t[..., 2, None])
    Ti[..., 3, 3] = 1.0
    return Ti


def ray(iK, x, y):
    """r[..., i] = (iK[i][0] x + iK[i][1] y) + iK[i][2]; iK [3,3] fp64, x and y fp64 arrays"""
    return np.stack([(iK[i, 0] * x + iK[i, 1] * y) + iK[i, 2] for i in range(3)], -1)


def project_ray(P, r, d):
    """p = d r; h[i] = ((P[i][0] p.x + P[i][1] p.y) + P[i][2] p.z) + P[i][3]; hz = h.z + 1e-7; u = h.x / hz, v = h.y / hz"""
    with np.errstate(all="ignore"):                                # d may be NaN or inf where the pair is not compared
        p = d[..., None] * r
        h = [((P[i, 0] * p[..., 0] + P[i, 1] * p[..., 1]) + P[i, 2] * p[..., 2]) + P[i, 3] for i in range(3)]
        hz = h[2] + 1e-7
        return h[0] / hz, h[1] / hz, hz


def axis_of(c, size):
    """view_geom.hpp's axis_of on fp32 coordinates: (i0, i1, w1 fp32)"""
    hi = F32(size - 1)
    with np.errstate(invalid="ignore"):
        cc = np.where(np.abs(c) <= F32(3.0e38), c, F32(0))
    cc = np.minimum(np.maximum(cc, F32(0)), hi)
    f = np.floor(cc)
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < size - 1)
    w1 = cc - f
    assert w1.dtype == F32
    return i0, i1, w1


def blend(a, b, c, d, wx1, wy1):
    """view_geom.hpp's Bilinear, every operation in fp32"""
    wx0, wy0 = F32(1) - wx1, F32(1) - wy1
    w00, w10, w01, w11 = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1
    out = ((a * w00 + b * w10) + c * w01) + d * w11
    assert out.dtype == F32
    return out


def forward_leg(d0, K, inv_K, T):
    """One item, one view: (u, v, hz) fp64 [H,W] of every pixel at depth d0 (fp32 [H,W])."""
    H, W = d0.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    r = ray(np.asarray(inv_K, F64)[:3, :3], xx, yy)
    return project_ray(cam_P(K, T), r, d0.astype(F64))


def return_leg(uf, vf, d1, K, inv_K, T):
    """One item, one view: (u2, v2, hz2) fp64 from the fp32 landing point (uf, vf) and the fp32 depth d1 sampled there."""
    r = ray(np.asarray(inv_K, F64)[:3, :3], uf.astype(F64), vf.astype(F64))
    return project_ray(cam_P(K, rigid_inverse(T)), r, d1.astype(F64))


def pairs(depth0, depths, T, K, inv_K, frame_valid=None, visible=None, min_depth=0.1, max_depth=2.0, taus=DEFAULT_TAUS,
          fuse_level=4):
    """Everything per (pixel, view) pair and per pixel: outcome [N,F,H,W] (the codes above), level uint8 [N,F,H,W], e2, e_px,
    e_rel, hz2 fp64 [N,F,H,W] (NaN where not compared), bin [N,F,H,W], n_cons uint8 [N,H,W], fused fp32 [N,H,W]."""
    assert depth0.dtype == F32 and depths.dtype == F32 and T.dtype == F32 and K.dtype == F32 and inv_K.dtype == F32
    N, F, H, W = depths.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    outcome = np.zeros((N, F, H, W), np.int64)
    level = np.zeros((N, F, H, W), np.uint8)
    nan = lambda: np.full((N, F, H, W), np.nan, F64)
    e2, e_px, e_rel, hz2 = nan(), nan(), nan(), nan()
    met = np.zeros((N, F, H, W, 3), bool)
    n_cons = np.zeros((N, H, W), np.uint8)
    fused = np.zeros((N, H, W), F32)
    for n in range(N):
        d0 = depth0[n]
        valid = in_range(d0, min_depth, max_depth)
        acc = d0.astype(F64)
        nc = np.zeros((H, W), np.int64)
        for f in range(F):
            out = np.full((H, W), -1, np.int64)
            out[~valid] = INVALID
            if frame_valid is not None and frame_valid[n, f] == 0:
                out[out < 0] = ABSENT
            if visible is not None:
                out[(out < 0) & (visible[n, f] == 0)] = FILTERED
            u, v, hz = forward_leg(d0, K[n], inv_K[n], T[n, f])
            uf, vf = u.astype(F32), v.astype(F32)                   # rounded once
            with np.errstate(invalid="ignore"):
                inside = (hz > 1e-3) & (uf >= F32(0)) & (uf <= F32(W - 1)) & (vf >= F32(0)) & (vf <= F32(H - 1))
            out[(out < 0) & ~inside] = OUTSIDE
            x0, x1, wx1 = axis_of(uf, W)
            y0, y1, wy1 = axis_of(vf, H)
            D = depths[n, f]
            v00, v10, v01, v11 = D[y0, x0], D[y0, x1], D[y1, x0], D[y1, x1]
            taps_ok = (in_range(v00, min_depth, max_depth) & in_range(v10, min_depth, max_depth) &
                       in_range(v01, min_depth, max_depth) & in_range(v11, min_depth, max_depth))
            out[(out < 0) & ~taps_ok] = HOLE
            with np.errstate(all="ignore"):
                d1 = blend(v00, v10, v01, v11, wx1, wy1)
                a2, b2, h2 = return_leg(uf, vf, d1, K[n], inv_K[n], T[n, f])
                back = h2 > 1e-3
            out[(out < 0) & ~back] = OUTSIDE
            cmp_ = out < 0
            out[cmp_] = COMPARED
            with np.errstate(all="ignore"):
                du, dv = a2 - xx, b2 - yy
                q2 = du * du + dv * dv
                d0d = d0.astype(F64)
                rel = np.abs(h2 - d0d) / d0d
            lv = np.where(cmp_, 1, 0).astype(np.uint8)
            for j, (tpx, trel) in enumerate(taus):
                with np.errstate(invalid="ignore"):
                    m = cmp_ & (q2 < F64(tpx) * F64(tpx)) & (rel < F64(trel))
                met[n, f, ..., j] = m
                lv[m] = 2 + j
            take = cmp_ & (lv >= fuse_level)
            acc = np.where(take, acc + np.where(take, h2, 0.0), acc)
            nc += take
            outcome[n, f], level[n, f] = out, lv
            e2[n, f] = np.where(cmp_, q2, np.nan)
            e_px[n, f] = np.where(cmp_, np.sqrt(np.where(cmp_, q2, 0.0)), np.nan)
            e_rel[n, f] = np.where(cmp_, rel, np.nan)
            hz2[n, f] = np.where(cmp_, h2, np.nan)
        n_cons[n] = nc
        fused[n] = np.where(valid, (acc / (1 + nc).astype(F64)).astype(F32), F32(0))
    with np.errstate(invalid="ignore"):
        b = np.floor(e_rel * 1024.0)
        bins = np.where(b < BINS - 1, b, BINS - 1)
    bins = np.where(outcome == COMPARED, bins, -1).astype(np.int64)
    return {"outcome": outcome, "level": level, "met": met, "e2": e2, "e_px": e_px, "e_rel": e_rel, "hz2": hz2, "bin": bins,
            "n_cons": n_cons, "fused": fused}


def records(pr, mask, classes):
    """The [N][K] records from ``pairs``' output: n, counters [N,K,8] (COUNTERS), sums [N,K,4], hist [N,K,256], and
    pixels [N,K] (the pixels of the class)."""
    N, F, H, W = pr["outcome"].shape
    K = len(classes)
    m = np.zeros((N, H, W), np.int64) if mask is None else np.asarray(mask).astype(np.int64)
    out = {"n": np.zeros((N, K), np.int64), "counters": np.zeros((N, K, 8), np.int64), "sums": np.zeros((N, K, 4)),
           "hist": np.zeros((N, K, BINS), np.int64), "pixels": np.zeros((N, K), np.int64)}
    for i in range(N):
        for k, (lo, hi) in enumerate(classes):
            cl = in_class(m[i], lo, hi)
            sel = np.broadcast_to(cl, (F, H, W))
            oc = pr["outcome"][i][sel]
            cmp_ = oc == COMPARED
            out["pixels"][i, k] = cl.sum()
            out["n"][i, k] = cmp_.sum()
            for j in range(3):
                out["counters"][i, k, j] = pr["met"][i][sel][:, j].sum()
            for c in (INVALID, ABSENT, FILTERED, OUTSIDE, HOLE):
                out["counters"][i, k, c] = (oc == c).sum()
            epx, erel, e2 = pr["e_px"][i][sel][cmp_], pr["e_rel"][i][sel][cmp_], pr["e2"][i][sel][cmp_]
            out["sums"][i, k] = [math.fsum(epx), math.fsum(erel), math.fsum(e2), math.fsum(erel * erel)]
            out["hist"][i, k] = np.bincount(pr["bin"][i][sel][cmp_], minlength=BINS)
    return out


def consistency(depth0, depths, T, K, inv_K, frame_valid=None, visible=None, mask=None, classes=((1, 0),), **kw):
    """pairs + records in one dict."""
    pr = pairs(depth0, depths, T, K, inv_K, frame_valid=frame_valid, visible=visible, **kw)
    pr.update(records(pr, mask, classes))
    return pr


# ------------------------------------------------------------------------------------------------ the shared scene
def rot(w):
    """Rodrigues: the rotation matrix of the axis-angle vector w, fp64."""
    w = np.asarray(w, F64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def camera(H, W):
    """fx = fy = 0.65 W, the principal point at the centre: K, inv_K [4,4] fp32"""
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 0.65 * W
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return K.astype(F32), np.linalg.inv(K).astype(F32)


def plane_depth(nrm, c, inv_K, H, W):
    """Depth of the plane nrm . X = c along the rays of every pixel, fp64 [H,W]"""
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    iK = np.asarray(inv_K, F64)[:3, :3]
    r = np.stack([iK[i, 0] * xx + iK[i, 1] * yy + iK[i, 2] for i in range(3)], -1)
    return c / (r @ nrm)


def plane_pair(N, F, H, W, seed, big_last=False):
    """Two or more views of an analytic plane: in view 0 the plane is nrm . X = c; in view f (X_f = R X + t) it has
    nrm_f = R nrm, c_f = c + nrm_f . t and depth c_f / (nrm_f . r).  Poses are small -- rotations within +-0.01 rad,
    translations of 3 cm +- 1 cm; with ``big_last`` the last view of the last item gets 8 x the rotation and 6 x the
    translation, so that pixels leave the frame.  -> depth0 [N,H,W], depths [N,F,H,W], T [N,F,4,4], K, inv_K [N,4,4], fp32"""
    rng = np.random.default_rng(seed)
    K1, iK1 = camera(H, W)
    depth0 = np.zeros((N, H, W), F32)
    depths = np.zeros((N, F, H, W), F32)
    T = np.zeros((N, F, 4, 4), F32)
    for n in range(N):
        nrm = np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), 1.0])
        nrm /= np.linalg.norm(nrm)
        c = rng.uniform(0.9, 1.2)
        depth0[n] = plane_depth(nrm, c, iK1, H, W)
        for f in range(F):
            w = rng.uniform(-0.01, 0.01, 3)
            t = rng.normal(size=3)
            t *= rng.uniform(0.02, 0.04) / np.linalg.norm(t)
            if big_last and n == N - 1 and f == F - 1:
                w, t = 8 * w, 6 * t
            R = rot(w)
            M = np.eye(4)
            M[:3, :3], M[:3, 3] = R, t
            T[n, f] = M
            nf = R @ nrm
            depths[n, f] = plane_depth(nf, c + nf @ t, iK1, H, W)
    return depth0, depths, T, np.broadcast_to(K1, (N, 4, 4)).copy(), np.broadcast_to(iK1, (N, 4, 4)).copy()
