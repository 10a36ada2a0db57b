"""The NumPy statement of pd_backproject / pd_cloud_nn / pd_cloud_stats (include/polardepth.h): the tiling of a depth map into
256-slot tiles, the tile boxes, the nearest-neighbour distance in float32 arithmetic in the header's operation order (a
minimum does not depend on the order of its terms, so it is bit-exact), the box lower bound and the count of target tiles a
pruned scan cannot avoid, and the records.  The two sums are formed with math.fsum (the exactly rounded sum, which no order
changes), so the kernel's ordered fp64 sums may differ from them by the (n - 1) 2^-53 of any summation order."""
import math

import numpy as np

TILE = 256
BINS = 512
F32 = np.float32


def edges2():
    """fp32((j * 0.0005)^2 in fp64), j = 1 .. 511."""
    return ((np.arange(1, BINS, dtype=np.float64) * 0.0005) ** 2).astype(np.float32)


def tiles_of(H, W):
    return ((H + 15) // 16) * ((W + 15) // 16)


def slot_pixels(H, W):
    """(v, u, inside) of every slot of the 16x16 pixel tiling, tiles row-major, slots row-major inside the tile."""
    tx = (W + 15) // 16
    s = np.arange(tiles_of(H, W) * TILE)
    t, r = s // TILE, s % TILE
    v, u = (t // tx) * 16 + r // 16, (t % tx) * 16 + r % 16
    return v, u, (v < H) & (u < W)


def backproject(depth, Kmat, gate, min_depth, max_depth, dtype=np.float32):
    """depth [N,H,W] fp32, Kmat [N,4,4] fp32, gate [N,H,W] or None -> points [N, T*256, 4] in ``dtype`` arithmetic (float32:
    the kernel's operations; float64: the exact pinhole model the kernel is measured against)."""
    N, H, W = depth.shape
    v, u, inside = slot_pixels(H, W)
    vv, uu = np.where(inside, v, 0), np.where(inside, u, 0)
    out = np.zeros((N, v.size, 4), dtype)
    g = depth if gate is None else gate
    for i in range(N):
        z = depth[i, vv, uu]
        gi = g[i, vv, uu]
        with np.errstate(invalid="ignore"):
            ok = inside & (gi >= F32(min_depth)) & (gi <= F32(max_depth))
            good = ok & np.isfinite(z) & (z > 0)
        fx, fy, cx, cy = (Kmat[i, 0, 0].astype(dtype), Kmat[i, 1, 1].astype(dtype), Kmat[i, 0, 2].astype(dtype),
                          Kmat[i, 1, 2].astype(dtype))
        zz = np.where(good, z, 0).astype(dtype)
        with np.errstate(all="ignore"):
            x = ((uu.astype(dtype) - cx) / fx) * zz
            y = ((vv.astype(dtype) - cy) / fy) * zz
        out[i, :, 0], out[i, :, 1], out[i, :, 2] = np.where(good, x, 0), np.where(good, y, 0), zz
        out[i, :, 3] = np.where(good, 1, np.where(ok, -1, 0))
    return out


def boxes_of(points):
    """points [N, T*256, 4] fp32 -> (lo [N,T,3], hi [N,T,3] fp32, count [N,T]) over the w = 1 slots; an empty tile has
    lo = +inf, hi = -inf."""
    N, S, _ = points.shape
    p = points.reshape(N, S // TILE, TILE, 4)
    is_pt = p[..., 3] == 1
    lo = np.where(is_pt[..., None], p[..., :3], np.inf).min(2).astype(np.float32)
    hi = np.where(is_pt[..., None], p[..., :3], -np.inf).max(2).astype(np.float32)
    return lo, hi, is_pt.sum(2)


def pack_boxes(lo, hi, count):
    """The header's 32-byte record as float32 [N,T,8] (the count's int32 bits in word 6)."""
    rec = np.zeros(lo.shape[:-1] + (8,), np.float32)
    rec[..., 0:3], rec[..., 3:6] = lo, hi
    rec.view(np.int32)[..., 6] = count
    return rec


def pair_d2(q, t):
    """((dx dx + dy dy) + dz dz) in float32, q [..., 3] against t [..., 3] (broadcast)."""
    assert q.dtype == np.float32 and t.dtype == np.float32
    dx, dy, dz = q[..., 0] - t[..., 0], q[..., 1] - t[..., 1], q[..., 2] - t[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def boxd2(lo_q, hi_q, lo_t, hi_t):
    """The lower bound of pair_d2 over two boxes, float32, in the same operation order."""
    assert all(a.dtype == np.float32 for a in (lo_q, hi_q, lo_t, hi_t))
    with np.errstate(invalid="ignore"):
        g = np.maximum(np.maximum(F32(0), lo_t - hi_q), lo_q - hi_t)
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def nn_d2(qpts, tpts, chunk=512):
    """qpts [N,Sq,4], tpts [N,St,4] fp32 -> d2 [N,Sq] fp32: the minimum of pair_d2 over the w = 1 targets for a w = 1 query
    (+inf without a target), NaN for the other slots."""
    N, Sq, _ = qpts.shape
    out = np.full((N, Sq), np.nan, np.float32)
    for i in range(N):
        qi = np.flatnonzero(qpts[i, :, 3] == 1)
        t = tpts[i][tpts[i, :, 3] == 1][:, :3]
        if t.shape[0] == 0:
            out[i, qi] = np.inf
            continue
        for c in range(0, qi.size, chunk):
            q = qpts[i, qi[c:c + chunk], :3]
            out[i, qi[c:c + chunk]] = pair_d2(q[:, None, :], t[None, :, :]).min(1)
    return out


def necessary_tiles(qpts, tpts, d2):
    """[N,Tq]: the target tiles a pruned scan of each query tile cannot avoid -- non-empty, with boxd2 <= the final R = the
    maximum d2 over the query tile's w = 1 slots.  0 for a query tile without a point."""
    qlo, qhi, qn = boxes_of(qpts)
    tlo, thi, tn = boxes_of(tpts)
    N, Tq = qn.shape
    out = np.zeros((N, Tq), np.int64)
    for i in range(N):
        for a in range(Tq):
            if qn[i, a] == 0:
                continue
            sl = slice(a * TILE, (a + 1) * TILE)
            R = d2[i, sl][qpts[i, sl, 3] == 1].max()
            bd = boxd2(qlo[i, a][None], qhi[i, a][None], tlo[i], thi[i])
            out[i, a] = ((tn[i] > 0) & (bd <= R)).sum()
    return out


def in_class(mask, lo, hi):
    return np.ones(mask.shape, bool) if lo > hi else (mask >= lo) & (mask <= hi)


def stats(d2, points, mask, classes, edges, H, W):
    """d2 [N,S] fp32, points [N,S,4] fp32 in the pixel tiling of H x W, mask [N,H,W] int or None, classes [(lo, hi)] ->
    dict(n, bad, unmatched [N,K] int64, sum_d, sum_d2 [N,K], hist [N,K,512] int64, dist [N,H,W] float64)."""
    N, S = d2.shape
    K = len(classes)
    v, u, inside = slot_pixels(H, W)
    assert S == v.size
    out = {"n": np.zeros((N, K), np.int64), "bad": np.zeros((N, K), np.int64), "unmatched": np.zeros((N, K), np.int64),
           "sum_d": np.zeros((N, K)), "sum_d2": np.zeros((N, K)), "hist": np.zeros((N, K, BINS), np.int64),
           "dist": np.full((N, H, W), np.nan)}
    for i in range(N):
        w = points[i, :, 3]
        point, bad = inside & (w == 1), inside & (w == -1)
        fin = point & np.isfinite(d2[i])
        unm = point & np.isposinf(d2[i])
        d2d = np.where(fin, d2[i], 0).astype(np.float64)
        dist = np.sqrt(d2d)
        b = np.searchsorted(edges, np.where(fin, d2[i], 0), side="right")        # #{ j : edges[j] <= d2 }
        out["dist"][i, v[fin], u[fin]] = dist[fin]
        out["dist"][i, v[unm], u[unm]] = np.inf
        m = np.zeros(S, np.int64)
        if mask is not None:
            m[inside] = mask[i, v[inside], u[inside]]
        for k, (lo, hi) in enumerate(classes):
            sel = in_class(m, lo, hi)
            f = sel & fin
            out["n"][i, k] = f.sum()
            out["bad"][i, k] = (sel & bad).sum()
            out["unmatched"][i, k] = (sel & unm).sum()
            out["sum_d"][i, k] = math.fsum(dist[f])
            out["sum_d2"][i, k] = math.fsum(d2d[f])
            out["hist"][i, k] = np.bincount(b[f], minlength=BINS)
    return out


def metrics_from_distances(acc_m, comp_m):
    """Plain NumPy on explicit distance lists (metres): acc, comp, chamfer (mean, mm), the two medians (mm), precision and
    recall [3] at 5 / 10 / 20 mm decided on the SQUARED distance against the edge table, as the bins are, F [3]."""
    e = edges2()
    a, c = np.asarray(acc_m, np.float64), np.asarray(comp_m, np.float64)
    a2, c2 = (a * a).astype(np.float32), (c * c).astype(np.float32)
    P = np.array([(a2 < e[j - 1]).mean() for j in (10, 20, 40)])
    R = np.array([(c2 < e[j - 1]).mean() for j in (10, 20, 40)])
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where(P + R > 0, 2 * P * R / (P + R), 0.0)
    return {"acc": a.mean() * 1e3, "comp": c.mean() * 1e3, "chamfer": (a.mean() + c.mean()) * 1e3,
            "acc_med": np.median(a) * 1e3, "comp_med": np.median(c) * 1e3, "P": P, "R": R, "F": F}
