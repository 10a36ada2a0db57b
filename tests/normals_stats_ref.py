"""The NumPy statement of pd_normals_stats (include/polardepth.h): the same fp32 normal maps and the same 719-entry cosine
table as the kernel, fp64 arithmetic in the header's order.  ``stats`` is vectorised, ``stats_loop`` the plain per-pixel loop
it must equal bit for bit; both form the two sums with math.fsum (the exactly rounded sum, which no order changes), so the
kernel's ordered fp64 sums may differ from them by the (n - 1) 2^-53 of any summation order."""
import math

import numpy as np

BINS = 720
DEG = 57.29577951308232


def window_ok(gt, min_depth, max_depth, gate):
    """[N,H,W] bool: gate 0 = the pixel's own depth is inside [min, max]; gate 1 = all nine depths of its replicate-clamped
    3x3 window are."""
    ok = (gt >= min_depth) & (gt <= max_depth)
    if not gate:
        return ok
    p = np.pad(ok, ((0, 0), (1, 1), (1, 1)), mode="edge")
    H, W = gt.shape[1:]
    out = np.ones_like(ok)
    for dy in range(3):
        for dx in range(3):
            out &= p[:, dy:dy + H, dx:dx + W]
    return out


def cosine(pred, gtn):
    """pred [..., >=3], gtn [..., >=3] float32 -> (c float64 with NaN where the pixel is not valid, valid)."""
    assert pred.dtype == np.float32 and gtn.dtype == np.float32
    px, py, pz = (pred[..., i].astype(np.float64) for i in range(3))
    gx, gy, gz = (gtn[..., i].astype(np.float64) for i in range(3))
    with np.errstate(all="ignore"):
        d = (px * gx + py * gy) + pz * gz
        a2 = (px * px + py * py) + pz * pz
        b2 = (gx * gx + gy * gy) + gz * gz
        c = d / (np.sqrt(a2) * np.sqrt(b2))
        valid = (a2 > 0) & (b2 > 0) & np.isfinite(c)
    return np.where(valid, np.clip(c, -1.0, 1.0), np.nan), valid


def bins_of(c, edges):
    """#{ j : c <= edges[j-1] } over the strictly decreasing table."""
    return np.searchsorted(-edges, -c, side="right")


def in_class(mask, lo, hi):
    return np.ones(mask.shape, bool) if lo > hi else (mask >= lo) & (mask <= hi)


def stats(pred, gtn, gt, mask, classes, edges, gate, min_depth, max_depth):
    """pred [N,H,W,>=3] fp32, gtn [N,H,W,4] fp32, gt [N,H,W] fp32, mask [N,H,W] int or None, classes [(lo, hi)] ->
    dict(n [N,K] int64, bad [N,K] int64, sum_deg [N,K], sum_deg2 [N,K], hist [N,K,720] int64, err_deg [N,H,W] float64)."""
    N, H, W = gt.shape
    K = len(classes)
    min_depth, max_depth = np.float32(min_depth), np.float32(max_depth)
    ok = window_ok(gt, min_depth, max_depth, gate)
    c, valid = cosine(pred, gtn)
    valid &= ok
    theta = np.where(valid, np.arccos(np.where(valid, c, 0.0)) * DEG, np.nan)
    b = bins_of(np.where(valid, c, 0.0), edges)
    m = np.zeros((N, H, W), np.int64) if mask is None else mask.astype(np.int64)
    out = {"n": np.zeros((N, K), np.int64), "bad": np.zeros((N, K), np.int64), "sum_deg": np.zeros((N, K)),
           "sum_deg2": np.zeros((N, K)), "hist": np.zeros((N, K, BINS), np.int64), "err_deg": theta}
    for i in range(N):
        for k, (lo, hi) in enumerate(classes):
            sel = in_class(m[i], lo, hi)
            v = sel & valid[i]
            out["n"][i, k] = v.sum()
            out["bad"][i, k] = (sel & ok[i] & ~valid[i]).sum()
            t = theta[i][v]
            out["sum_deg"][i, k] = math.fsum(t)
            out["sum_deg2"][i, k] = math.fsum(t * t)
            out["hist"][i, k] = np.bincount(b[i][v], minlength=BINS)
    return out


def stats_loop(pred, gtn, gt, mask, classes, edges, gate, min_depth, max_depth):
    """The same, one pixel at a time."""
    N, H, W = gt.shape
    K = len(classes)
    lo_d, hi_d = np.float32(min_depth), np.float32(max_depth)
    out = {"n": np.zeros((N, K), np.int64), "bad": np.zeros((N, K), np.int64), "sum_deg": np.zeros((N, K)),
           "sum_deg2": np.zeros((N, K)), "hist": np.zeros((N, K, BINS), np.int64), "err_deg": np.full((N, H, W), np.nan)}
    for i in range(N):
        terms = [[] for _ in range(K)]
        for y in range(H):
            for x in range(W):
                if gate:
                    win = [gt[i, min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
                else:
                    win = [gt[i, y, x]]
                if not all(lo_d <= d <= hi_d for d in win):
                    continue
                px, py, pz = (np.float64(pred[i, y, x, j]) for j in range(3))
                gx, gy, gz = (np.float64(gtn[i, y, x, j]) for j in range(3))
                with np.errstate(all="ignore"):
                    d = (px * gx + py * gy) + pz * gz
                    a2 = (px * px + py * py) + pz * pz
                    b2 = (gx * gx + gy * gy) + gz * gz
                    c = d / (np.sqrt(a2) * np.sqrt(b2))
                valid = bool(a2 > 0 and b2 > 0 and np.isfinite(c))
                if valid:
                    c = min(max(c, -1.0), 1.0)
                    b = sum(1 for e in edges if c <= e)
                    theta = np.arccos(c) * DEG
                    out["err_deg"][i, y, x] = theta
                mv = 0 if mask is None else int(mask[i, y, x])
                for k, (lo, hi) in enumerate(classes):
                    if lo > hi or lo <= mv <= hi:
                        if valid:
                            out["n"][i, k] += 1
                            out["hist"][i, k, b] += 1
                            terms[k].append(theta)
                        else:
                            out["bad"][i, k] += 1
        for k in range(K):
            out["sum_deg"][i, k] = math.fsum(terms[k])
            out["sum_deg2"][i, k] = math.fsum(t * t for t in terms[k])
    return out


def gt_normals(gt, Kmat, min_depth, max_depth):
    """pd_gt_normals' definition in fp64 (csrc/loss.hip gt_normals_kernel: Sobel / 8 of the unprojected points with replicate
    padding, normalised cross product, zero outside [min, max]) rounded to fp32 -- close to the kernel's fp32 values, for
    building inputs on the host; tests that compare against the kernel feed it the kernel's own gtn."""
    N, H, W = gt.shape
    out = np.zeros((N, H, W, 4), np.float32)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    for i in range(N):
        fx, fy, cx, cy = Kmat[i, 0, 0], Kmat[i, 1, 1], Kmat[i, 0, 2], Kmat[i, 1, 2]
        d = gt[i].astype(np.float64)
        P = np.stack([(xs - cx) / fx * d, (ys - cy) / fy * d, d], -1)
        Pp = np.pad(P, ((1, 1), (1, 1), (0, 0)), mode="edge")
        A = np.zeros_like(P)
        B = np.zeros_like(P)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                v = Pp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                A += (2.0 if dy == 0 else 1.0) * dx * 0.125 * v
                B += (2.0 if dx == 0 else 1.0) * dy * 0.125 * v
        n = np.cross(A, B)
        n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-12)
        ok = (gt[i] >= np.float32(min_depth)) & (gt[i] <= np.float32(max_depth))
        out[i, ..., :3] = np.where(ok[..., None], n, 0.0).astype(np.float32)
    return out
