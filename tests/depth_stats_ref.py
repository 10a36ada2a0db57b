"""The NumPy statement of pd_depth_medians / pd_depth_stats (include/polardepth.h): the gate, the classes, the clamp, the
scale, the fp32 ratio counters, the fp64 sums (math.fsum: the exactly rounded sum, which no order changes) and the
searchsorted bins.  The medians are np.sort(...)[rank]."""
import math

import numpy as np

BINS = 512
A_THRESH = (np.float32(1.25), np.float32(1.5625), np.float32(1.953125))


def edges_numpy():
    return np.arange(1, BINS, dtype=np.float64) * 0.0005


def in_class(mask, lo, hi):
    return np.ones(mask.shape, bool) if lo > hi else (mask >= lo) & (mask <= hi)


def gate_of(gt, pred, min_depth, max_depth):
    """(passes the gate [N,H,W], finite prediction [N,H,W], p0 fp32 [N,H,W])"""
    assert gt.dtype == np.float32 and pred.dtype == np.float32
    lo, hi = np.float32(min_depth), np.float32(max_depth)
    with np.errstate(invalid="ignore"):
        ok = (gt > lo) & (gt < hi)
        p0 = np.minimum(np.maximum(pred, lo), hi)
    return ok, np.isfinite(pred), p0


def medians(pred, gt, mask, classes, min_depth, max_depth):
    """(n [N,K] int64, med [N,K,4] float32): ranks (n-1)//2 and n//2 of gt, then of p0, over S(n,k); NaN where n == 0."""
    N = gt.shape[0]
    ok, fin, p0 = gate_of(gt, pred, min_depth, max_depth)
    m = np.zeros(gt.shape, np.int64) if mask is None else mask.astype(np.int64)
    n = np.zeros((N, len(classes)), np.int64)
    med = np.full((N, len(classes), 4), np.nan, np.float32)
    for i in range(N):
        for k, (lo, hi) in enumerate(classes):
            sel = in_class(m[i], lo, hi) & ok[i] & fin[i]
            n[i, k] = c = int(sel.sum())
            if c:
                g, p = np.sort(gt[i][sel]), np.sort(p0[i][sel])
                med[i, k] = g[(c - 1) // 2], g[c // 2], p[(c - 1) // 2], p[c // 2]
    return n, med


def scale_of(med, how):
    """[N,K] float32: "numpy" = np.median on float32 (the mean of the two middle values), "torch" = the lower middle."""
    med = med.astype(np.float32)
    with np.errstate(all="ignore"):
        if how == "numpy":
            return ((med[..., 0] + med[..., 1]) / np.float32(2)) / ((med[..., 2] + med[..., 3]) / np.float32(2))
        assert how == "torch"
        return med[..., 0] / med[..., 2]


def terms(g, p):
    """g, p float32 [n] -> (ratio fp32, |d|, the four fp64 terms [n,4])"""
    with np.errstate(all="ignore"):
        ratio = np.maximum(g / p, p / g)
        assert ratio.dtype == np.float32
        gd, pd = g.astype(np.float64), p.astype(np.float64)
        d = gd - pd
        l = np.log1p(d / pd)
        return ratio, np.abs(d), np.stack([np.abs(d) / gd, d * d / gd, d * d, l * l], -1)


def stats(pred, gt, mask, classes, edges, min_depth, max_depth, scale=None):
    """pred, gt [N,H,W] fp32, mask [N,H,W] int or None, classes [(lo, hi)], scale None or [N,K] fp32 -> dict(n, a [N,K,3],
    bad, sums [N,K,4], hist [N,K,512] int64, err [N,H,W] float64 (the unscaled |g - p0|; NaN where gated out or bad))."""
    N, H, W = gt.shape
    K = len(classes)
    lo_d, hi_d = np.float32(min_depth), np.float32(max_depth)
    ok, fin, p0 = gate_of(gt, pred, min_depth, max_depth)
    m = np.zeros((N, H, W), np.int64) if mask is None else mask.astype(np.int64)
    with np.errstate(invalid="ignore"):
        err = np.where(ok & fin, np.abs(gt.astype(np.float64) - p0.astype(np.float64)), np.nan)
    out = {"n": np.zeros((N, K), np.int64), "a": np.zeros((N, K, 3), np.int64), "bad": np.zeros((N, K), np.int64),
           "sums": np.zeros((N, K, 4)), "hist": np.zeros((N, K, BINS), np.int64), "err": err}
    for i in range(N):
        for k, (lo, hi) in enumerate(classes):
            sel = in_class(m[i], lo, hi) & ok[i]
            f = np.float32(1) if scale is None else np.float32(scale[i, k])
            if not np.isfinite(f):
                out["bad"][i, k] = sel.sum()
                continue
            v = sel & fin[i]
            out["bad"][i, k] = (sel & ~fin[i]).sum()
            g, p = gt[i][v], p0[i][v]
            if scale is not None:
                p = np.minimum(np.maximum(p * f, lo_d), hi_d)
                assert p.dtype == np.float32
            ratio, ad, t = terms(g, p)
            out["n"][i, k] = v.sum()
            for j, th in enumerate(A_THRESH):
                out["a"][i, k, j] = (ratio < th).sum()
            out["sums"][i, k] = [math.fsum(t[:, j]) for j in range(4)]
            out["hist"][i, k] = np.bincount(np.searchsorted(edges, ad, side="right"), minlength=BINS)
    return out


def errors_from(st, i, k):
    """The reference's seven figures (compute_depth_errors_numpy's order) from record [i, k]."""
    n = float(st["n"][i, k])
    s = st["sums"][i, k]
    return np.array([s[0] / n, s[1] / n, math.sqrt(s[2] / n), math.sqrt(s[3] / n)] + [a / n for a in st["a"][i, k]])
