"""The NumPy statement of pd_unc_stats (include/polardepth.h): the gate, the classes and the clamp of pd_depth_stats
(tests/depth_stats_ref.py), the Laplace scale of tests/unc_loss_ref.py, the two coverage counters decided in fp64, the fp64
sums (math.fsum), the histogram of the uncertainty bin and the three integer tables -- and the exact-sort sparsification
against which the binned one of polardepth/uncertainty_eval.py is checked."""
import math

import numpy as np

import depth_stats_ref as D
from unc_loss_ref import LN2, fma64

BINS = 512
LN10 = 2.302585092994046


def scale(unc, b_range):
    """(b, log b) float64 of fp32 u, with the exactly rounded fma of the definition."""
    logb = fma64(unc.astype(np.float64), math.log(b_range[1] / b_range[0]), math.log(b_range[0]))
    return np.exp(logb), logb


def pixels(pred, gt, unc, b_range, min_depth, max_depth):
    """Per pixel: (passes the gate, usable = finite pred and 0 <= u <= 1, e, b, log b, e_um int64, ub, eb)."""
    ok, fin, p0 = D.gate_of(gt, pred, min_depth, max_depth)
    with np.errstate(invalid="ignore"):
        good = fin & (unc >= 0) & (unc <= 1)
        u = np.where(good, unc, np.float32(0))
        e = np.where(ok & good, np.abs(gt.astype(np.float64) - p0.astype(np.float64)), 0.0)
    b, logb = scale(u, b_range)
    e_um = np.rint(e * 1e6).astype(np.int64)
    ub = np.minimum(BINS - 1, (u * np.float32(512)).astype(np.int64))
    eb = np.searchsorted(D.edges_numpy(), e, side="right")
    return ok, good, e, b, logb, e_um, ub, eb


def stats(pred, gt, unc, mask, classes, b_range, min_depth, max_depth):
    """pred, gt, unc [N,H,W] fp32, mask [N,H,W] int or None, classes [(lo, hi)] -> dict(n, bad, cover [N,K,2], sums [N,K,3]
    (nll, b, e), hist [N,K,512], tables [N,K,3,512]; all integers int64)."""
    N, H, W = gt.shape
    K = len(classes)
    ok, good, e, b, logb, e_um, ub, eb = pixels(pred, gt, unc, b_range, min_depth, max_depth)
    m = np.zeros((N, H, W), np.int64) if mask is None else mask.astype(np.int64)
    nll = e / b + (logb + LN2)
    c50, c90 = e <= b * LN2, e <= b * LN10
    out = {"n": np.zeros((N, K), np.int64), "bad": np.zeros((N, K), np.int64), "cover": np.zeros((N, K, 2), np.int64),
           "sums": np.zeros((N, K, 3)), "hist": np.zeros((N, K, BINS), np.int64), "tables": np.zeros((N, K, 3, BINS), np.int64)}
    for i in range(N):
        for k, (lo, hi) in enumerate(classes):
            sel = D.in_class(m[i], lo, hi) & ok[i]
            v = sel & good[i]
            out["bad"][i, k] = (sel & ~good[i]).sum()
            out["n"][i, k] = v.sum()
            out["cover"][i, k] = c50[i][v].sum(), c90[i][v].sum()
            out["sums"][i, k] = math.fsum(nll[i][v]), math.fsum(b[i][v]), math.fsum(e[i][v])
            out["hist"][i, k] = np.bincount(ub[i][v], minlength=BINS)
            np.add.at(out["tables"][i, k, 0], ub[i][v], e_um[i][v])
            out["tables"][i, k, 1] = np.bincount(eb[i][v], minlength=BINS)
            np.add.at(out["tables"][i, k, 2], eb[i][v], e_um[i][v])
    return out


def decision_margin(pred, gt, unc, b_range, min_depth, max_depth):
    """The smallest relative distance of any counted pixel's e from b ln 2 and b ln 10: a 1-ulp difference of exp cannot flip a
    coverage decision while this is far above 2^-52."""
    ok, good, e, b, *_ = pixels(pred, gt, unc, b_range, min_depth, max_depth)
    v = ok & good
    if not v.any():
        return np.inf
    return min(np.min(np.abs(e[v] - b[v] * t) / (b[v] * t)) for t in (LN2, LN10))


# ------------------------------------------------------------------------------------------------ exact sparsification
def exact_curve(key, err, steps=100):
    """The mean of ``err`` over what is left after removing the fraction i / steps of the items, largest ``key`` first (a
    stable sort; the item in which the removed count ends is removed proportionally).  err in any unit; float64 [steps]."""
    order = np.argsort(-np.asarray(key, np.float64), kind="stable")
    e = np.asarray(err, np.float64)[order]
    n = e.size
    cs = np.concatenate([[0.0], np.cumsum(e)])
    r = np.arange(steps) * n / steps
    j = np.minimum(np.floor(r).astype(np.int64), n - 1)
    removed = cs[j] + (r - j) * e[j]
    return (cs[-1] - removed) / (n - r)


def exact_figures(u, err_mm):
    """(AUSE, AURG) in the unit of ``err_mm`` from per-pixel u and error, by sorting."""
    s, o = exact_curve(u, err_mm), exact_curve(err_mm, err_mm)
    return float(np.mean(s - o)), float(np.mean(s[0] - s)), s, o
