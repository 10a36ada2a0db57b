"""The NumPy statement of pd_unc_loss_fwd / _bwd (include/polardepth.h): the align_corners=False bilinear sampling of the
uncertainty map in the kernel's operation order, the mask, the Laplace scale log b = fma(u, log(b_hi / b_lo), log b_lo), the
per-pixel terms, their sums (math.fsum: the exactly rounded sum, which no order changes) and the analytic gradients with the
transposed bilinear fold.

``statement`` is the contract: sampling in fp32, everything after it in fp64 with an exactly rounded fma.  ``evaluate`` is the
same mathematics wholly in one precision (np.float32 or np.float64), the pair of yardsticks of the project's gradient rule
|dev - ref64| <= 4 max|ref32 - ref64| + 1e-6 max|ref64|."""
import math
from fractions import Fraction

import numpy as np

LN2 = 0.6931471805599453


def up_index(out_size, in_size, dtype):
    """(i0, i1, l1) of every destination index: pd_up::src_index in ``dtype``."""
    scale = dtype(in_size) / dtype(out_size)
    s = np.maximum(scale * (np.arange(out_size).astype(dtype) + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, (s - i0.astype(dtype)).astype(dtype)


def upsample(u, H, W, dtype=np.float32):
    """u [N,hs,ws] -> [N,H,W]: pd_up::sample, every operation in ``dtype`` and in the kernel's order."""
    u = u.astype(dtype)
    y0, y1, ly1 = up_index(H, u.shape[1], dtype)
    x0, x1, lx1 = up_index(W, u.shape[2], dtype)
    ly0, lx0 = dtype(1) - ly1, dtype(1) - lx1
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    with np.errstate(invalid="ignore"):
        top = lx0 * u[:, y0][:, :, x0] + lx1 * u[:, y0][:, :, x1]
        bot = lx0 * u[:, y1][:, :, x0] + lx1 * u[:, y1][:, :, x1]
        out = ly0 * top + ly1 * bot
    assert out.dtype == dtype
    return out


def fold(gup, hs, ws, dtype):
    """The transpose of ``upsample``: gup [N,H,W] -> [N,hs,ws], in ``dtype`` (the order of the additions is NumPy's)."""
    N, H, W = gup.shape
    y0, y1, ly1 = up_index(H, hs, dtype)
    x0, x1, lx1 = up_index(W, ws, dtype)
    out = np.zeros((N, hs, ws), dtype)
    g = gup.astype(dtype)
    for yi, wy in ((y0, dtype(1) - ly1), (y1, ly1)):
        for xi, wx in ((x0, dtype(1) - lx1), (x1, lx1)):
            w = wy[:, None] * wx[None, :]
            np.add.at(out, (slice(None), yi[:, None], xi[None, :]), g * w[None])
    return out


def fma64(a, b, c):
    """The exactly rounded a * b + c of float64 arrays a and scalars b, c (Python 3.10 has no math.fma)."""
    fb, fc = Fraction(float(b)), Fraction(float(c))
    flat = np.asarray(a, np.float64).ravel()
    out = np.array([float(Fraction(float(v)) * fb + fc) if math.isfinite(v) else v for v in flat], np.float64)
    return out.reshape(np.shape(a))


def mask_of(gt, valid, u_up, min_depth, max_depth):
    assert gt.dtype == np.float32
    with np.errstate(invalid="ignore"):
        m = (gt >= np.float32(min_depth)) & (gt <= np.float32(max_depth)) & np.isfinite(u_up)
    return m if valid is None else m & (valid != 0)


def _pixel(depth, gt, unc, b_range, min_depth, max_depth, valid, dtype, sample_dtype, exact_fma):
    N, H, W = gt.shape
    b_lo, b_hi = b_range
    log_lo, log_ratio = math.log(b_lo), math.log(b_hi / b_lo)
    u = upsample(unc, H, W, sample_dtype)
    m = mask_of(gt, valid, u, min_depth, max_depth)
    with np.errstate(all="ignore"):
        uu = np.where(m, u, 0).astype(dtype)
        logb = fma64(uu, log_ratio, log_lo) if exact_fma else uu * dtype(log_ratio) + dtype(log_lo)
        b = np.exp(logb)
        diff = np.where(m, depth.astype(dtype) - gt.astype(dtype), 0)
        e = np.abs(diff)
    assert b.dtype == dtype and e.dtype == dtype
    return m, e, b, logb, diff, dtype(log_ratio)


def _forward(m, e, b, logb, dtype, exact_sums):
    with np.errstate(all="ignore"):
        r, l2b = e / b, logb + dtype(LN2)
    if exact_sums:
        sums = np.array([math.fsum(r[m]), math.fsum(l2b[m]), float(m.sum()), math.fsum(b[m])])
    else:
        sums = np.array([r[m].sum(dtype=dtype), l2b[m].sum(dtype=dtype), dtype(m.sum()), b[m].sum(dtype=dtype)], dtype)
    value = (sums[0] + sums[1]) / sums[2] if sums[2] > 0 else sums.dtype.type(0)
    nan = dtype(np.nan)
    return {"m": m, "sums": sums, "value": value, "term": np.where(m, r + l2b, nan), "b": np.where(m, b, nan), "ratio": r,
            "l2b": l2b}


def statement(depth, gt, unc, b_range, min_depth, max_depth, valid=None):
    """depth, gt [N,H,W] fp32, unc [N,hs,ws] fp32, valid [N,H,W] or None -> dict(m, sums float64 [4], value float64 (the
    device rounds it to fp32), term, b float64 [N,H,W] with NaN outside the mask, ratio = e / b)."""
    m, e, b, logb, _, _ = _pixel(depth, gt, unc, b_range, min_depth, max_depth, valid, np.float64, np.float32, True)
    return _forward(m, e, b, logb, np.float64, True)


def evaluate(depth, gt, unc, b_range, min_depth, max_depth, valid=None, dtype=np.float64, gout=1.0, detach=False):
    """Value and gradients wholly in ``dtype``: dict(value, sums, term, b, gdepth [N,H,W] or None, gup [N,H,W], gunc
    [N,hs,ws])."""
    m, e, b, logb, diff, log_ratio = _pixel(depth, gt, unc, b_range, min_depth, max_depth, valid, dtype, dtype, False)
    out = _forward(m, e, b, logb, dtype, False)
    c = dtype(gout) / out["sums"][2] if out["sums"][2] > 0 else dtype(0)
    with np.errstate(all="ignore"):
        out["gdepth"] = None if detach else np.where(m, c * np.sign(diff) / b, dtype(0)).astype(dtype)
        out["gup"] = np.where(m, c * (dtype(1) - e / b) * log_ratio, dtype(0)).astype(dtype)
    out["gunc"] = fold(out["gup"], unc.shape[1], unc.shape[2], dtype)
    return out
