"""NumPy restatement of csrc/student.hip (include/polardepth.h, "cost-volume student's step"): the consistency masks, the
adaptive depth-bin tracker and the masked reprojection / consistency loss of the reference's --train_student branch
(trainer.py:617-627, 650-664, 1112-1124, 1202-1236).  Per-pixel arithmetic in fp32, one rounding per operation; sums in fp64."""
import math

import numpy as np

import reproj_ref

F32, F64 = np.float32, np.float64


def _fsum(a):
    a = np.asarray(a, F64).ravel()
    return math.fsum(a) if np.isfinite(a).all() else float(a.sum(dtype=F64))


def masks(lowest, confidence, mono_depth, aug=None, motion_masking=True):
    """pd_student_masks: dict(rmask [N,H,W] uint8, cmask [N,H,W] fp32, lowest_up [N,H,W] fp32, minmax [N,2] fp32)."""
    lowest, confidence, mono = (np.asarray(a, F32) for a in (lowest, confidence, mono_depth))
    N, h, w = lowest.shape
    assert mono.shape == (N, 1, 4 * h, 4 * w)
    up = lambda a: a.repeat(4, axis=1).repeat(4, axis=2)            # pixel (y, x) reads (y >> 2, x >> 2)
    low, conf, t = up(lowest), up(confidence) != 0, mono[:, 0]
    with np.errstate(all="ignore"):
        md = (F32(1.0) / low).astype(F32)
        mm = (((md - t).astype(F32) / t).astype(F32) < 1) & (((t - md).astype(F32) / md).astype(F32) < 1)
    cm = conf & (mm if motion_masking else True)
    rm = (cm if motion_masking else np.ones_like(cm))
    if aug is not None:
        rm = rm & ~(np.asarray(aug, F32) != 0)[:, None, None]
    flat = t.reshape(N, -1)
    has_nan = np.isnan(flat).any(1)
    with np.errstate(all="ignore"):
        mnmx = np.stack([np.where(has_nan, F32(np.nan), np.nanmin(np.where(np.isnan(flat), np.inf, flat), 1)),
                         np.where(has_nan, F32(np.nan), np.nanmax(np.where(np.isnan(flat), -np.inf, flat), 1))], 1).astype(F32)
    return {"rmask": rm.astype(np.uint8), "cmask": cm.astype(F32), "lowest_up": low.copy(), "minmax": mnmx, "mm": mm, "conf": conf}


def linspace(start, stop, D):
    """numpy.linspace(start, stop, D) in fp64, spelled out as the header states it."""
    start, stop = F64(start), F64(stop)
    with np.errstate(all="ignore"):
        delta = stop - start
        j = np.arange(D, dtype=F64)
        if D == 1:
            return j * delta + start
        step = delta / F64(D - 1)
        y = (j / F64(D - 1)) * delta if step == 0 else j * step
        y = y + start
        y[-1] = stop
    return y


def bins_of(tmin, tmax, D, binning):
    with np.errstate(all="ignore"):
        if binning == "inverse":
            return (F64(1) / linspace(F64(1) / F64(tmax), F64(1) / F64(tmin), D)[::-1]).astype(F32)
        return linspace(tmin, tmax, D).astype(F32)


def bins_update(minmax, tracker, floor_depth, D, binning):
    """pd_depth_bins_update: (new tracker (min, max) as two Python floats, bins [D] fp32)."""
    minmax = np.asarray(minmax, F32)
    N = minmax.shape[0]
    smn, smx = F32(0), F32(0)
    with np.errstate(all="ignore"):
        for n in range(N):
            smn = F32(smn + minmax[n, 0])
            smx = F32(smx + minmax[n, 1])
        mn, mx = float(F32(smn / F32(N))), float(F32(smx / F32(N)))
        lo = mn * 0.9
        mn64 = lo if lo > floor_depth else float(floor_depth)
        mx64 = mx * 1.1
        tmin = float(tracker[0]) * 0.99 + mn64 * 0.01
        tmax = float(tracker[1]) * 0.99 + mx64 * 0.01
    return (tmin, tmax), bins_of(tmin, tmax, D, binning)


def combine(reproj, rmask, multi_depth, mono_depth, valid=None, avg=False):
    """pd_student_combine_fwd: dict(sel, r [N,H,W] fp32, sums (3 fp64), abs_sums (the same over |term|), loss (2 fp32), m)."""
    base = reproj_ref.combine(reproj, valid=valid, avg=avg)
    m = base["value"].astype(F32)
    N, H, W = m.shape
    keep = (np.asarray(rmask) != 0) & np.broadcast_to(base["nvalid"] > 0, (N, H, W))
    r = keep.astype(F32)
    multi, mono = np.asarray(multi_depth, F32)[:, 0], np.asarray(mono_depth, F32)[:, 0]
    with np.errstate(all="ignore"):
        t0 = (m * r).astype(F32).astype(F64)
        t2 = (np.abs((multi - mono).astype(F32)) * (F32(1) - r)).astype(F32).astype(F64)
        sums = np.array([_fsum(t0), _fsum(r.astype(F64)), _fsum(t2)], F64)         # correctly rounded sums
        abs_sums = np.array([_fsum(np.abs(t0)), sums[1], _fsum(np.abs(t2))], F64)
        loss = np.array([sums[0] / (sums[1] + 1e-7), sums[2] / F64(N * H * W)], F64).astype(F32)
    sel = np.where(keep, base["sel"] if not avg else 0, 255).astype(np.uint8)
    return {"sel": sel, "r": r, "sums": sums, "abs_sums": abs_sums, "loss": loss, "m": m}


def combine_grad(gloss, sel, sums, multi_depth, mono_depth, valid, F, avg=False):
    """pd_student_combine_bwd from the forward's own sums: (greproj: F maps [N,1,H,W] fp32, gmulti [N,1,H,W] fp32)."""
    sel = np.asarray(sel)
    N, H, W = sel.shape
    gloss = np.asarray(gloss, F32)
    val = np.ones((N, F), bool) if valid is None else np.asarray(valid) != 0
    with np.errstate(all="ignore"):
        g = F32(F64(gloss[0]) / (F64(sums[1]) + 1e-7))
        gc = F32(F64(gloss[1]) / F64(N * H * W))
        nv = val.sum(1)[:, None, None]
        greproj = []
        for f in range(F):
            if avg:
                ga = (g / np.maximum(nv, 1).astype(F32)).astype(F32)
                greproj.append(np.where((sel != 255) & val[:, f][:, None, None] & (nv > 0), ga, F32(0)).astype(F32)[:, None])
            else:
                greproj.append(np.where(sel == f, g, F32(0)).astype(F32)[:, None])
        d = (np.asarray(multi_depth, F32) - np.asarray(mono_depth, F32)).astype(F32)[:, 0]
        sg = (d > 0).astype(F32) - (d < 0).astype(F32)              # sign(0) = sign(NaN) = 0
        gmulti = ((gc * sg).astype(F32) * (sel == 255).astype(F32)).astype(F32)[:, None]
    return greproj, gmulti
