"""The statement of the per-pixel viewing-ray frame (csrc/ray_frame.hpp, include/polardepth.h) and of the evaluator and the
loss in it (pd_polar_normals_stats_ray, pd_polar_loss_fwd_ray / _bwd_ray), for the tests.  It stands beside
tests/polar_normals_ref.py and tests/polar_loss_ref.py, which stay the statements of the orthographic convention; with
``ray_frame=False`` everything here equals them bit for bit.

R(x, y) is the minimal rotation that takes the unit viewing ray u of the integer pixel (x, y) onto (0, 0, 1).  fp64 from the
fp32 intrinsics, only + - x / sqrt, in exactly this order:

    xt = (double(x) - cx) / fx          yt = (double(y) - cy) / fy
    L  = sqrt((xt*xt + yt*yt) + 1.0)    ux = xt / L    uy = yt / L    uz = 1.0 / L
    R p:    d = (px*ux + py*uy) + pz*uz     s = (d + pz) / (1.0 + uz)     p' = (px - s*ux, py - s*uy, d)
    R^T g:  d = (gx*ux + gy*uy) + gz*uz     s = (d + gz) / (1.0 + uz)     t = 2.0*gz
            ((gx - s*ux) + t*ux, (gy - s*uy) + t*uy, (gz - s*(uz + 1.0)) + t*uz)

In ray mode p' replaces the fp64 p from the `bad` gate on: a2, t2, m, q are formed from p' as the two statements form them
from p; the orientation p'z >= 0 is the visibility condition p.u >= 0; `frontal` means too frontal to the ray; the NEGATED bit
of the loss's state byte means p'z < 0.  ``pol_normal`` is R^T of the winning candidate on the prediction's side, formed in
fp64 and rounded once: a camera-frame normal map.  ``stats`` / ``terms`` are vectorised, ``stats_loop`` / ``terms_loop`` the
per-pixel loops they must equal bit for bit.  ``torch_loss`` restates the two values in torch from the DEPTH with the decisions
of a given state held fixed; autograd through it is the reference gradient (no gradient with respect to K)."""
import numpy as np
import torch

import polar_loss_ref as LR
import polar_normals_ref as NR
from oracle import losses as ol

f64 = np.float64


# ---- the frame

def frame1(fx, fy, cx, cy, x, y):
    """(ux, uy, uz) of one pixel; fx, fy, cx, cy fp32 scalars."""
    with np.errstate(all="ignore"):
        xt = (f64(x) - f64(cx)) / f64(fx)
        yt = (f64(y) - f64(cy)) / f64(fy)
        L = np.sqrt((xt * xt + yt * yt) + f64(1.0))
        return xt / L, yt / L, f64(1.0) / L


def frame(K, H, W):
    """K [N,4,4] fp32 -> (ux, uy, uz), each float64 [N,H,W]."""
    K = np.asarray(K)
    assert K.dtype == np.float32
    fx, fy, cx, cy = (K[:, i, j].astype(f64)[:, None, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    ys, xs = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    with np.errstate(all="ignore"):
        xt = (xs[None] - cx) / fx
        yt = (ys[None] - cy) / fy
        L = np.sqrt((xt * xt + yt * yt) + 1.0)
        return xt / L, yt / L, 1.0 / L


def rotate(u, px, py, pz):
    """R p; scalars or arrays of fp64."""
    ux, uy, uz = u
    with np.errstate(all="ignore"):
        d = (px * ux + py * uy) + pz * uz
        s = (d + pz) / (1.0 + uz)
        return px - s * ux, py - s * uy, d


def rotate_t(u, gx, gy, gz):
    """R^T g."""
    ux, uy, uz = u
    with np.errstate(all="ignore"):
        d = (gx * ux + gy * uy) + gz * uz
        s = (d + gz) / (1.0 + uz)
        t = 2.0 * gz
        return (gx - s * ux) + t * ux, (gy - s * uy) + t * uy, (gz - s * (uz + 1.0)) + t * uz


def _p64(pred, K, ray_frame):
    N, H, W = pred.shape[:3]
    px, py, pz = (pred[..., i].astype(f64) for i in range(3))
    if not ray_frame:
        return None, px, py, pz
    u = frame(K, H, W)
    return (u,) + rotate(u, px, py, pz)


# ---- the evaluator

def stats(pred, pol, xolp, mask, classes, edges, K=None, ray_frame=False, valid=None, rho_min=0.05, rho_max=1.0, tilt2_min=0.0,
          aolp_sign=1):
    """polar_normals_ref.stats on p' = R p (ray_frame) or on p; K [N,4,4] fp32 is needed with ray_frame.  Same result dict."""
    assert pred.dtype == np.float32 and pol.dtype == np.float32 and xolp.dtype == np.float32
    N, H, W = pred.shape[:3]
    Kc = len(classes)
    out = NR._empty(N, Kc, H, W)
    rmin, rmax, sign = f64(np.float32(rho_min)), f64(np.float32(rho_max)), f64(aolp_sign)
    rho = xolp[:, 0, :, :W].astype(f64)
    live = np.ones((N, H, W), bool) if valid is None else valid != 0
    u, px, py, pz = _p64(pred, K, ray_frame)
    C = pol[:, :, :, :W].astype(f64)
    cx, cy, cz = C[:, 0::3], sign * C[:, 1::3], C[:, 2::3]
    with np.errstate(all="ignore"):
        dolp_out = live & (~np.isfinite(rho) | (rho < rmin) | (rho > rmax))
        a2 = (px * px + py * py) + pz * pz
        b2 = (cx * cx + cy * cy) + cz * cz
        good = np.isfinite(a2) & (a2 > 0) & np.isfinite(C).all(1) & (b2 > 0).any(1)
        bad = live & ~dolp_out & ~good
        ok = live & ~dolp_out & good
        neg = ok & (pz < 0)
        px, py, pz = (np.where(neg, -v, v) for v in (px, py, pz))

        best = np.full((N, H, W), -np.inf)
        win = np.full((N, H, W), -1, np.int64)
        sa = np.sqrt(a2)
        for b in range(3):
            m = px * cx[:, b] + py * cy[:, b]
            q = pz * cz[:, b]
            den = sa * np.sqrt(b2[:, b])
            for j, c in enumerate(((m + q) / den, (-m + q) / den)):
                better = ok & (b2[:, b] > 0) & np.isfinite(c) & (c > best)
                best = np.where(better, c, best)
                win = np.where(better, 2 * b + j, win)
        cn = ok & (win >= 0)
        bad_n = bad | (ok & (win < 0))
        c = np.clip(np.where(cn, best, 0.0), -1.0, 1.0)
        bin_n = NR.bins_of(c, edges)
        deg_n = np.arccos(c) * NR.DEG
        out["n_deg"] = np.where(cn, deg_n, np.nan)
        out["choice"] = np.where(cn, win + 1, 0).astype(np.uint8)
        wb = np.clip(win, 0, 5) // 2
        take = lambda v: np.take_along_axis(v, wb[:, None], 1)[:, 0]
        ox, oy, oz = take(cx), take(cy), take(cz)
        flip = cn & (win % 2 == 1)
        ox, oy = np.where(flip, -ox, ox), np.where(flip, -oy, oy)
        ox, oy, oz = (np.where(neg, -v, v) for v in (ox, oy, oz))
        if ray_frame:
            ox, oy, oz = rotate_t(u, ox, oy, oz)                                   # back to camera coordinates
        for i, v in enumerate((ox, oy, oz)):
            out["pol_normal"][..., i] = np.where(cn, v, 0.0).astype(np.float32)

        t2 = px * px + py * py
        ud = cx[:, 0] * cx[:, 0] + cy[:, 0] * cy[:, 0]
        us = cx[:, 1] * cx[:, 1] + cy[:, 1] * cy[:, 1]
        frontal = ok & ((t2 <= f64(tilt2_min) * a2) | ~((ud > 0) | (us > 0)))
        ca = ok & ~frontal
        st = np.sqrt(t2)
        cd = np.where(ud > 0, np.minimum(np.abs(px * cx[:, 0] + py * cy[:, 0]) / (st * np.sqrt(ud)), 1.0), -1.0)
        cs = np.where(us > 0, np.minimum(np.abs(px * cx[:, 1] + py * cy[:, 1]) / (st * np.sqrt(us)), 1.0), -1.0)
        c = np.where(ca, np.maximum(cd, cs), 1.0)
        spec_a = ca & (cs > cd)
        bin_a = NR.bins_of(c, edges[:NR.ABINS - 1])
        deg_a = np.arccos(c) * NR.DEG
        out["az_deg"] = np.where(ca, deg_a, np.nan)

    mk = np.zeros((N, H, W), np.int64) if mask is None else mask.astype(np.int64)
    for i in range(N):
        for k, (lo, hi) in enumerate(classes):
            sel = NR.in_class(mk[i], lo, hi)
            for name, counts, bins, deg, nb, flags in (
                    ("normal", cn, bin_n, deg_n, NR.NBINS, {"bad": bad_n, "dolp_out": dolp_out, "spec": cn & (win >= 2), "flipped": flip}),
                    ("azimuth", ca, bin_a, deg_a, NR.ABINS, {"bad": bad, "dolp_out": dolp_out, "frontal": frontal, "spec": spec_a})):
                r = out[name]
                v = sel & counts[i]
                r["n"][i, k] = v.sum()
                for f, a in flags.items():
                    r[f][i, k] = (sel & a[i]).sum()
                r["sums"][i, k] = NR._fsums(deg[i][v], rho[i][v])
                r["hist"][i, k] = np.bincount(bins[i][v], minlength=nb)
    return out


def stats_loop(pred, pol, xolp, mask, classes, edges, K=None, ray_frame=False, valid=None, rho_min=0.05, rho_max=1.0,
               tilt2_min=0.0, aolp_sign=1):
    """The same, one pixel at a time."""
    N, H, W = pred.shape[:3]
    Kc = len(classes)
    out = NR._empty(N, Kc, H, W)
    rmin, rmax, sign, tilt2 = f64(np.float32(rho_min)), f64(np.float32(rho_max)), f64(aolp_sign), f64(tilt2_min)
    for i in range(N):
        terms_ = {"normal": [([], []) for _ in range(Kc)], "azimuth": [([], []) for _ in range(Kc)]}
        for y in range(H):
            for x in range(W):
                if valid is not None and not valid[i, y, x]:
                    continue
                mv = 0 if mask is None else int(mask[i, y, x])
                mine = [k for k, (lo, hi) in enumerate(classes) if lo > hi or lo <= mv <= hi]
                rho = f64(xolp[i, 0, y, x])

                def count(name, field):
                    for k in mine:
                        out[name][field][i, k] += 1

                if not np.isfinite(rho) or rho < rmin or rho > rmax:
                    count("normal", "dolp_out")
                    count("azimuth", "dolp_out")
                    continue
                px, py, pz = (f64(pred[i, y, x, j]) for j in range(3))
                u = None
                if ray_frame:
                    u = frame1(K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2], x, y)
                    px, py, pz = rotate(u, px, py, pz)
                cand = [(f64(pol[i, 3 * b, y, x]), sign * f64(pol[i, 3 * b + 1, y, x]), f64(pol[i, 3 * b + 2, y, x]))
                        for b in range(3)]
                with np.errstate(all="ignore"):
                    a2 = (px * px + py * py) + pz * pz
                    b2 = [(cx * cx + cy * cy) + cz * cz for cx, cy, cz in cand]
                if not (np.isfinite(a2) and a2 > 0 and all(np.isfinite(v) for c3 in cand for v in c3) and any(b > 0 for b in b2)):
                    count("normal", "bad")
                    count("azimuth", "bad")
                    continue
                neg = bool(pz < 0)
                if neg:
                    px, py, pz = -px, -py, -pz
                best, win = -np.inf, -1
                for b, (cx, cy, cz) in enumerate(cand):
                    if not b2[b] > 0:
                        continue
                    m = px * cx + py * cy
                    q = pz * cz
                    den = np.sqrt(a2) * np.sqrt(b2[b])
                    for j, c in enumerate(((m + q) / den, (-m + q) / den)):
                        if np.isfinite(c) and c > best:
                            best, win = c, 2 * b + j
                if win < 0:
                    count("normal", "bad")
                else:
                    c = min(max(best, -1.0), 1.0)
                    bn = sum(1 for e in edges if c <= e)
                    deg = np.arccos(c) * NR.DEG
                    out["n_deg"][i, y, x] = deg
                    out["choice"][i, y, x] = win + 1
                    cx, cy, cz = cand[win // 2]
                    if win % 2:
                        cx, cy = -cx, -cy
                    if neg:
                        cx, cy, cz = -cx, -cy, -cz
                    if ray_frame:
                        cx, cy, cz = rotate_t(u, cx, cy, cz)
                    out["pol_normal"][i, y, x] = (np.float32(cx), np.float32(cy), np.float32(cz), np.float32(0))
                    for k in mine:
                        out["normal"]["n"][i, k] += 1
                        out["normal"]["hist"][i, k, bn] += 1
                        terms_["normal"][k][0].append(deg)
                        terms_["normal"][k][1].append(rho)
                    if win >= 2:
                        count("normal", "spec")
                    if win % 2:
                        count("normal", "flipped")
                t2 = px * px + py * py
                u2 = [cand[b][0] * cand[b][0] + cand[b][1] * cand[b][1] for b in (0, 1)]
                if t2 <= tilt2 * a2 or not (u2[0] > 0 or u2[1] > 0):
                    count("azimuth", "frontal")
                    continue
                cb = [min(abs(px * cand[b][0] + py * cand[b][1]) / (np.sqrt(t2) * np.sqrt(u2[b])), 1.0) if u2[b] > 0 else -1.0
                      for b in (0, 1)]
                c = max(cb)
                ba = sum(1 for e in edges[:NR.ABINS - 1] if c <= e)
                deg = np.arccos(c) * NR.DEG
                out["az_deg"][i, y, x] = deg
                for k in mine:
                    out["azimuth"]["n"][i, k] += 1
                    out["azimuth"]["hist"][i, k, ba] += 1
                    terms_["azimuth"][k][0].append(deg)
                    terms_["azimuth"][k][1].append(rho)
                if cb[1] > cb[0]:
                    count("azimuth", "spec")
        for name in ("normal", "azimuth"):
            for k in range(Kc):
                d, r = (np.array(t, f64) for t in terms_[name][k])
                out[name]["sums"][i, k] = NR._fsums(d, r)
    return out


# ---- the loss

def terms(p, pol, xolp, valid=None, K=None, ray_frame=False, rho_min=0.05, rho_max=1.0, tilt2_min=0.0, aolp_sign=1,
          dolp_weighted=True):
    """polar_loss_ref.terms on p' = R p (ray_frame) or on p.  Same result dict."""
    assert p.dtype == np.float32 and pol.dtype == np.float32 and xolp.dtype == np.float32
    N, H, W = p.shape[:3]
    rmin, rmax, sign = f64(np.float32(rho_min)), f64(np.float32(rho_max)), f64(aolp_sign)
    rho = xolp[:, 0, :, :W].astype(f64)
    live = np.ones((N, H, W), bool) if valid is None else np.asarray(valid) != 0
    _, px, py, pz = _p64(p, K, ray_frame)
    C = pol[:, :, :, :W].astype(f64)
    cx, cy, cz = C[:, 0::3], sign * C[:, 1::3], C[:, 2::3]
    with np.errstate(all="ignore"):
        dolp_out = live & (~np.isfinite(rho) | (rho < rmin) | (rho > rmax))
        a2 = (px * px + py * py) + pz * pz
        b2 = (cx * cx + cy * cy) + cz * cz
        good = np.isfinite(a2) & (a2 > 0) & np.isfinite(C).all(1) & (b2 > 0).any(1)
        bad = live & ~dolp_out & ~good
        ok = live & ~dolp_out & good
        neg = ok & (pz < 0)
        px, py, pz = (np.where(neg, -v, v) for v in (px, py, pz))
        best = np.full((N, H, W), -np.inf)
        win = np.full((N, H, W), -1, np.int64)
        sa = np.sqrt(a2)
        for b in range(3):
            m = px * cx[:, b] + py * cy[:, b]
            q = pz * cz[:, b]
            den = sa * np.sqrt(b2[:, b])
            for j, c in enumerate(((m + q) / den, (-m + q) / den)):
                better = ok & (b2[:, b] > 0) & np.isfinite(c) & (c > best)
                best = np.where(better, c, best)
                win = np.where(better, 2 * b + j, win)
        cn = ok & (win >= 0)
        l_n = np.where(cn, 1.0 - np.minimum(np.maximum(best, -1.0), 1.0), np.nan)
        t2 = px * px + py * py
        md, ms = px * cx[:, 0] + py * cy[:, 0], px * cx[:, 1] + py * cy[:, 1]
        ud, us = cx[:, 0] * cx[:, 0] + cy[:, 0] * cy[:, 0], cx[:, 1] * cx[:, 1] + cy[:, 1] * cy[:, 1]
        frontal = ok & ((t2 <= f64(tilt2_min) * a2) | ~((ud > 0) | (us > 0)))
        ca = ok & ~frontal
        st = np.sqrt(t2)
        cd = np.where(ud > 0, np.minimum(np.abs(md) / (st * np.sqrt(ud)), 1.0), -1.0)
        cs = np.where(us > 0, np.minimum(np.abs(ms) / (st * np.sqrt(us)), 1.0), -1.0)
        spec = ca & (cs > cd)
        m, u2 = np.where(spec, ms, md), np.where(spec, us, ud)
        l_a = np.where(ca, np.minimum(np.maximum(1.0 - (m * m) / (t2 * u2), 0.0), 1.0), np.nan)
    gate = np.where(~live, LR.GATE_INVALID, np.where(dolp_out, LR.GATE_DOLP_OUT, np.where(bad, LR.GATE_BAD, LR.GATE_NONE)))
    branch = np.where(ca, np.where(spec, LR.BR_S, LR.BR_D), LR.BR_NONE)
    out = {"state": LR._pack(np.where(cn, win + 1, 0), neg, branch, gate), "l_n": l_n, "l_a": l_a}
    return LR._finish(out, rho, dolp_weighted)


def terms_loop(p, pol, xolp, valid=None, K=None, ray_frame=False, rho_min=0.05, rho_max=1.0, tilt2_min=0.0, aolp_sign=1,
               dolp_weighted=True):
    """The same, one pixel at a time."""
    N, H, W = p.shape[:3]
    rmin, rmax, sign, tilt2 = f64(np.float32(rho_min)), f64(np.float32(rho_max)), f64(aolp_sign), f64(tilt2_min)
    state = np.zeros((N, H, W), np.uint8)
    l_n, l_a = np.full((N, H, W), np.nan), np.full((N, H, W), np.nan)
    for i in range(N):
        for y in range(H):
            for x in range(W):
                if valid is not None and not valid[i, y, x]:
                    state[i, y, x] = LR.GATE_INVALID << LR.GATE_SHIFT
                    continue
                rho = f64(xolp[i, 0, y, x])
                if not np.isfinite(rho) or rho < rmin or rho > rmax:
                    state[i, y, x] = LR.GATE_DOLP_OUT << LR.GATE_SHIFT
                    continue
                px, py, pz = (f64(p[i, y, x, j]) for j in range(3))
                if ray_frame:
                    px, py, pz = rotate(frame1(K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2], x, y), px, py, pz)
                cand = [(f64(pol[i, 3 * b, y, x]), sign * f64(pol[i, 3 * b + 1, y, x]), f64(pol[i, 3 * b + 2, y, x]))
                        for b in range(3)]
                with np.errstate(all="ignore"):
                    a2 = (px * px + py * py) + pz * pz
                    b2 = [(cx * cx + cy * cy) + cz * cz for cx, cy, cz in cand]
                    if not (np.isfinite(a2) and a2 > 0 and all(np.isfinite(v) for c3 in cand for v in c3) and any(b > 0 for b in b2)):
                        state[i, y, x] = LR.GATE_BAD << LR.GATE_SHIFT
                        continue
                    s = 0
                    if pz < 0:
                        px, py, pz = -px, -py, -pz
                        s |= LR.NEGATED
                    best, win = -np.inf, -1
                    for b, (cx, cy, cz) in enumerate(cand):
                        if not b2[b] > 0:
                            continue
                        m = px * cx + py * cy
                        q = pz * cz
                        den = np.sqrt(a2) * np.sqrt(b2[b])
                        for j, c in enumerate(((m + q) / den, (-m + q) / den)):
                            if np.isfinite(c) and c > best:
                                best, win = c, 2 * b + j
                    if win >= 0:
                        s |= win + 1
                        l_n[i, y, x] = 1.0 - min(max(best, -1.0), 1.0)
                    t2 = px * px + py * py
                    u2 = [cand[b][0] * cand[b][0] + cand[b][1] * cand[b][1] for b in (0, 1)]
                    if not (t2 <= tilt2 * a2 or not (u2[0] > 0 or u2[1] > 0)):
                        mb = [px * cand[b][0] + py * cand[b][1] for b in (0, 1)]
                        cb = [min(abs(mb[b]) / (np.sqrt(t2) * np.sqrt(u2[b])), 1.0) if u2[b] > 0 else -1.0 for b in (0, 1)]
                        b = 1 if cb[1] > cb[0] else 0
                        s |= (LR.BR_S if b else LR.BR_D) << LR.BRANCH_SHIFT
                        l_a[i, y, x] = min(max(1.0 - (mb[b] * mb[b]) / (t2 * u2[b]), 0.0), 1.0)
                    state[i, y, x] = s
    rho = xolp[:, 0, :, :W].astype(f64)
    return LR._finish({"state": state, "l_n": l_n, "l_a": l_a}, rho, dolp_weighted)


# ---- the reference gradient

def torch_frame(K, H, W, dt):
    """(ux, uy, uz) [N,H,W] in dtype dt (no gradient with respect to K)."""
    K = torch.as_tensor(np.asarray(K)).to(dt)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    xt = (xs[None] - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None]
    yt = (ys[None] - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None]
    L = torch.sqrt(xt * xt + yt * yt + 1.0)
    return xt / L, yt / L, 1.0 / L


def torch_loss(depth, K, pol, xolp, state, dt, aolp_sign=1, dolp_weighted=True, ray_frame=True):
    """(L_n, L_a) in dtype ``dt`` from depth [N,1,H,W] with the decisions of ``state`` held fixed: polar_loss_ref.torch_loss
    with p' = R p in place of p."""
    if not ray_frame:
        return LR.torch_loss(depth, K, pol, xolp, state, dt, aolp_sign=aolp_sign, dolp_weighted=dolp_weighted)
    N, _, H, W = depth.shape
    st = torch.as_tensor(np.asarray(state)).long()
    win, neg, branch = st & LR.WINNER, (st & LR.NEGATED) != 0, (st >> LR.BRANCH_SHIFT) & 3
    cn, ca = win > 0, branch > 0
    p = ol.depth_to_normals(depth.to(dt), torch.as_tensor(K).to(dt)[:, :3, :3]).permute(0, 2, 3, 1)      # [N,H,W,3]
    ux, uy, uz = torch_frame(K, H, W, dt)
    d = p[..., 0] * ux + p[..., 1] * uy + p[..., 2] * uz
    s = (d + p[..., 2]) / (1.0 + uz)
    p = torch.stack([p[..., 0] - s * ux, p[..., 1] - s * uy, d], -1)
    p = torch.where(neg[..., None], -p, p)
    C = torch.as_tensor(np.asarray(pol))[:, :, :, :W].to(dt).reshape(N, 3, 3, H, W).permute(0, 3, 4, 1, 2)   # [N,H,W,cand,xyz]
    C = C * torch.tensor([1.0, float(aolp_sign), 1.0], dtype=dt)
    rho = torch.as_tensor(np.asarray(xolp))[:, 0, :, :W].to(dt)
    w = rho if dolp_weighted else torch.ones_like(rho)
    safe = torch.tensor([0.6, 0.0, 0.8], dtype=dt)

    def pick(index, mask):
        c = torch.gather(C, 3, index.clamp(0, 2)[..., None, None].expand(N, H, W, 1, 3))[..., 0, :]
        c = torch.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0)
        return torch.where(mask[..., None], c, safe), torch.where(mask[..., None], p, safe)

    c, q = pick((win - 1) // 2, cn)
    flip = torch.where((win % 2 == 0) & cn, -1.0, 1.0).to(dt)
    c = c * torch.stack([flip, flip, torch.ones_like(flip)], -1)
    cos = (q * c).sum(-1) / (q.norm(dim=-1) * c.norm(dim=-1))
    l_n = 1.0 - cos.clamp(-1.0, 1.0)
    wn = torch.where(cn, w, torch.zeros_like(w))
    L_n = (wn * l_n).sum() / wn.sum() if float(wn.sum()) > 0 else (l_n * 0.0).sum()
    c, q = pick(branch - 1, ca)
    m = (q[..., :2] * c[..., :2]).sum(-1)
    l_a = (1.0 - m * m / ((q[..., :2] ** 2).sum(-1) * (c[..., :2] ** 2).sum(-1))).clamp(0.0, 1.0)
    wa = torch.where(ca, w, torch.zeros_like(w))
    L_a = (wa * l_a).sum() / wa.sum() if float(wa.sum()) > 0 else (l_a * 0.0).sum()
    return L_n, L_a


def torch_grad(depth, K, pol, xolp, state, dt, g=(1.0, 1.0), **kw):
    """d (g[0] L_n + g[1] L_a) / d depth [N,1,H,W] by autograd, and the two values."""
    d = torch.as_tensor(np.asarray(depth)).to(dt).clone().requires_grad_(True)
    L_n, L_a = torch_loss(d, K, pol, xolp, state, dt, **kw)
    gt = torch.tensor(g, dtype=torch.float32).to(dt)
    (gt[0] * L_n + gt[1] * L_a).backward()
    return d.grad, (L_n.detach(), L_a.detach())


# ---- inputs for the tests

def intrinsics(N, H, W):
    """Per-item fp32 [N,4,4]: fx != fy, an off-centre principal point; item 0's principal point lies exactly on a pixel; the last
    item (of two or more) has a short focal length, fx = 0.3 W."""
    K = np.zeros((N, 4, 4), np.float32)
    for n in range(N):
        fx, fy = (0.58 + 0.03 * n) * W, (0.60 + 0.02 * n) * H
        cx, cy = 0.5 * W + 0.37 + 1.1 * n, 0.5 * H - 0.81 + 0.6 * n
        if n == 0:
            cx, cy = float(min(W - 1, W // 2 + 1)), float(H // 2)
        if n == N - 1 and N > 1:
            fx, fy = 0.3 * W, 0.33 * H
        K[n] = np.eye(4, dtype=np.float32)
        K[n, 0, 0], K[n, 1, 1], K[n, 0, 2], K[n, 1, 2] = fx, fy, cx, cy
    return K


def plane_scene(H=48, W=64, tilt_deg=20.0, f=0.58):
    """The perspective plane: a camera with fx = f W, fy = 0.60 H and an off-centre principal point looks at a plane whose one
    normal is tilted by tilt_deg against the optical axis (about an oblique axis).  Per pixel the normal is expressed exactly in
    the ray frame and its zenith and azimuth there give the diffuse candidate; the specular candidates lie at +pi/2 in azimuth
    with other zeniths, as the physics has them; rho = 0.5.  -> dict(K [1,4,4], normals [1,H,W,4] fp32, depth [1,1,H,W] fp32,
    pol [1,9,H,W], xolp [1,2,H,W])."""
    K = np.eye(4, dtype=np.float32)[None].copy()
    K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2] = f * W, 0.60 * H, 0.5 * W - 2.3, 0.5 * H + 1.7
    t, a = np.radians(tilt_deg), np.radians(30.0)
    n = np.array([np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), -np.cos(t)])          # faces the camera: n.z < 0 in camera coordinates
    ys, xs = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    rx, ry = (xs - f64(K[0, 0, 2])) / f64(K[0, 0, 0]), (ys - f64(K[0, 1, 2])) / f64(K[0, 1, 1])
    depth = (-n[2] * 3.0) / -(n[0] * rx + n[1] * ry + n[2])                           # n . (X - X0) = 0 with X0 = (0, 0, 3)
    assert (depth > 0).all(), "the plane must stay in front of the camera: a smaller tilt"
    normals = np.zeros((1, H, W, 4), np.float32)
    normals[0, ..., :3] = n
    u = frame(K, H, W)
    qx, qy, qz = rotate(u, *(normals[..., i].astype(f64) for i in range(3)))
    sgn = np.where(qz < 0, -1.0, 1.0)
    qx, qy, qz = sgn * qx, sgn * qy, sgn * qz
    theta, phi = np.arccos(np.clip(qz / np.sqrt(qx * qx + qy * qy + qz * qz), -1, 1)), np.arctan2(qy, qx)
    az = np.stack([phi, phi + np.pi / 2, phi + np.pi / 2])
    th = np.stack([theta, np.full_like(theta, 0.3), np.full_like(theta, 1.2)])
    cand = np.stack([np.cos(az) * np.sin(th), np.sin(az) * np.sin(th), np.cos(th)], 1)            # [3, 3, 1, H, W]
    pol = np.ascontiguousarray(np.moveaxis(cand.reshape(9, 1, H, W), 0, 1)).astype(np.float32)
    xolp = np.zeros((1, 2, H, W), np.float32)
    xolp[:, 0] = 0.5
    xolp[:, 1] = phi
    return {"K": K, "normals": normals, "depth": depth[None, None].astype(np.float32), "pol": pol, "xolp": xolp}


def loss_case(N, H, W, ldp=None, mirrored=False):
    """A case of polar_loss_cases.build (same surfaces, same special populations) with the per-item ``intrinsics`` above.
    mirrored: the last item's fx is negated.  A depth map's own normal always looks along its viewing ray (p . u > 0), so a
    sane camera never sets the NEGATED bit in ray mode; the mirrored item's normals look the other way and reach that path."""
    import loss_cases as LC
    import polar_loss_cases as PC
    key = (N, H, W, ldp, mirrored)
    if key not in _LOSS_CASES:
        c = LC.sup_case(N, H, W)
        K = intrinsics(N, H, W)
        if mirrored:
            K[N - 1, 0, 0] = -K[N - 1, 0, 0]
        _LOSS_CASES[key] = PC.build(c["pred"].numpy(), K, 7100 * N + 13 * H + W, ldp, False)
    return _LOSS_CASES[key]


_LOSS_CASES = {}


# The perspective plane (plane_scene(): 64 x 48, f = 0.58 W, tilt 20 degrees, the frame's outermost pixels left out), measured
# on this statement (tests/test_polar_ray_ref.py::test_plane_scene_on_the_statement prints the figures).  In the ray frame:
#   the plane's one normal through the evaluator     mean n_deg 6.0e-7, mean az_deg 5.2e-7 degrees (the fp32 candidates)
#   the plane as a depth map through the evaluator   mean n_deg 4.0e-5, mean az_deg 6.2e-5 degrees (the fp32 Sobel chain)
#   the plane as a depth map through the loss        L_n 3.3e-13, L_a 2.8e-12
# Orthographic: 13.2 and 22.3 degrees, L_n 0.033, L_a 0.180.  The bounds are the measured figures rounded up, times 4.
PLANE_NORMALS_DEG = 4 * 6e-7
PLANE_DEPTH_DEG = 4 * 7e-5
PLANE_LOSS = (4 * 4e-13, 4 * 3e-12)
