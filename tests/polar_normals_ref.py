"""The NumPy statement of pd_polar_normals_stats (include/polardepth.h): the same fp32 inputs and the same 719-entry cosine
table as the kernel, fp64 arithmetic in the header's order.  ``stats`` is vectorised, ``stats_loop`` the plain per-pixel loop it
must equal bit for bit; both form the four sums of a record with math.fsum (the exactly rounded sum, which no order changes),
so the kernel's ordered fp64 sums may differ from them by the (n - 1) 2^-53 of any summation order.

Per pixel, every fp32 value converted to fp64 first (all products are then exact):

GATES, in this order; a pixel that fails one adds 1 to that counter in each of its classes, in both record sets, and to nothing
else.  (A pixel with valid == 0 is in no counter at all.)
  1 dolp_out   rho is not finite, or rho < rho_min, or rho > rho_max
  2 bad        a2 = (px px + py py) + pz pz is not finite or not > 0; or any of the nine candidate components is not finite; or
               no candidate has b2 > 0
ORIENTATION: if pz < 0, p is negated.  For every candidate cy' = aolp_sign * cy.
NORMAL SET (720 bins of 0.25 degrees over [0, 180]): six candidates in the order (diff,+), (diff,-), (spec1,+), (spec1,-),
(spec2,+), (spec2,-), the "-" candidate being (-cx, -cy', cz).  With m = (px cx) + (py cy'), q = pz cz,
b2 = (cx cx + cy' cy') + cz cz:  c+ = (m + q) / (sqrt(a2) sqrt(b2)),  c- = (-m + q) / (sqrt(a2) sqrt(b2)).  The first strict
maximum wins; candidates with b2 == 0 or a non-finite c are skipped.  c is clamped to [-1, 1], bin = #{ j : c <= edges[j-1] },
deg = acos(c) * 57.29577951308232.  `spec`: the winner is specular; `flipped`: it is a "-" candidate.
AZIMUTH SET (360 bins over [0, 90]): t2 = px px + py py; branch d = the xy of N_diff, branch s = the xy of N_spec1;
u2 = cx cx + cy' cy', usable when u2 > 0.  `frontal` (and nothing else) when t2 <= tilt2_min * a2 or no branch is usable.
Otherwise c_b = |(px cx) + (py cy')| / (sqrt(t2) sqrt(u2)) clamped to [0, 1] (-1 when not usable), c = max(c_d, c_s), `spec`
when c_s > c_d, bin = #{ j in 1..359 : c <= edges[j-1] }, deg = acos(c) * 57.29577951308232.
SUMS of both sets: deg, deg * deg, rho * deg, rho."""
import math

import numpy as np

NBINS = 720
ABINS = 360
DEG = 57.29577951308232
NORMAL_COUNTERS = ("bad", "dolp_out", "spec", "flipped")
AZIMUTH_COUNTERS = ("bad", "dolp_out", "frontal", "spec")


def bins_of(c, edges):
    """#{ j : c <= edges[j-1] } over the strictly decreasing table."""
    return np.searchsorted(-edges, -c, side="right")


def in_class(mask, lo, hi):
    return np.ones(mask.shape, bool) if lo > hi else (mask >= lo) & (mask <= hi)


def _empty(N, K, H, W):
    rec = lambda names, bins: dict({"n": np.zeros((N, K), np.int64), "sums": np.zeros((N, K, 4)),
                                    "hist": np.zeros((N, K, bins), np.int64)},
                                   **{c: np.zeros((N, K), np.int64) for c in names})
    return {"normal": rec(NORMAL_COUNTERS, NBINS), "azimuth": rec(AZIMUTH_COUNTERS, ABINS),
            "az_deg": np.full((N, H, W), np.nan), "n_deg": np.full((N, H, W), np.nan),
            "choice": np.zeros((N, H, W), np.uint8), "pol_normal": np.zeros((N, H, W, 4), np.float32)}


def _fsums(deg, rho):
    return [math.fsum(deg), math.fsum(deg * deg), math.fsum(rho * deg), math.fsum(rho)]


def stats(pred, pol, xolp, mask, classes, edges, valid=None, rho_min=0.05, rho_max=1.0, tilt2_min=0.0, aolp_sign=1):
    """pred [N,H,W,>=3] fp32, pol [N,9,H,>=W] fp32, xolp [N,2,H,>=W] fp32, mask [N,H,W] int or None, classes [(lo, hi)],
    edges float64 [719], valid [N,H,W] or None -> dict(normal = dict(n, bad, dolp_out, spec, flipped [N,K] int64, sums [N,K,4],
    hist [N,K,720] int64), azimuth = dict(n, bad, dolp_out, frontal, spec, sums, hist [N,K,360]), az_deg, n_deg [N,H,W] float64
    with NaN, choice [N,H,W] uint8, pol_normal [N,H,W,4] float32)."""
    assert pred.dtype == np.float32 and pol.dtype == np.float32 and xolp.dtype == np.float32
    N, H, W = pred.shape[:3]
    K = len(classes)
    out = _empty(N, K, H, W)
    rmin, rmax, sign = np.float64(np.float32(rho_min)), np.float64(np.float32(rho_max)), np.float64(aolp_sign)
    rho = xolp[:, 0, :, :W].astype(np.float64)
    live = np.ones((N, H, W), bool) if valid is None else valid != 0
    px, py, pz = (pred[..., i].astype(np.float64) for i in range(3))
    C = pol[:, :, :, :W].astype(np.float64)
    cx, cy, cz = C[:, 0::3], sign * C[:, 1::3], C[:, 2::3]                     # [N,3,H,W]: diff, spec1, spec2
    with np.errstate(all="ignore"):
        dolp_out = live & (~np.isfinite(rho) | (rho < rmin) | (rho > rmax))
        a2 = (px * px + py * py) + pz * pz
        b2 = (cx * cx + cy * cy) + cz * cz
        good = np.isfinite(a2) & (a2 > 0) & np.isfinite(C).all(1) & (b2 > 0).any(1)
        bad = live & ~dolp_out & ~good
        ok = live & ~dolp_out & good
        neg = ok & (pz < 0)
        px, py, pz = (np.where(neg, -v, v) for v in (px, py, pz))

        # ---- normal set
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
        bin_n = bins_of(c, edges)
        deg_n = np.arccos(c) * DEG
        out["n_deg"] = np.where(cn, deg_n, np.nan)
        out["choice"] = np.where(cn, win + 1, 0).astype(np.uint8)
        wb = np.clip(win, 0, 5) // 2
        take = lambda v: np.take_along_axis(v, wb[:, None], 1)[:, 0]
        ox, oy, oz = take(cx), take(cy), take(cz)
        flip = cn & (win % 2 == 1)
        ox, oy = np.where(flip, -ox, ox), np.where(flip, -oy, oy)
        ox, oy, oz = (np.where(neg, -v, v) for v in (ox, oy, oz))
        for i, v in enumerate((ox, oy, oz)):
            out["pol_normal"][..., i] = np.where(cn, v, 0.0).astype(np.float32)

        # ---- azimuth set
        t2 = px * px + py * py
        ud = cx[:, 0] * cx[:, 0] + cy[:, 0] * cy[:, 0]
        us = cx[:, 1] * cx[:, 1] + cy[:, 1] * cy[:, 1]
        frontal = ok & ((t2 <= np.float64(tilt2_min) * a2) | ~((ud > 0) | (us > 0)))
        ca = ok & ~frontal
        st = np.sqrt(t2)
        cd = np.where(ud > 0, np.minimum(np.abs(px * cx[:, 0] + py * cy[:, 0]) / (st * np.sqrt(ud)), 1.0), -1.0)
        cs = np.where(us > 0, np.minimum(np.abs(px * cx[:, 1] + py * cy[:, 1]) / (st * np.sqrt(us)), 1.0), -1.0)
        c = np.where(ca, np.maximum(cd, cs), 1.0)
        spec_a = ca & (cs > cd)
        bin_a = bins_of(c, edges[:ABINS - 1])
        deg_a = np.arccos(c) * DEG
        out["az_deg"] = np.where(ca, deg_a, np.nan)

    mk = np.zeros((N, H, W), np.int64) if mask is None else mask.astype(np.int64)
    for i in range(N):
        for k, (lo, hi) in enumerate(classes):
            sel = in_class(mk[i], lo, hi)
            for name, counts, bins, deg, nb, flags in (
                    ("normal", cn, bin_n, deg_n, NBINS, {"bad": bad_n, "dolp_out": dolp_out, "spec": cn & (win >= 2), "flipped": flip}),
                    ("azimuth", ca, bin_a, deg_a, ABINS, {"bad": bad, "dolp_out": dolp_out, "frontal": frontal, "spec": spec_a})):
                r = out[name]
                v = sel & counts[i]
                r["n"][i, k] = v.sum()
                for f, a in flags.items():
                    r[f][i, k] = (sel & a[i]).sum()
                r["sums"][i, k] = _fsums(deg[i][v], rho[i][v])
                r["hist"][i, k] = np.bincount(bins[i][v], minlength=nb)
    return out


def stats_loop(pred, pol, xolp, mask, classes, edges, valid=None, rho_min=0.05, rho_max=1.0, tilt2_min=0.0, aolp_sign=1):
    """The same, one pixel at a time."""
    N, H, W = pred.shape[:3]
    K = len(classes)
    out = _empty(N, K, H, W)
    f64 = np.float64
    rmin, rmax, sign, tilt2 = f64(np.float32(rho_min)), f64(np.float32(rho_max)), f64(aolp_sign), f64(tilt2_min)
    for i in range(N):
        terms = {"normal": [([], []) for _ in range(K)], "azimuth": [([], []) for _ in range(K)]}
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
                # ---- normal set
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
                    deg = np.arccos(c) * DEG
                    out["n_deg"][i, y, x] = deg
                    out["choice"][i, y, x] = win + 1
                    cx, cy, cz = cand[win // 2]
                    if win % 2:
                        cx, cy = -cx, -cy
                    if neg:
                        cx, cy, cz = -cx, -cy, -cz
                    out["pol_normal"][i, y, x] = (np.float32(cx), np.float32(cy), np.float32(cz), np.float32(0))
                    for k in mine:
                        out["normal"]["n"][i, k] += 1
                        out["normal"]["hist"][i, k, bn] += 1
                        terms["normal"][k][0].append(deg)
                        terms["normal"][k][1].append(rho)
                    if win >= 2:
                        count("normal", "spec")
                    if win % 2:
                        count("normal", "flipped")
                # ---- azimuth set
                t2 = px * px + py * py
                u2 = [cand[b][0] * cand[b][0] + cand[b][1] * cand[b][1] for b in (0, 1)]
                if t2 <= tilt2 * a2 or not (u2[0] > 0 or u2[1] > 0):
                    count("azimuth", "frontal")
                    continue
                cb = [min(abs(px * cand[b][0] + py * cand[b][1]) / (np.sqrt(t2) * np.sqrt(u2[b])), 1.0) if u2[b] > 0 else -1.0
                      for b in (0, 1)]
                c = max(cb)
                ba = sum(1 for e in edges[:ABINS - 1] if c <= e)
                deg = np.arccos(c) * DEG
                out["az_deg"][i, y, x] = deg
                for k in mine:
                    out["azimuth"]["n"][i, k] += 1
                    out["azimuth"]["hist"][i, k, ba] += 1
                    terms["azimuth"][k][0].append(deg)
                    terms["azimuth"][k][1].append(rho)
                if cb[1] > cb[0]:
                    count("azimuth", "spec")
        for name in ("normal", "azimuth"):
            for k in range(K):
                d, r = (np.array(t, np.float64) for t in terms[name][k])
                out[name]["sums"][i, k] = _fsums(d, r)
    return out


# ---- inputs for the tests

def random_case(seed, N, H, W, ldp=None, ld=4, masked=True):
    """Seeded inputs that exercise every counter and all six choices: candidates from random DoLP / AoLP-like angles, a
    prediction near a randomly chosen candidate (or its flip, or anti-oriented, or frontal), and a share of special pixels (NaN,
    zero, out-of-range rho, zero candidates).  -> dict(pred [N,H,W,ld], pol [N,9,H,ldp], xolp [N,2,H,ldp], mask, valid)."""
    rng = np.random.default_rng(seed)
    ldp = W if ldp is None else ldp
    P = N * H * W
    phi = rng.uniform(-np.pi / 2, np.pi / 2, P)
    th = rng.uniform(0.05, 1.4, (3, P))
    az = np.stack([phi, phi + np.pi / 2, phi + np.pi / 2])
    cand = np.stack([np.cos(az) * np.sin(th), np.sin(az) * np.sin(th), np.cos(th)], 1)          # [3 bases, 3 comps, P]
    pick, flip = rng.integers(0, 3, P), rng.integers(0, 2, P)
    p = cand[pick, :, np.arange(P)].copy()                                                       # [P, 3]
    p[:, :2] *= np.where(flip, -1.0, 1.0)[:, None]
    p += rng.normal(0, 0.15, (P, 3))
    p *= rng.uniform(0.5, 2.0, (P, 1))                                                           # need not be unit length
    p[rng.random(P) < 0.15] *= -1.0                                                              # pz < 0: to be negated
    rho = rng.uniform(0.0, 1.1, P)
    kind = rng.random(P)
    p[kind < 0.04] = (0.0, 0.0, 1.0)                                                             # frontal
    p[(kind >= 0.04) & (kind < 0.06)] = 0.0                                                      # zero prediction: bad
    p[(kind >= 0.06) & (kind < 0.08), 1] = np.nan                                                # NaN prediction: bad
    cand[:, :, (kind >= 0.08) & (kind < 0.10)] = 0.0                                             # no candidate: bad
    cand[2, 0, (kind >= 0.10) & (kind < 0.11)] = np.inf                                          # a non-finite component: bad
    cand[0, :, (kind >= 0.11) & (kind < 0.14)] = 0.0                                             # no diffuse candidate
    cand[:2, :2, (kind >= 0.14) & (kind < 0.16)] = 0.0                                           # no azimuth: frontal
    rho[(kind >= 0.16) & (kind < 0.17)] = np.nan
    rho[(kind >= 0.17) & (kind < 0.18)] = 0.05                                                   # at the lower bound: counts
    pred = np.zeros((N, H, W, ld), np.float32)
    pred[..., :3] = p.reshape(N, H, W, 3)
    if ld > 3:
        pred[..., 3:] = 7.0                                                                      # never read
    pol = np.full((N, 9, H, ldp), np.nan, np.float32)                                            # the padding is never read
    pol[..., :W] = np.moveaxis(cand.reshape(9, N, H, W), 0, 1)
    xolp = np.full((N, 2, H, ldp), np.nan, np.float32)
    xolp[:, 0, :, :W] = rho.reshape(N, H, W)
    xolp[:, 1, :, :W] = phi.reshape(N, H, W)
    greys = np.array([0, 20, 40, 60, 80, 100, 120, 140, 160, 180, 200, 255])
    mask = greys[rng.integers(0, len(greys), (N, H, W))].astype(np.int32) if masked else None
    valid = (rng.random((N, H, W)) > 0.1).astype(np.uint8)
    return {"pred": pred, "pol": pol, "xolp": xolp, "mask": mask, "valid": valid}


DEFAULT_RANGES = [(1, 0), (20, 160)] + [(g, g) for g in range(20, 201, 20)]                      # K = 12, overlapping
