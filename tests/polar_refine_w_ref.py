"""The statement of the WEIGHTED polarimetric depth refinement (pd_polar_refine_setup_w, _table_w, _weights; include/polardepth.h)
in NumPy, on top of tests/polar_refine_ref.py, which it leaves as it is.

The prior is trusted per pixel: lam_i = lam * clamp(weight_i).  lam_i enters diag, rhs and the lower end of the spectrum; the
live pixels, the edges, the steps and the finish are polar_refine_ref's.  fp64, only + - x / in the order written here.

    clamp(weight, ...)   w_i of the definition, fp64
    setup(...)           polar_refine_ref.setup with lam_i: idiag, rhs, and a (per pixel, +inf where untouched), A (per item)
    table(A, iters)      the Chebyshev scalars from the lower end A of the spectrum
    weights(...)         the raw map (float)(u * h) from the stated Laplace scale b and the previous solution
    refine(...)          the whole weighted route, rounds and the robust reweighting included, as polardepth.refine.polar_refine
                         runs it with ready normals
    normal_matrix        the weighted normal equations as a scipy.sparse matrix
    bump_scene, spike_scene   the two scenes of the value claims"""
import numpy as np

import polar_refine_ref as R

f64 = np.float64

UNC_REF, WEIGHT_MIN, WEIGHT_MAX, ROBUST = 0.002, 1.0 / 16, 1.0, 0.005        # the conventions of polardepth/refine.py


def clamp(weight, weight_min=WEIGHT_MIN, weight_max=WEIGHT_MAX):
    """fp32 [N,H,W], any values -> w_i fp64: weight_min where !(w >= weight_min) (a NaN, a zero, a negative), weight_max where
    w > weight_max (+inf), else (double)w."""
    assert weight.dtype == np.float32
    w = weight.astype(f64)
    lo, hi = f64(weight_min), f64(weight_max)
    with np.errstate(invalid="ignore"):
        return np.where(~(w >= lo), lo, np.where(w > hi, hi, w))


def setup(depth, K, pol_normal, rho, valid=None, weight=None, lam=R.LAM, edge_max=R.EDGE_MAX, cos_inc=None, zeta0=None,
          weight_min=WEIGHT_MIN, weight_max=WEIGHT_MAX):
    """polar_refine_ref.setup's dict with lam_i in idiag and rhs, plus w (the clamped map), lam_i, a [N,H,W] (lam_i / (lam_i + s)
    where s > 0, +inf elsewhere) and A [N] (its minimum per item, 0 where nothing is touched)."""
    st = R.setup(depth, K, pol_normal, rho, valid, lam, edge_max, cos_inc, zeta0=zeta0)
    w = clamp(np.ones(depth.shape, np.float32) if weight is None else weight, weight_min, weight_max)
    lam_i = f64(lam) * w
    wE, wS, gE, gS = st["wE"], st["wS"], st["gE"], st["gS"]
    wW, gW, wN, gN = R._shift(wE, -1, 0), R._shift(gE, -1, 0), R._shift(wS, 0, -1), R._shift(gS, 0, -1)
    with np.errstate(all="ignore"):
        diag = (((lam_i + wE) + wW) + wS) + wN
        st["idiag"] = 1.0 / diag
        st["rhs"] = (((lam_i * st["zeta0"] - wE * gE) + wW * gW) - wS * gS) + wN * gN
        st["a"] = np.where(st["s"] > 0, lam_i / (lam_i + st["s"]), np.inf)
    st["w"], st["lam_i"] = w, lam_i
    st["A"] = lower_end(st["a"])
    return st


def lower_end(a):
    """[N,H,W] -> [N]: the minimum per item, 0 where it is +inf (nothing touched)."""
    m = a.reshape(len(a), -1).min(1) if a[0].size else np.full(len(a), np.inf)
    return np.where(np.isfinite(m), m, 0.0)


def table(A, iters=R.ITERS):
    """[N, iters, 2] fp64 = (alpha_k, beta_k) by polar_refine_ref.table's recurrence, started from a = A[n]; zero where A is 0."""
    A = np.asarray(A, f64)
    t = np.zeros((len(A), iters, 2), f64)
    for n, a in enumerate(A):
        if not (a > 0 and np.isfinite(a)):
            continue
        delta = f64(1.0) - a
        sigma = f64(1.0) / delta
        rho = f64(1.0) / sigma
        t[n, 0] = (0.0, 1.0)
        for k in range(1, iters):
            rk = f64(1.0) / (f64(2.0) * sigma - rho)
            t[n, k] = (rk * rho, (f64(2.0) * rk) / delta)
            rho = rk
    return t


def weights(depth, b=None, unc_ref=UNC_REF, zeta_prev=None, zeta0=None, c=ROBUST):
    """The raw map fp32 [N,H,W] = (float)(u * h).  u = t*t, t = (unc_ref * (double)z) / (double)b, NaN where z or b is not
    finite or not positive, 1 without b.  h = c / r where r = |zeta_prev - zeta0| > c, else 1; 1 without zeta_prev."""
    assert depth.dtype == np.float32 and (b is None or b.dtype == np.float32) and (zeta_prev is None) == (zeta0 is None)
    u = np.ones(depth.shape, f64)
    h = np.ones(depth.shape, f64)
    with np.errstate(all="ignore"):
        if b is not None:
            z, bb = depth.astype(f64), b.astype(f64)
            t = (f64(unc_ref) * z) / bb
            ok = np.isfinite(depth) & (depth > 0) & np.isfinite(b) & (b > 0)
            u = np.where(ok, t * t, np.nan)
        if zeta_prev is not None:
            r = np.abs(zeta_prev - zeta0)
            h = np.where(r > f64(c), f64(c) / r, 1.0)
        return (u * h).astype(np.float32)


def refine(depth, K, pol_normal, rho, valid=None, weight=None, uncertainty=None, unc_ref=UNC_REF, robust=None, rounds=1,
           lam=R.LAM, iters=R.ITERS, edge_max=R.EDGE_MAX, incidence_max_deg=R.INCIDENCE_MAX_DEG, weight_min=WEIGHT_MIN,
           weight_max=WEIGHT_MAX, zeta0=None):
    """polardepth.refine.polar_refine(normals=pol_normal, ...) -> dict(depth, touched, residual, zeta, setup, weight).  Every
    round solves from the prior; with ``robust`` every round after the first reweights from the previous round's zeta.  A given
    ``weight`` multiplies (in fp32) the map made from ``uncertainty`` and ``robust``.  ``weight``: the raw map of the last round,
    None where no source was given (then the round is polar_refine_ref.refine's)."""
    assert robust is None or rounds >= 2
    zprev, out = None, None
    for _ in range(rounds):
        wmap = weight
        if uncertainty is not None or zprev is not None:
            wmap = weights(depth, uncertainty, unc_ref, zprev, None if zprev is None else out["setup"]["zeta0"], robust)
            if weight is not None:
                with np.errstate(all="ignore"):
                    wmap = weight * wmap
        if wmap is None:
            out = R.refine(depth, K, pol_normal, rho, valid, lam, iters, edge_max, incidence_max_deg, zeta0=zeta0)
        else:
            st = setup(depth, K, pol_normal, rho, valid, wmap, lam, edge_max, R.cos_inc_of(incidence_max_deg), zeta0, weight_min,
                       weight_max)
            coef = R.coef_planes(st)
            z, _ = R.solve(coef, table(st["A"], iters), st["zeta0"])
            d, touched, res = R.finish(depth, coef, z)
            out = {"depth": d, "touched": touched, "residual": res, "zeta": z, "setup": st}
        zprev = out["zeta"] if robust is not None else None
    out["weight"] = wmap
    return out


def normal_matrix(st, n):
    """(A, b) of item n of a weighted setup: diag_i = lam_i + s_i on the diagonal, -w on the edges, rhs."""
    import scipy.sparse as sp
    A, b = R.normal_matrix(st, n, lam=0.0)
    return (A + sp.diags(st["lam_i"][n].ravel())).tocsr(), b


# ---- the scenes of the value claims (measured figures: tests/test_polar_refine_w_ref.py)

SWEEP = tuple(0.00125 * 2 ** k for k in range(9))                             # 0.00125 .. 0.32


def bump_scene():
    """A regional bias the network knows of: polar_refine_ref.scene(48, 64) without noise, bias and hole; the prior is the truth
    + a bump of 25 mm + 3 mm white noise, the stated scale b = 3 mm + 0.8 bump.  -> the scene's dict with prior, b fp32 [1,H,W],
    region (bump > 5 mm, 211 pixels)."""
    sc = R.scene(48, 64, noise=0.0, bias=0.0, seed=0, hole=False)
    ys, xs = np.meshgrid(np.arange(48, dtype=f64), np.arange(64, dtype=f64), indexing="ij")
    bump = 0.025 * np.exp(-(((xs - 40) / 7) ** 2 + ((ys - 30) / 6) ** 2))
    prior = sc["truth"][0] + bump + 0.003 * np.random.default_rng(5).standard_normal((48, 64))
    sc["prior"] = prior[None].astype(np.float32)
    sc["b"] = (0.003 + 0.8 * bump)[None].astype(np.float32)
    sc["region"] = (bump > 0.005)[None]
    return sc


def spike_scene():
    """Outliers nobody announces: the same scene, the prior is the truth + 3 mm white noise (no bump) with 3 % of the pixels moved
    by +-5 cm (82 pixels with this generator)."""
    sc = R.scene(48, 64, noise=0.0, bias=0.0, seed=0, hole=False)
    rng = np.random.default_rng(7)
    spikes = rng.random((48, 64)) < 0.03
    sign = np.where(rng.random((48, 64)) < 0.5, -1.0, 1.0)
    prior = sc["truth"][0] + 0.003 * np.random.default_rng(5).standard_normal((48, 64)) + np.where(spikes, 0.05 * sign, 0.0)
    sc["prior"] = prior[None].astype(np.float32)
    sc["spikes"] = spikes[None]
    return sc


def mae_mm(depth, truth, mask=None):
    e = np.abs(depth.astype(f64) - truth)
    return 1e3 * float(e.mean() if mask is None else e[mask].mean())
