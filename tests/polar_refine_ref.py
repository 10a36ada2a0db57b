"""The statement of the polarimetric depth refinement (csrc/polar_refine.hip, include/polardepth.h) in NumPy, for the tests.

The disambiguated polarisation normals are integrated back into the depth prior: per item a screened Poisson problem in
zeta = log z, solved by Chebyshev semi-iteration on the Jacobi-preconditioned normal equations.  fp64, only + - x / sqrt in
exactly the order written here, one log on the way in and one exp on the way out.

    setup(...)      zeta0, the coefficient planes (wE, wS, rhs, idiag), p, q, live, s, S
    table(S, ...)   the Chebyshev scalars (alpha_k, beta_k), [N, iters, 2]
    residual(...)   r of a step and the touched mask
    step(...)       one Chebyshev step
    refine(...)     setup -> table -> iters steps -> finish, the whole definition
    normal_matrix   the same normal equations as a scipy.sparse matrix, for the direct solve
    scene(...)      a perspective sphere in front of a tilted plane, with its true normals"""
import numpy as np

f64 = np.float64

LAM, ITERS, EDGE_MAX, INCIDENCE_MAX_DEG = 0.02, 100, 0.05, 80.0          # the conventions of polardepth/refine.py


def cos_inc_of(incidence_max_deg):
    import math
    return math.cos(math.radians(float(incidence_max_deg)))


def pixels(depth, K, pol_normal, rho, valid=None, cos_inc=None):
    """Per pixel -> dict(live bool, zeta0, p, q, rho, margin): depth fp32 [N,H,W], K fp32 [N,4,4], pol_normal fp32 [N,H,W,>=3], rho
    fp32 [N,H,W] (the DoLP).  margin = |n.r| / (|n| |r|) - cos_inc, the distance of the incidence gate's decision (NaN where n = 0)."""
    assert depth.dtype == np.float32 and K.dtype == np.float32 and pol_normal.dtype == np.float32 and rho.dtype == np.float32
    cos_inc = f64(cos_inc_of(INCIDENCE_MAX_DEG) if cos_inc is None else cos_inc)
    N, H, W = depth.shape
    fx, fy, cx, cy = (K[:, i, j].astype(f64)[:, None, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    ys, xs = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    z = depth.astype(f64)
    nx, ny, nz = (pol_normal[..., i].astype(f64) for i in range(3))
    r = rho.astype(f64)
    with np.errstate(all="ignore"):
        zok = np.isfinite(z) & (z > 0)
        zeta0 = np.where(zok, np.log(np.where(zok, z, 1.0)), 0.0)
        xt = (xs[None] - cx) / fx
        yt = (ys[None] - cy) / fy
        nr = (nx * xt + ny * yt) + nz
        n2 = (nx * nx + ny * ny) + nz * nz
        r2 = (xt * xt + yt * yt) + 1.0
        den = np.sqrt(n2) * np.sqrt(r2)
        live = zok & np.isfinite(n2) & (n2 > 0) & np.isfinite(r) & (r > 0) & (np.abs(nr) >= cos_inc * den)
        if valid is not None:
            live &= np.asarray(valid) != 0
        p = np.where(live, -nx / (fx * nr), 0.0)
        q = np.where(live, -ny / (fy * nr), 0.0)
        margin = np.abs(nr) / den - cos_inc
    return {"live": live, "zeta0": zeta0, "p": p, "q": q, "rho": np.where(live, r, 0.0), "margin": margin}


def _shift(a, dx, dy):
    """a at (x + dx, y + dy), zero (False) outside the image; dx, dy in {-1, 0, 1}."""
    o = np.zeros_like(a)
    H, W = a.shape[-2:]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    o[..., yd, xd] = a[..., ys, xs]
    return o


def setup(depth, K, pol_normal, rho, valid=None, lam=LAM, edge_max=EDGE_MAX, cos_inc=None, zeta0=None):
    """-> dict(zeta0, wE, wS, gE, gS, rhs, idiag, s, S, p, q, live, dz_margin, margin).  ``zeta0``: use this [N,H,W] fp64 in
    place of log(depth) where the prior is good (the tests' perturbation of the device's logarithm).  dz_margin: the smallest
    | |zeta0_b - zeta0_a| - edge_max | over the edges between two live pixels."""
    px = pixels(depth, K, pol_normal, rho, valid, cos_inc)
    lam, edge_max = f64(lam), f64(edge_max)
    live, p, q, r = px["live"], px["p"], px["q"], px["rho"]
    z0 = px["zeta0"] if zeta0 is None else np.where(np.isfinite(depth) & (depth > 0), zeta0, 0.0)
    out = dict(px, zeta0=z0)
    dzm = np.inf
    with np.errstate(all="ignore"):
        for name, dx, dy, grad in (("E", 1, 0, p), ("S", 0, 1, q)):
            both = live & _shift(live, dx, dy)
            dz = np.abs(_shift(z0, dx, dy) - z0)
            if both.any():
                dzm = min(dzm, float(np.abs(dz[both] - edge_max).min()))
            on = both & (dz <= edge_max)
            out["w" + name] = np.where(on, np.sqrt(r * _shift(r, dx, dy)), 0.0)
            out["g" + name] = np.where(on, (grad + _shift(grad, dx, dy)) * 0.5, 0.0)
        wE, wS, gE, gS = out["wE"], out["wS"], out["gE"], out["gS"]
        wW, gW, wN, gN = _shift(wE, -1, 0), _shift(gE, -1, 0), _shift(wS, 0, -1), _shift(gS, 0, -1)
        out["s"] = ((wE + wW) + wS) + wN
        diag = (((lam + wE) + wW) + wS) + wN
        out["idiag"] = 1.0 / diag
        out["rhs"] = (((lam * z0 - wE * gE) + wW * gW) - wS * gS) + wN * gN
    out["S"] = out["s"].reshape(len(depth), -1).max(1) if depth[0].size else np.zeros(len(depth))
    out["dz_margin"] = dzm
    return out


def coef_planes(st):
    """[N,4,H,W] fp64: wE, wS, rhs, idiag -- what pd_polar_refine_setup writes."""
    return np.stack([st["wE"], st["wS"], st["rhs"], st["idiag"]], 1)


def table(S, lam=LAM, iters=ITERS):
    """[N, iters, 2] fp64 = (alpha_k, beta_k); all zero where S is 0 or not finite."""
    S = np.asarray(S, f64)
    t = np.zeros((len(S), iters, 2), f64)
    lam = f64(lam)
    for n, s in enumerate(S):
        if not (s > 0 and np.isfinite(s)):
            continue
        a = lam / (lam + s)
        delta = f64(1.0) - a
        sigma = f64(1.0) / delta
        rho = f64(1.0) / sigma
        t[n, 0] = (0.0, 1.0)
        for k in range(1, iters):
            rk = f64(1.0) / (f64(2.0) * sigma - rho)
            t[n, k] = (rk * rho, (f64(2.0) * rk) / delta)
            rho = rk
    return t


def residual(coef, zeta):
    """(r, touched): r = touched ? (rhs + (((wE zE + wW zW) + wS zS) + wN zN)) idiag - zeta : 0, a zero weight's term is 0."""
    wE, wS, rhs, idiag = coef[:, 0], coef[:, 1], coef[:, 2], coef[:, 3]
    wE, wS = wE.copy(), wS.copy()
    wE[..., :, -1] = 0.0                                         # an edge that leaves the image carries nothing
    wS[..., -1, :] = 0.0
    wW, wN = _shift(wE, -1, 0), _shift(wS, 0, -1)
    touched = ((wE + wW) + wS) + wN > 0
    with np.errstate(all="ignore"):
        term = lambda w, z: np.where(w > 0, w * z, 0.0)
        acc = ((term(wE, _shift(zeta, 1, 0)) + term(wW, _shift(zeta, -1, 0))) + term(wS, _shift(zeta, 0, 1))) + term(wN, _shift(zeta, 0, -1))
        r = np.where(touched, (rhs + acc) * idiag - zeta, 0.0)
    return r, touched


def step(coef, tab, k, zeta, d):
    """One Chebyshev step -> (zeta_{k+1}, d_k); d is not read at k == 0."""
    r, _ = residual(coef, zeta)
    alpha, beta = tab[:, k, 0][:, None, None], tab[:, k, 1][:, None, None]
    with np.errstate(all="ignore"):
        dk = beta * r if k == 0 else alpha * d + beta * r
    return zeta + dk, dk


def solve(coef, tab, zeta0, iters=None):
    """zeta after ``iters`` steps from zeta0 (default: the table's length), and the last d."""
    iters = tab.shape[1] if iters is None else iters
    z, d = zeta0.copy(), np.zeros_like(zeta0)
    for k in range(iters):
        z, d = step(coef, tab, k, z, d)
    return z, d


def finish(depth, coef, zeta):
    """-> (depth_out fp32, touched uint8, residual [N] fp64)."""
    r, touched = residual(coef, zeta)
    with np.errstate(all="ignore"):
        out = np.where(touched, np.exp(zeta).astype(np.float32), depth)
        ar = np.where(np.isnan(r), 0.0, np.abs(r))
    res = ar.reshape(len(depth), -1).max(1) if depth[0].size else np.zeros(len(depth))
    return out.astype(np.float32), touched.astype(np.uint8), res


def refine(depth, K, pol_normal, rho, valid=None, lam=LAM, iters=ITERS, edge_max=EDGE_MAX, incidence_max_deg=INCIDENCE_MAX_DEG,
           zeta0=None):
    """The whole definition -> dict(depth, touched, residual, zeta, setup)."""
    st = setup(depth, K, pol_normal, rho, valid, lam, edge_max, cos_inc_of(incidence_max_deg), zeta0=zeta0)
    coef = coef_planes(st)
    z, _ = solve(coef, table(st["S"], lam, iters), st["zeta0"])
    out, touched, res = finish(depth, coef, z)
    return {"depth": out, "touched": touched, "residual": res, "zeta": z, "setup": st}


def normal_matrix(st, n, lam=LAM):
    """(A, b) of item n: the normal equations diag zeta - sum w zeta_nb = rhs as scipy.sparse CSR over all H*W pixels."""
    import scipy.sparse as sp
    wE, wS = st["wE"][n], st["wS"][n]
    H, W = wE.shape
    idx = np.arange(H * W).reshape(H, W)
    wW, wN = _shift(wE, -1, 0), _shift(wS, 0, -1)
    diag = (((f64(lam) + wE) + wW) + wS) + wN
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [diag.ravel()]
    for w, a, b in ((wE[:, :-1], idx[:, :-1], idx[:, 1:]), (wS[:-1], idx[:-1], idx[1:])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
        vals += [-w.ravel(), -w.ravel()]
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))
    return A, st["rhs"][n].ravel()


# ---- inputs for the tests

def camera(N, H, W):
    """fp32 [N,4,4]: fx = 0.58 W, fy != fx, an off-centre principal point that differs per item."""
    K = np.zeros((N, 4, 4), np.float32)
    for n in range(N):
        K[n] = np.eye(4, dtype=np.float32)
        K[n, 0, 0], K[n, 1, 1] = 0.58 * W + 0.5 * n, 0.80 * H + 0.25 * n
        K[n, 0, 2], K[n, 1, 2] = 0.5 * W - 0.8 + 0.6 * n, 0.5 * H + 0.6 - 0.4 * n
    return K


def scene(H=48, W=64, noise=0.004, bias=0.004, seed=0, hole=True):
    """A perspective sphere (radius 0.35 at 1.6 m) in front of a tilted plane (at 2 m), one item.  -> dict(K [1,4,4], truth
    [1,H,W] fp64, normal [1,H,W,4] fp32 (the true normals), prior [1,H,W] fp32 = truth + white noise + a low-frequency bias,
    rho [1,H,W] fp32 = 0.3 with a hole of zeros)."""
    rng = np.random.default_rng(seed)
    K = camera(1, H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    rx, ry = (xs - f64(K[0, 0, 2])) / f64(K[0, 0, 0]), (ys - f64(K[0, 1, 2])) / f64(K[0, 1, 1])
    npl = np.array([0.25, -0.15, -1.0])
    npl /= np.linalg.norm(npl)
    zp = (npl[2] * 2.0) / (npl[0] * rx + npl[1] * ry + npl[2])                  # n . (z r - (0, 0, 2)) = 0
    c, R = np.array([0.05, -0.03, 1.6]), 0.35
    rr = rx * rx + ry * ry + 1.0
    rc = rx * c[0] + ry * c[1] + c[2]
    disc = rc * rc - rr * (c @ c - R * R)
    hit = disc > 0
    zs = np.where(hit, (rc - np.sqrt(np.where(hit, disc, 0.0))) / rr, np.inf)
    truth = np.where(hit, zs, zp)
    normal = np.zeros((1, H, W, 4), np.float32)
    for i in range(3):
        sph = ((rx, ry, 1.0)[i] * zs - c[i]) / R
        normal[0, ..., i] = np.where(hit, np.where(hit, sph, 0.0), npl[i])
    yy, xx = ys / max(H - 1, 1), xs / max(W - 1, 1)
    low = np.sin(2.1 * np.pi * xx + 0.4) * np.cos(1.3 * np.pi * yy - 0.2)
    prior = truth + noise * rng.standard_normal((H, W)) + bias * low
    rho = np.full((1, H, W), 0.3, np.float32)
    if hole:
        rho[0, H // 5:H // 5 + max(H // 8, 1), W // 6:W // 6 + max(W // 8, 1)] = 0.0
    return {"K": K, "truth": truth[None], "normal": normal, "prior": prior[None].astype(np.float32), "rho": rho}


def case(N, H, W, seed=0, ldp=None, dead_item=None):
    """Random-but-smooth inputs for the kernel tests -> dict(depth fp32 [N,H,W], K, normal fp32 [N,H,W,4], xolp fp32
    [N,2,H,ldp] (a padded row pitch where ldp > W; the padding holds NaN), rho (the [N,H,W] view of channel 0), valid uint8).
    The special populations: a depth step larger than edge_max, non-finite and non-positive priors, zero normals, zero and
    negative DoLP, grazing normals beyond the incidence gate, invalid pixels; ``dead_item`` has no polarisation at all."""
    rng = np.random.default_rng(1000 * seed + 131 * N + 17 * H + W)
    ldp = W if ldp is None else ldp
    K = camera(N, H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    depth = np.zeros((N, H, W), np.float32)
    normal = np.zeros((N, H, W, 4), np.float32)
    xolp = np.full((N, 2, H, ldp), np.nan, np.float32)
    valid = np.ones((N, H, W), np.uint8)
    for n in range(N):
        z = 1.5 + 0.3 * n + 0.02 * np.sin(0.31 * xs + n) * np.cos(0.23 * ys) + 0.004 * rng.standard_normal((H, W))
        z = z + np.where(xs + 0.5 * ys > 0.7 * W, 0.4, 0.0)                     # a step of about 0.2 in zeta
        depth[n] = z
        v = rng.standard_normal((H, W, 3)) * 0.35 + np.array([0.0, 0.0, -1.0])
        normal[n, ..., :3] = v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(0.5, 2.0, (H, W, 1))
        normal[n, ..., 3] = rng.standard_normal((H, W))                         # not read
        xolp[n, 0, :, :W] = rng.uniform(0.02, 0.9, (H, W))
        xolp[n, 1, :, :W] = rng.uniform(0, np.pi, (H, W))
        pick = lambda frac: rng.random((H, W)) < frac
        depth[n][pick(0.02)] = np.nan
        depth[n][pick(0.02)] = 0.0
        depth[n][pick(0.01)] = -1.0
        depth[n][pick(0.01)] = np.inf
        normal[n][pick(0.04)] = 0.0
        xolp[n, 0, :, :W][pick(0.03)] = 0.0
        xolp[n, 0, :, :W][pick(0.01)] = -0.1
        graz = pick(0.04)
        normal[n, ..., :3][graz] = np.array([1.0, 0.2, 0.02], np.float32)
        sgn = np.where(pick(0.5), -1.0, 1.0).astype(np.float32)                 # both orientations occur
        normal[n, ..., :3] *= sgn[..., None]
        valid[n][pick(0.03)] = 0
    if dead_item is not None:
        xolp[dead_item, 0] = 0.0
    return {"depth": depth, "K": K, "normal": normal, "xolp": xolp, "rho": xolp[:, 0, :, :W], "valid": valid, "ldp": ldp}
