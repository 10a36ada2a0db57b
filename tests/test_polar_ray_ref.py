"""tests/polar_ray_ref.py, the NumPy statement of the per-pixel viewing-ray frame (no GPU): the vectorised statements equal
their per-pixel loops; with the frame off they are the orthographic statements bit for bit; the rotation is what the header
says it is; and a perspective camera looking at a diffuse sphere agrees with the sphere's own normals in the ray frame -- and
is tens of degrees off without it."""
import numpy as np
import pytest
import torch

import polar_general_ref as G
import polar_loss_cases as PC
import polar_loss_ref as LR
import polar_normals_ref as NR
import polar_ray_ref as RR
from oracle import polar as opolar
from polardepth import normals_eval as NE

EDGES = NE.cos_edges_numpy()
ALL = [(1, 0)]
T5 = np.sin(np.radians(5.0)) ** 2


def _same_stats(a, b):
    for name in ("normal", "azimuth"):
        for f in a[name]:
            assert np.array_equal(a[name][f], b[name][f]), (name, f)
    for f in ("az_deg", "n_deg"):
        assert np.array_equal(a[f], b[f], equal_nan=True), f
    assert np.array_equal(a["choice"], b["choice"])
    assert np.array_equal(a["pol_normal"].view(np.int32), b["pol_normal"].view(np.int32))


def _same_terms(a, b):
    assert np.array_equal(a["state"], b["state"])
    for f in ("l_n", "l_a", "w"):
        assert np.array_equal(a[f], b[f], equal_nan=True), f
    assert a["counters"] == b["counters"] and a["sums"] == b["sums"] and a["n_terms"] == b["n_terms"]
    assert np.array_equal(a["values"], b["values"])


EVAL_SHAPES = [((1, 1, 4, 4, 3), False), ((2, 5, 20, 24, 4), True), ((3, 9, 33, 33, 3), True)]


@pytest.mark.parametrize("shape,masked", EVAL_SHAPES)
def test_evaluator_vectorised_equals_loop(shape, masked):
    N, H, W, ldp, ld = shape
    case = NR.random_case(11, N, H, W, ldp, ld, masked)
    K = RR.intrinsics(N, H, W)
    classes = NR.DEFAULT_RANGES if masked else ALL
    for kw in ({}, {"aolp_sign": -1, "tilt2_min": T5}, {"rho_min": 0.2, "rho_max": 0.8, "valid": case["valid"]}):
        args = (case["pred"], case["pol"], case["xolp"], case["mask"], classes, EDGES)
        a = RR.stats(*args, K=K, ray_frame=True, **kw)
        _same_stats(a, RR.stats_loop(*args, K=K, ray_frame=True, **kw))
        live = np.ones((N, H, W), bool) if "valid" not in kw else case["valid"] != 0
        for name, extra in (("normal", ()), ("azimuth", ("frontal",))):
            r = a[name]
            assert np.array_equal(r["n"], r["hist"].sum(-1))
            assert np.array_equal(r["n"][:, 0] + r["bad"][:, 0] + r["dolp_out"][:, 0] + sum(r[e][:, 0] for e in extra),
                                  live.reshape(N, -1).sum(1))
        # the frame off: the orthographic statement, both forms
        off = RR.stats(*args, K=K, ray_frame=False, **kw)
        _same_stats(off, NR.stats(*args, **kw))
        _same_stats(RR.stats_loop(*args, ray_frame=False, **kw), off)
        assert not np.array_equal(off["n_deg"], a["n_deg"], equal_nan=True)


@pytest.mark.parametrize("geom", PC.SMALL)
def test_loss_vectorised_equals_loop(geom):
    c = RR.loss_case(*geom)
    for kw in ({}, {"aolp_sign": -1, "dolp_weighted": False}):
        opt = dict(rho_min=PC.RHO_MIN, rho_max=PC.RHO_MAX, tilt2_min=PC.TILT2, **kw)
        a = RR.terms(c["p"], c["pol"], c["xolp"], c["valid"], K=c["K"], ray_frame=True, **opt)
        _same_terms(a, RR.terms_loop(c["p"], c["pol"], c["xolp"], c["valid"], K=c["K"], ray_frame=True, **opt))


@pytest.mark.parametrize("geom", PC.GEOMS)
def test_frame_off_is_the_orthographic_statement_on_the_loss_cases(geom):
    c = PC.case(*geom)
    opt = dict(rho_min=PC.RHO_MIN, rho_max=PC.RHO_MAX, tilt2_min=PC.TILT2)
    _same_terms(RR.terms(c["p"], c["pol"], c["xolp"], c["valid"], K=c["K"], ray_frame=False, **opt), PC.terms_of(c))
    if geom in PC.SMALL:
        _same_terms(RR.terms_loop(c["p"], c["pol"], c["xolp"], c["valid"], ray_frame=False, **opt), PC.terms_of(c))
        args = (c["p"], c["pol"], c["xolp"], None, ALL, EDGES)
        kw = dict(valid=c["valid"], tilt2_min=PC.TILT2)
        _same_stats(RR.stats(*args, K=c["K"], ray_frame=False, **kw), NR.stats(*args, **kw))


def test_the_rotation_is_the_identity_on_the_principal_point():
    K = RR.intrinsics(2, 9, 12)
    cx, cy = int(K[0, 0, 2]), int(K[0, 1, 2])
    assert K[0, 0, 2] == cx and K[0, 1, 2] == cy
    u = RR.frame(K, 9, 12)
    assert (u[0][0, cy, cx], u[1][0, cy, cx], u[2][0, cy, cx]) == (0.0, 0.0, 1.0)
    assert RR.frame1(K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2], cx, cy) == (0.0, 0.0, 1.0)
    rng = np.random.default_rng(5)
    v = rng.normal(0, 1, (100, 3)).astype(np.float32).astype(np.float64)
    for f in (RR.rotate, RR.rotate_t):
        got = f((0.0, 0.0, 1.0), v[:, 0], v[:, 1], v[:, 2])
        assert all(np.array_equal(g.view(np.int64), v[:, i].view(np.int64)) for i, g in enumerate(got))
    # and the statements agree there with the orthographic ones, pixel for pixel
    case = NR.random_case(4, 2, 9, 12)
    a = RR.stats(case["pred"], case["pol"], case["xolp"], None, ALL, EDGES, K=K, ray_frame=True)
    b = NR.stats(case["pred"], case["pol"], case["xolp"], None, ALL, EDGES)
    for f in ("n_deg", "az_deg", "choice"):
        assert np.array_equal(a[f][0, cy, cx], b[f][0, cy, cx], equal_nan=True)
    assert np.array_equal(a["pol_normal"][0, cy, cx].view(np.int32), b["pol_normal"][0, cy, cx].view(np.int32))


def test_rotation_identities_on_random_vectors():
    H, W = 40, 52
    K = RR.intrinsics(3, H, W)
    u = RR.frame(K, H, W)
    rng = np.random.default_rng(6)
    v, w = (tuple(rng.normal(0, 1, (3, H, W)) for _ in range(3)) for _ in range(2))
    tol = 1e-14
    ru = RR.rotate(u, *u)
    assert np.abs(ru[0]).max() <= tol and np.abs(ru[1]).max() <= tol and np.abs(ru[2] - 1.0).max() <= tol
    rv = RR.rotate(u, *v)
    n2 = lambda t: np.sqrt(t[0] ** 2 + t[1] ** 2 + t[2] ** 2)
    assert np.abs(n2(rv) / n2(v) - 1.0).max() <= tol
    back = RR.rotate_t(u, *rv)
    scale = n2(v)
    assert max(np.abs((b - a) / scale).max() for a, b in zip(v, back)) <= tol
    dot = lambda s, t: s[0] * t[0] + s[1] * t[1] + s[2] * t[2]
    assert np.abs((dot(rv, w) - dot(v, RR.rotate_t(u, *w))) / (n2(v) * n2(w))).max() <= tol
    # the zenith is exact: p'z = p . u
    assert np.array_equal(rv[2], (v[0] * u[0] + v[1] * u[1]) + v[2] * u[2])


@pytest.mark.parametrize("fx", [0.0, np.nan])
def test_a_zero_or_nan_focal_length_is_bad(fx):
    case = NR.random_case(7, 2, 5, 6, masked=False)
    case["pred"][:] = np.float32([0.3, -0.2, 0.9, 7.0])
    case["xolp"][:, 0] = 0.5
    case["pol"][:] = np.float32(0.5)
    K = RR.intrinsics(2, 5, 6)
    K[1, 0, 0] = fx
    a = RR.stats(case["pred"], case["pol"], case["xolp"], None, ALL, EDGES, K=K, ray_frame=True)
    _same_stats(a, RR.stats_loop(case["pred"], case["pol"], case["xolp"], None, ALL, EDGES, K=K, ray_frame=True))
    for name in ("normal", "azimuth"):
        assert a[name]["bad"][1, 0] == 30 and a[name]["n"][1, 0] == 0 and a[name]["bad"][0, 0] == 0
    t = RR.terms(case["pred"], case["pol"], case["xolp"], None, K=K, ray_frame=True)
    assert (t["state"][1] >> LR.GATE_SHIFT == LR.GATE_BAD).all() and (t["state"][0] >> LR.GATE_SHIFT == LR.GATE_NONE).all()


def test_seeded_cases_reach_every_counter_choice_and_branch():
    N, H, W = 2, 5, 20
    case = NR.random_case(3, N, H, W, 24, 4)
    a = RR.stats(case["pred"], case["pol"], case["xolp"], case["mask"], NR.DEFAULT_RANGES, EDGES, K=RR.intrinsics(N, H, W),
                 ray_frame=True, valid=case["valid"], tilt2_min=T5)
    for name, counters in (("normal", NR.NORMAL_COUNTERS), ("azimuth", NR.AZIMUTH_COUNTERS)):
        for c in counters:
            assert a[name][c][:, 0].sum() > 0, (name, c)
    assert set(np.unique(a["choice"])) == set(range(7))
    for geom in [(2, 9, 65), (2, 21, 70)]:
        c = RR.loss_case(*geom)
        t = RR.terms(c["p"], c["pol"], c["xolp"], c["valid"], K=c["K"], ray_frame=True, rho_min=PC.RHO_MIN, rho_max=PC.RHO_MAX,
                     tilt2_min=PC.TILT2)
        assert all(v > 0 for v in t["counters"].values()), t["counters"]
        st = t["state"]
        assert set(np.unique(st & LR.WINNER)) == set(range(7)) and set(np.unique((st >> LR.BRANCH_SHIFT) & 3)) == {0, 1, 2}
        assert set(np.unique(st >> LR.GATE_SHIFT)) == {0, 1, 2, 3}
    # p'z < 0 means "seen from behind": only a mirrored camera makes a depth map's own normals so
    c = RR.loss_case(2, 9, 65, mirrored=True)
    st = RR.terms(c["p"], c["pol"], c["xolp"], c["valid"], K=c["K"], ray_frame=True, rho_min=PC.RHO_MIN, rho_max=PC.RHO_MAX,
                  tilt2_min=PC.TILT2)["state"]
    neg = (st & LR.NEGATED) != 0
    assert not neg[0].any() and neg[1].sum() > 100 and ((st[1] & LR.WINNER) > 0)[neg[1]].all()


# ---- physics, end to end on the CPU

SPH_H, SPH_W, SPH_C, SPH_R = 48, 64, (0.9, -0.6, 3.0), 2.4


def _sphere(n=1.5):
    """A perspective camera (fx = 0.58 W, fy = 0.60 H, the principal point 2.3 px left of and 1.7 px below the centre) looks at
    a diffuse sphere of radius 2.4 around (0.9, -0.6, 3.0): off the optical axis, since on it normal, ray and axis lie in one
    plane and the azimuth cannot tell the two frames apart.  Its angular radius is 48.8 degrees (about 42 px along x, 33 px
    along y); rays that miss it are left out.  Per pixel: the true normal by ray-sphere intersection, rotated into the ray frame;
    zenith and azimuth there give DoLP and AoLP and from them the four fp32 polarizer planes; K1's CPU statement gives xolp and
    the nine candidates.  Pixels with a zenith of 10 .. 70 degrees are kept.
    -> K [1,4,4], true normals [1,H,W,4] fp32, depth [1,1,H,W] fp32, keep [H,W], xolp [1,2,H,W], candidates [1,9,H,W]."""
    H, W = SPH_H, SPH_W
    K = np.eye(4, dtype=np.float32)[None].copy()
    K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2] = 0.58 * W, 0.60 * H, 0.5 * W - 2.3, 0.5 * H + 1.7
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rx, ry = (xs - float(K[0, 0, 2])) / float(K[0, 0, 0]), (ys - float(K[0, 1, 2])) / float(K[0, 1, 1])
    rr = rx * rx + ry * ry + 1.0
    cxs, cys, czs = SPH_C
    rc = rx * cxs + ry * cys + czs
    disc = rc * rc - rr * (cxs * cxs + cys * cys + czs * czs - SPH_R * SPH_R)
    hit = disc > 0
    d = np.where(hit, (rc - np.sqrt(np.where(hit, disc, 0.0))) / rr, 10.0)   # the depth z of the near intersection
    nrm = np.stack([d * rx - cxs, d * ry - cys, d - czs], -1) / SPH_R      # outward: towards the camera
    nrm[~hit] = (0.0, 0.0, -1.0)
    u = RR.frame(K, H, W)
    q = RR.rotate(tuple(a[0] for a in u), -nrm[..., 0], -nrm[..., 1], -nrm[..., 2])      # oriented to q_z > 0
    th, phi = np.arccos(np.clip(q[2], -1.0, 1.0)), np.arctan2(q[1], q[0])
    keep = hit & (th >= np.radians(10.0)) & (th <= np.radians(70.0))
    s2 = np.sin(th) ** 2
    rho = ((n - 1 / n) ** 2 * s2) / (2 + 2 * n ** 2 - (n + 1 / n) ** 2 * s2 + 4 * np.cos(th) * np.sqrt(n ** 2 - s2))
    ang = np.radians([0.0, 45.0, 90.0, 135.0])
    planes = (100.0 * (1.0 + rho[..., None] * np.cos(2 * ang - 2 * phi[..., None]))).astype(np.float32)
    P = np.array([[.25, .25, .25, .25], [.5, 0, -.5, 0], [0, .5, 0, -.5]])
    k1 = G.restate(planes, P)
    xolp = np.stack([k1["rho"], k1["phi"]])[None]
    cands = opolar.get_normals(torch.from_numpy(xolp), n).float().numpy()
    normals = np.zeros((1, H, W, 4), np.float32)
    normals[0, ..., :3] = nrm
    return K, normals, d[None, None].astype(np.float32), keep, xolp, cands


# measured (docstring of the test), rounded up, times 4 as in tests/test_polar_normals_ref.py
MEAN_ON, PIXEL_ON, DEPTH_MEAN_ON = 4e-5, 6e-4, 0.03
RAY_MEAN_BOUND_DEG = 4 * MEAN_ON
RAY_PIXEL_BOUND_DEG = 4 * PIXEL_ON
DEPTH_MEAN_BOUND_DEG = 4 * DEPTH_MEAN_ON


def _figures(a, P):
    return {name: (a[name]["sums"][0, 0, 0] / P, np.nanmax(a["n_deg" if name == "normal" else "az_deg"])) for name in ("normal", "azimuth")}


def test_perspective_sphere_agrees_with_its_own_normals_in_the_ray_frame():
    """Measured on this CPU pipeline (64 x 48 frame, fx = 0.58 W, fy = 0.60 H, sphere of radius 2.4 around (0.9, -0.6, 3.0),
    n = 1.5, zeniths of 10 .. 70 degrees against the ray, 2216 pixels, fp32 planes, K1's CPU statement).
    True normals, ray frame:     normal mean 3.8e-5 degrees (largest pixel 1.8e-4), azimuth mean 3.2e-5 (largest pixel 5.7e-4).
    True normals, orthographic:  normal mean 16.6 degrees (largest pixel 35.1), azimuth mean 22.8 (largest pixel 45.0).
    The bounds are the larger measured figure of each kind, rounded up to 4e-5 and 6e-4 degrees, times 4, the rule of
    tests/test_polar_normals_ref.py; the orthographic means must be at least 100 times the mean bound.
    The same scene as a depth map through depth_normals (the sphere's angular radius is 48.8 degrees, about 42 px along x and
    33 px along y; 1974 pixels whose 3 x 3 window lies on the patch), Sobel discretisation included:
    ray frame normal mean 0.030 degrees (largest pixel 0.20), azimuth mean 0.014 (largest pixel 0.065); orthographic 16.2 and
    23.2.  Bound: 0.03 degrees times 4 on both means, and the orthographic means at least 100 times that."""
    K, normals, depth, keep, xolp, cands = _sphere()
    valid = keep.astype(np.uint8)[None]
    P = int(keep.sum())
    kw = dict(valid=valid, rho_min=0.0, tilt2_min=T5)
    on = RR.stats(normals, cands, xolp, None, ALL, EDGES, K=K, ray_frame=True, **kw)
    off = RR.stats(normals, cands, xolp, None, ALL, EDGES, K=K, ray_frame=False, **kw)
    fon, foff = _figures(on, P), _figures(off, off["azimuth"]["n"][0, 0])
    foff["normal"] = _figures(off, off["normal"]["n"][0, 0])["normal"]
    print("pixels", P, "on", fon, "off", foff)
    for name in ("normal", "azimuth"):
        r = on[name]
        assert r["n"][0, 0] == P and r["bad"][0, 0] == 0 and r["dolp_out"][0, 0] == 0 and r["spec"][0, 0] == 0
        assert fon[name][0] <= RAY_MEAN_BOUND_DEG and fon[name][1] <= RAY_PIXEL_BOUND_DEG
        assert foff[name][0] >= 100 * RAY_MEAN_BOUND_DEG
    assert on["azimuth"]["frontal"][0, 0] == 0
    # pol_normal is a camera-frame map: the true normal again, negated onto the side the statement oriented it to
    pn = on["pol_normal"][0][keep][:, :3].astype(np.float64)
    cosang = np.clip((pn * normals[0][keep][:, :3]).sum(-1) / np.linalg.norm(pn, axis=-1), -1, 1)
    assert np.degrees(np.arccos(cosang)).max() <= RAY_PIXEL_BOUND_DEG + 0.02          # 0.02: acos of an fp32 cosine near 1

    # the same scene as a depth map: the Sobel window over a sphere of about 42 x 33 px radius belongs to the figure
    p = LR.depth_normals(depth, K)
    inner = np.zeros_like(keep)                                               # the whole 3 x 3 window on the kept patch
    inner[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner[1:-1, 1:-1] &= keep[1 + dy:keep.shape[0] - 1 + dy, 1 + dx:keep.shape[1] - 1 + dx]
    vd = inner.astype(np.uint8)[None]
    kd = dict(valid=vd, rho_min=0.0, tilt2_min=T5)
    don = RR.stats(p, cands, xolp, None, ALL, EDGES, K=K, ray_frame=True, **kd)
    doff = RR.stats(p, cands, xolp, None, ALL, EDGES, K=K, ray_frame=False, **kd)
    Pd = int(vd.sum())
    print("depth: pixels", Pd, "on", _figures(don, Pd), "off", _figures(doff, Pd))
    for name in ("normal", "azimuth"):
        assert don[name]["sums"][0, 0, 0] / max(1, don[name]["n"][0, 0]) <= DEPTH_MEAN_BOUND_DEG
        assert doff[name]["sums"][0, 0, 0] / max(1, doff[name]["n"][0, 0]) >= 100 * DEPTH_MEAN_BOUND_DEG


def test_plane_scene_on_the_statement():
    """The perspective plane of tests/test_polar_ray_gpu.py on the statement: the bounds of polar_ray_ref.PLANE_* hold with the
    frame on, and the orthographic figures are more than 100 times above them."""
    s = RR.plane_scene()
    inner = np.zeros((1,) + s["normals"].shape[1:3], np.uint8)
    inner[:, 1:-1, 1:-1] = 1
    for pred, bound in ((s["normals"], RR.PLANE_NORMALS_DEG), (LR.depth_normals(s["depth"], s["K"]), RR.PLANE_DEPTH_DEG)):
        for ray in (True, False):
            a = RR.stats(pred, s["pol"], s["xolp"], None, ALL, EDGES, K=s["K"], ray_frame=ray, valid=inner, tilt2_min=T5)
            t = RR.terms(pred, s["pol"], s["xolp"], inner, K=s["K"], ray_frame=ray, tilt2_min=T5)
            means = [a[k]["sums"][0, 0, 0] / a[k]["n"][0, 0] for k in ("normal", "azimuth")]
            print("ray" if ray else "orthographic", "mean n_deg, az_deg", means, "L_n, L_a", t["values"], t["counters"])
            assert a["normal"]["n"][0, 0] == inner.sum() and a["azimuth"]["n"][0, 0] > 0.95 * inner.sum()
            if ray:
                assert max(means) <= bound
            else:
                assert min(means) >= 100 * bound
            if bound == RR.PLANE_DEPTH_DEG:
                for v, b in zip(t["values"], RR.PLANE_LOSS):
                    assert (v <= b) if ray else (v >= 100 * b)
