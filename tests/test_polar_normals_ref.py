"""tests/polar_normals_ref.py, the NumPy statement of pd_polar_normals_stats (no GPU): the vectorised statement equals the
per-pixel loop on every field; hand-made pixels pin each rule of the definition; and a synthetic diffuse sphere patch, run
through the CPU statement of K1, agrees with its own true normals -- until the scene is mirrored or the AoLP handedness is
wrong."""
import numpy as np
import pytest
import torch

import polar_general_ref as G
import polar_normals_ref as R
from oracle import polar as opolar
from polardepth import normals_eval as NE

EDGES = NE.cos_edges_numpy()
ALL = [(1, 0)]
S = np.sin
C = np.cos


def _same(a, b):
    for name in ("normal", "azimuth"):
        for f in a[name]:
            assert np.array_equal(a[name][f], b[name][f]), (name, f)
    for f in ("az_deg", "n_deg"):
        assert np.array_equal(a[f], b[f], equal_nan=True), f
    assert np.array_equal(a["choice"], b["choice"])
    assert np.array_equal(a["pol_normal"].view(np.int32), b["pol_normal"].view(np.int32))


@pytest.mark.parametrize("shape,masked", [((1, 1, 4, 4, 3), False), ((2, 5, 20, 24, 4), True), ((2, 9, 33, 33, 3), True)])
def test_vectorised_equals_loop(shape, masked):
    N, H, W, ldp, ld = shape
    case = R.random_case(11, N, H, W, ldp, ld, masked)
    classes = R.DEFAULT_RANGES if masked else ALL
    for kw in ({}, {"aolp_sign": -1, "tilt2_min": S(np.radians(5.0)) ** 2}, {"rho_min": 0.2, "rho_max": 0.8, "valid": case["valid"]}):
        a = R.stats(case["pred"], case["pol"], case["xolp"], case["mask"], classes, EDGES, **kw)
        b = R.stats_loop(case["pred"], case["pol"], case["xolp"], case["mask"], classes, EDGES, **kw)
        _same(a, b)
        for name, extra in (("normal", ()), ("azimuth", ("frontal",))):
            r = a[name]
            assert np.array_equal(r["n"], r["hist"].sum(-1))
            live = np.ones((N, H, W), bool) if "valid" not in kw else case["valid"] != 0
            assert np.array_equal(r["n"][:, 0] + r["bad"][:, 0] + r["dolp_out"][:, 0] + sum(r[e][:, 0] for e in extra),
                                  live.reshape(N, -1).sum(1))


def test_random_case_reaches_every_counter_and_choice():
    case = R.random_case(3, 2, 5, 20, 24, 4)
    a = R.stats(case["pred"], case["pol"], case["xolp"], case["mask"], R.DEFAULT_RANGES, EDGES, valid=case["valid"],
                tilt2_min=S(np.radians(5.0)) ** 2)
    for name, counters in (("normal", R.NORMAL_COUNTERS), ("azimuth", R.AZIMUTH_COUNTERS)):
        for c in counters:
            assert a[name][c][:, 0].sum() > 0, (name, c)
    assert set(np.unique(a["choice"])) == set(range(7))


# ---- hand-made pixels: one row, one pixel per column

def _cand(phi, th):
    return np.array([C(phi) * S(th), S(phi) * S(th), C(th)])


def _pixels(preds, cands, rhos, **kw):
    """preds [n][3]; cands [n][3 bases][3]; rhos [n] -> stats and stats_loop (which must agree) on a 1 x n frame."""
    n = len(preds)
    pred = np.zeros((1, 1, n, 3), np.float32)
    pred[0, 0] = np.asarray(preds, np.float32)
    pol = np.zeros((1, 9, 1, n), np.float32)
    pol[0, :, 0, :] = np.asarray(cands, np.float32).reshape(n, 9).T
    xolp = np.zeros((1, 2, 1, n), np.float32)
    xolp[0, 0, 0] = np.asarray(rhos, np.float32)
    mask, classes = kw.pop("mask", None), kw.pop("classes", ALL)
    a = R.stats(pred, pol, xolp, mask, classes, EDGES, **kw)
    _same(a, R.stats_loop(pred, pol, xolp, mask, classes, EDGES, **kw))
    return a, pol


D, S1, S2 = _cand(0.3, 0.6), _cand(0.3 + np.pi / 2, 0.4), _cand(0.3 + np.pi / 2, 1.1)
CANDS = [D, S1, S2]


def test_parallel_to_the_diffuse_candidate():
    a, pol = _pixels([2.0 * np.float32(D).astype(np.float64)], [CANDS], [0.3])
    assert a["choice"][0, 0, 0] == 1 and a["normal"]["hist"][0, 0, 0] == 1 and a["normal"]["n"][0, 0] == 1
    assert a["normal"]["spec"][0, 0] == 0 and a["normal"]["flipped"][0, 0] == 0
    assert a["azimuth"]["hist"][0, 0, 0] == 1 and a["azimuth"]["spec"][0, 0] == 0
    assert a["n_deg"][0, 0, 0] < 1e-3 and np.array_equal(a["pol_normal"][0, 0, 0, :3], pol[0, 0:3, 0, 0])
    assert np.allclose(a["normal"]["sums"][0, 0, 3], np.float32(0.3)) and a["normal"]["sums"][0, 0, 2] <= 0.3 * 1e-3


def test_pi_flipped_spec2_is_choice_6():
    s2 = np.float32(S2).astype(np.float64)
    a, pol = _pixels([(-s2[0], -s2[1], s2[2])], [CANDS], [0.3])
    assert a["choice"][0, 0, 0] == 6 and a["normal"]["spec"][0, 0] == 1 and a["normal"]["flipped"][0, 0] == 1
    assert a["normal"]["hist"][0, 0, 0] == 1 and a["azimuth"]["spec"][0, 0] == 1
    assert np.array_equal(a["pol_normal"][0, 0, 0], np.float32([-s2[0], -s2[1], s2[2], 0]))


def test_a_tie_takes_the_first_candidate():
    # spec1 == spec2 == diff: (diff,+) wins; p on the z axis: + and - of a candidate tie (m == 0), the least tilted candidate
    # (spec1) wins with its +; diff absent and spec1 == spec2: spec1 first
    a, _ = _pixels([D, (0, 0, 1), S1], [[D, D, D], CANDS, [np.zeros(3), S1, S1]], [0.3, 0.3, 0.3])
    assert list(a["choice"][0, 0]) == [1, 3, 3]
    # p halfway (in azimuth) between a candidate and its flip: m == 0 exactly, + wins
    a, _ = _pixels([(0, 1, 1)], [[(0.5, 0, 0.5), (0, 0, 0), (0, 0, 0)]], [0.3])
    assert a["choice"][0, 0, 0] == 1 and a["azimuth"]["hist"][0, 0, 359] == 1          # and exactly 90 degrees: the last bin
    assert a["az_deg"][0, 0, 0] == 90.0


def test_pz_below_zero_is_negated_and_pol_normal_follows():
    d = np.float32(D).astype(np.float64)
    a, _ = _pixels([-d, d], [CANDS, CANDS], [0.3, 0.3])
    assert list(a["choice"][0, 0]) == [1, 1] and a["normal"]["hist"][0, 0, 0] == 2
    assert np.array_equal(a["pol_normal"][0, 0, 0, :3], np.float32(-d)) and np.array_equal(a["pol_normal"][0, 0, 1, :3], np.float32(d))
    assert not np.signbit(a["pol_normal"][0, 0, :, 3]).any()


def test_frontal_pixels():
    t5 = S(np.radians(5.0)) ** 2
    tilt = lambda deg: (S(np.radians(deg)), 0.0, C(np.radians(deg)))
    a, _ = _pixels([(0, 0, 1), tilt(4.9), tilt(5.1), tilt(30)], [CANDS, CANDS, CANDS, [(0, 0, 1), (0, 0, 1), S2]], [0.3] * 4,
                   tilt2_min=t5)
    assert a["azimuth"]["frontal"][0, 0] == 3 and a["azimuth"]["n"][0, 0] == 1 and a["normal"]["n"][0, 0] == 4
    assert list(np.isnan(a["az_deg"][0, 0])) == [True, True, False, True] and not np.isnan(a["n_deg"]).any()
    # tilt2_min = 0: only t2 == 0 is frontal
    a, _ = _pixels([(0, 0, 1), tilt(0.01)], [CANDS, CANDS], [0.3] * 2)
    assert a["azimuth"]["frontal"][0, 0] == 1 and a["azimuth"]["n"][0, 0] == 1


def test_each_rho_gate_at_and_beside_its_bound():
    lo, hi = np.float32(0.05), np.float32(1.0)
    rhos = [np.nextafter(lo, np.float32(0)), lo, np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0)), hi,
            np.nextafter(hi, np.float32(2)), np.nan, np.inf, -np.inf]
    a, _ = _pixels([D] * 9, [CANDS] * 9, rhos)
    want = [False, True, True, True, True, False, False, False, False]
    assert list(~np.isnan(a["n_deg"][0, 0])) == want and list(~np.isnan(a["az_deg"][0, 0])) == want
    for name in ("normal", "azimuth"):
        assert a[name]["dolp_out"][0, 0] == 5 and a[name]["n"][0, 0] == 4 and a[name]["bad"][0, 0] == 0
    assert list(a["choice"][0, 0] != 0) == want


def test_nan_and_zero_predictions_and_candidates_are_bad():
    inf_c = [D, S1, (np.inf, 0, 0)]
    a, _ = _pixels([(np.nan, 0, 1), (0, 0, 0), D, D, (np.inf, 0, 1), D], [CANDS, CANDS, [np.zeros(3)] * 3, inf_c, CANDS, CANDS],
                   [0.3] * 6)
    for name in ("normal", "azimuth"):
        assert a[name]["bad"][0, 0] == 5 and a[name]["n"][0, 0] == 1 and a[name]["dolp_out"][0, 0] == 0
    assert not a["pol_normal"][0, 0, :5].any() and list(a["choice"][0, 0]) == [0, 0, 0, 0, 0, 1]
    # the rho gate comes first
    a, _ = _pixels([(np.nan, 0, 1)], [CANDS], [0.01])
    assert a["normal"]["dolp_out"][0, 0] == 1 and a["normal"]["bad"][0, 0] == 0


def test_aolp_sign_mirrors_cy():
    d = np.float32(D).astype(np.float64)
    mirrored = (d[0], -d[1], d[2])
    a, pol = _pixels([mirrored, d], [CANDS, CANDS], [0.3, 0.3], aolp_sign=-1)
    assert a["normal"]["hist"][0, 0, 0] == 1 and a["choice"][0, 0, 0] == 1 and a["n_deg"][0, 0, 1] > 10
    assert np.array_equal(a["pol_normal"][0, 0, 0, :3], np.float32(mirrored))
    b, _ = _pixels([mirrored, d], [CANDS, CANDS], [0.3, 0.3])
    assert b["n_deg"][0, 0, 0] == a["n_deg"][0, 0, 1] and b["az_deg"][0, 0, 0] == a["az_deg"][0, 0, 1]


def test_a_pixel_in_two_classes_and_valid():
    mask = np.array([[[40, 200, 40]]], np.int32)
    a, _ = _pixels([D, D, D], [CANDS] * 3, [0.3, 0.3, 0.01], mask=mask, classes=[(1, 0), (20, 160), (40, 40), (60, 60)],
                   valid=np.array([[[1, 1, 1]]], np.uint8))
    assert list(a["normal"]["n"][0]) == [2, 1, 1, 0] and list(a["normal"]["dolp_out"][0]) == [1, 1, 1, 0]
    assert list(a["azimuth"]["n"][0]) == [2, 1, 1, 0]
    a, _ = _pixels([D, D, D], [CANDS] * 3, [0.3, 0.3, 0.01], mask=mask, classes=[(1, 0), (40, 40)],
                   valid=np.array([[[0, 1, 0]]], np.uint8))
    assert list(a["normal"]["n"][0]) == [1, 0] and list(a["normal"]["dolp_out"][0]) == [0, 0]
    assert list(a["choice"][0, 0]) == [0, 1, 0]


# ---- physics, end to end on the CPU

def _sphere(size=48, n=1.5):
    """A diffuse sphere patch: true normals [size,size,3] with tilts of 10 .. 70 degrees, and what K1's CPU statement makes of
    its four float32 polarizer planes: xolp [1,2,H,W] and the nine normals [1,9,H,W], fp32."""
    ax = np.linspace(-0.95, 0.95, size)
    x, y = np.meshgrid(ax, ax)
    r2 = x * x + y * y
    keep = (r2 >= S(np.radians(10.0)) ** 2) & (r2 <= S(np.radians(70.0)) ** 2)
    z = np.sqrt(np.where(keep, 1.0 - r2, 1.0))
    nrm = np.stack([x, y, z], -1)
    th, phi = np.arccos(z), np.arctan2(y, x)
    s2 = S(th) ** 2
    rho = ((n - 1 / n) ** 2 * s2) / (2 + 2 * n ** 2 - (n + 1 / n) ** 2 * s2 + 4 * C(th) * np.sqrt(n ** 2 - s2))
    ang = np.radians([0.0, 45.0, 90.0, 135.0])
    planes = (100.0 * (1.0 + rho[..., None] * C(2 * ang - 2 * phi[..., None]))).astype(np.float32)
    P = np.array([[.25, .25, .25, .25], [.5, 0, -.5, 0], [0, .5, 0, -.5]])
    k1 = G.restate(planes, P)
    xolp = np.stack([k1["rho"], k1["phi"]])[None]
    normals = opolar.get_normals(torch.from_numpy(xolp), n).float().numpy()
    return nrm.astype(np.float32), keep, xolp, normals


SPHERE_MEAN_BOUND_DEG = 4 * 4e-5           # pooled means
SPHERE_PIXEL_BOUND_DEG = 4 * 7e-4          # any one pixel


def test_diffuse_sphere_agrees_with_its_own_normals():
    """Measured on this CPU pipeline (48 x 48 patch, n = 1.5, tilts of 10 .. 70 degrees, 1000-node theta tables, fp32 planes,
    DoLP and AoLP): the pooled mean of the normal residual is 3.8e-5 degrees (largest pixel 1.5e-4) and of the azimuth
    residual 3.1e-5 degrees (largest pixel 6.9e-4).  The bounds are the larger measured figure of each kind, rounded up to
    4e-5 and 7e-4 degrees, times 4 for the fp32 rounding of the planes.  Mirrored, the azimuth mean is 22.6 degrees."""
    nrm, keep, xolp, normals = _sphere()
    valid = keep.astype(np.uint8)[None]
    a = R.stats(nrm[None], normals, xolp, None, ALL, EDGES, valid=valid, rho_min=0.0, tilt2_min=S(np.radians(5.0)) ** 2)
    P = int(keep.sum())
    for name in ("normal", "azimuth"):
        r = a[name]
        assert r["n"][0, 0] == P and r["bad"][0, 0] == 0 and r["dolp_out"][0, 0] == 0 and r["spec"][0, 0] == 0
        print(name, "mean", r["sums"][0, 0, 0] / P, "max", np.nanmax(a["n_deg" if name == "normal" else "az_deg"]))
        assert r["sums"][0, 0, 0] / P <= SPHERE_MEAN_BOUND_DEG
    assert a["azimuth"]["frontal"][0, 0] == 0
    assert np.nanmax(a["n_deg"]) <= SPHERE_PIXEL_BOUND_DEG and np.nanmax(a["az_deg"]) <= SPHERE_PIXEL_BOUND_DEG
    assert set(np.unique(a["choice"][valid != 0])) == {1, 2}                 # the pi ambiguity is resolved both ways

    # the scene mirrored in y against the measurement, or the wrong AoLP handedness: tens of degrees
    mirrored = nrm * np.float32([1, -1, 1])
    for pred, sign in ((mirrored, 1), (nrm, -1)):
        b = R.stats(pred[None], normals, xolp, None, ALL, EDGES, valid=valid, rho_min=0.0, tilt2_min=S(np.radians(5.0)) ** 2,
                    aolp_sign=sign)
        mean = b["azimuth"]["sums"][0, 0, 0] / b["azimuth"]["n"][0, 0]
        print("mirrored" if sign == 1 else "aolp_sign = -1", "azimuth mean", mean)
        assert mean > 10 * SPHERE_MEAN_BOUND_DEG and mean > 10.0
    # both at once cancel
    c = R.stats(mirrored[None], normals, xolp, None, ALL, EDGES, valid=valid, rho_min=0.0, tilt2_min=S(np.radians(5.0)) ** 2,
                aolp_sign=-1)
    assert c["azimuth"]["sums"][0, 0, 0] / P <= SPHERE_MEAN_BOUND_DEG
