"""tests/polar_refine_ref.py against itself and against a direct sparse solve (CPU): the definition of the polarimetric depth
refinement does what it is for, before any kernel is compared with it.  The import of polardepth.refine ties the file to the
feature: the statement and the device code arrive together."""
import numpy as np
import pytest

import polardepth.refine  # noqa: F401
import polar_refine_ref as R

f64 = np.float64


@pytest.fixture(scope="module")
def sphere():
    sc = R.scene(48, 64)
    sc["setup"] = R.setup(sc["prior"], sc["K"], sc["normal"], sc["rho"])
    return sc


def test_chebyshev_converges_to_the_direct_solve(sphere):
    """Measured: 2.1e-10 after 100 steps, 3.9e-15 after 200 (lam = 0.02, 48 x 64; S = 1.2, a = 0.0164)."""
    from scipy.sparse.linalg import spsolve
    st = sphere["setup"]
    A, b = R.normal_matrix(st, 0)
    direct = spsolve(A.tocsc(), b).reshape(48, 64)
    coef = R.coef_planes(st)
    for iters, bound in ((100, 1e-8), (200, 1e-12)):
        z, _ = R.solve(coef, R.table(st["S"], iters=iters), st["zeta0"])
        err = float(np.abs(z[0] - direct).max())
        print(f"iters {iters}: |chebyshev - direct| = {err:.3g}")
        assert err <= bound


def test_the_spectrum_bound_holds(sphere):
    """The eigenvalues of D^-1 A lie in [a, 2 - a] with a = lam / (lam + S): what the table is built on."""
    st = sphere["setup"]
    A, _ = R.normal_matrix(st, 0)
    d = A.diagonal()
    M = (A.toarray() / np.sqrt(d)[:, None]) / np.sqrt(d)[None, :]             # similar to D^-1 A, symmetric
    ev = np.linalg.eigvalsh(M)
    a = R.LAM / (R.LAM + st["S"][0])
    assert ev.min() >= a - 1e-12 and ev.max() <= 2 - a + 1e-12


def test_refinement_halves_the_error(sphere):
    """4 mm white noise + 4 mm low-frequency bias: measured 3.60 mm -> 1.60 mm (ratio 0.444) with this generator; at 96 x 128
    3.63 -> 1.76 mm (0.484).  lam = 0.1 / 0.02 / 0.005 at 48 x 64: 1.88 / 1.60 / 1.17 mm."""
    out = R.refine(sphere["prior"], sphere["K"], sphere["normal"], sphere["rho"])
    truth = sphere["truth"][0]
    e0 = np.abs(sphere["prior"][0].astype(f64) - truth).mean()
    e1 = np.abs(out["depth"][0].astype(f64) - truth).mean()
    print(f"prior {1e3 * e0:.3f} mm, refined {1e3 * e1:.3f} mm, ratio {e1 / e0:.3f}")
    assert e1 <= 0.6 * e0


def test_pixels_without_a_live_edge_keep_the_priors_bits(sphere):
    out = R.refine(sphere["prior"], sphere["K"], sphere["normal"], sphere["rho"])
    untouched = out["touched"] == 0
    hole = sphere["rho"] == 0
    assert untouched.any() and (untouched >= hole).all()                      # the hole and nothing but dead pixels
    assert np.array_equal(out["depth"][untouched].view(np.uint32), sphere["prior"][untouched].view(np.uint32))
    assert (out["depth"][~untouched] != sphere["prior"][~untouched]).mean() > 0.9
    # special priors ride through: every bit of a NaN, an infinity, a zero, a negative depth
    c = R.case(2, 13, 67)
    o = R.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"])
    special = ~(np.isfinite(c["depth"]) & (c["depth"] > 0))
    assert special.sum() > 20 and not o["touched"][special].any()
    assert np.array_equal(o["depth"][special].view(np.uint32), c["depth"][special].view(np.uint32))
    assert np.isfinite(o["depth"][o["touched"] == 1]).all()


def test_an_item_without_polarisation_stays_at_its_prior():
    c = R.case(3, 9, 21, dead_item=1)
    o = R.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"])
    assert o["setup"]["S"][1] == 0 and not o["touched"][1].any() and o["residual"][1] == 0
    assert np.array_equal(o["depth"][1].view(np.uint32), c["depth"][1].view(np.uint32))
    assert np.array_equal(o["zeta"][1], o["setup"]["zeta0"][1])
    assert (R.table(o["setup"]["S"])[1] == 0).all()
    assert o["touched"][0].any() and o["touched"][2].any() and o["residual"][0] > 0


def test_a_step_of_the_prior_is_not_smoothed_across():
    """A prior with a step of 0.2 in log depth (> edge_max) under the normals of ONE plane: the normals deny the step, the
    edge gate keeps it.  Each side's relaxation towards its own normals is what the reference yields with the other side
    removed; the refined step differs from the prior's by no more than those two."""
    H, W = 12, 20
    K = R.camera(1, H, W)
    depth = np.full((1, H, W), 2.0, np.float32)
    depth[..., W // 2:] = np.float32(2.0 * np.exp(0.2))
    depth += np.random.default_rng(3).normal(0, 0.002, (1, H, W)).astype(np.float32)
    normal = np.zeros((1, H, W, 4), np.float32)
    normal[..., 2] = -1.0
    rho = np.full((1, H, W), 0.4, np.float32)
    full = R.refine(depth, K, normal, rho)
    st = full["setup"]
    assert (st["wE"][0, :, W // 2 - 1] == 0).all() and (st["wE"][0, :, :W // 2 - 1] > 0).all()      # the cut, and only there
    sides = []
    for keep in (slice(0, W // 2), slice(W // 2, W)):
        r = rho.copy()
        r[...] = 0
        r[..., keep] = 0.4
        sides.append(R.refine(depth, K, normal, r))
    l, r = W // 2 - 1, W // 2
    assert np.array_equal(full["zeta"][0, :, :W // 2], sides[0]["zeta"][0, :, :W // 2])             # the sides do not see each other
    assert np.array_equal(full["zeta"][0, :, W // 2:], sides[1]["zeta"][0, :, W // 2:])
    prior_step = st["zeta0"][0, :, r] - st["zeta0"][0, :, l]
    own = np.abs(sides[0]["zeta"][0, :, l] - st["zeta0"][0, :, l]) + np.abs(sides[1]["zeta"][0, :, r] - st["zeta0"][0, :, r])
    refined_step = full["zeta"][0, :, r] - full["zeta"][0, :, l]
    assert (prior_step > 0.15).all() and (refined_step >= prior_step - own).all() and (refined_step > 0.15).all()
    # with the gate open the same normals pull the two sides together
    merged = R.refine(depth, K, normal, rho, edge_max=1.0)
    assert ((merged["zeta"][0, :, r] - merged["zeta"][0, :, l]) < 0.5 * prior_step).all()


def test_the_sign_of_a_normal_changes_nothing():
    c = R.case(2, 13, 67)
    flip = np.random.default_rng(5).random(c["normal"].shape[:3]) < 0.5
    n2 = c["normal"].copy()
    n2[flip] = -n2[flip]
    a = R.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], iters=20)
    b = R.refine(c["depth"], c["K"], n2, c["rho"], c["valid"], iters=20)
    for k in ("wE", "wS", "rhs", "idiag", "p", "q"):
        assert np.array_equal(a["setup"][k].view(np.uint64), b["setup"][k].view(np.uint64)), k
    assert np.array_equal(a["zeta"].view(np.uint64), b["zeta"].view(np.uint64))
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))


def test_the_kernel_cases_hold_every_population_away_from_the_gates():
    """What tests/test_polar_refine_gpu.py relies on: no gate decision within reach of an ulp, every path populated."""
    for N, H, W, dead in ((1, 1, 1, None), (1, 1, 7, None), (1, 5, 1, None), (2, 13, 67, None), (3, 37, 130, 1)):
        c = R.case(N, H, W, dead_item=dead)
        st = R.setup(c["depth"], c["K"], c["normal"], c["rho"], c["valid"])
        assert st["dz_margin"] > 1e-9
        m = st["margin"][np.isfinite(st["margin"])]
        assert m.size == 0 or np.abs(m).min() > 1e-9
        if H * W > 500:
            live = st["live"]
            assert 0.5 < live.mean() < 0.95 and (st["margin"][np.isfinite(st["margin"])] < 0).any()
            both = live[..., :, :-1] & live[..., :, 1:]
            assert (both & (st["wE"][..., :, :-1] == 0)).any()                 # an edge cut by the step of the prior
