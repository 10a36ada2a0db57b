"""tests/polar_refine_w_ref.py against polar_refine_ref.py, against a direct sparse solve and against what the weight is for (CPU).
The definition of the per-pixel weight of the prior does what it claims before any kernel is compared with it.  The import of
polardepth.refine's weighted entry ties the file to the feature: the statement and the device code arrive together."""
import numpy as np
import pytest

from polardepth.refine import weights as _device_weights  # noqa: F401
import polar_refine_ref as R
import polar_refine_w_ref as RW

f64 = np.float64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_a_weight_of_one_is_the_scalar_definition_bit_for_bit():
    """lam * 1.0 = lam, and min_i lam / (lam + s_i) = lam / (lam + max_i s_i): fp addition and division are monotone."""
    for N, H, W, dead in ((1, 1, 1, None), (1, 1, 7, None), (2, 13, 67, None), (3, 37, 130, 1)):
        c = R.case(N, H, W, dead_item=dead)
        st = R.setup(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], lam=0.02)
        sw = RW.setup(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], np.ones((N, H, W), np.float32), lam=0.02)
        assert np.array_equal(bits(R.coef_planes(sw)), bits(R.coef_planes(st)))
        assert np.array_equal(bits(RW.table(sw["A"])), bits(R.table(st["S"], lam=0.02)))
        assert np.array_equal(sw["A"] == 0, st["S"] == 0)
        if dead is not None:
            assert sw["A"][dead] == 0 and (RW.table(sw["A"])[dead] == 0).all() and (sw["A"][[0, 2]] > 0).all()
    # a weight above weight_max and +inf clamp to 1 too; nothing below: the same bits again
    w = np.full((N, H, W), np.inf, np.float32)
    w[:, ::2] = 3.0
    sw = RW.setup(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], w, lam=0.02)
    assert np.array_equal(bits(R.coef_planes(sw)), bits(R.coef_planes(st)))


def test_the_clamp_and_the_raw_weight():
    w = np.array([[[np.nan, 0.0, -2.0, -np.inf, 0.01, 1.0 / 16, 0.5, 1.0, 7.0, np.inf]]], np.float32)
    assert np.array_equal(RW.clamp(w)[0, 0], [1 / 16, 1 / 16, 1 / 16, 1 / 16, 1 / 16, 1 / 16, 0.5, 1.0, 1.0, 1.0])
    assert np.array_equal(RW.clamp(w, 0.25, 4.0)[0, 0], [0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.5, 1.0, 4.0, 4.0])
    z = np.array([[[2.0, 2.0, 1.0, np.nan, 0.0, 2.0, 2.0, -1.0]]], np.float32)
    b = np.array([[[0.004, 0.008, 0.002, 0.004, 0.004, 0.0, np.inf, 0.004]]], np.float32)
    u = RW.weights(z, b, unc_ref=0.002)[0, 0]
    assert u.dtype == np.float32 and np.allclose(u[:3], [1.0, 0.25, 1.0], rtol=1e-6) and np.isnan(u[3:]).all()
    assert (RW.weights(z)[0, 0] == 1).all()                                     # no source: the prior as it is, NaN depth or not
    z0 = np.zeros((1, 1, 4))
    zp = np.array([[[0.001, -0.005, 0.02, np.nan]]])
    h = RW.weights(z[..., :4], None, zeta_prev=zp, zeta0=z0, c=0.005)[0, 0]
    assert np.array_equal(h, np.array([1.0, 1.0, 0.25, 1.0], np.float32))


@pytest.fixture(scope="module")
def bump():
    return RW.bump_scene()


def test_chebyshev_converges_to_the_direct_solve_of_the_weighted_equations(bump):
    """Measured: |zeta - direct| = 1.82e-06 after 200 steps at weight_min = 1/16 (A = 1.04e-3; the scalar problem has
    a = 1.6e-2 and is at 3.9e-15 by then): a smaller weight_min needs more steps."""
    from scipy.sparse.linalg import spsolve
    wmap = RW.weights(bump["prior"], bump["b"])
    st = RW.setup(bump["prior"], bump["K"], bump["normal"], bump["rho"], None, wmap)
    assert (st["w"] == RW.WEIGHT_MIN).sum() > 50 and (st["w"] == 1).sum() > 50 and ((st["w"] > RW.WEIGHT_MIN) & (st["w"] < 1)).any()
    A, b = RW.normal_matrix(st, 0)
    direct = spsolve(A.tocsc(), b).reshape(48, 64)
    z, _ = R.solve(R.coef_planes(st), RW.table(st["A"], 200), st["zeta0"])
    err = float(np.abs(z[0] - direct).max())
    print(f"200 steps: |chebyshev - direct| = {err:.3g}, A = {st['A'][0]:.3g}")
    assert err <= 10 * 1.82e-06                                                 # measured 1.82e-06
    # the spectrum bound the table is built on
    d = A.diagonal()
    ev = np.linalg.eigvalsh((A.toarray() / np.sqrt(d)[:, None]) / np.sqrt(d)[None, :])
    assert ev.min() >= st["A"][0] - 1e-12 and ev.max() <= 2 - st["A"][0] + 1e-12
    assert st["A"][0] >= R.LAM * RW.WEIGHT_MIN / (R.LAM * RW.WEIGHT_MIN + 4 * float(bump["rho"].max()))


def test_a_stated_regional_bias_is_bridged_and_the_rest_holds(bump):
    """Measured (mm, whole frame / region of 211 pixels), 100 steps: prior 3.16 / 12.44; scalar lam = 0.02 1.25 / 8.78; the best
    scalar of the sweep 0.00125 .. 0.32 1.16 (lam = 0.0025) / 3.85 (lam = 0.00125); weighted with lam = 0.02, unc_ref = 0.002,
    weight_min = 1/16 0.66 / 3.39: 0.57 of the best scalar on the frame, 0.39 of the scalar route at the same lam in the region."""
    truth, region = bump["truth"], bump["region"]
    args = (bump["prior"], bump["K"], bump["normal"], bump["rho"])
    assert int(region.sum()) == 211
    sweep = [R.refine(*args, lam=lam)["depth"] for lam in RW.SWEEP]
    best = min(RW.mae_mm(d, truth) for d in sweep)
    same_lam = R.refine(*args, lam=0.02)["depth"]
    w = RW.refine(*args, uncertainty=bump["b"], lam=0.02, unc_ref=0.002, weight_min=1 / 16)["depth"]
    whole, reg = RW.mae_mm(w, truth), RW.mae_mm(w, truth, region)
    print(f"prior {RW.mae_mm(bump['prior'], truth):.2f} / {RW.mae_mm(bump['prior'], truth, region):.2f} mm; scalar 0.02 "
          f"{RW.mae_mm(same_lam, truth):.2f} / {RW.mae_mm(same_lam, truth, region):.2f}; best scalar {best:.2f} / "
          f"{min(RW.mae_mm(d, truth, region) for d in sweep):.2f}; weighted {whole:.2f} / {reg:.2f}")
    assert whole < 0.75 * best                                                  # measured 0.57
    assert reg < 0.5 * RW.mae_mm(same_lam, truth, region)                       # measured 0.39


def test_two_robust_rounds_shed_the_outliers():
    """Measured, 3 % spikes of +-5 cm, lam = 0.02, c = 0.005, 100 steps: one round 0.718 mm, two rounds 0.363 mm (0.51); the best
    scalar of the sweep 0.366 mm."""
    sc = RW.spike_scene()
    args = (sc["prior"], sc["K"], sc["normal"], sc["rho"])
    one = RW.refine(*args, lam=0.02)
    two = RW.refine(*args, lam=0.02, robust=0.005, rounds=2)
    e1, e2 = RW.mae_mm(one["depth"], sc["truth"]), RW.mae_mm(two["depth"], sc["truth"])
    print(f"one round {e1:.3f} mm, two robust rounds {e2:.3f} mm, ratio {e2 / e1:.2f}")
    assert e2 < 0.7 * e1                                                        # measured 0.51
    # the spikes are what lost weight, and the first round is the unweighted one
    w = two["weight"][0]
    assert w.dtype == np.float32 and (w[sc["spikes"][0]] < 0.5).mean() > 0.9 and (w[~sc["spikes"][0]] == 1).mean() > 0.9
    assert one["weight"] is None
    assert np.array_equal(bits(one["zeta"]), bits(R.refine(*args, lam=0.02)["zeta"]))


def test_a_given_weight_multiplies_the_other_sources(bump):
    args = (bump["prior"], bump["K"], bump["normal"], bump["rho"])
    half = np.full(bump["prior"].shape, 0.5, np.float32)
    both = RW.refine(*args, weight=half, uncertainty=bump["b"], iters=20)
    assert np.array_equal(both["weight"], half * RW.weights(bump["prior"], bump["b"]))
    alone = RW.refine(*args, weight=half, iters=20)
    assert alone["weight"] is half and not np.array_equal(alone["zeta"], both["zeta"])
    # pixels without a live edge keep the prior's bits under any weight
    c = R.case(2, 13, 67)
    wild = np.random.default_rng(2).standard_normal(c["depth"].shape).astype(np.float32)
    o = RW.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], weight=wild, iters=20)
    plain = R.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], iters=20)
    assert np.array_equal(o["touched"], plain["touched"])
    un = o["touched"] == 0
    assert np.array_equal(o["depth"][un].view(np.uint32), c["depth"][un].view(np.uint32))
