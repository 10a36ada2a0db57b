"""The statement of the polarimetric normals loss (tests/polar_loss_ref.py) and its cases (tests/polar_loss_cases.py), no GPU:
the vectorised statement against the per-pixel loop, the populations of the cases, the reference gradients in fp32 and fp64
and their conditioning, and the minimum of the loss."""
import numpy as np
import pytest
import torch

import loss_cases as LC
import polar_loss_cases as C
import polar_loss_ref as R
import polar_normals_ref as PN

# a one-row frame has no fp64 reference gradient: its fp32 normals are the rounding residue of a Sobel y-sum that cancels
# exactly in fp64 (test_one_row_and_one_column_frames)
GRAD_GEOMS = [g for g in C.GEOMS if g[1] > 1]


def _same(a, b):
    assert np.array_equal(a["state"], b["state"])
    for k in ("l_n", "l_a"):
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k          # NaN patterns included
    assert a["counters"] == b["counters"] and a["sums"] == b["sums"]
    assert np.array_equal(a["values"].view(np.int32), b["values"].view(np.int32))


@pytest.mark.parametrize("geom", C.SMALL + [C.PITCHED], ids=str)
@pytest.mark.parametrize("sign,weighted", [(1, True), (-1, False)])
def test_vectorised_statement_equals_the_loop(geom, sign, weighted):
    c = C.case(*geom)
    kw = dict(rho_min=C.RHO_MIN, rho_max=C.RHO_MAX, tilt2_min=C.TILT2, aolp_sign=sign, dolp_weighted=weighted)
    _same(R.terms(c["p"], c["pol"], c["xolp"], c["valid"], **kw), R.terms_loop(c["p"], c["pol"], c["xolp"], c["valid"], **kw))


def test_statement_makes_the_evaluators_decisions():
    """The winner is the evaluator's `choice`, the counted sets are the evaluator's, and the terms are 1 - cos(n_deg) and
    sin^2(az_deg) of its maps up to the rounding of acos."""
    c = C.case(2, 21, 70)
    t = C.terms_of(c)
    edges = np.cos(np.radians(0.25 * np.arange(1, 720)))
    e = PN.stats(c["p"], c["pol"], c["xolp"], None, [(1, 0)], edges, valid=c["valid"], rho_min=C.RHO_MIN, rho_max=C.RHO_MAX,
                 tilt2_min=C.TILT2)
    assert np.array_equal(t["state"] & R.WINNER, e["choice"])
    assert np.array_equal(np.isnan(t["l_n"]), np.isnan(e["n_deg"])) and np.array_equal(np.isnan(t["l_a"]), np.isnan(e["az_deg"]))
    k = t["counters"]
    assert k["n_normal"] == e["normal"]["n"].sum() and k["n_azimuth"] == e["azimuth"]["n"].sum()
    assert k["dolp_out"] == e["normal"]["dolp_out"].sum() and k["bad"] == e["normal"]["bad"].sum()
    assert k["frontal"] == e["azimuth"]["frontal"].sum() and k["spec"] == e["normal"]["spec"].sum()
    assert k["flipped"] == e["normal"]["flipped"].sum()
    assert ((t["state"] >> R.BRANCH_SHIFT) & 3 == R.BR_S).sum() == e["azimuth"]["spec"].sum()
    cn, ca = ~np.isnan(t["l_n"]), ~np.isnan(t["l_a"])
    assert np.abs(t["l_n"][cn] - (1 - np.cos(np.radians(e["n_deg"][cn])))).max() < 1e-12
    assert np.abs(t["l_a"][ca] - np.sin(np.radians(e["az_deg"][ca])) ** 2).max() < 1e-7      # acos near 1 loses half the digits


def test_every_population_occurs():
    wins, branches, gates, neg, at_min = set(), set(), set(), 0, 0
    for g in C.GEOMS + [C.PITCHED]:
        c = C.case(*g)
        st = C.terms_of(c)["state"]
        wins |= set(np.unique(st & R.WINNER).tolist())
        branches |= set(np.unique((st >> R.BRANCH_SHIFT) & 3).tolist())
        gates |= set(np.unique(st >> R.GATE_SHIFT).tolist())
        neg += int(((st & R.NEGATED) != 0).sum())
        rho = c["xolp"][:, 0, :, :c["W"]]
        at_min += int(((rho == np.float32(C.RHO_MIN)) & (st >> R.GATE_SHIFT == R.GATE_NONE)).sum())
        frontal = (st >> R.GATE_SHIFT == R.GATE_NONE) & ((st >> R.BRANCH_SHIFT) & 3 == 0)
        if g[1] > 8 and g[2] > 8:
            assert frontal.any() and ((st & R.WINNER == 0) & (st >> R.GATE_SHIFT == R.GATE_NONE)).sum() == 0
    assert wins == set(range(7)) and branches == {0, 1, 2} and gates == {0, 1, 2, 3} and neg > 0 and at_min > 0
    assert np.isnan(C.case(*C.PITCHED)["pol"][..., C.PITCHED[2]:]).all() and C.PITCHED[3] > C.PITCHED[2]
    big = C.GEOMS[-1]
    assert big[0] * big[1] * big[2] > C.FWD_CAP
    assert big[0] * -(-big[1] // LC.TILE_R) * -(-big[2] // LC.TILE_C) > C.BWD_TILE_CAP


@pytest.mark.parametrize("geom", GRAD_GEOMS + [C.PITCHED], ids=str)
def test_reference_gradients_and_their_conditioning(geom):
    """The torch restatement with the decisions held fixed reproduces the statement's values in fp64, and its gradients by
    autograd in fp32 and fp64 agree within the cap: a condition on the inputs, which the GPU tolerance rests on."""
    c = C.case(*geom)
    t = C.terms_of(c)
    for g in ((1.0, 0.0), (0.0, 1.0), (1.3, 0.7)):
        g64, v64 = R.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], t["state"], torch.float64, g=g)
        g32, _ = R.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], t["state"], torch.float32, g=g)
        assert torch.isfinite(g64).all() and torch.isfinite(g32).all()
        cond = LC.conditioning(g32, g64)
        print(f"{geom} g = {g}: conditioning {cond:.2e}, max |g64| {g64.abs().max().item():.3e}")
        assert cond <= C.COND, (geom, g, cond)
        assert g64.abs().max() > 0 or t["n_terms"] == (0, 0)
    # the fp64 chain forms p in fp64, the statement in fp32: the values agree to fp32 rounding of p, not bit for bit
    for k in range(2):
        assert abs(float(v64[k]) - float(t["values"][k])) <= 2e-5 * max(float(t["values"][k]), 1e-3), (k, v64, t["values"])


@pytest.mark.parametrize("zoom", C.ZOOMS)
def test_disparity_gradients_and_their_conditioning(zoom):
    c = C.disp_case(*C.DISP_GEOM, zoom)
    g32, g64 = (C.disp_grad(c, C.terms_of(c)["state"], dt) for dt in (torch.float32, torch.float64))
    assert tuple(g64.shape) == c["disp"].shape and g64.abs().max() > 0
    assert LC.conditioning(g32, g64) <= C.COND


def test_options_reach_the_restatement():
    c = C.case(2, 9, 65)
    for sign, weighted in ((-1, True), (1, False)):
        t = C.terms_of(c, aolp_sign=sign, dolp_weighted=weighted)
        assert not np.array_equal(t["state"], C.terms_of(c)["state"]) or not weighted
        d = torch.from_numpy(c["depth"])
        v = R.torch_loss(d, c["K"], c["pol"], c["xolp"], t["state"], torch.float64, aolp_sign=sign, dolp_weighted=weighted)
        for k in range(2):
            assert abs(float(v[k]) - float(t["values"][k])) <= 2e-5 * max(float(t["values"][k]), 1e-3)


def test_a_surface_scored_against_its_own_normal_is_at_the_minimum():
    geom = (2, 21, 70)
    c = C.case(*geom, exact=True)
    t = C.terms_of(c)
    cn = ~np.isnan(t["l_n"])
    assert cn.sum() > 0.8 * cn.size
    assert t["l_n"][cn].max() <= 2.0 ** -50
    # diff+ wins wherever no other candidate reaches the same cosine: recompute the six cosines and look for ties
    win = t["state"] & R.WINNER
    other = win[cn] != 1
    if other.any():
        p = c["p"][..., :3].astype(np.float64)
        p = np.where(p[..., 2:3] < 0, -p, p)
        C9 = c["pol"][:, :, :, :c["W"]].astype(np.float64).reshape(c["N"], 3, 3, c["H"], c["W"])
        cos = [(s * (p[..., 0] * C9[:, b, 0] + p[..., 1] * C9[:, b, 1]) + p[..., 2] * C9[:, b, 2]) /
               (np.sqrt((p * p).sum(-1)) * np.sqrt((C9[:, b] ** 2).sum(1))) for b in range(3) for s in (1.0, -1.0)]
        tie = np.stack(cos[1:]).max(0) >= cos[0]
        assert tie[cn][other].all()
    assert (win[cn] == 1).mean() > 0.99
    assert np.nanmax(t["l_a"]) <= 2.0 ** -50
    # the gradient vanishes there.  The fp64 chain's normal differs from the fp32 p by the rounding of the Sobel differences
    # (about 1e-5 relative here), so the candidate it is scored against is its OWN normal, in fp64
    noisy = C.case(*geom)
    gn, _ = R.torch_grad(noisy["depth"], noisy["K"], noisy["pol"], noisy["xolp"], C.terms_of(noisy)["state"], torch.float64)
    ge, _ = R.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], t["state"], torch.float64, diffuse_is_own_normal=True)
    assert gn.abs().max() > 0 and ge.abs().max() < 1e-6 * gn.abs().max()


def test_one_row_and_one_column_frames():
    """W = 1: the Sobel x-sum of a row is -a + 0 + a, exactly zero in fp32, every normal is the zero vector, every pixel `bad`,
    both values 0.  H = 1: the y-sum runs over three passes of the same row, (-a - 2b - c) + a + 2b + c, whose fp32 rounding
    residue is not zero: pd_gt_normals gives such a frame normals made of rounding noise, and the loss scores them as the
    evaluator does.  Its value is stated, its fp64 gradient does not exist."""
    t = C.terms_of(C.case(2, 40, 1))
    assert t["counters"]["n_normal"] == 0 and t["counters"]["n_azimuth"] == 0 and t["counters"]["bad"] > 0
    assert t["values"].tolist() == [0.0, 0.0] and t["sums"] == [0.0, 0.0, 0.0, 0.0]
    c = C.case(3, 1, 40)
    assert (c["p"][..., :3] != 0).any() and np.isfinite(C.terms_of(c)["values"]).all()
