"""tests/unc_stats_ref.py and polardepth/uncertainty_eval.py on the CPU: the binned sparsification against an exact sort, the
two limiting rankings, the host-side figures against the statement's records, and the precondition of the GPU test's exact
coverage counters."""
import math

import numpy as np
import pytest

import unc_cases as C
import unc_stats_ref as R
from polardepth import uncertainty_eval as UE

ALL = [(1, 0)]


def _laplace_case(H, W, seed=0):
    """One frame whose errors are Laplace draws of the stated scale: u uniform, gt 1 m, no holes."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.15, 0.75, (1, H, W)).astype(np.float32)
    b = np.exp(math.log(C.B_RANGE[0]) + u.astype(np.float64) * math.log(C.B_RANGE[1] / C.B_RANGE[0]))
    gt = np.ones((1, H, W), np.float32)
    pred = (gt + rng.laplace(0.0, 1.0, (1, H, W)) * b).astype(np.float32)
    return gt, pred, u


def _both(gt, pred, u):
    st = R.stats(pred, gt, u, None, ALL, C.B_RANGE, C.MIN_D, C.MAX_D)
    ok, good, e, *_ = R.pixels(pred, gt, u, C.B_RANGE, C.MIN_D, C.MAX_D)
    v = ok & good
    binned = UE.figures(st["hist"][0, 0], st["tables"][0, 0])
    exact = R.exact_figures(u[v], e[v] * 1e3)
    return st, binned, exact, (u[v], e[v] * 1e3)


# (H, W) -> the largest |binned - exact| this seeded case may show, in mm: (AUSE, AURG, the S curve, the oracle's curve).
# Measured on the CPU (u uniform in [0.15, 0.75], so that b runs from 1.4 mm to 89 mm and few errors reach the open bin):
#   320 x 480: AUSE 2.512 binned / 2.524 exact, AURG 14.275 / 14.275, S within 0.013 mm, O within 0.213 mm;
#   24 x 40:   AUSE 2.940 / 2.951, AURG 13.627 / 13.627, S within 0.136 mm, O within 0.228 mm.
# The oracle's largest difference is at f = 0.99: what is left lies in the first 0.5 mm error bin, whose removal in proportion
# leaves the bin's mean (about 0.25 mm) where the sort leaves its smallest members.  The open last bin (563 of 153600
# pixels) costs less than that at small f.  The bounds leave a factor of two over the measured differences.
AGREEMENT = {(320, 480): (0.025, 0.002, 0.03, 0.45), (24, 40): (0.025, 0.002, 0.3, 0.45)}


@pytest.mark.parametrize("shape", list(AGREEMENT))
def test_binned_sparsification_agrees_with_an_exact_sort(shape):
    gt, pred, u = _laplace_case(*shape)
    st, binned, (ause, aurg, s_exact, o_exact), _ = _both(gt, pred, u)
    s_bin, o_bin = UE.sparsification(st["hist"][0, 0], st["tables"][0, 0])
    d_s, d_o = np.abs(s_bin - s_exact).max(), np.abs(o_bin - o_exact).max()
    print(shape, "AUSE binned", binned[0], "exact", ause, "| AURG binned", binned[1], "exact", aurg, "| curves: S", d_s, "O", d_o)
    cap_ause, cap_aurg, cap_s, cap_o = AGREEMENT[shape]
    assert abs(binned[0] - ause) <= cap_ause and abs(binned[1] - aurg) <= cap_aurg and d_s <= cap_s and d_o <= cap_o
    assert s_bin[0] == pytest.approx(s_exact[0], rel=1e-3)                   # S(0): the mean error, up to the micrometre rounding
    assert aurg > 0 and ause > 0 and binned[2] == pytest.approx(binned[0] / s_bin[0]) and binned[3] == pytest.approx(binned[1] / s_bin[0])


def _tie_resolution(key_bin, err_mm, n, steps=100):
    """What proportional removal inside a bin can cost one curve: inside the bin where the removed count ends, the removed
    sum lies between r' min and r' max of the bin's members, the binned one is r' times their mean, so the difference is at
    most r' (count - r') / count times the bin's spread <= count / 4 times the spread; over the n - r pixels that are left."""
    worst = 0.0
    for j in np.unique(key_bin):
        e = err_mm[key_bin == j]
        worst = max(worst, e.size / 4.0 * (e.max() - e.min()))
    left = n - np.arange(steps) * n / steps
    return float(np.mean(worst / left))


def test_a_perfect_ranking_has_no_sparsification_error_beyond_the_ties():
    rng = np.random.default_rng(3)
    H, W = 24, 40
    u = np.sort(rng.uniform(0.0, 1.0, H * W)).astype(np.float32).reshape(1, H, W)
    e = np.sort(rng.uniform(0.0, 0.2, H * W)).reshape(1, H, W)                # monotone in u, below the open bin
    gt = np.ones((1, H, W), np.float32)
    pred = (gt - e).astype(np.float32)
    st, binned, exact, (uv, ev) = _both(gt, pred, u)
    assert abs(exact[0]) < 1e-12                                             # the sort itself: S = O
    ub = np.minimum(511, (uv * np.float32(512)).astype(np.int64))
    eb = np.searchsorted(R.D.edges_numpy(), ev / 1e3, side="right")
    assert st["tables"][0, 0, 1, 511] == 0
    tie = _tie_resolution(ub, ev, uv.size) + _tie_resolution(eb, ev, uv.size) + 2 * 0.0005      # + the micrometre rounding
    print("perfect ranking: AUSE", binned[0], "tie resolution", tie)
    assert abs(binned[0]) <= tie and binned[1] > 0


def test_a_reversed_ranking_is_worse_than_random():
    gt, pred, u = _laplace_case(24, 40, seed=1)
    st, binned, exact, _ = _both(gt, pred, (np.float32(1) - u).astype(np.float32))
    # the scale now read from 1 - u says the opposite of the truth: the most trusted pixels carry the largest errors
    assert binned[1] < 0 and exact[1] < 0 and binned[0] > 0


def test_curve_by_hand_and_empty_records():
    # four items in two bins: keys high -> low = [bin 1: two items of 30 + 10], [bin 0: two items of 4 + 2]
    c = UE.curve([2, 2], [6, 40], steps=4)                                   # remove 0, 1, 2, 3 items
    assert c.tolist() == [46 / 4, (46 - 20) / 3, 6 / 2, 3 / 1]
    assert np.isnan(UE.curve([0, 0], [0, 0])).all() and np.isnan(UE.figures(np.zeros(512), np.zeros((3, 512)))).all()
    big = UE.curve([1, 2 ** 40], [2 ** 60, 3 * 2 ** 60], steps=2)             # Python integers of any size go in
    assert big[0] == pytest.approx(4 * 2 ** 60 / (2 ** 40 + 1))


@pytest.mark.parametrize("shape", C.STATS_SHAPES)
def test_figures_follow_the_records_and_the_pool_adds_exactly(shape):
    gt, pred, u, mask = C.stats_case(*shape)
    classes = [(1, 0), (20, 160), (40, 100)]
    st = R.stats(pred, gt, u, mask, classes, C.B_RANGE, C.MIN_D, C.MAX_D)
    m = UE.metrics_from_fields(st["n"], st["cover"], st["sums"], st["hist"], st["tables"])
    assert m.shape == (shape[0], 3, len(UE.METRIC_NAMES))
    i = shape[0] - 1
    n = st["n"][i, 0]
    assert n > 0 and m[i, 0, 9] == n
    assert m[i, 0, 0] == pytest.approx(st["sums"][i, 0, 2] / n * 1e3) and m[i, 0, 3] == st["cover"][i, 0, 0] / n
    assert st["tables"][i, 0, 0].sum() == st["tables"][i, 0, 2].sum() and st["tables"][i, 0, 1].sum() == n == st["hist"][i, 0].sum()
    assert abs(st["tables"][i, 0, 0].sum() / 1e6 - st["sums"][i, 0, 2]) <= n * 0.5e-6       # micrometres, rounded per pixel
    pooled = UE.metrics_from_fields(st["n"].sum(0), st["cover"].sum(0), st["sums"].sum(0), st["hist"].sum(0),
                                    st["tables"].astype(object).sum(0))
    assert pooled[0, 9] == st["n"][:, 0].sum() and np.isfinite(pooled[0, :9]).all()
    if shape == (3, 1, 40):                                                   # the image without a pixel: NaN, n = 0
        assert st["n"][0].tolist() == [0, 0, 0] and np.isnan(m[0, :, :9]).all() and (m[0, :, 9] == 0).all()


@pytest.mark.parametrize("shape", C.STATS_SHAPES)
def test_no_coverage_decision_of_the_cases_is_within_reach_of_an_ulp(shape):
    """The GPU test compares cover50 / cover90 exactly although the device's exp may differ from NumPy's by an ulp or two
    (2.2e-16 relative): no pixel's e may lie that close to b ln 2 or b ln 10."""
    gt, pred, u, _ = C.stats_case(*shape)
    margin = R.decision_margin(pred, gt, u, C.B_RANGE, C.MIN_D, C.MAX_D)
    print(shape, "smallest relative distance of e from a coverage threshold:", margin)
    assert margin > 1e-12
    st = R.stats(pred, gt, u, None, ALL, C.B_RANGE, C.MIN_D, C.MAX_D)
    assert st["bad"].sum() >= 2 and 0 < st["cover"][..., 0].sum() < st["cover"][..., 1].sum() < st["n"].sum()
