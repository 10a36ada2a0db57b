"""The NumPy statement of pd_normals_stats (tests/normals_stats_ref.py) against itself and against NumPy's own statistics, no
GPU: the vectorised form equals the per-pixel loop bit for bit; the histogram prefix sums are the threshold counts; the
histogram median lies within one bin of np.median."""
import numpy as np
import pytest
import torch

import normals_stats_ref as R
from polardepth import normals_eval as NE

EDGES = NE.cos_edges_numpy()
CLASSES = [(1, 0), (20, 160), (40, 40), (40, 60), (500, 600)]      # all | a range | one value | overlapping it | empty


def scene(N, H, W, seed):
    """Depth with holes (zeros and a NaN) and out-of-range values, a mask of grey values, unit-ish predicted normals with a zero
    and a NaN among them, and the host-side ground-truth normals."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.3, 1.8, (N, H, W)).astype(np.float32)
    gt[:, 1, 2] = 0.0                               # a hole away from the border
    gt[0, 0, 0] = 0.0                               # a hole in the corner
    gt[-1, H - 1, W - 2] = np.nan
    gt[0, 3, 4] = 2.5                               # beyond max_depth
    Kmat = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    Kmat[:, 0, 0], Kmat[:, 1, 1], Kmat[:, 0, 2], Kmat[:, 1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    mask = (rng.integers(0, 11, (N, H, W)) * 20).astype(np.int32)
    pred = rng.normal(size=(N, H, W, 3)).astype(np.float32)
    pred[0, 3, 0] = 0.0                             # both away from every hole: they pass the window gate too
    pred[-1, 4, 0, 1] = np.nan
    return pred, R.gt_normals(gt, Kmat, 0.1, 2.0), gt, mask


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 9, 12)])
@pytest.mark.parametrize("gate", [0, 1])
def test_vectorised_equals_the_loop(shape, gate):
    pred, gtn, gt, mask = scene(*shape, seed=sum(shape))
    a = R.stats(pred, gtn, gt, mask, CLASSES, EDGES, gate, 0.1, 2.0)
    b = R.stats_loop(pred, gtn, gt, mask, CLASSES, EDGES, gate, 0.1, 2.0)
    for k in ("n", "bad", "hist"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("sum_deg", "sum_deg2", "err_deg"):
        assert a[k].tobytes() == b[k].tobytes(), k                     # bit for bit, NaN pattern included
    assert np.array_equal(a["hist"].sum(-1), a["n"])
    assert (a["n"][:, 4] == 0).all() and (a["bad"][:, 4] == 0).all()      # the empty class
    assert a["n"][:, 0].sum() > 0 and a["bad"][:, 0].sum() >= 1           # the zero / NaN predictions are counted
    assert (a["n"][:, 2] <= a["n"][:, 3]).all() and (a["n"][:, 3] <= a["n"][:, 1]).all()      # 40 within 40..60 within 20..160
    if gate == 0:                                                      # the window gate only removes pixels
        g1 = R.stats(pred, gtn, gt, mask, CLASSES, EDGES, 1, 0.1, 2.0)
        assert (g1["n"] <= a["n"]).all() and g1["n"][:, 0].sum() < a["n"][:, 0].sum()


def _random_normals(n=100000, seed=7):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(1, 1, n, 3)).astype(np.float32)
    g = rng.normal(size=(1, 1, n, 3)).astype(np.float32)
    g /= np.linalg.norm(g, axis=-1, keepdims=True)
    # predictions near the ground truth, so that all three thresholds see a share well inside (0, 1)
    p = (g + 0.35 * p).astype(np.float32)
    gtn = np.concatenate([g, np.zeros((1, 1, n, 1), np.float32)], -1)
    return p, gtn, np.ones((1, 1, n), np.float32)


def test_prefix_sums_are_the_threshold_counts():
    p, gtn, gt = _random_normals()
    out = R.stats(p, gtn, gt, None, [(1, 0)], EDGES, 0, 0.1, 2.0)
    theta = out["err_deg"].ravel()
    assert np.isfinite(theta).all() and out["n"][0, 0] == theta.size
    for deg, nbins in ((11.25, 45), (22.5, 90), (30.0, 120)):
        assert np.abs(theta - deg).min() > 1e-9                        # no angle sits on a threshold: fp64 acos cannot flip a count
        count = int((theta < deg).sum())
        assert 0.02 * theta.size < count < 0.98 * theta.size
        assert int(out["hist"][0, 0, :nbins].sum()) == count, deg
    m = NE.metrics_from_fields(torch.from_numpy(out["n"]), torch.from_numpy(out["sum_deg"]), torch.from_numpy(out["sum_deg2"]),
                               torch.from_numpy(out["hist"]))[0, 0].numpy()
    assert m[3] == (theta < 11.25).sum() / theta.size and m[4] == (theta < 22.5).sum() / theta.size
    assert m[5] == (theta < 30.0).sum() / theta.size and m[6] == theta.size
    assert m[0] == pytest.approx(theta.mean(), rel=1e-12) and m[2] == pytest.approx(np.sqrt((theta ** 2).mean()), rel=1e-12)


@pytest.mark.parametrize("n", [100000, 99999, 7, 1])
def test_histogram_median_is_within_one_bin(n):
    p, gtn, gt = _random_normals()
    p, gtn, gt = p[:, :, :n], gtn[:, :, :n], gt[:, :, :n]
    out = R.stats(p, gtn, gt, None, [(1, 0)], EDGES, 0, 0.1, 2.0)
    m = NE.metrics_from_fields(torch.from_numpy(out["n"]), torch.from_numpy(out["sum_deg"]), torch.from_numpy(out["sum_deg2"]),
                               torch.from_numpy(out["hist"]))[0, 0].numpy()
    print(n, "median", m[1], np.median(out["err_deg"]))
    assert abs(m[1] - np.median(out["err_deg"])) <= 0.25               # the bin width: a bound, not a measurement


def test_empty_record_gives_nan():
    z = torch.zeros(2, dtype=torch.int64)
    m = NE.metrics_from_fields(z, z.double(), z.double(), torch.zeros(2, 720, dtype=torch.int64)).numpy()
    assert np.isnan(m[:, :6]).all() and (m[:, 6] == 0).all()


def test_table_and_constructed_bins():
    assert EDGES.shape == (719,) and EDGES.dtype == np.float64 and (np.diff(EDGES) < 0).all()
    assert np.abs(EDGES - np.cos(np.deg2rad(np.arange(1, 720) * 0.25))).max() < 1e-15 and EDGES[359] == 0.0
    assert R.bins_of(np.array([1.0, 0.0, -1.0]), EDGES).tolist() == [0, 360, 719]
    # every bin k holds the angles of [k / 4, (k + 1) / 4) degrees
    mid = np.cos(np.deg2rad((np.arange(720) + 0.5) * 0.25))
    assert R.bins_of(mid, EDGES).tolist() == list(range(720))


def test_default_classes():
    from manydepth import evaluation
    assert NE.MATERIAL_GREY == evaluation._MATERIAL_GREY
    assert [n for n, _ in NE.DEFAULT_CLASSES] == ["all", "objects"] + list(evaluation._MATERIAL_GREY) and len(NE.DEFAULT_CLASSES) == 12
    assert NE.DEFAULT_CLASSES[0][1] is None and NE.DEFAULT_CLASSES[1][1] == (20, 160) and NE.DEFAULT_CLASSES[9][1] == (160, 160)
    names, table = NE.class_table(NE.DEFAULT_CLASSES)
    assert list(table)[:6] == [1, 0, 20, 160, 20, 20] and len(table) == 24
