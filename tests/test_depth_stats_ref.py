"""tests/depth_stats_ref.py, the NumPy statement of pd_depth_stats / pd_depth_medians, against the reference's own
compute_depth_errors_numpy (tests/golden/g11_depth_errors.npz, made by tests/golden/make_golden_depth.py) and against
np.median / torch.median.  No GPU."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import depth_stats_ref as R

G11 = os.path.join(GOLDEN, "g11_depth_errors.npz")


@pytest.fixture(scope="module")
def g11():
    return np.load(G11)


def _case(g, case):
    lohi = (int(g["mask_value"]), int(g["mask_value"])) if case == "material" else (1, 0)
    return g[f"{case}__gt"][None], g[f"{case}__pred"][None], g[f"{case}__mask"][None], [lohi]


@pytest.mark.parametrize("case", ["material", "frame"])
def test_ref_reproduces_the_reference_figures(g11, case):
    """1e-5: the tolerance tests/test_loss_gpu.py uses for these metrics, which the reference computes in fp32"""
    gt, pred, mask, classes = _case(g11, case)
    lo, hi = float(g11["min_depth"]), float(g11["max_depth"])
    st = R.stats(pred, gt, mask, classes, R.edges_numpy(), lo, hi)
    assert st["n"][0, 0] == int(g11[f"{case}__count"]) and st["bad"][0, 0] == 0 and st["hist"][0, 0].sum() == st["n"][0, 0]
    got = R.errors_from(st, 0, 0)
    print(case, "max abs diff", np.abs(got - g11[f"{case}__errors"]).max())
    assert np.allclose(got, g11[f"{case}__errors"], rtol=0.0, atol=1e-5)


@pytest.mark.parametrize("case", ["material", "frame"])
def test_ref_reproduces_the_median_scaled_figures(g11, case):
    gt, pred, mask, classes = _case(g11, case)
    lo, hi = float(g11["min_depth"]), float(g11["max_depth"])
    n, med = R.medians(pred, gt, mask, classes, lo, hi)
    scale = R.scale_of(med, "numpy")
    assert n[0, 0] == int(g11[f"{case}__count"])
    assert scale.dtype == np.float32 and scale[0, 0] == g11[f"{case}__ratio"]            # np.median in float32, bit for bit
    st = R.stats(pred, gt, mask, classes, R.edges_numpy(), lo, hi, scale=scale)
    got = R.errors_from(st, 0, 0)
    print(case, "scaled: max abs diff", np.abs(got - g11[f"{case}__errors_scaled"]).max())
    assert np.allclose(got, g11[f"{case}__errors_scaled"], rtol=0.0, atol=1e-5)
    unscaled = R.errors_from(R.stats(pred, gt, mask, classes, R.edges_numpy(), lo, hi), 0, 0)
    assert not np.allclose(got, unscaled, atol=1e-3)                                    # the fixture does need its scale


def test_medians_are_the_sorted_values_and_both_conventions():
    rng = np.random.default_rng(3)
    for count in (1, 2, 3, 10, 11):
        gt = rng.uniform(0.3, 1.5, (1, 1, count)).astype(np.float32)
        pred = rng.uniform(0.3, 1.5, (1, 1, count)).astype(np.float32)
        n, med = R.medians(pred, gt, None, [(1, 0)], 0.1, 2.0)
        assert n[0, 0] == count
        assert np.float32(np.median(gt)) == (med[0, 0, 0] + med[0, 0, 1]) / np.float32(2)
        assert torch.median(torch.from_numpy(pred)).item() == med[0, 0, 2]               # the lower middle
        a, b = R.scale_of(med, "numpy")[0, 0], R.scale_of(med, "torch")[0, 0]
        assert a == np.median(gt) / np.median(pred)
        if count % 2:
            assert a == b and med[0, 0, 0] == med[0, 0, 1] and med[0, 0, 2] == med[0, 0, 3]
    # even n, constructed: the two conventions differ
    gt = np.array([[[0.5, 1.0, 1.5, 1.75]]], np.float32)
    pred = np.array([[[0.25, 0.5, 1.0, 1.25]]], np.float32)
    n, med = R.medians(pred, gt, None, [(1, 0)], 0.1, 2.0)
    assert med[0, 0].tolist() == [1.0, 1.5, 0.5, 1.0]
    assert R.scale_of(med, "numpy")[0, 0] == np.float32(1.25) / np.float32(0.75)
    assert R.scale_of(med, "torch")[0, 0] == np.float32(2.0)
    assert R.scale_of(med, "numpy")[0, 0] != R.scale_of(med, "torch")[0, 0]
    # an empty class: no medians, no scale, and with that scale its (absent) pixels are bad
    n, med = R.medians(pred, gt, np.zeros((1, 1, 4), np.int32), [(5, 5)], 0.1, 2.0)
    assert n[0, 0] == 0 and np.isnan(med).all() and np.isnan(R.scale_of(med, "numpy")).all()


def test_rules_of_the_statement():
    e = R.edges_numpy()
    assert e.shape == (511,) and e[249] == 0.125 and e[9] == 10 * 0.0005
    gt = np.array([[[1.0, 1.0, 1.0, 0.1, 2.0, 1.0, 1.0]]], np.float32)
    pred = np.array([[[0.875, 0.7, 0.8, 1.0, 1.0, np.nan, 5.0]]], np.float32)
    st = R.stats(pred, gt, None, [(1, 0)], e, 0.1, 2.0)
    # gt at min_depth and at max_depth is gated out; the NaN is bad; 5.0 is clamped to 2.0
    assert st["n"][0, 0] == 4 and st["bad"][0, 0] == 1
    assert st["hist"][0, 0, 250] == 1                        # |d| = 0.125 sits on edge 250 and belongs to the bin above it
    assert st["hist"][0, 0, 511] == 2                        # 0.3 (fp32) and 1.0 are beyond 255.5 mm
    assert st["a"][0, 0].tolist() == [1, 3, 3]               # 1 / 0.8f rounds to 1.25 exactly in fp32: not below 1.25
    assert np.isnan(st["err"][0, 0, [3, 4, 5]]).all() and st["err"][0, 0, 6] == 1.0


def test_default_classes_are_the_normals_evaluators():
    from polardepth import depth_eval, normals_eval
    assert depth_eval.DEFAULT_CLASSES is normals_eval.DEFAULT_CLASSES and len(depth_eval.DEFAULT_CLASSES) == 12
    assert np.array_equal(depth_eval.edges_numpy(), R.edges_numpy())
    assert depth_eval.BINS == R.BINS
