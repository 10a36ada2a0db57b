"""tests/matching_ref.py -- the NumPy statement of pd_cost_volume that the device is held to bit for bit -- against the
reference's own float64 run of match_features / compute_confidence_mask / the lowest-cost map (tests/golden/g13_matching.npz,
written by tests/golden/make_golden_matching.py).  No GPU.

Excluded: pixels with a (bin, frame) coordinate within 1e-3 px of a threshold of the edge mask ("near": a float32 coordinate
may fall on the other side) and pixels whose two smallest costs differ by less than 1e-5 ("tie": the argmin may differ).  The
cost bound is 2 * dev_cost_max, the recorded |float32 - float64| of the REFERENCE's two runs: matching_ref and the reference's
float32 run are both float32 sums of 64 terms, in different orders.  The bound comes from the fixture, never from this code."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import matching_ref as MR
from polardepth import matching

BINNINGS = ("linear", "inverse")


@pytest.fixture(scope="module")
def g13():
    return dict(np.load(os.path.join(GOLDEN, "g13_matching.npz")))


def _inner(shape):
    m = np.zeros(shape, bool)
    m[:, 2:-2, 2:-2] = True
    return m


def test_fixture_meets_its_conditions(g13):
    inner = _inner(g13["near"].shape)
    assert g13["near"][inner].mean() <= 0.05
    for g in BINNINGS:
        assert g13[f"tie_{g}"][inner].mean() <= 0.02
        assert 0.2 < g13[f"confidence_{g}"][inner].mean() < 0.9
        assert (g13[f"share_frames_{g}"] >= 0.1).all()
        assert g13[f"cost_{g}"].dtype == np.float64 and g13[f"cost_{g}"].shape == (2, 16, 24, 40)
    assert (g13["poses"][1, 1] == 0).all() and 0 < g13["dev_cost_max"] < 1e-5


@pytest.mark.parametrize("binning", BINNINGS)
def test_depth_bins_bit_equal(g13, binning):
    got = matching.depth_bins(0.3, 2.0, 16, binning)
    assert got.dtype == torch.float32 and got.device.type == "cpu"
    assert np.array_equal(got.numpy().view(np.uint32), g13[f"bins_{binning}"].view(np.uint32))
    with pytest.raises(NotImplementedError):
        matching.depth_bins(0.3, 2.0, 16, "log")


@pytest.mark.parametrize("binning", BINNINGS)
def test_matching_ref_against_the_reference_float64_run(g13, binning):
    valid = MR.frame_valid(g13["poses"])
    assert valid.tolist() == [[True, True], [True, False]]
    r = MR.cost_volume(g13["cur"], g13["lookup"], g13["poses"], g13["K"], g13["inv_K"], g13[f"bins_{binning}"], valid)
    keep = ~(g13["near"] | g13[f"tie_{binning}"])
    assert keep[_inner(keep.shape)].mean() > 0.9         # (every border pixel is a tie: all its costs are 0)
    k4 = np.broadcast_to(keep[:, None], r["cost"].shape)
    assert np.array_equal(r["missing"][k4], g13[f"missing_{binning}"][k4])
    assert np.array_equal(r["confidence"][keep], g13[f"confidence_{binning}"][keep].astype(np.float32))
    # a border pixel (all costs 0, hence a "tie") still has to come out as the reference's: empty, argmin 0
    border = ~_inner(keep.shape)
    assert np.array_equal(r["argmin"][border], g13[f"argmin_{binning}"][border]) and not r["argmin"][border].any()
    assert not r["cost"][np.broadcast_to(border[:, None], r["cost"].shape)].any() and not r["confidence"][border].any()
    assert np.array_equal(r["argmin"][keep], g13[f"argmin_{binning}"][keep])
    dev = np.abs(r["cost"].astype(np.float64) - g13[f"cost_{binning}"])[k4].max()
    print("cost deviation", dev, "bound", 2 * float(g13["dev_cost_max"]))
    assert dev <= 2 * float(g13["dev_cost_max"])
    assert np.allclose(r["lowest"][keep], g13[f"lowest_{binning}"][keep], rtol=1e-6, atol=0)
    assert r["cost"].dtype == np.float32 and r["lowest"].dtype == np.float32
    # the frames that contributed are the fixture's shares
    inner = np.broadcast_to(_inner(keep.shape)[:, None], r["nframes"].shape)
    shares = np.array([(r["nframes"][inner] == k).mean() for k in range(3)])
    assert np.abs(shares - g13[f"share_frames_{binning}"]).max() < 0.01


def test_channel_sum_order():
    # 16 partials of 4 consecutive channels (+64k), then a binary tree: distinguishable from a left-to-right sum in fp32
    a = (np.float32(1) + np.arange(128, dtype=np.float32) * np.float32(2.0 ** -20)) * np.float32(1 / 3)
    part = [np.float32(0)] * 16
    for c0 in (0, 64):
        for l in range(16):
            for k in range(4):
                part[l] = np.float32(part[l] + a[c0 + 4 * l + k])
    while len(part) > 1:
        part = [np.float32(part[i] + part[i + 1]) for i in range(0, len(part), 2)]
    assert MR.channel_sum(a[None]).view(np.uint32)[0] == part[0].view(np.uint32)
    assert MR.channel_sum(a[None, :16])[0] == np.float32(np.float32(np.float32(a[0] + a[1]) + a[2]) + a[3]) + \
        np.float32(np.float32(np.float32(a[4] + a[5]) + a[6]) + a[7]) + \
        (np.float32(np.float32(np.float32(a[8] + a[9]) + a[10]) + a[11]) +
         np.float32(np.float32(np.float32(a[12] + a[13]) + a[14]) + a[15]))


def test_count_plus_epsilon_is_evaluated_in_float32():
    # one frame: c = s / (1 + 1e-7f) = s / 1.0000001 (1 + 1e-7 rounds UP in fp32); two frames: (2 + 1e-7f) == 2
    assert np.float32(1) + np.float32(1e-7) > np.float32(1) and np.float32(2) + np.float32(1e-7) == np.float32(2)
