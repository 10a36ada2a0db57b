"""tests/reproj_ref.py (the fp64 NumPy statement of csrc/reproj.hip's definitions) against fixture G12, the reference's own
BackprojectDepth / Project3D / grid_sample / compute_reprojection_loss / compute_loss_masks run in float64
(tests/golden/make_golden_reproj.py): coordinates, warped images, the depth gradient and the reduction agree to 1e-12."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import reproj_ref as R

TOL = 1e-12


@pytest.fixture(scope="module")
def g12():
    return dict(np.load(os.path.join(GOLDEN, "g12_reproj.npz")))


def test_fixture_is_what_the_issue_asks_for(g12):
    assert g12["depth"].shape == (2, 1, 19, 37) and g12["src0"].shape == (2, 3, 19, 37) and g12["T1"].shape == (2, 4, 4)
    assert all(g12[k].dtype == np.float32 for k in ("depth", "target", "src0", "src1", "K", "inv_K", "T0", "T1", "noise"))
    assert not np.array_equal(g12["K"][0], g12["K"][1])
    assert (g12["past_borders"] >= 0.2).all()
    assert g12["share_near_boundary"] <= 0.03 and g12["share_near_tie"] <= 0.01
    assert g12["coords0_f64"].dtype == np.float64 and g12["warped0_f32"].dtype == np.float32


@pytest.mark.parametrize("f", [0, 1])
def test_view_synthesis_matches_the_reference_in_fp64(g12, f):
    H, W = 19, 37
    out = R.view_synth(g12["depth"], g12[f"src{f}"], g12["K"], g12["inv_K"], g12[f"T{f}"])
    assert np.abs(out["coords"] - g12[f"coords{f}_f64"]).max() <= TOL * max(1.0, np.abs(g12[f"coords{f}_f64"]).max())
    assert np.abs(out["warped"] - g12[f"warped{f}_f64"]).max() <= TOL
    c = g12[f"coords{f}_f64"]
    assert np.array_equal(out["free_x"], (c[..., 0] > 0) & (c[..., 0] < W - 1))
    assert np.array_equal(out["free_y"], (c[..., 1] > 0) & (c[..., 1] < H - 1))
    if f == 1:
        assert (~out["free_x"]).mean() > 0.4 and (~out["free_y"]).mean() > 0.4       # the large pose leaves on all four sides


@pytest.mark.parametrize("f", [0, 1])
def test_depth_gradient_matches_the_reference_autograd_in_fp64(g12, f):
    out = R.view_synth(g12["depth"], g12[f"src{f}"], g12["K"], g12["inv_K"], g12[f"T{f}"])
    g = R.view_synth_grad(g12[f"gw{f}"], g12[f"src{f}"], out["coords"], g12["depth"], g12["K"], g12["inv_K"], g12[f"T{f}"])
    want = g12[f"gdepth{f}_f64"]
    assert np.abs(g - want).max() <= TOL * max(1.0, np.abs(want).max())
    both_clamped = ~out["free_x"] & ~out["free_y"]
    assert both_clamped.any() or f == 0
    assert (g[:, 0][both_clamped] == 0).all() and (want[:, 0][both_clamped] == 0).all()


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_combine_matches_the_reference(g12, tag):
    """Fed the reference's own maps (of either precision) the reduction reproduces its mask, its minimum's frame and its loss;
    the fp32 run's loss is an fp32 sum, so it is met to fp32 rounding only."""
    reproj = [g12[f"reproj{f}_{tag}"] for f in range(2)]
    ident = [g12[f"ident{f}_{tag}"] for f in range(2)]
    noise = g12["noise"].astype(reproj[0].dtype)
    out = R.combine(reproj, ident, noise)
    mask = g12[f"mask_{tag}"][:, 0] != 0
    assert np.array_equal(out["mask"], mask)
    assert np.array_equal(out["sel"][mask], g12[f"argmin_{tag}"][:, 0][mask].astype(np.uint8)) and (out["sel"][~mask] == 255).all()
    assert out["count"] == mask.sum()
    want = float(g12[f"loss_{tag}"])
    assert abs(out["loss"] - want) <= (TOL if tag == "f64" else 64 * 2.0 ** -24 * want)


def test_combine_rules_for_invalid_frames_ties_and_avg():
    rng = np.random.default_rng(0)
    a, b = rng.random((2, 1, 4, 5)), rng.random((2, 1, 4, 5))
    b[0, 0, :2] = a[0, 0, :2]                                                       # planted ties: the earlier frame wins
    out = R.combine([a, b])
    assert (out["sel"][0, :2] == 0).all() and out["count"] == 40 and set(np.unique(out["sel"])) <= {0, 1}
    assert np.isclose(out["loss"], np.minimum(a, b).sum() / (40 + 1e-7), rtol=1e-15)
    valid = np.array([[0.0, 1.0], [0.0, 0.0]])
    out = R.combine([a, b], valid=valid)
    assert (out["sel"][0] == 1).all() and (out["sel"][1] == 255).all() and out["count"] == 20       # an item without a frame
    assert np.isclose(out["sum"], b[0].sum(), rtol=1e-15)
    ident = [a + 1.0, b - 1.0]                                                      # frame 1's identity always beats frame 1
    out = R.combine([a, b], ident, valid=np.array([[1.0, 0.0], [1.0, 1.0]]))
    assert (out["sel"][0] == 0).all() and (out["sel"][1] == 255).all()              # ... but it is invalid for item 0
    out = R.combine([a, b], avg=True)
    assert np.isclose(out["sum"], ((a + b) / 2).sum(), rtol=1e-15) and (out["sel"] == 0).all()
    g = R.combine_grad(2.0, out["sel"], out["count"], None, 2, avg=True)
    assert np.allclose(g[0], 2.0 / (40 + 1e-7) / 2) and np.allclose(g[1], g[0])
    sel = R.combine([a, b])["sel"]
    g = R.combine_grad(1.0, sel, 40.0, None, 2)
    assert np.array_equal(g[0][:, 0] != 0, sel == 0) and np.array_equal(g[1][:, 0] != 0, sel == 1)


@pytest.mark.parametrize("f", [0, 1])
def test_gradient_magnitude_bounds_the_gradient_and_frame_1_holds_the_clamped_populations(g12, f):
    """view_synth_grad(magnitude=True) is the same expression with |.| on every summand: never below |gradient|, equal to it
    where one channel term and one axis are all there is; frame 1 has at least 50 pixels with exactly one clamped axis and 50
    with both (tests/test_reproj_gpu.py compares those with the single-axis value and with exactly 0)."""
    a = (g12[f"gw{f}"], g12[f"src{f}"], g12[f"coords{f}_f32"], g12["depth"], g12["K"], g12["inv_K"], g12[f"T{f}"])
    g, mag = R.view_synth_grad(*a), R.view_synth_grad(*a, magnitude=True)
    assert (mag >= np.abs(g) * (1 - 1e-14)).all() and (mag[g != 0] > 0).all()
    s = R.sample(g12[f"src{f}"], g12[f"coords{f}_f32"])
    one, both = s["free_x"] ^ s["free_y"], ~s["free_x"] & ~s["free_y"]
    assert (mag[:, 0][both] == 0).all()
    if f == 1:
        assert one.sum() >= 50 and both.sum() >= 50
    one_channel = (a[0][:, :1], a[1][:, :1]) + a[2:]
    g1, m1 = R.view_synth_grad(*one_channel), R.view_synth_grad(*one_channel, magnitude=True)
    only_x = s["free_x"] & ~s["free_y"]                   # gu alone: a sum of two tap terms times du
    assert (m1[:, 0][only_x] >= np.abs(g1[:, 0][only_x]) * (1 - 1e-14)).all() and only_x.any()


def test_no_gate_undecided_ssim_pixel_on_the_fixture_images(g12):
    """The whole-term disparity-gradient test excludes disparity pixels that hear of an SSIM gate-undecided pixel, capped at
    5 %: on the fixture's images (fp64 warped frames against the target) there is none, so nothing is blended."""
    import torch
    import ssim_cases as sc
    tgt = torch.from_numpy(g12["target"])
    for f in range(2):
        und = sc.gate_undecided(torch.from_numpy(g12[f"warped{f}_f64"]).float(), tgt, dilate=True)
        print(f"frame {f}: undecided (dilated) {und.double().mean().item():.4f}")
        assert und.double().mean().item() <= 0.05
