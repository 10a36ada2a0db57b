"""oracle/reproj.py (the PyTorch-CPU restatement of the photometric term, differentiable by autograd) pinned two ways:

* in fp64 against fixture G12, the reference's own float64 run (tests/golden/make_golden_reproj.py): warped images, the
  reproj / identity maps, the loss and its depth gradient to 1e-12 relative -- the bar tests/reproj_ref.py meets for its
  pieces -- and the mask and the minimum's frame exactly;
* against tests/reproj_ref.combine, the fp64 NumPy statement of the project's reduction rule, on every case of the device
  test's table (tests/reproj_cases.py: ``valid`` rows with a missing frame, an item without frames, ``avg``, ties), with the
  oracle's own selection and with the selection given."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import reproj_ref as R
from reproj_cases import COMBINE_CASES, combine_cases
from oracle import reproj as orp

TOL = 1e-12


@pytest.fixture(scope="module")
def g12():
    return dict(np.load(os.path.join(GOLDEN, "g12_reproj.npz")))


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = np.abs(got - want).max(), max(1.0, np.abs(want).max())
    assert err <= TOL * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


def _term(g12, dtype, **kw):
    t = {k: torch.from_numpy(g12[k]) for k in ("depth", "target", "src0", "src1", "K", "inv_K", "T0", "T1", "noise")}
    depth = t["depth"].to(dtype).requires_grad_(True)
    out = orp.photometric_term(depth, t["target"], [t["src0"], t["src1"]], t["K"], t["inv_K"], [t["T0"], t["T1"]],
                               noise=t["noise"], details=True, **kw)
    return depth, out


def test_fp64_oracle_reproduces_the_reference_run(g12):
    depth, out = _term(g12, torch.float64)
    for f in range(2):
        _close(out["warped"][f].detach(), g12[f"warped{f}_f64"], f"warped{f}")
        _close(out["reproj"][f].detach(), g12[f"reproj{f}_f64"], f"reproj{f}")
        _close(out["identity"][f].detach(), g12[f"ident{f}_f64"], f"ident{f}")
    assert np.array_equal(out["mask"].numpy(), g12["mask_f64"][:, 0] != 0)
    assert np.array_equal(out["arg"].numpy(), g12["argmin_f64"][:, 0])
    assert 0.1 < out["mask"].double().mean().item() < 0.9 and set(np.unique(out["sel"].numpy())) == {0, 1, 255}
    want = float(g12["loss_f64"])
    assert abs(out["loss"].item() - want) <= TOL * abs(want)
    out["loss"].backward()
    assert np.abs(g12["gloss_depth_f64"]).max() > 0
    _close(depth.grad, g12["gloss_depth_f64"], "gloss_depth")


def test_one_text_runs_in_fp32_and_the_given_selection_reproduces_the_own_one(g12):
    """The fp32 run stays fp32 end to end and lands where the reference's fp32 run did (2x its recorded distance from its
    fp64 run); handing the oracle its own selection changes neither the loss nor the gradient, in both dtypes."""
    for dtype in (torch.float32, torch.float64):
        depth, out = _term(g12, dtype)
        assert out["loss"].dtype == dtype and all(w.dtype == dtype for w in out["warped"])
        out["loss"].backward()
        depth2, again = _term(g12, dtype, sel=out["sel"])
        again["loss"].backward()
        assert torch.equal(again["sel"], out["sel"]) and again["count"] == out["count"]
        tol = 8 * torch.finfo(dtype).eps
        assert abs(again["loss"].item() - out["loss"].item()) <= tol * abs(out["loss"].item())
        assert (depth2.grad - depth.grad).abs().max().item() <= tol * depth.grad.abs().max().item()
        if dtype == torch.float32:
            assert abs(out["loss"].item() - float(g12["loss_f64"])) <= max(2.0 * float(g12["dev_loss"]), 1e-6)


def test_options_change_the_term_and_a_foreign_selection_is_obeyed(g12):
    _, base = _term(g12, torch.float64)
    vals = {"base": base["loss"].item()}
    for name, kw in (("no_ssim", {"no_ssim": True}), ("no_automask", {"automask": False}), ("avg", {"avg": True})):
        vals[name] = _term(g12, torch.float64, **kw)[1]["loss"].item()
    assert len(set(vals.values())) == 4, vals
    _, plain = _term(g12, torch.float64, automask=False)
    assert plain["mask"].all() and plain["count"].item() == plain["mask"].numel()
    # frame 1 everywhere on item 0, everything masked on item 1: the mean of reproj1 over item 0
    sel = torch.full((2, 19, 37), 255, dtype=torch.uint8)
    sel[0] = 1
    _, out = _term(g12, torch.float64, sel=sel)
    want = g12["reproj1_f64"][0].sum() / (19 * 37 + 1e-7)
    assert abs(out["loss"].item() - want) <= TOL * want


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_given_sampling_cells_reproduce_grid_sample_away_from_cell_boundaries(g12, tag):
    """``coords`` = the reference's own coordinates (of its fp64 run: the oracle's own cells; of its fp32 run: cells decided
    at another rounding): warped images, loss and depth gradient are grid_sample's -- to 1e-12 with the own cells, and with
    the fp32 run's cells everywhere except the pixels within 1e-3 px of a cell boundary or border, where the slope may be
    the neighbouring cell's.  Frame 1 leaves the image on all four sides, so clamped axes are among the given cells."""
    coords = [torch.from_numpy(g12[f"coords{f}_{tag}"]) for f in range(2)]
    depth, ref = _term(g12, torch.float64)
    ref["loss"].backward()
    depth2, out = _term(g12, torch.float64, coords=coords, sel=ref["sel"])
    out["loss"].backward()
    near = np.zeros((2, 19, 37), bool)
    tol = TOL if tag == "f64" else 1e-6       # across a boundary: (1e-6 px of fp32 rounding) x (a second difference of the image)
    for f in range(2):
        assert np.abs(out["warped"][f].detach().numpy() - g12[f"warped{f}_f64"]).max() <= tol
        near |= R.near_boundary(g12[f"coords{f}_f64"], 19, 37)
    assert abs(out["loss"].item() - float(g12["loss_f64"])) <= tol
    near = torch.from_numpy(near)[:, None]
    near = torch.nn.functional.max_pool2d(near.double(), 5, 1, 2) > 0       # ... and what hears of it through the SSIM windows
    if tag == "f64":
        near[:] = False
    assert near.double().mean().item() <= 0.5
    _close(depth2.grad[~near], depth.grad[~near], "gloss_depth")


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


@pytest.mark.parametrize("given", [False, True], ids=["own_selection", "given_selection"])
@pytest.mark.parametrize("case", COMBINE_CASES)
def test_combine_agrees_with_the_numpy_statement(g12, case, given):
    """In fp64 (both sides fed the case's maps cast to fp64; the casts keep the planted ties): selection and count exactly,
    loss and the gradient w.r.t. the maps to 1e-12.  In fp32 (the maps' own dtype, the per-pixel arithmetic of ``avg`` and
    the noise in fp32 on both sides): selection and count exactly; the oracle's sums are fp32 sums, met to fp32 rounding."""
    kw = combine_cases(g12)[case]
    valid, avg = kw.get("valid"), kw.get("avg", False)
    for dtype, np_dt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        cast = lambda maps: None if maps is None else [np.asarray(m, np_dt) for m in maps]
        want = R.combine(cast(kw["reproj"]), cast(kw.get("identity")),
                         None if kw.get("noise") is None else kw["noise"].astype(np_dt), valid, avg)
        maps = [_t(r, dtype).requires_grad_(True) for r in kw["reproj"]]
        ident = None if kw.get("identity") is None else [_t(i, dtype) for i in kw["identity"]]
        out = orp.combine(maps, ident, _t(kw.get("noise"), dtype), valid, avg,
                          sel=torch.from_numpy(want["sel"]) if given else None)
        assert np.array_equal(out["sel"].numpy(), want["sel"]), (case, dtype)
        assert out["count"].item() == want["count"]
        assert out["loss"].dtype == dtype
        tol = TOL if dtype == torch.float64 else 64 * 2.0 ** -24
        assert abs(out["loss"].item() - want["loss"]) <= tol * abs(want["loss"]), (case, dtype, out["loss"].item(), want["loss"])
        out["loss"].backward()
        for m, w in zip(maps, R.combine_grad(1.0, want["sel"], want["count"], valid, 2, avg)):
            g = m.grad.numpy()
            assert np.array_equal(g != 0, w != 0)
            assert np.abs(g - w).max() <= (TOL if dtype == torch.float64 else 4 * 2.0 ** -24) * np.abs(w).max()
    sel = want["sel"]
    if case == "item_without_frames":
        assert (sel[0] == 255).all() and (sel[1] != 255).any()
    if case == "tie_between_frames":
        assert (sel[:, 3:9] == 0).all() and (sel == 1).any()
    if case == "tie_with_identity":
        assert (sel[0, :5] != 255).all()
    if case == "first_frame_invalid":
        assert set(np.unique(sel[0])) <= {1, 255} and set(np.unique(sel[1])) <= {0, 255}
