"""CPU half of the SSIM kernel tests (tests/ssim_cases.py, tests/test_ssim_kernels_gpu.py): the named inputs hold the
populations the GPU tests rely on, the fp32 oracle reproduces fixture G5, the share of the gradient excluded as
gate-undecided stays under its cap, the NumPy fp32 transcription of the kernels' order passes every check the device has to
pass -- with the mean ratios that support MEAN_MARGIN printed per case -- and four mutations of the transcription each fail
at least one of those checks.

Conditioning max|o32 - o64| / max|o64| at the statistics shape (printed; capped for `noise` only, at 2 x the measurement):
  noise 4.6e-06   training 1.2e-03   dark 1.3e-03   flat 1.1e+01   identical 0   signed 1.5e-02   steps 1.5e-04"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import loss_cases as lc
import ssim_cases as sc

F32, F64 = sc.F32, sc.F64
SMALL = [g for g in sc.GEOMS if g != sc.STRIDE]
LAUNCHES = ((0, False), (1, False), (1, True))


def test_geometries_cover_the_folds_the_odd_sizes_and_the_second_grid_stride_trip():
    assert (1, 1, 2, 2) in sc.GEOMS                                # both reflections of a window fold onto the same pixel
    assert any(g[1] not in (1, 3) and g[2] % 2 and g[3] % 2 for g in sc.GEOMS)
    N, C, H, W = sc.STRIDE
    assert C == 1 and N * H * W > sc.GRID_CAP == lc.GRID_CAP       # forward (pixels) and backward (elements) both stride
    assert all(g[0] * g[1] * g[2] * g[3] <= sc.GRID_CAP for g in SMALL)
    assert sc.forward_cases(sc.STRIDE) == ["noise"] == sc.backward_cases(sc.STRIDE)
    assert sc.STAT[0] * sc.STAT[1] * sc.STAT[2] * sc.STAT[3] >= sc.MEAN_MIN
    for g in SMALL:
        assert {"noise", "steps"} <= set(sc.forward_cases(g)) and {"noise", "steps"} <= set(sc.backward_cases(g))
    assert sc.forward_cases(sc.STAT) == sc.CASES and set(sc.backward_cases(sc.STAT)) == set(sc.GRAD_CASES)


@pytest.mark.parametrize("case", sc.CASES)
def test_case_populations_and_conditioning(case):
    x, y = sc.make(case, sc.STAT)
    assert x.dtype == y.dtype == F32 and x.shape == y.shape == sc.STAT
    x2, y2 = sc.make.__wrapped__(case, sc.STAT)
    assert torch.equal(x, x2) and torch.equal(y, y2)               # a function of the seed alone
    u = sc.unclamped(x, y, F64)
    r32, r64 = sc.ref_ssim(x, y, F32), sc.ref_ssim(x, y, F64)
    cond = lc.conditioning(r32, r64)
    print(f"{case}: fp64 mean {r64.mean().item():.3e}, unclamped in [{u.min().item():.3e}, {u.max().item():.3e}], "
          f"oracle fp32 deviation max {(r32 - r64).abs().max().item():.2e} mean {(r32 - r64).abs().mean().item():.2e}, "
          f"conditioning {cond:.2e}, undecided {sc.gate_undecided(x, y).double().mean().item():.4f}")
    # |n| <= d for any real images (module docstring of ssim_cases): the exact value never leaves [0, 1]
    assert u.min().item() >= -1e-12 and u.max().item() <= 1 + 1e-12
    assert not sc.beyond_clamp(x, y).any()
    kinks = (x == y).double().mean().item()
    if case == "noise":
        assert cond <= sc.NOISE_COND_CAP
        assert x.min() >= 0 and y.min() >= 0 and y.max() <= 1
    if case in ("training", "dark"):
        s = 1.0 if case == "training" else 0.05
        assert x.min().item() > 0.7 * s and x.max().item() < s           # bright (dark: x 0.05), smooth, nearly equal
        assert (y - x).abs().max().item() < 5 * sc.TRAIN_AMP * s and (x[..., 1:] - x[..., :-1]).abs().max().item() < 0.02 * s
        assert cond > 20 * sc.NOISE_COND_CAP                              # the cancellation regime, unlike noise
    if case == "dark":
        xt, yt = sc.make("training", sc.STAT)
        assert not torch.equal(x, xt) and (x - 0.05 * xt).abs().max().item() <= 1e-3 * 0.05
    if case == "flat":
        assert x.unique().numel() == 1 and y.unique().numel() == 1 and abs((y - x).mean().item() - 0.003) < 1e-6
        assert sc.gate_undecided(x, y).all()                             # fp32 noise is ten times the true value
    if case == "identical":
        assert y is x and (u == 0).all() and x.unique().numel() > 1000
    if case == "signed":
        assert abs(x.mean().item()) < 0.05 and abs(y.mean().item()) < 0.05 and x.min() < -1 and y.min() < -1
        assert (u > 1 - 1e-4).double().mean().item() >= 0.50 and (u < 1e-4).double().mean().item() >= 0.25
        em = sc.emulate_fwd(x, y, 0)                                      # fp32 lands on both clamps by rounding
        assert (em == 1).double().mean().item() >= 0.10 and (em == 0).double().mean().item() >= 0.02
    if case == "steps":
        flat = sum((x[..., 1 + dy:x.shape[2] - 1 + dy, 1 + dx:x.shape[3] - 1 + dx] == x[..., 1:-1, 1:-1])
                   for dy in (-1, 0, 1) for dx in (-1, 0, 1)) == 9
        share = flat.double().mean().item()
        assert 0.2 < share < 0.6                                          # flat and textured windows alternate
        assert (y - x).abs().min().item() >= 0.049
    assert (kinks == 1.0) if case == "identical" else (kinks == 0.0)     # only `identical` sits on the kink of |y - x|


def test_steps_has_an_edge_in_every_geometry():
    for g in SMALL:
        x, y = sc.make("steps", g)
        assert (x.amax((2, 3)) > x.amin((2, 3))).all() and (y.amax((2, 3)) > y.amin((2, 3))).all()


def test_fp32_oracle_reproduces_the_fixture():
    G5 = np.load(os.path.join(GOLDEN, "g5_loss.npz"))
    x, y, out = (torch.from_numpy(G5[k]) for k in ("ssim.x", "ssim.y", "ssim.out"))
    r32, r64 = sc.ref_ssim(x, y, F32), sc.ref_ssim(x, y, F64)
    err, tol = lc.assert_elem(out, r32, r64, "fixture G5 vs oracle")
    print(f"fixture vs fp64 oracle: {err:.2e} (tol {tol:.2e}); vs fp32 oracle {(out - r32).abs().max().item():.2e}")
    assert (out - r32).abs().max().item() <= 2 * (r32.double() - r64).abs().max().item()
    assert torch.allclose(sc.unclamped(x, y, F64).clamp(0, 1), r64, rtol=0, atol=1e-15)


@pytest.mark.parametrize("geom", sc.GEOMS)
def test_excluded_share_of_the_gradient_is_capped(geom):
    for case in sc.backward_cases(geom):
        x, y = sc.make(case, geom)
        for mode in (0, 1):
            ex = 1.0 - sc.grad_keep(x, y, mode).double().mean().item()
            print(f"{case} {geom} mode {mode}: excluded {ex:.4f}")
            assert ex <= sc.EXCLUDED_CAP
        assert sc.cot_zero(geom).double().mean().item() >= 0.25 or min(geom[2:]) < 4
        assert (sc.cotangent(geom, 0)[sc.cot_zero(geom)] == 0).all()


@pytest.mark.parametrize("geom", SMALL)
def test_transcription_passes_every_check_and_supports_the_mean_margin(geom):
    worst = 0.0
    for case in sc.forward_cases(geom):
        x, y = sc.make(case, geom)
        out0 = sc.emulate_fwd(x, y, 0)
        for mode, ns in LAUNCHES:
            r = sc.check_forward(sc.emulate_fwd(x, y, mode, ns), case, geom, mode, ns)
            worst = max(worst, r or 0.0)
        sc.check_mode1_from_mode0(sc.emulate_fwd(x, y, 1), out0, x, y, f"mode 1 from mode 0 {case} {geom}")
    for case in sc.backward_cases(geom):
        x, y = sc.make(case, geom)
        for mode, ns in LAUNCHES:
            r = sc.check_backward(*sc.emulate_bwd(x, y, sc.cotangent(geom, mode), mode, ns), case, geom, mode, ns)
            worst = max(worst, r or 0.0)
    print(f"{geom}: worst mean ratio {worst:.3f} (margin {sc.MEAN_MARGIN})")
    assert worst <= 1.1 < sc.MEAN_MARGIN                                # what is measured here has to support the margin


def _failures(mut):
    """Names of the checks the mutated transcription fails."""
    failed = []
    for geom in SMALL:
        for case in sc.forward_cases(geom):
            x, y = sc.make(case, geom)
            for mode, ns in LAUNCHES[:2]:
                try:
                    sc.check_forward(sc.emulate_fwd(x, y, mode, ns, mut), case, geom, mode, ns)
                except AssertionError:
                    failed.append(f"fwd {case} {geom} mode {mode}")
        for case in sc.backward_cases(geom):
            x, y = sc.make(case, geom)
            for mode, ns in LAUNCHES[:2]:
                try:
                    sc.check_backward(*sc.emulate_bwd(x, y, sc.cotangent(geom, mode), mode, ns, mut), case, geom, mode, ns)
                except AssertionError:
                    failed.append(f"bwd {case} {geom} mode {mode}")
    return failed


@pytest.mark.parametrize("mut", sc.MUTATIONS)
def test_each_mutation_of_the_transcription_fails_a_check(mut):
    failed = _failures(mut)
    print(f"mutation {mut}: {len(failed)} checks fail, e.g. {failed[:4]}")
    assert failed
    if mut == "no_mult":
        assert all(f.startswith("bwd") for f in failed)             # the forward pass has no such factor
    if mut == "fp16_sums":
        # the max-based rule alone is loose on the smooth cases: the mean condition is what catches a precision class there
        assert any("training" in f or "dark" in f for f in failed)


def test_identical_images_give_exact_zeros_in_the_transcription():
    x, y = sc.make("identical", sc.STAT)
    for mode, ns in LAUNCHES:
        assert (sc.emulate_fwd(x, y, mode, ns) == 0).all()
        gx, gy = sc.emulate_bwd(x, y, sc.cotangent(sc.STAT, mode), mode, ns)
        assert (gx == 0).all() and (gy == 0).all()
