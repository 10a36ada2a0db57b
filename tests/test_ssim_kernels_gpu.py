"""pd_ssim_fwd and pd_ssim_bwd (csrc/loss.hip) through the C ABI against the fp64 oracle, elementwise, on the inputs
training gives them.  Inputs, references, the gate-undecided set and the checks live in tests/ssim_cases.py;
tests/test_ssim_cases.py proves on the CPU what the cases hold, runs the same checks on a NumPy transcription of the kernels'
order and shows that four mutations of it fail them.  Every tolerance is the project rule (4 x the fp32 oracle's own
deviation from fp64, tests/loss_cases.py), the mean margin of ssim_cases (1.25, measured on the CPU), or a counted bound
(mode 1 from the device's mode-0 map: a division by C, two products, a sum -> 4 * 2^-24 * max(1, max|.|)).  Exact where the
arithmetic is exact: identical images, the clamp gate, gy == NULL, repeated runs, everything outside a NaN's neighbourhood.

Each test prints its table (SSIMFIG lines: worst error, tolerance, mean ratio, excluded share).

Measured on an MI355X at the statistics shape and the stride shape (the smaller shapes print the same columns):

  output and case                                        max err tolerance  ratio   excl.
  fwd noise (2, 3, 24, 40) mode 0                       3.19e-06  1.35e-05      -       -
  fwd noise (2, 3, 24, 40) mode 1                       8.81e-07  3.78e-06      -       -
  fwd noise (2, 3, 24, 40) mode 1 no_ssim               1.99e-08  3.93e-07      -       -
  fwd training (2, 3, 24, 40) mode 0                    1.79e-04  7.25e-04  0.990       -
  fwd training (2, 3, 24, 40) mode 1                    9.38e-05  4.11e-04  0.993       -
  fwd training (2, 3, 24, 40) mode 1 no_ssim            6.21e-10  2.44e-08      -       -
  fwd dark (2, 3, 24, 40) mode 0                        6.73e-07  3.04e-06  1.000       -
  fwd dark (2, 3, 24, 40) mode 1                        2.56e-07  1.19e-06  0.989       -
  fwd dark (2, 3, 24, 40) mode 1 no_ssim                3.88e-11  1.23e-09      -       -
  fwd flat (2, 3, 24, 40) mode 0                        4.97e-05  1.99e-04      -       -
  fwd flat (2, 3, 24, 40) mode 1                        4.22e-05  1.69e-04      -       -
  fwd flat (2, 3, 24, 40) mode 1 no_ssim                0.00e+00  3.00e-09      -       -
  fwd identical (2, 3, 24, 40) mode 0                   0.00e+00  0.00e+00      -       -
  fwd identical (2, 3, 24, 40) mode 1                   0.00e+00  0.00e+00      -       -
  fwd identical (2, 3, 24, 40) mode 1 no_ssim           0.00e+00  0.00e+00      -       -
  fwd signed (2, 3, 24, 40) mode 0                      1.18e-02  6.11e-02      -       -
  fwd signed (2, 3, 24, 40) mode 1                      5.08e-03  1.90e-02      -       -
  fwd signed (2, 3, 24, 40) mode 1 no_ssim              4.77e-07  1.79e-05      -       -
  fwd steps (2, 3, 24, 40) mode 0                       1.32e-04  5.28e-04  1.048       -
  fwd steps (2, 3, 24, 40) mode 1                       6.27e-05  2.51e-04  1.017       -
  fwd steps (2, 3, 24, 40) mode 1 no_ssim               9.93e-09  1.81e-07      -       -
  fwd noise (1, 1, 513, 1024) mode 0                    6.69e-06  3.79e-05      -       -
  fwd noise (1, 1, 513, 1024) mode 1                    5.70e-06  3.21e-05      -       -
  fwd noise (1, 1, 513, 1024) mode 1 no_ssim            0.00e+00  6.72e-07      -       -
  bwd gx noise (2, 3, 24, 40) mode 0                    2.12e-05  9.25e-05      -  0.0000
  bwd gy noise (2, 3, 24, 40) mode 0                    1.05e-05  4.36e-05      -  0.0000
  bwd gx noise (2, 3, 24, 40) mode 1                    2.96e-06  1.30e-05      -  0.0000
  bwd gy noise (2, 3, 24, 40) mode 1                    2.06e-06  9.70e-06      -  0.0000
  bwd gx noise (2, 3, 24, 40) mode 1 no_ssim            7.95e-08  1.35e-06      -  0.0000
  bwd gy noise (2, 3, 24, 40) mode 1 no_ssim            7.95e-08  1.35e-06      -  0.0000
  bwd gx training (2, 3, 24, 40) mode 0                 2.67e-03  1.06e-02  0.994  0.0026
  bwd gy training (2, 3, 24, 40) mode 0                 2.98e-03  1.35e-02  0.979  0.0026
  bwd gx training (2, 3, 24, 40) mode 1                 9.06e-04  3.86e-03  0.985  0.0026
  bwd gy training (2, 3, 24, 40) mode 1                 1.18e-03  4.04e-03  0.981  0.0026
  bwd gx training (2, 3, 24, 40) mode 1 no_ssim         7.95e-08  1.35e-06      -  0.0000
  bwd gy training (2, 3, 24, 40) mode 1 no_ssim         7.95e-08  1.35e-06      -  0.0000
  bwd gx dark (2, 3, 24, 40) mode 0                     8.63e-06  3.61e-05  0.967  0.0000
  bwd gy dark (2, 3, 24, 40) mode 0                     8.99e-06  3.70e-05  0.894  0.0000
  bwd gx dark (2, 3, 24, 40) mode 1                     2.58e-06  1.21e-05  0.949  0.0000
  bwd gy dark (2, 3, 24, 40) mode 1                     2.40e-06  1.74e-05  0.961  0.0000
  bwd gx dark (2, 3, 24, 40) mode 1 no_ssim             7.95e-08  1.35e-06      -  0.0000
  bwd gy dark (2, 3, 24, 40) mode 1 no_ssim             7.95e-08  1.35e-06      -  0.0000
  bwd gx steps (2, 3, 24, 40) mode 0                    6.69e-04  2.26e-03  1.030  0.0000
  bwd gy steps (2, 3, 24, 40) mode 0                    1.31e-03  4.90e-03  1.032  0.0000
  bwd gx steps (2, 3, 24, 40) mode 1                    2.26e-04  8.98e-04  1.048  0.0000
  bwd gy steps (2, 3, 24, 40) mode 1                    2.48e-04  8.97e-04  1.059  0.0000
  bwd gx steps (2, 3, 24, 40) mode 1 no_ssim            7.95e-08  1.35e-06      -  0.0000
  bwd gy steps (2, 3, 24, 40) mode 1 no_ssim            7.95e-08  1.35e-06      -  0.0000
  bwd gx noise (1, 1, 513, 1024) mode 0                 3.33e-05  1.21e-04      -  0.0000
  bwd gy noise (1, 1, 513, 1024) mode 0                 3.65e-05  1.04e-04      -  0.0000
  bwd gx noise (1, 1, 513, 1024) mode 1                 2.05e-05  9.39e-05      -  0.0000
  bwd gy noise (1, 1, 513, 1024) mode 1                 2.12e-05  8.93e-05      -  0.0000
  bwd gx noise (1, 1, 513, 1024) mode 1 no_ssim         0.00e+00  4.64e-06      -  0.0000
  bwd gy noise (1, 1, 513, 1024) mode 1 no_ssim         0.00e+00  4.64e-06      -  0.0000
  fwd non-finite nan at (3, 4) mode 0                   7.22e-07  1.73e-06      -       -
  fwd non-finite nan at (3, 4) mode 1                   6.15e-07  1.49e-06      -       -
  fwd non-finite nan at (3, 4) mode 1 no_ssim           0.00e+00  3.21e-07      -       -
  fwd non-finite nan at (0, 0) mode 0                   7.22e-07  2.23e-06      -       -
  fwd non-finite nan at (0, 0) mode 1                   6.15e-07  1.94e-06      -       -
  fwd non-finite nan at (0, 0) mode 1 no_ssim           0.00e+00  3.21e-07      -       -
  fwd non-finite inf at (3, 4) mode 0                   7.22e-07  1.73e-06      -       -
  fwd non-finite inf at (3, 4) mode 1                   6.15e-07  1.49e-06      -       -
  fwd non-finite inf at (3, 4) mode 1 no_ssim           0.00e+00  3.21e-07      -       -
  fwd non-finite inf at (0, 0) mode 0                   7.22e-07  2.23e-06      -       -
  fwd non-finite inf at (0, 0) mode 1                   6.15e-07  1.94e-06      -       -
  fwd non-finite inf at (0, 0) mode 1 no_ssim           0.00e+00  3.21e-07      -       -
"""
import functools

import pytest
import torch

import ssim_cases as sc
from polardepth._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
F32, F64 = sc.F32, sc.F64
LAUNCHES = ((0, False), (1, False), (1, True))           # (mode, no_ssim); mode 0 has no L1 term to switch to
GUARD = 1024
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def _dev(case, geom):
    x, y = sc.make(case, geom)
    return x.cuda(), x.cuda() if y is x else y.cuda()


def _fwd(x, y, mode, no_ssim=False):
    N, C, H, W = x.shape
    out = torch.full((N, C if mode == 0 else 1, H, W), float("nan"), device="cuda")
    check(lib.pd_ssim_fwd(ptr(x), ptr(y), ptr(out), N, C, H, W, mode, int(no_ssim), stream_ptr()), "pd_ssim_fwd")
    torch.cuda.synchronize()
    return out


def _bwd(x, y, cot, mode, no_ssim=False, with_gy=True):
    """(gx, gy or None).  Both output buffers are followed by GUARD floats nobody may write; without gy, its whole buffer."""
    N, C, H, W = x.shape
    n = x.numel()
    ws = torch.full((5 * n,), float("nan"), device="cuda")
    bx = torch.full((n + GUARD,), SENTINEL, device="cuda")
    by = torch.full((n + GUARD,), SENTINEL, device="cuda")
    check(lib.pd_ssim_bwd(ptr(x), ptr(y), ptr(cot), ptr(ws), ptr(bx), ptr(by) if with_gy else None, N, C, H, W, mode, int(no_ssim),
                          stream_ptr()), "pd_ssim_bwd")
    torch.cuda.synchronize()
    assert (bx[n:] == SENTINEL).all() and (by[n if with_gy else 0:] == SENTINEL).all()
    return bx[:n].view(x.shape), by[:n].view(x.shape) if with_gy else None


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("geom", sc.GEOMS)
def test_forward_map_and_mix(geom):
    for case in sc.forward_cases(geom):
        x, y = _dev(case, geom)
        outs = {}
        for mode, ns in LAUNCHES:
            outs[mode, ns] = _fwd(x, y, mode, ns)
            sc.check_forward(outs[mode, ns], case, geom, mode, ns)
        xc, yc = sc.make(case, geom)
        sc.check_mode1_from_mode0(outs[1, False], outs[0, False], xc, yc, f"mode 1 from mode 0 {case} {geom}")
        if case == "identical":                           # nn == dd bit for bit: 2 mx mx = mx mx + mx mx, one variance thrice
            assert all((o == 0).all() for o in outs.values())


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("geom", sc.GEOMS)
def test_backward_both_images(geom):
    for case in sc.backward_cases(geom):
        x, y = _dev(case, geom)
        for mode, ns in LAUNCHES:
            gx, gy = _bwd(x, y, sc.cotangent(geom, mode).cuda(), mode, ns)
            sc.check_backward(gx, gy, case, geom, mode, ns)


@pytest.mark.parametrize("geom", [(1, 1, 2, 2), sc.STAT, sc.STRIDE])
def test_backward_without_gy_writes_the_same_gx_and_nothing_else(geom):
    """gy == NULL is the call training makes (the target needs no gradient)."""
    x, y = _dev("noise", geom)
    for mode, ns in LAUNCHES:
        cot = sc.cotangent(geom, mode).cuda()
        gx, gy = _bwd(x, y, cot, mode, ns)
        gx1, none = _bwd(x, y, cot, mode, ns, with_gy=False)              # _bwd asserts the guards and the untouched gy buffer
        assert none is None and torch.equal(gx, gx1) and gx.abs().max().item() > 0 and gy.abs().max().item() > 0


def test_clamped_pixels_contribute_exactly_nothing():
    """No exact value lies beyond the clamp (ssim_cases docstring), so the pixels "beyond the clamp by more than the margin"
    are none; what reaches the clamp is the fp32 value, by rounding.  Pinned here: a pixel whose forward value the device
    itself clamped (exactly 0 or exactly 1 in its own mode-0 map) passes nothing back, because pass A repeats the forward
    arithmetic.  `signed` has both populations.  `identical`: f == 0 everywhere and sign(x - y) == 0, zeros in every mode."""
    x, y = _dev("signed", sc.STAT)
    assert not sc.beyond_clamp(*sc.make("signed", sc.STAT)).any()
    out = _fwd(x, y, 0)
    lo, hi = out == 0, out == 1
    print(f"signed: device value == 0 on {lo.float().mean().item():.3f}, == 1 on {hi.float().mean().item():.3f} of the pixels")
    assert lo.float().mean().item() >= 0.02 and hi.float().mean().item() >= 0.10
    cot = sc.cotangent(sc.STAT, 0).cuda() + 3.0
    for sel in (lo, hi, lo | hi):
        gx, gy = _bwd(x, y, cot * sel, 0)
        assert (gx == 0).all() and (gy == 0).all()
    gx, gy = _bwd(x, y, cot * ~(lo | hi), 0)                              # the gate is not simply shut
    assert torch.isfinite(gx).all() and gx.abs().max().item() > 0 and gy.abs().max().item() > 0
    x, y = _dev("identical", sc.STAT)
    for mode, ns in LAUNCHES:
        gx, gy = _bwd(x, y, sc.cotangent(sc.STAT, mode).cuda() + 3.0, mode, ns)
        assert (gx == 0).all() and (gy == 0).all()


def test_flat_planes_give_finite_gradients():
    """fp32 noise is ten times the true value here and decides the gate pixel by pixel: no oracle comparison of the gradient
    (the forward value is under the rule in test_forward_map_and_mix), but it has to be finite and repeatable."""
    x, y = _dev("flat", sc.STAT)
    for mode, ns in LAUNCHES:
        cot = sc.cotangent(sc.STAT, mode).cuda()
        gx, gy = _bwd(x, y, cot, mode, ns)
        hx, hy = _bwd(x, y, cot, mode, ns)
        assert torch.isfinite(gx).all() and torch.isfinite(gy).all() and torch.equal(gx, hx) and torch.equal(gy, hy)


def test_two_runs_give_identical_bytes_at_the_stride_shape():
    x, y = _dev("noise", sc.STRIDE)
    for mode, ns in LAUNCHES:
        cot = sc.cotangent(sc.STRIDE, mode).cuda()
        a, b = _fwd(x, y, mode, ns), _fwd(x, y, mode, ns)
        assert torch.equal(a, b)
        (gx, gy), (hx, hy) = _bwd(x, y, cot, mode, ns), _bwd(x, y, cot, mode, ns)
        assert torch.equal(gx, hx) and torch.equal(gy, hy)


# ------------------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("where", [(3, 4), (0, 0)])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_pixel_gives_nan_on_its_windows_like_the_reference(bad, where):
    """torch.clamp propagates NaN; fminf(fmaxf(v, 0), 1) alone would turn it into SSIM loss 0 on the windows that hold the
    pixel.  Backward: non-finite gradients stay inside the 5 x 5 neighbourhood, everything outside is the clean run's bits."""
    geom = (1, 1, 8, 8)
    xc, yc = sc.make("noise", geom)
    xb = xc.clone()
    xb[0, 0, where[0], where[1]] = bad
    x, y, xclean = xb.cuda(), yc.cuda(), xc.cuda()
    rows, cols = torch.meshgrid(torch.arange(8), torch.arange(8), indexing="ij")
    dist = torch.maximum((rows - where[0]).abs(), (cols - where[1]).abs())[None, None]
    for mode, ns in LAUNCHES:
        want = sc.ref_out(xb, yc, F64, mode, ns)
        got = _fwd(x, y, mode, ns).cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (mode, ns, torch.isnan(got).sum().item(), torch.isnan(want).sum().item())
        assert torch.equal(torch.isinf(got), torch.isinf(want))
        if not ns:
            assert torch.equal(torch.isnan(want), dist <= 1)              # the windows that contain the pixel
        fin = torch.isfinite(want)
        clean32, clean64 = sc.ref_out(xc, yc, F32, mode, ns), sc.ref_out(xc, yc, F64, mode, ns)
        assert torch.equal(want[fin], clean64[fin])
        err, tol = sc.assert_elem(got[fin], clean32[fin], clean64[fin], f"finite part, mode {mode}")
        sc.fig(f"fwd non-finite {bad} at {where} mode {mode}" + (" no_ssim" if ns else ""), err, tol)
        cot = sc.cotangent(geom, mode).cuda()
        gx, gy = _bwd(x, y, cot, mode, ns)
        cx, cy = _bwd(xclean, y, cot, mode, ns)
        far = (dist > 2).cuda()
        assert torch.isfinite(gx[far]).all() and torch.isfinite(gy[far]).all()
        assert torch.equal(gx[far], cx[far]) and torch.equal(gy[far], cy[far])
