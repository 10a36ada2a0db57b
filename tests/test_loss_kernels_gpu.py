"""Every K5 loss kernel (csrc/loss.hip) on its own against the fp64 oracle (oracle/losses.py), elementwise.

Inputs, references and the comparison rule live in tests/loss_cases.py; tests/test_loss_cases.py proves on the CPU that
the inputs hold the edge populations (ties, holes, exact mask bounds, a wholly masked image) and that every reference is
well-conditioned.  The rule, computed inside each test from the oracle alone:

  elementwise   |dev - ref64| <= 4 * max|ref32 - ref64| + 1e-6 * max|ref64|        (every element, none excluded)
  scalar sums   |dev - ref64| <= 4 * |ref32 - ref64| + 1e-6 * |ref64|
  counts        exact
  bookkeeping   fp64 sums to rows * 2^-52, fp32 results to one rounding (2^-23 relative, 2^-22 of the term magnitudes for
                the three-operation weights): the precision of the number formats

Measured on an MI355X; the worst comparison of each group, n = comparisons in the group (forms, caches, slots, images).
The degenerate (3, 1, 40) rows show the reference's own noise, not a precision.

  output and case                                        n    max err  tolerance
  gt normals (2, 21, 70)                                 1   3.20e-06   1.52e-05
  gt normals (1, 8, 130)                                 1   2.61e-06   1.15e-05
  gt normals (3, 1, 40)                                  1   1.00e+00   4.00e+00
  gt normals (2, 40, 1)                                  1   0.00e+00   0.00e+00
  gt normals (1, 2, 2)                                   1   1.07e-06   3.85e-06
  gt normals (1, 32808, 17)                              1   1.39e-06   6.55e-06
  sum L1 (2, 21, 70)                                     4   5.44e-06   5.93e-04
  sum 2-cos (2, 21, 70)                                  2   1.28e-04   4.94e-03
  sum L1 (1, 8, 130)                                     4   6.27e-06   2.56e-04
  sum 2-cos (1, 8, 130)                                  2   2.57e-05   1.72e-03
  sum L1 (3, 1, 40)                                      4   5.81e-07   2.24e-05
  sum 2-cos (3, 1, 40)                                   2   5.35e+00   2.14e+01
  sum L1 (2, 40, 1)                                      4   2.09e-07   1.10e-05
  sum 2-cos (2, 40, 1)                                   2   0.00e+00   1.32e-04
  sum L1 (1, 2, 2)                                       4   2.24e-08   1.97e-06
  sum 2-cos (1, 2, 2)                                    2   5.12e-09   7.53e-06
  sum L1 (1, 32808, 17)                                  4   1.34e-04   3.45e-02
  sum 2-cos (1, 32808, 17)                               2   2.57e-02   6.98e-01
  masked normals loss (2, 21, 70)                        1   1.07e-07   1.90e-06
  masked normals loss (1, 8, 130)                        1   5.81e-08   2.07e-06
  masked normals loss (3, 1, 40)                         1   1.05e-01   4.22e-01
  masked normals loss (2, 40, 1)                         1   0.00e+00   2.00e-06
  masked normals loss (1, 2, 2)                          1   4.34e-08   1.75e-06
  masked normals loss (1, 32808, 17)                     1   3.06e-08   1.20e-06
  sup grad (2, 21, 70) L1 only                           2   2.44e-12   2.92e-10
  sup grad (2, 21, 70) L1 only to_disp                   2   6.68e-10   8.17e-09
  sup grad (2, 21, 70)                                   4   2.39e-08   1.19e-07
  sup grad (2, 21, 70) to_disp                           4   1.77e-07   8.94e-07
  sup grad (1, 8, 130) L1 only                           2   9.08e-12   8.39e-10
  sup grad (1, 8, 130) L1 only to_disp                   2   1.56e-09   2.46e-08
  sup grad (1, 8, 130)                                   4   9.20e-08   4.21e-07
  sup grad (1, 8, 130) to_disp                           4   8.20e-07   4.25e-06
  sup grad (3, 1, 40) L1 only                            2   2.07e-10   7.90e-09
  sup grad (3, 1, 40) L1 only to_disp                    2   1.91e-08   2.32e-07
  sup grad (3, 1, 40)                                    4   5.12e-01   1.98e+00
  sup grad (3, 1, 40) to_disp                            4   7.58e+00   2.93e+01
  sup grad (2, 40, 1) L1 only                            2   3.10e-10   1.18e-08
  sup grad (2, 40, 1) L1 only to_disp                    2   2.09e-08   2.32e-07
  sup grad (2, 40, 1)                                    4   3.10e-10   1.18e-08
  sup grad (2, 40, 1) to_disp                            4   2.09e-08   2.32e-07
  sup grad (1, 2, 2) L1 only                             2   4.97e-09   2.53e-07
  sup grad (1, 2, 2) L1 only to_disp                     2   7.28e-08   4.49e-06
  sup grad (1, 2, 2)                                     4   3.18e-07   1.28e-06
  sup grad (1, 2, 2) to_disp                             4   4.96e-06   1.70e-05
  sup grad (1, 32808, 17) L1 only                        2   5.26e-15   1.31e-12
  sup grad (1, 32808, 17) (late tiles) L1 only           2   5.26e-15   1.31e-12
  sup grad (1, 32808, 17) L1 only to_disp                2   4.81e-12   5.46e-11
  sup grad (1, 32808, 17) (late tiles) L1 only to_disp   2   4.00e-12   5.13e-11
  sup grad (1, 32808, 17)                                4   3.11e-12   1.37e-11
  sup grad (1, 32808, 17) (late tiles)                   4   8.66e-14   1.63e-12
  sup grad (1, 32808, 17) to_disp                        4   8.54e-11   3.78e-10
  sup grad (1, 32808, 17) (late tiles) to_disp           4   4.79e-12   5.44e-11
  sup grad (2, 9, 65) L1 only                            2   2.07e-11   8.75e-10
  sup grad (2, 9, 65) L1 only to_disp                    2   1.49e-09   2.41e-08
  sup grad (2, 9, 65)                                    4   3.67e-08   1.82e-07
  sup grad (2, 9, 65) to_disp                            4   5.42e-07   2.62e-06
  sup grad (1, 17, 129) L1 only                          2   5.02e-12   3.97e-10
  sup grad (1, 17, 129) L1 only to_disp                  2   8.43e-10   1.19e-08
  sup grad (1, 17, 129)                                  4   1.15e-07   4.94e-07
  sup grad (1, 17, 129) to_disp                          4   1.33e-06   5.66e-06
  updisp (2, 6, 10, 6, 10)                               1   0.00e+00   9.72e-07
  depth (2, 6, 10, 6, 10)                                1   9.90e-08   2.33e-06
  updisp (2, 6, 10, 12, 20)                              1   8.57e-08   1.32e-06
  depth (2, 6, 10, 12, 20)                               1   4.40e-08   8.35e-07
  updisp (2, 6, 10, 24, 40)                              1   1.04e-07   1.28e-06
  depth (2, 6, 10, 24, 40)                               1   5.77e-08   1.16e-06
  updisp (2, 6, 10, 48, 80)                              1   1.10e-07   1.36e-06
  depth (2, 6, 10, 48, 80)                               1   1.23e-07   2.18e-06
  updisp (1, 5, 7, 13, 10)                               1   2.13e-07   1.76e-06
  depth (1, 5, 7, 13, 10)                                1   1.81e-06   8.50e-06
  updisp (1, 91, 100, 728, 800)                          1   1.18e-07   1.41e-06
  depth (1, 91, 100, 728, 800)                           1   1.36e-07   2.26e-06
  up gather (3, 7, 13, 1, 1)                             4   2.38e-07   5.63e-06
  up gather (3, 7, 13, 2, 2)                             4   5.18e-07   4.61e-06
  up gather (3, 7, 13, 4, 4)                             4   1.54e-06   1.39e-05
  up gather (3, 7, 13, 8, 8)                             4   8.38e-06   5.68e-05
  up gather (2, 1, 9, 4, 4)                              4   7.97e-07   1.09e-05
  up gather (2, 6, 10, 3, 5)                             4   3.12e-06   1.69e-05
  up gather (2, 6, 10, 2, 4)                             4   6.07e-07   1.04e-05
  up gather (1, 725, 724, 1, 1)                          4   2.38e-07   7.70e-06
  up gather (1, 725, 724, 2, 2)                          4   1.18e-06   1.01e-05
  smooth sum x (5, 3, 7)                                 4   1.42e-06   1.25e-05
  smooth sum y (5, 3, 7)                                 4   2.05e-07   5.89e-06
  smooth grad (5, 3, 7)                                  8   3.65e-09   5.04e-08
  edge weights (5, 3, 7)                                 2   4.31e-08   1.09e-06
  image mean (5, 3, 7)                                   2   1.99e-08   7.79e-07
  smooth sum x (3, 9, 29)                                4   1.94e-06   4.08e-05
  smooth sum y (3, 9, 29)                                4   4.45e-07   6.18e-05
  smooth grad (3, 9, 29)                                 8   5.03e-10   5.21e-09
  edge weights (3, 9, 29)                                2   5.36e-08   1.20e-06
  image mean (3, 9, 29)                                  2   1.87e-08   6.24e-07
  smooth sum x (2, 2, 2)                                 4   6.04e-08   6.55e-07
  smooth sum y (2, 2, 2)                                 4   1.49e-07   1.16e-06
  smooth grad (2, 2, 2)                                  8   1.02e-08   1.93e-07
  edge weights (2, 2, 2)                                 2   3.36e-08   1.02e-06
  image mean (2, 2, 2)                                   2   0.00e+00   6.90e-07
  smooth sum x (2, 16, 24)                               4   2.18e-06   6.85e-05
  smooth sum y (2, 16, 24)                               4   3.94e-06   5.35e-05
  smooth grad (2, 16, 24)                                8   6.41e-10   5.82e-09
  edge weights (2, 16, 24)                               2   6.29e-08   1.23e-06
  image mean (2, 16, 24)                                 2   1.99e-08   6.27e-07
  smooth sum x (2, 5, 7)                                 4   2.21e-07   5.07e-06
  smooth sum y (2, 5, 7)                                 4   6.01e-07   5.83e-06
  smooth grad (2, 5, 7)                                  8   4.48e-09   4.07e-08
  edge weights (2, 5, 7)                                 2   5.23e-08   1.13e-06
  image mean (2, 5, 7)                                   2   2.21e-08   7.86e-07
  smooth sum x (1, 1040, 520)                            4   2.65e-03   4.60e-02
  smooth sum y (1, 1040, 520)                            4   2.76e-03   4.20e-02
  smooth grad (1, 1040, 520)                             8   1.18e-12   9.24e-12
  edge weights (1, 1040, 520)                            2   7.79e-08   1.27e-06
  image mean (1, 1040, 520)                              2   1.36e-08   7.34e-07
  loss values (2, 64, 96)                               40   1.58e-08   3.30e-07
  depth (2, 64, 96)                                     12   1.65e-07   2.03e-06
  disparity gradient (2, 64, 96)                        12   8.99e-07   3.57e-06
  loss values (1, 32808, 24)                             7   3.64e-08   1.87e-06
  depth (1, 32808, 24)                                   2   1.93e-07   2.42e-06
  disparity gradient (1, 32808, 24)                      2   3.19e-11   2.39e-10
  disparity gradient (1, 32808, 24) (late tiles)         2   5.91e-11   6.01e-10
  loss values (2, 32, 48) S=8                           25   4.52e-08   9.04e-07
  depth (2, 32, 48)                                      8   1.53e-07   2.03e-06
  disparity gradient (2, 32, 48)                         8   8.99e-07   3.23e-06
  normals_pred loss (3, 6, 10, 3, 4)                     1   1.49e-08   1.98e-06
  normals_pred grad (3, 6, 10, 3, 4)                     1   3.81e-09   4.20e-08
  normals_pred loss (3, 6, 10, 5, 3)                     1   1.49e-08   1.98e-06
  normals_pred grad (3, 6, 10, 5, 3)                     1   3.81e-09   4.20e-08
  normals_pred loss (1, 32808, 16, 3, 5)                 1   4.92e-08   2.28e-06
  normals_pred grad (1, 32808, 16, 3, 5)                 1   4.97e-12   2.57e-11
  metrics bounds                                        21   4.03e-08   7.06e-07
  metrics one_pixel_by_mask                             14   6.98e-08   1.15e-06
  metrics p1                                            14   1.34e-07   2.34e-06
  metrics stride_loop                                   14   3.77e-08   6.63e-07
"""
import functools

import pytest
import torch

import loss_cases as lc
from polardepth import functional as PF
from polardepth import ops
from polardepth._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NAN = float("nan")


def _buf(*shape, fill=NAN, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def _sync():
    torch.cuda.synchronize()


def _rec(what, err_tol):
    print(f"K5FIG | {what} | err {err_tol[0]:.2e} | tol {err_tol[1]:.2e}")


def _elem(dev, r32, r64, what):
    _rec(what, lc.assert_elem(dev, r32, r64, what))


def _scalar(dev, r32, r64, what):
    _rec(what, lc.assert_scalar(dev, r32, r64, what))


# ------------------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def _sup(geom):
    c = lc.sup_case(*geom)
    c["d"] = {k: c[k].cuda() for k in ("gt", "pred", "K")}
    return c


@functools.lru_cache(maxsize=None)
def _sup_ref(geom, what, *args):
    c = _sup(geom)
    fn = {"gtn": lc.ref_gt_normals, "sums": lc.ref_sup_sums, "grad": lc.ref_sup_grad}[what]
    return fn(c, F32, *args), fn(c, F64, *args)


def _device_gtn(geom):
    c = _sup(geom)
    N, H, W = geom
    gtn = _buf(N, H, W, 4)
    check(lib.pd_gt_normals(ptr(c["d"]["gt"]), ptr(c["d"]["K"]), ptr(gtn), N, H, W, lc.MIN_D, lc.MAX_D, stream_ptr()), "pd_gt_normals")
    return gtn


def _device_sup_sums(geom, gtn, with_normals):
    c = _sup(geom)
    N, H, W = geom
    rows = lib.pd_loss_rows(N * H * W)
    part = _buf(rows, 3)
    check(lib.pd_sup_loss_fwd(ptr(c["d"]["pred"]), ptr(c["d"]["gt"]), ptr(c["d"]["K"]), ptr(gtn), ptr(part), N, H, W, lc.MIN_D,
                              lc.MAX_D, with_normals, stream_ptr()), "pd_sup_loss_fwd")
    _sync()
    return part.double().sum(0)


# ------------------------------------------------------------------------------------------------ supervised terms
@pytest.mark.parametrize("geom", lc.SUP_GEOMS)
def test_gt_normals(geom):
    """pd_gt_normals vs ol.depth_to_normals on the masked pixels, zero elsewhere and in the fourth lane.  (3, 1, 40): the
    reference's normals are rounding noise blown up to unit length (see test_loss_cases); compared all the same."""
    gtn = _device_gtn(geom)
    _sync()
    r32, r64 = _sup_ref(geom, "gtn")
    _elem(gtn[..., :3], r32, r64, f"gt normals {geom}")
    assert (gtn[..., 3] == 0).all()
    assert (gtn[..., :3][~_sup(geom)["valid"][:, 0].cuda()] == 0).all()


@pytest.mark.parametrize("with_normals", [0, 1])
@pytest.mark.parametrize("cached", [0, 1])
@pytest.mark.parametrize("geom", lc.SUP_GEOMS)
def test_sup_loss_fwd(geom, cached, with_normals):
    """The three sums after the fp64 row reduction: sum |gt - d| m, sum (2 - cos) m, and the mask count (exact, with gt at
    exactly float32(0.1) and float32(2.0) inside)."""
    got = _device_sup_sums(geom, _device_gtn(geom) if cached else None, with_normals)
    r32, r64 = _sup_ref(geom, "sums", bool(with_normals))
    _scalar(got[0], r32[0], r64[0], f"sum L1 {geom}")
    if with_normals:
        _scalar(got[1], r32[1], r64[1], f"sum 2-cos {geom} cached={cached}")
    else:
        assert got[1].item() == 0.0
    assert got[2].item() == r64[2].item() == _sup(geom)["valid"].sum().item()


@pytest.mark.parametrize("geom", lc.SUP_GEOMS)
def test_normals_loss_masked(geom):
    c = _sup(geom)
    N, H, W = geom
    m = lc.arbitrary_mask(c)
    dm = m.cuda()
    part, out = _buf(lib.pd_loss_rows(N * H * W), 2), _buf(1)
    check(lib.pd_normals_loss_masked(ptr(c["d"]["pred"]), ptr(c["d"]["gt"]), ptr(c["d"]["K"]), ptr(dm), ptr(part), ptr(out),
                                     N, H, W, stream_ptr()), "pd_normals_loss_masked")
    _sync()
    _scalar(out[0], lc.ref_normals_loss_masked(c, m, F32), lc.ref_normals_loss_masked(c, m, F64), f"masked normals loss {geom}")
    assert part.double().sum(0)[1].item() == m.double().sum().item()


@pytest.mark.parametrize("to_disp", [0, 1])
@pytest.mark.parametrize("with_normals", [0, 1])
@pytest.mark.parametrize("geom", lc.SUP_BWD_GEOMS)
def test_sup_loss_bwd(geom, with_normals, to_disp):
    """pd_sup_loss_bwd, fused and two-pass form, cached and recomputed gt normals, against fp64 autograd of w0 L1 + w1 LN on
    every pixel; non-uniform weights, sums[2] from the forward kernel.  Rows of tiles the fused kernel reaches only on its
    second trip are asserted on their own.  L1 only: exactly 0 on the tie pixels."""
    c = _sup(geom)
    N, H, W = geom
    d = c["d"]
    sums = torch.zeros(5, dtype=F64, device="cuda")
    sums[:3] = _device_sup_sums(geom, None, with_normals)
    wts = torch.tensor(lc.SUP_WTS, dtype=F32, device="cuda")
    r32, r64 = _sup_ref(geom, "grad", bool(with_normals), bool(to_disp))
    late = lc.late_tile_rows(N, H, W)
    ab = _buf(N, H, W, 6)
    for two_pass in (0, 1):
        for cached in ((0, 1) if with_normals else (0,)):
            gout = _buf(N, 1, H, W)
            gtn = _device_gtn(geom) if cached else None
            check(lib.pd_sup_loss_bwd(ptr(d["pred"]), ptr(d["gt"]), ptr(d["K"]), ptr(gtn), ptr(wts),
                                      ptr(sums), ptr(ab), ptr(gout), N, H, W, lc.MIN_D, lc.MAX_D, with_normals, to_disp, two_pass,
                                      stream_ptr()), "pd_sup_loss_bwd")
            _sync()
            tag = f"sup grad {geom} normals={with_normals} to_disp={to_disp} two_pass={two_pass} cached={cached}"
            _elem(gout, r32, r64, tag)
            if late is not None:
                _elem(gout[:, :, late:], r32[:, :, late:], r64[:, :, late:], tag + " late tiles")
            if not with_normals:
                g = gout.cpu()
                assert (g[c["tie"]] == 0).all() and (g[c["valid"] & ~c["tie"]] != 0).all() and (g[~c["valid"]] == 0).all()


# ------------------------------------------------------------------------------------------------ up / down sampling
@pytest.mark.parametrize("case", lc.D2D_CASES)
def test_disp_to_depth(case):
    N, hs, ws, H, W = case
    disp = lc.d2d_case(*case)
    dd = disp.cuda()
    depth, up, depth2 = _buf(N, 1, H, W), _buf(N, 1, H, W), _buf(N, 1, H, W)
    check(lib.pd_disp_to_depth(ptr(dd), ptr(depth), ptr(up), N, hs, ws, H, W, lc.MIN_D, lc.MAX_D, stream_ptr()), "pd_disp_to_depth")
    check(lib.pd_disp_to_depth(ptr(dd), ptr(depth2), None, N, hs, ws, H, W, lc.MIN_D, lc.MAX_D, stream_ptr()), "pd_disp_to_depth")
    _sync()
    (u32, d32), (u64, d64) = lc.ref_d2d(disp, H, W, F32), lc.ref_d2d(disp, H, W, F64)
    _elem(up, u32, u64, f"updisp {case}")
    _elem(depth, d32, d64, f"depth {case}")
    assert torch.equal(depth, depth2)


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("case", lc.GATHER_CASES)
def test_up_gather_bwd(case, generic):
    N, hs, ws, fh, fw = case
    gup, prior = lc.gather_case(*case)
    dgup = gup.cuda()
    r32, r64 = lc.ref_gather(gup, hs, ws, F32), lc.ref_gather(gup, hs, ws, F64)
    for accumulate in (0, 1):
        gd = prior.clone().cuda() if accumulate else _buf(N, 1, hs, ws)
        check(lib.pd_up_gather_bwd(ptr(dgup), ptr(gd), N, hs, ws, hs * fh, ws * fw, accumulate, generic, stream_ptr()), "pd_up_gather_bwd")
        _sync()
        if accumulate:
            _elem(gd, prior + r32, prior.double() + r64, f"up gather {case} generic={generic} accumulate")
        else:
            _elem(gd, r32, r64, f"up gather {case} generic={generic}")


# ------------------------------------------------------------------------------------------------ smoothness
@pytest.mark.parametrize("use_edge", [0, 1])
@pytest.mark.parametrize("use_mean", [0, 1])
@pytest.mark.parametrize("geom", lc.SMOOTH_GEOMS)
def test_smooth_fwd_and_bwd(geom, use_mean, use_edge):
    """pd_smooth_fwd: both sums, the per-image mean, the edge-weight map (zeros on the last column / row); pd_smooth_bwd:
    the disparity gradient on every pixel, written and accumulated.  (2, 16, 24) runs on a view one float off a 16-byte
    boundary."""
    N, h, w = geom
    disp, img = lc.smooth_case(*geom)
    if geom == (2, 16, 24):
        base = _buf(disp.numel() + 4)
        dd = base[1:1 + disp.numel()].view(N, 1, h, w)
        dd.copy_(disp)
        assert dd.data_ptr() % 16 == 4
    else:
        dd = disp.cuda()
    di = img.cuda()
    rows = lib.pd_loss_rows(N * h * w)
    mean = _buf(N) if use_mean else None
    edge = _buf(N, h, w, 2) if use_edge else None
    part = _buf(rows, 2)
    check(lib.pd_smooth_fwd(ptr(dd), ptr(di), ptr(mean), ptr(part), ptr(edge), N, h, w, stream_ptr()), "pd_smooth_fwd")
    _sync()
    r32, r64 = lc.ref_smooth(disp, img, F32, bool(use_mean)), lc.ref_smooth(disp, img, F64, bool(use_mean))
    got = part.double().sum(0)
    tag = f"{geom} mean={use_mean} edge={use_edge}"
    _scalar(got[0], r32[0], r64[0], f"smooth sum x {tag}")
    _scalar(got[1], r32[1], r64[1], f"smooth sum y {tag}")
    if use_mean:
        _elem(mean, lc.ref_image_mean(disp, F32), lc.ref_image_mean(disp, F64), f"image mean {tag}")
    if use_edge:
        _elem(edge, lc.ref_edge_weights(img, F32), lc.ref_edge_weights(img, F64), f"edge weights {tag}")
        assert (edge[:, :, -1, 0] == 0).all() and (edge[:, -1, :, 1] == 0).all()
    wts = torch.tensor([0.0, 0.0, lc.SMOOTH_W], dtype=F32, device="cuda")
    g = torch.Generator().manual_seed(h * w)
    prior = 1e-3 * torch.randn(N, 1, h, w, generator=g)
    for accumulate in (0, 1):
        gd = prior.clone().cuda() if accumulate else _buf(N, 1, h, w)
        gws, gacc = _buf(N, h, w), _buf(N, dtype=F64)
        check(lib.pd_smooth_bwd(ptr(dd), ptr(di), ptr(mean), ptr(wts), ptr(edge), ptr(gws), ptr(gacc), ptr(gd), N, h, w, accumulate,
                                stream_ptr()), "pd_smooth_bwd")
        _sync()
        if accumulate:
            _elem(gd, prior + r32[3], prior.double() + r64[3], f"smooth grad {tag} accumulate")
        else:
            _elem(gd, r32[3], r64[3], f"smooth grad {tag}")
            if not use_mean and h > 4 and w > 4:          # inside a constant patch: sign(0) = 0 on all four sides
                assert (gd[:, 0, h // 2 + 1, w // 2 + 1] == 0).all()


# ------------------------------------------------------------------------------------------------ the whole loss
MS_CASES = [((2, 64, 96), (1, 2, 4, 8), True), ((2, 64, 96), (1, 2, 4, 8), False), ((1, 32808, 24), (1, 2), True),
            ((2, 32, 48), (1, 1, 2, 2, 4, 4, 8, 8), True), ((2, 64, 96), (1, 4), True), ((2, 64, 96), (2, 8), False)]


@pytest.mark.parametrize("geom,zooms,multi", MS_CASES)
def test_multiscale_loss(geom, zooms, multi, monkeypatch):
    """pd_multiscale_loss_fwd / _bwd (and, multi = False, the per-scale launches) through PF.multiscale_loss against
    ol.compute_losses slot by slot: every value, every depth map, every disparity gradient; eight slots with a disparity
    each; scale ids [0, 2] and [1, 3]; the geometry whose supervised backward needs a second trip over the tiles."""
    monkeypatch.setattr(PF, "USE_MULTISCALE_LAUNCH", multi)
    monkeypatch.setattr(PF, "USE_GT_NORMAL_CACHE", True)
    monkeypatch.setattr(PF, "USE_EDGE_WEIGHT_CACHE", True)
    monkeypatch.setattr(PF, "SUP_BWD_TWO_PASS", False)
    N, H, W = geom
    c = lc.ms_case(N, H, W, zooms)
    S = len(zooms)
    cfg = PF.LossCfg(c["scale_ids"], lc.MIN_D, lc.MAX_D, 0.35, 1e-3, H, W)
    disps = [d.cuda().requires_grad_(True) for d in c["disps"]]
    vals, depths = PF.multiscale_loss(cfg, c["gt"].cuda(), c["K"].cuda(), disps, [x.cuda() for x in c["colors"]])
    assert vals.shape == (1 + 3 * S,) and len(depths) == S
    (lc.MS_GVALS_HEAD * vals[0] + vals[1:].sum()).backward()
    _sync()
    v32, d32, g32 = lc.ref_multiscale(c, F32)
    v64, d64, g64 = lc.ref_multiscale(c, F64)
    tag = f"{geom} zooms={zooms} multi={multi}"
    for i in range(1 + 3 * S):
        _scalar(vals[i], v32[i], v64[i], f"vals[{i}] {tag}")
    late = lc.late_tile_rows(N, H, W)
    for i, f in enumerate(zooms):
        _elem(depths[i], d32[i], d64[i], f"depth slot {i} {tag}")
        _elem(disps[i].grad, g32[i], g64[i], f"disparity gradient slot {i} {tag}")
        if late is not None:
            r = late // f + 1
            _elem(disps[i].grad[:, :, r:], g32[i][:, :, r:], g64[i][:, :, r:], f"disparity gradient slot {i} {tag} late tiles")


# ------------------------------------------------------------------------------------------------ scalar bookkeeping
FIN_CASES = [(S, 257, 300, [s % 4 for s in range(S)]) for S in range(1, 9)] + \
            [(2, rows, max(rows, 2) + 3, [0, 1]) for rows in (1, 255, 256, 2048)] + \
            [(2, 257, 257, [0, 2]), (2, 257, 2048, [1, 3])]


@pytest.mark.parametrize("S,rows,stride,scale_ids", FIN_CASES)
def test_loss_finalize_from_sums_and_weights(S, rows, stride, scale_ids):
    """pd_loss_finalize on synthetic partial rows (NaN beyond the row count) vs fp64 arithmetic; pd_loss_from_sums on the
    sums it wrote reproduces its values bit for bit; pd_loss_weights vs its formula at fp32 rounding."""
    from polardepth.functional import _iarr
    wn, wsm = 0.35, 1e-3
    sup, sup_rows, sm, sm_rows, dims = lc.finalize_case(S, rows, stride, scale_ids)
    dsup, dsm = sup.cuda(), sm.cuda()
    sums, vals, vals2 = _buf(S * 5, dtype=F64), _buf(1 + 3 * S), _buf(1 + 3 * S)
    check(lib.pd_loss_finalize(ptr(dsup), _iarr(sup_rows), ptr(dsm), _iarr(sm_rows), _iarr(dims), _iarr(scale_ids), S, stride,
                               wn, wsm, ptr(sums), ptr(vals), stream_ptr()), "pd_loss_finalize")
    check(lib.pd_loss_from_sums(ptr(sums), _iarr(dims), _iarr(scale_ids), S, wn, wsm, ptr(vals2), stream_ptr()), "pd_loss_from_sums")
    g = torch.Generator().manual_seed(S + rows)
    gvals = torch.randn(1 + 3 * S, generator=g)
    wts, dg = _buf(3 * S), gvals.cuda()
    check(lib.pd_loss_weights(ptr(dg), _iarr(scale_ids), S, wn, wsm, ptr(wts), stream_ptr()), "pd_loss_weights")
    _sync()
    rs, rv = lc.ref_finalize(sup, sup_rows, sm, sm_rows, dims, scale_ids, wn, wsm)
    assert torch.isfinite(sums).all() and torch.isfinite(vals).all()
    assert ((sums.cpu() - rs).abs() <= max(rows, 2) * 2.0 ** -52 * rs.abs()).all()
    assert torch.equal(sums.cpu().view(S, 5)[:, 2], rs.view(S, 5)[:, 2])            # counts: integers, exact
    assert ((vals.cpu().double() - rv).abs() <= 2.0 ** -23 * rv.abs()).all(), (vals.cpu().double() - rv).abs().max()
    assert torch.equal(vals, vals2)
    rw, mag = lc.ref_loss_weights(gvals, scale_ids, wn, wsm)
    assert torch.isfinite(wts).all()
    assert ((wts.cpu().double() - rw).abs() <= 2.0 ** -22 * mag).all(), ((wts.cpu().double() - rw).abs() / mag).max()


# ------------------------------------------------------------------------------------------------ predicted normals
@pytest.mark.parametrize("case", lc.NPRED_CASES)
def test_normals_pred_loss_fwd_and_bwd(case):
    """Pixel strides 3 and 5 with another stride for the gradient; the lanes beyond the three channels hold NaN on the way in
    and keep their contents on the way out; one image wholly masked, gt at exactly both bounds."""
    N, H, W, ld, ldd = case
    c = lc.npred_case(N, H, W)
    gt, K = c["gt"].cuda(), c["K"].cuda()
    pred = _buf(N, H, W, ld)
    pred[..., :3] = c["normals"].permute(0, 2, 3, 1).cuda()
    gtn = _buf(N, H, W, 4)
    check(lib.pd_gt_normals(ptr(gt), ptr(K), ptr(gtn), N, H, W, lc.MIN_D, lc.MAX_D, stream_ptr()), "pd_gt_normals")
    part, out = _buf(lib.pd_loss_rows(N * H * W), 2), _buf(2)
    check(lib.pd_normals_pred_loss_fwd(ptr(pred), ld, ptr(gtn), ptr(gt), ptr(part), ptr(out), N, H, W, lc.MIN_D, lc.MAX_D, stream_ptr()),
          "pd_normals_pred_loss_fwd")
    gout = torch.tensor([lc.NPRED_GOUT], dtype=F32, device="cuda")
    dpred = _buf(N, H, W, ldd, fill=7.0)
    check(lib.pd_normals_pred_loss_bwd(ptr(pred), ld, ptr(gtn), ptr(gt), ptr(gout), ptr(out), ptr(dpred), ldd, N, H, W, lc.MIN_D,
                                       lc.MAX_D, stream_ptr()), "pd_normals_pred_loss_bwd")
    _sync()
    r32, r64 = lc.ref_npred(c, F32), lc.ref_npred(c, F64)
    _scalar(out[0], r32[0], r64[0], f"normals_pred loss {case}")
    assert out[1].item() == r64[1]
    _elem(dpred[..., :3], r32[2].permute(0, 2, 3, 1), r64[2].permute(0, 2, 3, 1), f"normals_pred grad {case}")
    assert (dpred[..., 3:] == 7.0).all()
    if N > 1:
        assert (dpred[1, ..., :3] == 0).all()


# ------------------------------------------------------------------------------------------------ depth metrics
@pytest.mark.parametrize("name", lc.METRIC_CASES)
def test_depth_metrics(name):
    gt, pred, mask, mv = lc.metrics_case(name)
    got = ops.depth_metrics(gt.cuda(), pred.cuda(), lc.MIN_D, lc.MAX_D, mask=None if mask is None else mask.cuda(), mask_value=mv).cpu()
    r32, r64 = lc.ref_metrics(gt, pred, mask, mv, F32), lc.ref_metrics(gt, pred, mask, mv, F64)
    for n in range(gt.shape[0]):
        assert got[n, 7].item() == r64[n, 7].item()
        for k, what in enumerate(("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")):
            _scalar(got[n, k], r32[n, k], r64[n, k], f"metrics {name} image {n} {what}")
