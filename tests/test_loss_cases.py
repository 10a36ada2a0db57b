"""CPU half of the K5 loss-kernel tests (tests/loss_cases.py, tests/test_loss_kernels_gpu.py): the inputs hold the edge
populations the GPU tests rely on, the fp64 restatements agree with oracle/losses.py, and every case is well-conditioned:
the fp32 oracle deviates from its own fp64 evaluation by at most 1e-5 of the output's scale at every element, so that an
elementwise comparison of the device with fp64 means something.

Measured (worst case of each reference; the cap is 1e-5):

  reference             worst |o32 - o64| / scale  at
  gt normals                             3.65e-06  (1, 17, 129)
  sum L1 / sum 2-cos / count    4.1e-08 / 1.3e-07 / 0
  supervised gradient                    3.67e-06  (1, 17, 129), normals, to_disp
  masked normals loss                    3.16e-08  (1, 8, 130)
  updisp / depth                  2.3e-07 / 1.4e-06  5 x 7 -> 13 x 10
  upsample gather                        6.56e-07  (3, 7, 13) zoom 8
  image mean / edge weights       3.6e-08 / 7.0e-08
  smoothness sums, loss, gradient        2.45e-07  (1, 1040, 520), gradient
  whole loss: values / depths / gradients  1.5e-07 / 1.4e-06 / 3.86e-06  (2, 64, 96) slot 0
  predicted normals: loss / gradient  3.5e-08 / 1.02e-06  (1, 32808, 16)
  depth metrics                          4.94e-08

Two things had to be built into the inputs to get there (tests/loss_cases.py).  Tall images (32808 rows): the depth is a
sawtooth in y and the special ground-truth values fill whole rows, because a depth that is flat in y leaves the y-gradient
of Y = (y - cy) / fy * d at the mercy of 2^-24 |y - cy| (1e-3 at the fp32 oracle).  H == 1: the normals of the reference
are rounding noise in every precision (1.9e+4 of the fp64 "scale"); only there, and only for what depends on the normals,
the cap is not asserted."""
import pytest
import torch

import loss_cases as lc


def _cond(r32, r64, what, degenerate=False):
    c = lc.conditioning(r32, r64)
    print(f"conditioning {what}: {c:.2e}")
    assert degenerate or c <= lc.COND, f"{what}: fp32 oracle is {c:.2e} of the scale away from fp64"


# ------------------------------------------------------------------------------------------------ populations
@pytest.mark.parametrize("geom", lc.SUP_BWD_GEOMS)
def test_supervised_cases_hold_the_edge_populations(geom):
    N, H, W = geom
    c = lc.sup_case(N, H, W)
    P = H * W
    need = 1 if P < 20 else min(8, P // 8)
    assert c["tie"].sum().item() >= need * N                    # pred == gt bit for bit, inside the mask
    assert torch.equal(c["pred"][c["tie"]], c["gt"][c["tie"]]) and c["valid"][c["tie"]].all()
    assert (c["pred"] != c["gt"])[c["valid"]].any()
    for n in range(N):
        assert c["at_lo"][n].any() and c["at_hi"][n].any() and c["hole"][n].any()
        assert c["valid"][n].any() and not c["valid"][n].all()
    assert c["valid"][c["at_lo"]].all() and c["valid"][c["at_hi"]].all()         # the bounds are inclusive
    assert (c["gt"][~c["valid"]] > lc.HI).any() or P < 20
    K = c["K"]
    assert (K[:, 0, 0] != K[:, 1, 1]).all() and (K[:, 0, 2] != 0.5 * W).all() and (K[:, 1, 2] != 0.5 * H).all()
    assert N == 1 or not torch.equal(K[0], K[1])
    assert (c["pred"] >= lc.LO).all()


def test_the_large_geometry_crosses_both_caps_and_the_seam_cases_sit_one_past_a_tile():
    N, H, W = lc.SUP_GEOMS[-1]
    assert N * H * W > lc.GRID_CAP
    assert lc.late_tile_rows(N, H, W) == 32768 and H - 32768 > 8
    assert lc.late_tile_rows(1, 32808, 24) == 32768 and 32808 * 24 > lc.GRID_CAP
    assert all(lc.late_tile_rows(*g) is None for g in lc.SUP_BWD_GEOMS if g != (N, H, W))
    assert (2, 9, 65) in lc.SUP_BWD_GEOMS and 9 == lc.TILE_R + 1 and 65 == lc.TILE_C + 1
    assert (1, 17, 129) in lc.SUP_BWD_GEOMS and 17 == 2 * lc.TILE_R + 1 and 129 == 2 * lc.TILE_C + 1
    assert any(n * H_ * W_ > lc.GRID_CAP for n, _, _, H_, W_ in lc.D2D_CASES)
    assert any(n * hs * ws > lc.GRID_CAP for n, hs, ws, _, _ in lc.GATHER_CASES)
    assert any(n * hs * ws > 256 and ws % 64 for n, hs, ws, _, _ in lc.GATHER_CASES)
    assert any(hs == 1 for _, hs, _, _, _ in lc.GATHER_CASES) and {(3, 5), (2, 4)} <= {c[3:] for c in lc.GATHER_CASES}
    assert any(n * h * w > lc.GRID_CAP for n, h, w in lc.SMOOTH_GEOMS)
    assert any(n * H_ * W_ > lc.GRID_CAP for n, H_, W_, _, _ in lc.NPRED_CASES)
    assert any(h * w < 128 and n >= 3 for n, h, w in lc.SMOOTH_GEOMS) and any((h * w) % 4 for _, h, w in lc.SMOOTH_GEOMS)


def test_predicted_normals_case_has_one_dead_image_and_exact_bounds():
    c = lc.npred_case(3, 6, 10)
    assert not c["valid"][1].any() and c["valid"][0].any() and c["valid"][2].any()
    assert c["at_lo"][0].any() and c["at_hi"][0].any()
    nrm = c["normals"].norm(dim=1)
    assert nrm.min() > 0.4 and nrm.max() < 1.6


@pytest.mark.parametrize("geom", lc.SMOOTH_GEOMS)
def test_smoothness_cases_hold_ties_and_distinct_neighbours_are_far_apart(geom):
    d, img = lc.smooth_case(*geom)
    tx, ty = lc.smooth_ties(d)
    assert tx >= geom[0] and (ty >= geom[0] or geom[1] * geom[2] <= 4)
    dx = (d[:, :, :, 1:] - d[:, :, :, :-1]).abs()
    dy = (d[:, :, 1:, :] - d[:, :, :-1, :]).abs()
    assert dx[dx > 0].min() >= 2.0 ** -10 and dy[dy > 0].min() >= 2.0 ** -10
    assert (dx > 0).any() and (dy > 0).any() and d.min() > 0.05


@pytest.mark.parametrize("name", lc.METRIC_CASES)
def test_metric_cases_hold_bounds_clamps_and_the_single_pixel(name):
    gt, pred, mask, mv = lc.metrics_case(name)
    ref = lc.ref_metrics(gt, pred, mask, mv, torch.float64)
    assert (ref[:, 7] >= 1).all()
    if name == "p1":
        assert gt.shape[1] == 1 and (pred[0] > lc.HI).all()
        return
    assert (gt == lc.LO).any() and (gt == lc.HI).any() and (pred < lc.LO).any() and (pred > lc.HI).any()
    if name == "one_pixel_by_mask":
        assert (ref[:, 7] == 1).all()
    if name == "stride_loop":
        assert gt.shape[1] == 64 * 256 * 2 + 3
    _cond(lc.ref_metrics(gt, pred, mask, mv, torch.float32), ref, f"metrics {name}")


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("geom", lc.SUP_BWD_GEOMS)
def test_supervised_references_are_well_conditioned(geom):
    c = lc.sup_case(*geom)
    # H == 1: the three rows of the Sobel window are one row, the y-gradient is 0 up to the rounding of (-a - 2b - c) + a + 2b
    # + c, and F.normalize blows that residue up to a unit vector in fp32 (|v| > 1e-12) but not in fp64: the reference's
    # normals are noise there, in every precision.  Everything that does not depend on the normals is still held to the cap.
    deg = geom[1] == 1
    _cond(lc.ref_gt_normals(c, torch.float32), lc.ref_gt_normals(c, torch.float64), f"gt normals {geom}", deg)
    for wn in (True, False):
        s32, s64 = lc.ref_sup_sums(c, torch.float32, wn), lc.ref_sup_sums(c, torch.float64, wn)
        for a, b, what in zip(s32, s64, ("sum L1", "sum 2-cos", "count")):
            _cond(a, b, f"{what} {geom}", deg and wn and what == "sum 2-cos")
        assert s32[2].item() == s64[2].item() == c["valid"].sum().item()
        for td in (False, True):
            g64 = lc.ref_sup_grad(c, torch.float64, wn, td)
            _cond(lc.ref_sup_grad(c, torch.float32, wn, td), g64, f"sup grad normals={wn} to_disp={td} {geom}", deg and wn)
            if not wn and not td:                 # L1 only: the tie pixels carry exactly sign(0) = 0
                assert (g64[c["tie"]] == 0).all() and (g64[c["valid"] & ~c["tie"]] != 0).all()
    m = lc.arbitrary_mask(c)
    if geom in lc.SUP_GEOMS:
        _cond(lc.ref_normals_loss_masked(c, m, torch.float32), lc.ref_normals_loss_masked(c, m, torch.float64), f"masked normals {geom}", deg)


@pytest.mark.parametrize("case", lc.D2D_CASES)
def test_upsample_references_are_well_conditioned(case):
    N, hs, ws, H, W = case
    d = lc.d2d_case(*case)
    for a, b, what in zip(lc.ref_d2d(d, H, W, torch.float32), lc.ref_d2d(d, H, W, torch.float64), ("updisp", "depth")):
        _cond(a, b, f"{what} {case}")


@pytest.mark.parametrize("case", lc.GATHER_CASES)
def test_gather_references_are_well_conditioned(case):
    gup, _ = lc.gather_case(*case)
    _cond(lc.ref_gather(gup, case[1], case[2], torch.float32), lc.ref_gather(gup, case[1], case[2], torch.float64), f"gather {case}")


@pytest.mark.parametrize("geom", lc.SMOOTH_GEOMS)
def test_smoothness_references_are_well_conditioned_and_consistent(geom):
    N, h, w = geom
    d, img = lc.smooth_case(*geom)
    _cond(lc.ref_image_mean(d, torch.float32), lc.ref_image_mean(d, torch.float64), f"mean {geom}")
    _cond(lc.ref_edge_weights(img, torch.float32), lc.ref_edge_weights(img, torch.float64), f"edge weights {geom}")
    e = lc.ref_edge_weights(img, torch.float64)
    assert (e[:, :, -1, 0] == 0).all() and (e[:, -1, :, 1] == 0).all() and (e[:, :, :-1, 0] > 0).all()
    for normalise in (True, False):
        r32, r64 = lc.ref_smooth(d, img, torch.float32, normalise), lc.ref_smooth(d, img, torch.float64, normalise)
        for a, b, what in zip(r32, r64, ("sum x", "sum y", "loss", "grad")):
            _cond(a, b, f"smooth {what} normalise={normalise} {geom}")
        sx, sy, loss, _ = r64
        # the restated sums are the numerators of the two means of ol.get_smooth_loss
        assert abs((sx / (N * h * (w - 1)) + sy / (N * (h - 1) * w) - loss).item()) <= 1e-13 * loss.item()
    # the mean of the restatement is the one compute_losses normalises with
    dd = d.double()
    assert torch.equal(lc.ref_image_mean(d, torch.float64), dd.mean(2, True).mean(3, True).reshape(-1)) or torch.allclose(
        lc.ref_image_mean(d, torch.float64), dd.mean(2, True).mean(3, True).reshape(-1), rtol=1e-14, atol=0)
    # ties: an interior pixel of a constant patch has zero gradient without the mean normalisation
    g = lc.ref_smooth(d, img, torch.float64, False)[3]
    if h > 4 and w > 4:
        assert (g[:, 0, h // 2 + 1, w // 2 + 1] == 0).all()


MS_CASES = [((2, 64, 96), (1, 2, 4, 8)), ((1, 32808, 24), (1, 2)), ((2, 32, 48), (1, 1, 2, 2, 4, 4, 8, 8))]


@pytest.mark.parametrize("geom,zooms", MS_CASES)
def test_whole_loss_references_are_well_conditioned(geom, zooms):
    c = lc.ms_case(*geom, zooms)
    v32, d32, g32 = lc.ref_multiscale(c, torch.float32)
    v64, d64, g64 = lc.ref_multiscale(c, torch.float64)
    for i in range(len(v64)):
        _cond(v32[i], v64[i], f"vals[{i}] {geom}")
    for i in range(len(zooms)):
        _cond(d32[i], d64[i], f"depth slot {i} {geom}")
        _cond(g32[i], g64[i], f"disparity gradient slot {i} {geom}")


@pytest.mark.parametrize("case", lc.NPRED_CASES)
def test_predicted_normals_references_are_well_conditioned(case):
    c = lc.npred_case(*case[:3])
    r32, r64 = lc.ref_npred(c, torch.float32), lc.ref_npred(c, torch.float64)
    _cond(r32[0], r64[0], f"normals_pred loss {case}")
    _cond(r32[2], r64[2], f"normals_pred grad {case}")
    assert r32[1] == r64[1] > 0
    if case[0] > 1:
        assert (r64[2][1] == 0).all()


# ------------------------------------------------------------------------------------------------ restatements vs the oracle
def test_finalize_restatement_reproduces_compute_losses():
    """ref_finalize fed with the oracle's own sums (one partial row per scale) gives the values of ol.compute_losses."""
    c = lc.ms_case(2, 64, 96, (1, 4))
    vals, depths, _ = lc.ref_multiscale(c, torch.float64)
    S = 2
    sup, sm, dims = torch.zeros(S, 1, 3, dtype=torch.float64), torch.zeros(S, 1, 2, dtype=torch.float64), []
    for i in range(S):
        cc = dict(c, pred=depths[i])
        sup[i, 0] = torch.stack(lc.ref_sup_sums(cc, torch.float64))
        sm[i, 0] = torch.stack(lc.ref_smooth(c["disps"][i], c["colors"][i], torch.float64, True)[:2])
        dims += [2, 64 // c["zooms"][i], 96 // c["zooms"][i]]
    sums, got = lc.ref_finalize(sup, [1, 1], sm, [1, 1], dims, c["scale_ids"], 0.35, 1e-3)
    assert torch.equal(sums.view(S, 5)[:, :3], sup[:, 0]) and torch.equal(sums.view(S, 5)[:, 3:], sm[:, 0])
    # w_normals and w_smooth are rounded to fp32 in the restatement, as in the C ABI
    assert (got - vals).abs().max().item() <= 1e-7 * vals.abs().max().item()


@pytest.mark.parametrize("scale_ids", [[0], [0, 2], [1, 3], [0, 0, 1, 1, 2, 2, 3, 3]])
def test_loss_weights_restatement_is_the_gradient_of_the_finalize_arithmetic(scale_ids):
    S = len(scale_ids)
    g = torch.Generator().manual_seed(S)
    gvals = torch.randn(1 + 3 * S, generator=g)
    wn, wsm = 0.35, 1e-3
    wn32, wsm32 = float(torch.tensor(wn, dtype=torch.float32)), float(torch.tensor(wsm, dtype=torch.float32))
    terms = torch.rand(S, 3, dtype=torch.float64, generator=g).requires_grad_(True)        # (L1, LN, smooth) per scale
    ls = terms[:, 0] + wn32 * terms[:, 1] + wsm32 * terms[:, 2] / torch.tensor([2.0 ** s for s in scale_ids], dtype=torch.float64)
    vals = torch.cat([ls.mean()[None], torch.stack([ls, terms[:, 0], terms[:, 1]], 1).reshape(-1)])
    (vals * gvals.double()).sum().backward()
    ref, mag = lc.ref_loss_weights(gvals, scale_ids, wn, wsm)
    assert (ref - terms.grad.reshape(-1)).abs().max().item() <= 1e-14 * mag.max().item()
    assert (mag >= ref.abs() - 1e-15).all()


def test_finalize_case_poisons_the_unused_rows():
    sup, sup_rows, sm, sm_rows, dims = lc.finalize_case(3, 257, 300, [0, 1, 2])
    for s in range(3):
        assert torch.isfinite(sup[s, :sup_rows[s]]).all() and torch.isnan(sup[s, sup_rows[s]:]).all()
        assert torch.isfinite(sm[s, :sm_rows[s]]).all() and torch.isnan(sm[s, sm_rows[s]:]).all()
    assert sup_rows[0] == 257 and len(dims) == 9
