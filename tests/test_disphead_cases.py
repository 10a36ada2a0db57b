"""CPU side of the disparity-head tests (tests/disphead_cases.py): the NumPy reference agrees with torch float64 autograd, every row's
data is exactly summable, and the table covers every kernel instantiation in every regime -- a second pass of each grid-stride
loop, a ragged tail, the borders, and every slice count of the reduce kernel -- as the restated launch arithmetic counts them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disphead_cases as dc


def _autograd(d, w, add_elu):
    """sigmoid(conv2d(pad(x, reflect))) in float64 through torch autograd.  add_elu: x = ELU(pre) and the gradient asked for is that
    of pre, with a second consumer of x contributing `add`."""
    x = torch.from_numpy(d["x"]).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w)).permute(2, 0, 1)[None].contiguous().requires_grad_(True)
    b = torch.tensor([d["b"]], dtype=torch.float64, requires_grad=True)
    if add_elu:
        # the pre-activation whose ELU is x: x itself where x > 0, log(x + 1) where x <= 0
        leaf = torch.where(x > 0, x, torch.log1p(x.clamp(max=0))).requires_grad_(True)
        xin = F.elu(leaf)
    else:
        leaf = xin = x.clone().requires_grad_(True)
    y = torch.sigmoid(F.conv2d(F.pad(xin, (1, 1, 1, 1), mode="reflect"), wt, b))[:, 0]
    obj = (y * torch.from_numpy(d["dy"])).sum()
    if add_elu:
        obj = obj + (xin * torch.from_numpy(d["add"]).permute(0, 3, 1, 2)).sum()
    obj.backward()
    return y.detach().numpy(), leaf.grad.permute(0, 2, 3, 1).numpy(), wt.grad[0].permute(1, 2, 0).numpy(), b.grad.item()


def _rel(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize("add_elu", [False, True], ids=["plain", "add+elu"])
@pytest.mark.parametrize("shape", dc.shapes(dc.ENTRIES, regimes=("border",)), ids=dc.sid)
def test_reference_matches_float64_autograd(shape, add_elu):
    """The reference against autograd to 1e-12 relative on the border shapes of all four widths.  The backward takes y as an argument:
    it is given the forward's own y here, which is what autograd differentiates."""
    N, C, H, W = shape
    g = np.random.default_rng(sum(shape))
    d = {"x": g.standard_normal((N, H, W, C)), "b": 0.3, "dy": g.standard_normal((N, H, W)), "add": g.standard_normal((N, H, W, C))}
    w = g.standard_normal((3, 3, C)) / (9 * C) ** 0.5
    if add_elu:
        d["x"] = np.where(d["x"] > 0, d["x"], np.expm1(d["x"]))        # an ELU output: values in (-1, inf)
    fwd = dc.ref_forward(d["x"], w, d["b"])
    y, dx, dw, db = _autograd(d, w, add_elu)
    assert _rel(fwd["y"], y) <= 1e-12
    bwd = dc.ref_backward(d["x"], w, fwd["y"], d["dy"], add=d["add"] if add_elu else None, elu=add_elu)
    assert _rel(bwd["dx"], dx) <= 1e-12 and _rel(bwd["dw"], dw) <= 1e-12 and abs(bwd["db"] - db) <= 1e-12 * abs(db)
    assert (bwd["dx_abs"] >= np.abs(bwd["dx"]) * (1 - 1e-12)).all() and (bwd["dw_abs"] >= np.abs(bwd["dw"]) * (1 - 1e-12)).all()
    # the number of terms: every output pixel reads nine padded positions, each of which folds onto one pixel
    assert bwd["dx_terms"].sum() == 9 * H * W and bwd["dx_terms"].min() >= 4


def test_fold_of_the_big_rows_is_the_reference_fold():
    """big_forward / big_dx (torch fp64, used where a tensor has 64 MiB) against ref_forward / ref_backward on small shapes."""
    for shape in ((2, 16, 2, 2), (1, 32, 3, 3), (2, 16, 4, 5), (1, 64, 9, 7)):
        d = dc.case(shape, "random")
        got = dc.big_dx(d["w"], d["y"], d["dy"], with_abs=True)
        assert _rel(got["dx"].numpy(), d["bwd"]["dx"]) <= 1e-12 and _rel(got["dx_abs"].numpy(), d["bwd"]["dx_abs"]) <= 1e-12
        assert np.array_equal(got["dx_terms"].numpy(), d["bwd"]["dx_terms"])
        f = dc.big_forward(d["x"], d["w"], d["b"])
        assert _rel(f["y"], d["fwd"]["y"]) <= 1e-12 and _rel(f["z_abs"], d["fwd"]["z_abs"]) <= 1e-12


@pytest.mark.parametrize("shape", dc.shapes(dc.ENTRIES), ids=dc.sid)
def test_rows_are_exactly_summable(shape):
    dc.check_conditions(shape)


def test_big_rows_are_exactly_summable():
    big = [r for r in dc.ROWS if r.big]
    assert len(big) == 6
    for r in big:
        dc.check_conditions_big(r)
        assert 64 * 2 ** 20 < r.N * r.H * r.W * r.C * 4 < 65 * 2 ** 20


def test_window_pixels_are_what_the_reference_reads():
    """The locality tests take their expected sets from window_pixels: it must name the pixels whose change moves y[h0, w0]."""
    for H, W in ((2, 2), (3, 3), (5, 6)):
        for h0 in range(H):
            for w0 in range(W):
                x = np.zeros((1, H, W, 1))
                w = np.ones((3, 3, 1))
                base = dc.ref_forward(x, w, 0.0)["z"][0, h0, w0]
                moved = set()
                for h in range(H):
                    for q in range(W):
                        x[0, h, q, 0] = 1.0
                        if dc.ref_forward(x, w, 0.0)["z"][0, h0, w0] != base:
                            moved.add((h, q))
                        x[0, h, q, 0] = 0.0
                assert moved == dc.window_pixels(H, W, h0, w0)


def test_rows_name_the_kernel_they_reach():
    for r in dc.ROWS:
        assert dc.launch(r.entry, r.N, r.C, r.H, r.W).kernel == r.want, r.id
    assert {r.want for r in dc.ROWS} == set(dc.WANT.values()) and len(set(dc.WANT.values())) == 16


def test_launch_arithmetic_on_known_shapes():
    """The restatement against numbers worked out by hand from csrc/disphead.hip."""
    assert [dc.ppw(C) for C in dc.WIDTHS] == [16, 8, 4, 2]
    assert dc.grid_for(5120, 16) == 80 and dc.grid_for(2 ** 21, 16) == 16384
    assert dc.launch(dc.FWD, 2, 16, 33, 21) == dc.Launch("disphead_fwd_kernel<4>", 10, 1, True, 0)
    assert dc.launch(dc.FWD, 4097, 32, 2, 2) == dc.Launch("disphead_fwd_kernel<8>", 4096, 2, True, 0)
    assert dc.launch(dc.BWD, 1025, 128, 2, 2) == dc.Launch("disphead_bwd_kernel<32>", 1024, 2, True, 1024)
    assert dc.launch(dc.BWD, 2, 64, 8, 64) == dc.Launch("disphead_bwd_kernel<16>", 2, 1, False, 2)
    assert dc.launch(dc.BWD_WEIGHT, 1, 16, 200, 328) == dc.Launch("disphead_bwd_weight_kernel<4>", 1024, 2, False, 1024)
    assert dc.launch(dc.BWD_WEIGHT, 1, 128, 25, 328) == dc.Launch("disphead_bwd_weight_kernel<32>", 1024, 2, False, 1024)
    assert dc.launch(dc.BWD_DATA, 1, 16, 1024, 1025) == dc.Launch("disphead_bwd_data_kernel<4>", 16384, 2, False, 0)
    assert dc.launch(dc.FWD, 1, 128, 128, 1025) == dc.Launch("disphead_fwd_direct_kernel<32>", 16384, 2, False, 0)
    assert dc.launch(dc.BWD_DATA, 3, 128, 5, 7) == dc.Launch("disphead_bwd_data_kernel<32>", 14, 1, True, 0)


def test_table_covers_every_kernel_in_every_regime():
    for entry in dc.ENTRIES:
        for C in dc.WIDTHS:
            rows = [r for r in dc.ROWS if r.entry == entry and r.C == C]
            ls = [dc.launch(r.entry, r.N, r.C, r.H, r.W) for r in rows]
            assert any(l.iters >= 2 for l in ls), f"{entry} C={C}: no second grid-stride pass"
            assert any(l.ragged for l in ls), f"{entry} C={C}: no ragged tail"
            assert any(l.blocks > 1 and l.ragged for l in ls), f"{entry} C={C}: no ragged tail with more than one workgroup"
            assert {(r.H, r.W) for r in rows if r.regime == "border"} == set(dc.BORDER_HW), f"{entry} C={C}: border rows"
            if entry == dc.BWD or (entry == dc.FWD and C < 64):
                assert {(r.N, r.H, r.W) for r in rows if r.regime == "tile edge"} == {(2, H, W) for H, W in dc.TILE_EDGE_HW}
    # the wave forms' ragged rows are no multiple of 4 * PPW either
    for r in dc.ROWS:
        if r.regime == "ragged":
            assert (r.N * r.H * r.W) % (4 * dc.ppw(r.C)) != 0 and (r.N * r.H * r.W) % dc.ppw(r.C) != 0
    # slice counts of the reduce kernel
    S = {dc.launch(r.entry, r.N, r.C, r.H, r.W).S for r in dc.ROWS if r.entry in (dc.BWD, dc.BWD_WEIGHT)}
    assert set(dc.REDUCE_S) <= S, sorted(set(dc.REDUCE_S) - S)
    # second passes stay small: 1 MiB and under for the tile forms' rows, 64 MiB only where the cap of 16384 workgroups asks for it
    for r in dc.ROWS:
        if r.regime == "second pass" and not r.big:
            assert r.N * r.H * r.W * r.C * 4 <= 5 * 2 ** 20
