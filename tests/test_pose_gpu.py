"""csrc/pose.hip and pd_view_synth_bwd_pose on the device against tests/pose_ref.py (fp64 NumPy) and fixture G15 (the
reference's own chain under autograd, tests/golden/make_golden_pose.py).

Bounds.  Matrices and decoder outputs: one float32 ulp of max(1, |entry|) -- the kernels evaluate in fp64 and round once, and
the device's fp64 sin / cos may differ from NumPy's in the last bit before that rounding.  Gradients: one float32 ulp of the
largest entry of that gradient.  gP: (HW - 1) 2^-53 sum|term| per entry, the bound of ANY order of HW fp64 additions, against
the exactly rounded sum.  gT: bit-equal to K^T gP formed in fp64 from the device's own gP.  Against the fixture's float64
autograd: 4 x the reference's own float32 deviation (recorded in the fixture)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import pose_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    d = dict(np.load(os.path.join(GOLDEN, "g15_pose.npz")))
    g12 = np.load(os.path.join(GOLDEN, "g12_reproj.npz"))
    d.update({k: g12[k] for k in ("depth", "src0", "src1", "K", "inv_K", "gw0", "gw1")})
    return d


def _cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _ulp1(ref):
    """One float32 ulp of max(1, |ref|), elementwise."""
    return np.spacing(np.maximum(1.0, np.abs(ref)).astype(np.float32)).astype(np.float64)


def _ulp_of_max(ref):
    return float(np.spacing(np.float32(np.abs(ref).max())))


# ------------------------------------------------------------------ pd_pose_matrix_*
@pytest.mark.parametrize("invert", [0, 1])
def test_pose_matrix_forward_and_backward(g, invert):
    from polardepth import ops
    rng = np.random.default_rng(7 + invert)
    # the fixture's three poses (small, ~1 rad, axisangle exactly 0) and 130 drawn ones: three workgroups of 64 threads
    aa = np.concatenate([g["aa"], rng.uniform(-1.2, 1.2, (130, 1, 3)).astype(np.float32)])
    tr = np.concatenate([g["tr"], rng.uniform(-1, 1, (130, 1, 3)).astype(np.float32)])
    gM = rng.standard_normal((133, 4, 4)).astype(np.float32)
    a, t = _cu(aa).requires_grad_(True), _cu(tr).requires_grad_(True)
    T = ops.pose_matrix(a, t, invert)
    ref = P.pose_matrix(aa, tr, invert)
    err = np.abs(T.detach().cpu().numpy().astype(np.float64) - ref)
    print("matrix: max err / ulp", (err / _ulp1(ref)).max())
    assert (err <= _ulp1(ref)).all()
    np.testing.assert_array_equal(T.detach().cpu().numpy()[:, 3], np.tile([0, 0, 0, 1], (133, 1)))
    (T * _cu(gM)).sum().backward()
    ga, gt = P.pose_matrix_grad(gM, aa, tr, invert)
    for got, want, name in ((a.grad, ga, "gaxisangle"), (t.grad, gt, "gtranslation")):
        e = np.abs(got.cpu().numpy().reshape(-1, 3).astype(np.float64) - want)
        # per item: the gradient of one pose, relative to that pose's largest entry
        tol = np.spacing(np.abs(want).max(1).astype(np.float32)).astype(np.float64)[:, None]
        print(name, "max err / ulp of the item's largest entry", (e / tol).max())
        assert (e <= tol).all(), name
    assert (a.grad[2] == 0).all()                                      # angle == 0: exactly zero
    # two calls give equal bits
    T2 = ops.pose_matrix(_cu(aa), _cu(tr), invert)
    assert torch.equal(T2, T.detach())
    a2, t2 = _cu(aa).requires_grad_(True), _cu(tr).requires_grad_(True)
    (ops.pose_matrix(a2, t2, invert) * _cu(gM)).sum().backward()
    assert torch.equal(a2.grad, a.grad) and torch.equal(t2.grad, t.grad)


def test_layers_facade_matches_the_reference_float32_matrices(g):
    from manydepth import layers as L
    a, t = _cu(g["aa"]), _cu(g["tr"])
    for inv in (False, True):
        M = L.transformation_from_parameters(a, t, inv).cpu().numpy()
        np.testing.assert_allclose(M, g[f"M_inv{int(inv)}"], rtol=0, atol=1.5e-6)   # the reference's own float32 chain: test_pose_ref derives 1.37e-6, + one rounding
    R4, T4 = L.rot_from_axisangle(a), L.get_translation_matrix(t)
    assert torch.equal(R4[:, :3, :3], L.transformation_from_parameters(a, t).detach()[:, :3, :3])
    assert (R4[:, :3, 3] == 0).all() and torch.equal(T4[:, :3, 3], t[:, 0]) and torch.equal(T4[:, :3, :3], torch.eye(3).cuda().expand(3, 3, 3))


# ------------------------------------------------------------------ pd_pose_head_*
@pytest.mark.parametrize("tag,invert", [("head", 0), ("head", 1), ("head1", 1)])
def test_pose_head_forward_and_backward(g, tag, invert):
    from polardepth import ops
    rng = np.random.default_rng(11)
    x, w, b = g[f"{tag}_x"], g["head_w"], g["head_b"]
    N, h, wd, Cin = x.shape

    def run(grads):
        xt = _cu(x).permute(0, 3, 1, 2).requires_grad_(True)          # [N,Cin,h,w] over NHWC storage
        wt, bt = _cu(w).reshape(12, Cin, 1, 1).requires_grad_(True), _cu(b).requires_grad_(True)
        outs = ops.pose_head(xt, wt, bt, invert)
        loss = sum((o * _cu(c)).sum() for o, c in zip(outs, grads) if c is not None)
        loss.backward()
        return [o.detach() for o in outs], (xt.grad, wt.grad, bt.grad)

    gaa, gtr = rng.standard_normal((N, 2, 1, 3)).astype(np.float32), rng.standard_normal((N, 2, 1, 3)).astype(np.float32)
    gT, gTi = rng.standard_normal((N, 4, 4)).astype(np.float32), rng.standard_normal((N, 4, 4)).astype(np.float32)
    (aa, tr, T, Ti), (gx, gw, gb) = run((gaa, gtr, gT, gTi))
    ref = P.pose_head(x, w, b, invert)
    o = ref["o64"].reshape(N, 2, 1, 6)
    for got, want in ((aa, o[..., :3]), (tr, o[..., 3:])):
        assert tuple(got.shape) == (N, 2, 1, 3)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= _ulp1(want)).all()
    # the matrices from the device's own float32 outputs
    a_dev, t_dev = aa.cpu().numpy(), tr.cpu().numpy()
    for got, inv in ((T, invert), (Ti, 1 - invert)):
        want = P.pose_matrix(a_dev[:, 0], t_dev[:, 0], inv)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= _ulp1(want)).all()
    prod = (T.double() @ Ti.double()).cpu().numpy()
    np.testing.assert_allclose(prod, np.tile(np.eye(4), (N, 1, 1)), atol=1e-6)
    # gradients, at the device's float32 outputs (the restatement's means: fsum, exactly rounded)
    rgx, rgw, rgb = P.pose_head_grad(x.shape, w, ref["mean"], a_dev, t_dev, invert, gT, gTi, gaa, gtr)
    for got, want, name in ((gx.permute(0, 2, 3, 1), rgx, "gx"), (gw.reshape(12, Cin), rgw, "gw"), (gb, rgb, "gb")):
        e = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(tag, name, "max err", e, "ulp of the largest entry", _ulp_of_max(want))
        assert e <= _ulp_of_max(want), name
    # matrices only: the rows of slot 1 receive exactly zero
    _, (gx0, gw0, gb0) = run((None, None, gT, gTi))
    assert (gw0[6:] == 0).all() and (gb0[6:] == 0).all() and (gw0[:6] != 0).any() and (gb0[:6] != 0).all()
    rgx0, rgw0, rgb0 = P.pose_head_grad(x.shape, w, ref["mean"], a_dev, t_dev, invert, gT, gTi)
    assert np.abs(gw0.reshape(12, Cin).cpu().numpy() - rgw0).max() <= _ulp_of_max(rgw0)
    assert np.abs(gx0.permute(0, 2, 3, 1).cpu().numpy() - rgx0).max() <= _ulp_of_max(rgx0)
    # two calls give equal bits
    outs2, grads2 = run((gaa, gtr, gT, gTi))
    assert all(torch.equal(p, q) for p, q in zip(outs2, (aa, tr, T, Ti)))
    assert all(torch.equal(p, q) for p, q in zip(grads2, (gx, gw, gb)))


def test_pose_head_accumulates_into_given_buffers(g):
    """accumulate = 1 adds to gw / gb (what the modules' gradient buffers need); gx is always written with "="."""
    from polardepth._lib import lib, check, ptr, stream_ptr
    x, w, b = _cu(g["head_x"]), _cu(g["head_w"]), _cu(g["head_b"])
    N, h, wd, Cin = x.shape
    aa, tr = torch.empty(N, 2, 1, 3, device="cuda"), torch.empty(N, 2, 1, 3, device="cuda")
    T, Ti = torch.empty(N, 4, 4, device="cuda"), torch.empty(N, 4, 4, device="cuda")
    mean = torch.empty(N, Cin, dtype=torch.float64, device="cuda")
    check(lib.pd_pose_head_fwd(ptr(x), ptr(w), ptr(b), ptr(aa), ptr(tr), ptr(T), ptr(Ti), ptr(mean), N, h, wd, Cin, 12, 0,
                               stream_ptr()), "fwd")
    gT = _cu(np.random.default_rng(5).standard_normal((N, 4, 4)).astype(np.float32))
    ws = torch.empty(N, 12, dtype=torch.float64, device="cuda")
    out = {}
    for acc in (0, 1):
        gx = torch.full_like(x, 3.0)
        gw, gb = torch.full_like(w, 2.0), torch.full_like(b, -1.0)
        check(lib.pd_pose_head_bwd(ptr(gT), None, None, None, ptr(aa), ptr(tr), ptr(w), ptr(mean), ptr(gx), ptr(gw), ptr(gb),
                                   ptr(ws), N, h, wd, Cin, 12, 0, acc, stream_ptr()), "bwd")
        out[acc] = (gx, gw, gb)
    assert torch.equal(out[0][0], out[1][0])
    np.testing.assert_allclose(out[1][1].cpu().numpy(), out[0][1].cpu().numpy() + 2.0, rtol=0, atol=2.4e-7)
    np.testing.assert_allclose(out[1][2].cpu().numpy(), out[0][2].cpu().numpy() - 1.0, rtol=0, atol=1.2e-7)


# ------------------------------------------------------------------ pd_view_synth_bwd_pose
def _bwd_pose(gw, src, coords, depth, K, inv_K, T, want_gdepth=True, want_gP=True):
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, C, h, w = src.shape
    gd = torch.full((N, 1, h, w), float("nan"), device="cuda") if want_gdepth else None
    rows = lib.pd_view_synth_pose_rows(h, w)
    part = torch.full((N, rows, 12), float("nan"), dtype=torch.float64, device="cuda")
    gP = torch.full((N, 12), float("nan"), dtype=torch.float64, device="cuda") if want_gP else None
    gT = torch.full((N, 4, 4), float("nan"), device="cuda")
    check(lib.pd_view_synth_bwd_pose(ptr(gw), ptr(src), ptr(coords), ptr(depth), ptr(K), ptr(inv_K), ptr(T), ptr(gd), ptr(part),
                                     ptr(gP), ptr(gT), N, C, h, w, 0, stream_ptr()), "pd_view_synth_bwd_pose")
    torch.cuda.synchronize()
    return gd, gP, gT


def _bwd_depth(gw, src, coords, depth, K, inv_K, T):
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, C, h, w = src.shape
    gd = torch.full((N, 1, h, w), float("nan"), device="cuda")
    check(lib.pd_view_synth_bwd(ptr(gw), ptr(src), ptr(coords), ptr(depth), ptr(K), ptr(inv_K), ptr(T), ptr(gd), N, C, h, w, 0,
                                stream_ptr()), "pd_view_synth_bwd")
    return gd


def _check_pose_gradient(gw, src, depth, K, iK, T, what):
    """Everything the issue asks of one call, on NumPy float32 inputs; returns (restatement, device gT as fp64)."""
    from polardepth import ops
    d = [_cu(a) for a in (gw, src, depth, K, iK, T)]
    dgw, dsrc, ddepth, dK, diK, dT = d
    with torch.no_grad():
        _, coords = ops.view_synthesis(ddepth, dsrc, dK, diK, dT)
    gd, gP, gT = _bwd_pose(dgw, dsrc, coords, ddepth, dK, diK, dT)
    assert torch.equal(gd.view(torch.int32), _bwd_depth(dgw, dsrc, coords, ddepth, dK, diK, dT).view(torch.int32)), what
    ref = P.view_synth_pose_grad(gw, src, coords.cpu().numpy(), depth, K, iK, T)
    HW = src.shape[2] * src.shape[3]
    gPn = gP.cpu().numpy()
    tol = (HW - 1) * 2.0 ** -53 * ref["abs"]
    err = np.abs(gPn - ref["gP"])
    print(what, "gP: max err", err.max(), "max bound", tol.max(), "max err / bound", (err / np.maximum(tol, 1e-300)).max())
    assert (err <= tol).all(), what
    want_gT = P.gT_from_gP(gPn, K).astype(np.float32)
    np.testing.assert_array_equal(gT.cpu().numpy().view(np.int32), want_gT.view(np.int32), err_msg=what)
    # two calls give equal bits; the optional outputs may be left out
    gd2, gP2, gT2 = _bwd_pose(dgw, dsrc, coords, ddepth, dK, diK, dT)
    assert torch.equal(gP2.view(torch.int64), gP.view(torch.int64)) and torch.equal(gT2.view(torch.int32), gT.view(torch.int32))
    _, _, gT3 = _bwd_pose(dgw, dsrc, coords, ddepth, dK, diK, dT, want_gdepth=False, want_gP=False)
    assert torch.equal(gT3.view(torch.int32), gT.view(torch.int32))
    return ref, gT.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("case", ["0", "1", "s"])
def test_pose_gradient_on_the_fixture(g, case):
    if case == "s":
        a = [g[k] for k in ("s_gw", "s_src", "s_depth", "s_K", "s_inv_K", "s_T")]
        want = g["s_dT_f64"]
    else:
        a = [g[f"gw{case}"], g[f"src{case}"], g["depth"], g["K"], g["inv_K"], g[f"wT{case}"]]
        want = g[f"dT{case}_f64"]
    ref, gT = _check_pose_gradient(*a, what=f"fixture {case}")
    dev = np.abs(gT - want).max() / np.abs(want).max()
    print("case", case, "device vs float64 autograd", dev, "reference float32 vs float64", float(g["dev_gT_rel"]))
    assert dev <= 4 * float(g["dev_gT_rel"])


def test_pose_gradient_all_clamped_item_and_non_finite_depth(g):
    """Item 0: a pose that sends every pixel past a border -- gT exactly 0.  Item 1: a depth map with one inf and one 0 --
    gT finite and equal to the restatement, in which those two pixels contribute nothing."""
    depth = g["depth"].copy()
    depth[1, 0, 4, 7], depth[1, 0, 11, 30] = np.inf, 0.0
    T = g["wT0"].copy()
    T[0, 0, 3], T[0, 1, 3] = 50.0, 50.0                                # far past the right and the bottom border for every pixel
    T[1, 2, 3] = 0.0                                                   # depth 0 then projects to t.xy / 1e-7: far outside
    ref, gT = _check_pose_gradient(g["gw0"], g["src0"], depth, g["K"], g["inv_K"], T, what="clamped / non-finite")
    assert not (ref["free_x"][0] | ref["free_y"][0]).any()
    assert (gT[0] == 0).all()
    for (y, x) in ((4, 7), (11, 30)):
        assert not (ref["free_x"][1, y, x] or ref["free_y"][1, y, x])
    assert np.isfinite(gT).all() and np.isfinite(ref["gP"]).all() and np.abs(gT[1]).max() > 0
    np.testing.assert_allclose(gT[1], ref["gT"][1], rtol=0, atol=_ulp_of_max(ref["gT"][1]))


def test_pose_gradient_with_more_than_256_rows():
    """260 x 260: pd_view_synth_pose_rows = 265 > 256, so the strided part of finalize_rows runs."""
    from polardepth._lib import lib
    H = W = 260
    assert lib.pd_view_synth_pose_rows(H, W) == 265
    rng = np.random.default_rng(26)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = (1.0 + 0.2 * np.sin(xx / 40) * np.cos(yy / 31))[None, None].astype(np.float32)
    src = rng.uniform(0, 1, (1, 2, H, W)).astype(np.float32)
    gw = rng.standard_normal((1, 2, H, W)).astype(np.float32)
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 0.8 * W, 0.9 * H, W / 2 - 0.3, H / 2 + 0.4
    iK = np.linalg.pinv(K.astype(np.float32))
    T = np.eye(4)
    T[:3, 3] = (0.05, -0.03, -0.2)
    ref, gT = _check_pose_gradient(gw, src, depth, K[None].astype(np.float32), iK[None], T[None].astype(np.float32), what="260 x 260")
    clamped = 1 - (ref["free_x"] & ref["free_y"]).mean()
    assert 0.02 < clamped < 0.9
    np.testing.assert_allclose(gT, ref["gT"], rtol=0, atol=_ulp_of_max(ref["gT"]))


def test_view_synthesis_backward_takes_the_pose_entry_only_when_asked(g):
    from polardepth import ops
    d = {k: _cu(g[k]) for k in ("depth", "src0", "K", "inv_K", "wT0", "gw0")}
    depth = d["depth"].clone().requires_grad_(True)
    warped, coords = ops.view_synthesis(depth, d["src0"], d["K"], d["inv_K"], d["wT0"])
    (warped * d["gw0"]).sum().backward()
    want = _bwd_depth(d["gw0"], d["src0"], coords, d["depth"], d["K"], d["inv_K"], d["wT0"])
    assert torch.equal(depth.grad.view(torch.int32), want.view(torch.int32))          # the parent's bits
    # a pose that requires a gradient receives one, and the depth gradient keeps its bits
    depth2, T = d["depth"].clone().requires_grad_(True), d["wT0"].clone().requires_grad_(True)
    warped2, _ = ops.view_synthesis(depth2, d["src0"], d["K"], d["inv_K"], T)
    (warped2 * d["gw0"]).sum().backward()
    _, _, gT = _bwd_pose(d["gw0"], d["src0"], coords, d["depth"], d["K"], d["inv_K"], d["wT0"])
    assert T.grad is not None and torch.equal(T.grad.view(torch.int32), gT.view(torch.int32))
    assert torch.equal(depth2.grad.view(torch.int32), want.view(torch.int32))
    # the pose alone
    T3 = d["wT0"].clone().requires_grad_(True)
    ops.view_synthesis(d["depth"], d["src0"], d["K"], d["inv_K"], T3)[0].mul(d["gw0"]).sum().backward()
    assert torch.equal(T3.grad.view(torch.int32), gT.view(torch.int32))
    # through pose_matrix: the parameters of a predicted pose receive a gradient
    a = _cu(g["aa"][:2]).requires_grad_(True)
    t = _cu(g["tr"][:2] * 0.05).requires_grad_(True)
    ops.view_synthesis(d["depth"], d["src0"], d["K"], d["inv_K"], ops.pose_matrix(a, t))[0].mul(d["gw0"]).sum().backward()
    assert a.grad.abs().min() > 0 and t.grad.abs().min() > 0
