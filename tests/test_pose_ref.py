"""tests/pose_ref.py (the fp64 yardstick of the pose-network kernels) against what the reference itself computed
(tests/golden/g15_pose.npz, make_golden_pose.py) and against autograd in fp64.  CPU only."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import pose_ref as P
import reproj_ref as R

U32 = 2.0 ** -24                     # unit roundoff of float32


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "g15_pose.npz")))


def test_matrices_against_the_reference_float32_ones(g):
    """The reference evaluates in float32.  An entry of R is a chain of at most ~12 float32 roundings of quantities <= 1
    (norm 2.5 u, axis + 1 u, cos / sin 1 u + the angle's 2.5 u, C, three products, one sum) for |angle| <= 1.1, so
    |R32 - R| <= 12 u; the inverted last column is a three-term float32 dot product of those entries with -t: the entries'
    errors times |t| plus (3 + 1) u sum|R||t| for the products and sums.  Hence 12 u max(1, sum|t|) + 4 u sum|R||t|."""
    a = g["aa"].astype(np.float64).reshape(-1, 3)
    assert np.linalg.norm(a, axis=1).max() <= 1.1 and (a[2] == 0).all()
    t = np.abs(g["tr"].astype(np.float64).reshape(-1, 3))
    for inv in (0, 1):
        M = P.pose_matrix(g["aa"], g["tr"], inv)
        ref = g[f"M_inv{inv}"].astype(np.float64)
        Rt = np.einsum("nki,nk->ni", np.abs(M[:, :3, :3]), t)             # sum_k |R[k][i]| |t[k]|
        tol = 12 * U32 * np.maximum(1.0, t.sum(1)) + 4 * U32 * Rt.max(1)
        err = np.abs(M - ref).reshape(3, -1).max(1)
        print("invert", inv, "err", err, "tol", tol)
        assert (err <= tol).all()
        np.testing.assert_array_equal(M[:, 3], [[0, 0, 0, 1]] * 3)
    # the two are inverses of each other
    prod = P.pose_matrix(g["aa"], g["tr"], 0) @ P.pose_matrix(g["aa"], g["tr"], 1)
    np.testing.assert_allclose(prod, np.tile(np.eye(4), (3, 1, 1)), atol=1e-6)     # 1e-7 in the axis normalisation


def test_matrix_and_its_gradient_against_autograd_fp64(g):
    rng = np.random.default_rng(3)
    gM = rng.standard_normal((3, 4, 4))
    for inv in (False, True):
        aa = torch.from_numpy(g["aa"]).double().requires_grad_(True)
        tr = torch.from_numpy(g["tr"]).double().requires_grad_(True)
        M = P.torch_matrix(aa, tr, inv)
        np.testing.assert_allclose(P.pose_matrix(g["aa"], g["tr"], inv), M.detach().numpy(), rtol=0, atol=1e-15)
        (M * torch.from_numpy(gM)).sum().backward()
        ga, gt = P.pose_matrix_grad(gM, g["aa"], g["tr"], inv)
        scale = max(np.abs(aa.grad.numpy()).max(), np.abs(tr.grad.numpy()).max())
        np.testing.assert_allclose(ga, aa.grad.numpy().reshape(3, 3), rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(gt, tr.grad.numpy().reshape(3, 3), rtol=0, atol=1e-12 * scale)
        assert (ga[2] == 0).all() and (aa.grad.numpy()[2] == 0).all()      # angle == 0: exactly zero, as PyTorch's norm rule gives
        assert np.abs(ga[:2]).min() > 0


@pytest.mark.parametrize("tag", ["head", "head1"])
def test_head_against_the_reference_decoder_tail_fp64(g, tag):
    x, w, b = g[f"{tag}_x"], g["head_w"], g["head_b"]
    out = P.pose_head(x, w, b, False)
    o = out["o64"].reshape(3, 2, 1, 6)
    hw, Cin = x.shape[1] * x.shape[2], x.shape[3]
    # both are fp64 sums of the same hw * Cin products per output in different orders
    mag = 0.01 * (np.abs(b.astype(np.float64))[:, None]
                  + np.abs(w.astype(np.float64)) @ np.abs(x.astype(np.float64)).mean((1, 2)).T).max()
    tol = (hw + Cin + 4) * 2.0 ** -53 * mag
    np.testing.assert_allclose(o[..., :3], g[f"{tag}_aa"], rtol=0, atol=tol)
    np.testing.assert_allclose(o[..., 3:], g[f"{tag}_tr"], rtol=0, atol=tol)
    np.testing.assert_array_equal(out["axisangle"], o[..., :3].astype(np.float32))
    np.testing.assert_array_equal(out["T"], P.pose_matrix(out["axisangle"][:, 0], out["translation"][:, 0], False))
    np.testing.assert_array_equal(out["T_inv"], P.pose_matrix(out["axisangle"][:, 0], out["translation"][:, 0], True))


def test_head_gradient_against_autograd_fp64(g):
    """The chain x -> mean -> 1x1 convolution -> 0.01 -> both matrices of slot 0, without the rounding of o to float32 in
    between (autograd cannot see it): the restatement's gradient at the unrounded o would differ by 1e-7 relative, so the
    comparison feeds autograd the float32 o as a leaf for the matrix part and checks the linear part separately."""
    rng = np.random.default_rng(4)
    x, w, b = g["head_x"], g["head_w"], g["head_b"]
    fwd = P.pose_head(x, w, b, True)
    gT, gTi = rng.standard_normal((3, 4, 4)), rng.standard_normal((3, 4, 4))
    gaa, gtr = rng.standard_normal((3, 2, 1, 3)), rng.standard_normal((3, 2, 1, 3))
    gx, gw, gb = P.pose_head_grad(x.shape, w, fwd["mean"], fwd["axisangle"], fwd["translation"], True, gT, gTi, gaa, gtr)
    o = torch.from_numpy(np.concatenate([fwd["axisangle"], fwd["translation"]], -1)).double().requires_grad_(True)
    loss = (P.torch_matrix(o[:, 0, 0, :3], o[:, 0, 0, 3:], True) * torch.from_numpy(gT)).sum() \
        + (P.torch_matrix(o[:, 0, 0, :3], o[:, 0, 0, 3:], False) * torch.from_numpy(gTi)).sum() \
        + (o[..., :3] * torch.from_numpy(gaa)).sum() + (o[..., 3:] * torch.from_numpy(gtr)).sum()
    go = torch.autograd.grad(loss, o)[0].reshape(3, 12)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    bt = torch.from_numpy(b).double().requires_grad_(True)
    lin = 0.01 * (xt.mean((1, 2)) @ wt.T + bt)
    (lin * go).sum().backward()
    for mine, ref in ((gx, xt.grad), (gw, wt.grad), (gb, bt.grad)):
        np.testing.assert_allclose(mine, ref.numpy(), rtol=0, atol=1e-12 * np.abs(ref.numpy()).max())
    # slot 1 receives nothing unless gaxisangle / gtranslation are given
    _, gw0, gb0 = P.pose_head_grad(x.shape, w, fwd["mean"], fwd["axisangle"], fwd["translation"], True, gT, gTi)
    assert (gw0[6:] == 0).all() and (gb0[6:] == 0).all() and np.abs(gw0[:6]).min() > 0


@pytest.mark.parametrize("case", ["0", "1", "s"])
def test_pose_gradient_of_the_warp_against_autograd_fp64(g, case):
    """The formula of pd_view_synth_bwd_pose, evaluated in fp64 throughout (dt=float64, fp64 coordinates), against autograd
    through the reference's BackprojectDepth / Project3D / grid_sample in float64: 1e-10 relative to the largest entry."""
    if case == "s":
        a = [g[k] for k in ("s_gw", "s_src", "s_depth", "s_K", "s_inv_K", "s_T")]
        ref = g["s_dT_f64"]
    else:
        g12 = np.load(os.path.join(GOLDEN, "g12_reproj.npz"))
        a = [g12[f"gw{case}"], g12[f"src{case}"], g12["depth"], g12["K"], g12["inv_K"], g[f"wT{case}"]]
        ref = g[f"dT{case}_f64"]
    gw, src, depth, K, iK, T = a
    H, W = src.shape[2:]
    coords, _, _ = R.project(depth, K, iK, T)
    assert not P.near_boundary(coords, H, W).any() and g["share_near_boundary"] == 0
    out = P.view_synth_pose_grad(gw, src, coords, depth, K, iK, T, dt=np.float64)
    clamped = 1 - (out["free_x"] & out["free_y"]).mean()
    print("case", case, "clamped share", clamped, "max|dT|", np.abs(ref).max())
    assert 0.05 < clamped < 0.9
    np.testing.assert_array_equal(out["gT"][:, 3, :3], 0.0)
    err = np.abs(out["gT"] - ref).max() / np.abs(ref).max()
    print("relative error", err)
    assert err <= 1e-10
    # float32 gu / gv at the float32-rounded coordinates (what the kernel computes) stay within the reference's own float32
    # deviation with the margin the GPU test allows
    out32 = P.view_synth_pose_grad(gw, src, coords.astype(np.float32), depth, K, iK, T)
    err32 = np.abs(out32["gT"] - ref).max() / np.abs(ref).max()
    print("float32 taps:", err32, "reference float32:", float(g["dev_gT_rel"]))
    assert err32 <= 4 * float(g["dev_gT_rel"])
