"""tests/pose_loss_ref.py (the fp64 yardstick of csrc/pose_loss.hip) against SciPy's Rotation.from_matrix / as_rotvec -- the
algorithm roma.rotmat_to_rotvec was adapted from; roma itself is not a dependency, so parity with it is pinned through
SciPy's identical algorithm only -- and against autograd in float64.  CPU only."""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import pose_loss_ref as L

ANGLES = (1e-5, 5e-4, 2e-3, 0.5, 2.9)


def exact_rotations(rng, n, a):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return Rotation.from_rotvec(v * rng.uniform(0.0, a, (n, 1))).as_matrix()


def test_rotvec_against_scipy_on_exact_rotations():
    rng = np.random.default_rng(0)
    small = []
    for a in ANGLES:
        M = exact_rotations(rng, 3000, a)
        rv, c = L.rotvec(M)
        ref = Rotation.from_matrix(M).as_rotvec()
        err = np.abs(rv - ref).max()
        counts = np.bincount(c, minlength=4)
        print("a", a, "max err", err, "branches", counts)
        assert err <= 1e-12
        if a == 2.9:
            assert (counts > 0).all(), counts
        small.append(L.small_angle(M))
    small = np.concatenate(small)
    assert small.any() and (~small).any()


def test_rotvec_against_scipy_on_the_pose_heads_float32_matrices():
    """SciPy first orthogonalises a matrix that is orthogonal only to float32 rounding; that is the whole difference."""
    rng = np.random.default_rng(1)
    T = L.head_matrices(rng, 2000, max_angle=3.0)
    M = T[:, :3, :3].astype(np.float64)
    rv, c = L.rotvec(M)
    assert np.linalg.norm(rv, axis=1).max() < 3.0 + 1e-6 and (np.bincount(c, minlength=4) > 0).all()
    err = np.abs(rv - Rotation.from_matrix(M).as_rotvec()).max()
    print("max err", err)
    assert err <= 5e-7


def grad_cases():
    """Float64 matrices that cover the four branches, the small-angle branch and the identity."""
    rng = np.random.default_rng(2)
    M = np.concatenate([exact_rotations(rng, 200, 2.9), exact_rotations(rng, 20, 5e-4), exact_rotations(rng, 20, 2e-3),
                        np.eye(3)[None]])
    # not exactly orthogonal, like a prediction
    M[:200] += 1e-3 * rng.standard_normal((200, 3, 3))
    M[200:240] += 1e-7 * rng.standard_normal((40, 3, 3))
    return M


def test_rotvec_grad_against_autograd_fp64():
    M = grad_cases()
    rv, c = L.rotvec(M)
    assert (np.bincount(c, minlength=4) > 0).all() and L.small_angle(M).any() and (~L.small_angle(M)).any()
    rng = np.random.default_rng(3)
    g = rng.standard_normal(rv.shape)
    Mt = torch.from_numpy(M).requires_grad_(True)
    out = L.torch_rotvec(Mt)
    np.testing.assert_allclose(rv, out.detach().numpy(), rtol=0, atol=1e-14)
    (out * torch.from_numpy(g)).sum().backward()
    mine, ref = L.rotvec_grad(M, g), Mt.grad.numpy()
    assert np.isfinite(mine).all() and np.isfinite(ref).all()
    scale = np.abs(ref).reshape(len(M), -1).max(1)
    err = (np.abs(mine - ref).reshape(len(M), -1).max(1) / scale).max()
    print("relative error", err)
    assert err <= 1e-9
    # the identity: rv = (M21 - M12, M02 - M20, M10 - M01) / 2 to first order
    e = np.zeros((3, 3, 3))
    e[0, 2, 1], e[0, 1, 2] = 0.5, -0.5
    e[1, 0, 2], e[1, 2, 0] = 0.5, -0.5
    e[2, 1, 0], e[2, 0, 1] = 0.5, -0.5
    I3 = np.tile(np.eye(3), (3, 1, 1))
    np.testing.assert_array_equal(L.rotvec_grad(I3, np.eye(3)), e)
    np.testing.assert_array_equal(L.rotvec(np.eye(3))[0], np.zeros((1, 3)))


def loss_inputs(F, n=24, seed=4):
    rng = np.random.default_rng(seed)
    Tp = [L.head_matrices(rng, n, 3.0) for _ in range(F)]
    Tg = [L.head_matrices(rng, n, 3.0, invert=bool(f & 1)) for f in range(F)]
    for T in Tp:                                              # a small-angle pair and an identity in every frame
        T[0] = L.head_matrices(rng, 1, 5e-4)[0]
        T[1] = np.eye(4, dtype=np.float32)
    return Tp, Tg


@pytest.mark.parametrize("F", [1, 2, 3])
def test_pose_loss_is_the_references_running_sums(F):
    """The default weights [F .. 1] reproduce total_loss += r_loss + t_loss inside the loop over the frames."""
    Tp, Tg = loss_inputs(F)
    vals = L.pose_loss(Tp, Tg)
    ref = L.torch_pose_loss([torch.from_numpy(t).double() for t in Tp], [torch.from_numpy(t).double() for t in Tg])
    np.testing.assert_allclose(vals[:3], [float(x) for x in ref], rtol=1e-13, atol=0)
    np.testing.assert_allclose(vals[0], vals[3::2].sum(), rtol=1e-15)
    np.testing.assert_allclose(vals[1], vals[4::2].sum(), rtol=1e-15)
    assert L.default_weights(F) == [float(F - f) for f in range(F)]


@pytest.mark.parametrize("F", [1, 2, 3])
def test_pose_loss_grad_against_autograd_fp64(F):
    Tp, Tg = loss_inputs(F)
    gv = np.array([0.7, -1.3, 0.9], np.float32)
    tp = [torch.from_numpy(t).double().requires_grad_(True) for t in Tp]
    r, t, tot = L.torch_pose_loss(tp, [torch.from_numpy(t).double() for t in Tg])
    (float(gv[0]) * r + float(gv[1]) * t + float(gv[2]) * tot).backward()
    mine = L.pose_loss_grad(gv, Tp, Tg)
    for f in range(F):
        ref = tp[f].grad.numpy()
        assert (mine[f][:, 3] == 0).all() and (ref[:, 3] == 0).all()
        scale = np.abs(ref).reshape(len(ref), -1).max(1)
        assert scale.min() > 0
        err = (np.abs(mine[f] - ref).reshape(len(ref), -1).max(1) / scale).max()
        print("frame", f, "relative error", err)
        assert err <= 1e-9


def test_valid_mask():
    F, n = 3, 24
    Tp, Tg = loss_inputs(F, n)
    gv = np.array([0.3, 0.5, 1.0], np.float32)
    ones = np.ones((n, F), np.float32)
    np.testing.assert_array_equal(L.pose_loss(Tp, Tg, ones), L.pose_loss(Tp, Tg))
    for a, b in zip(L.pose_loss_grad(gv, Tp, Tg, ones), L.pose_loss_grad(gv, Tp, Tg)):
        np.testing.assert_array_equal(a, b)
    # some items invalid: the loss of the sub-batch, frame by frame
    rng = np.random.default_rng(5)
    valid = (rng.random((n, F)) < 0.6).astype(np.float32)
    valid[:, 2] = 0                                           # a frame without a valid item
    assert 0 < valid[:, 0].sum() < n and 0 < valid[:, 1].sum() < n
    vals = L.pose_loss(Tp, Tg, valid)
    grads = L.pose_loss_grad(gv, Tp, Tg, valid)
    w = L.default_weights(F)
    for f in range(2):
        m = valid[:, f] != 0
        sub = L.pose_loss([Tp[f][m]], [Tg[f][m]], frame_weight=[w[f]])
        np.testing.assert_allclose(vals[3 + 2 * f:5 + 2 * f], sub[3:5], rtol=1e-15)
        gsub = L.pose_loss_grad(gv, [Tp[f][m]], [Tg[f][m]], frame_weight=[w[f]])[0]
        np.testing.assert_allclose(grads[f][m], gsub, rtol=1e-15)
        assert (grads[f][~m] == 0).all() and np.abs(grads[f][m]).max() > 0
    assert vals[7] == 0 and vals[8] == 0 and (grads[2] == 0).all()
    np.testing.assert_allclose(vals[2], w[0] * (vals[3] + vals[4]) + w[1] * (vals[5] + vals[6]), rtol=1e-15)
    # given weights are used as given
    np.testing.assert_allclose(L.pose_loss(Tp, Tg, valid, [1.0, 1.0, 1.0])[2], vals[0] + vals[1], rtol=1e-15)


def test_metrics_against_direct_formulas():
    rng = np.random.default_rng(6)
    F, M = 2, 37
    Tp = [L.head_matrices(rng, M, 0.3, 0.05) for _ in range(F)]
    Tg = [L.head_matrices(rng, M, 0.3, 0.05) for _ in range(F)]
    Tg[0][3, :3, 3] = 1e-5                                    # |t_gt| below 1 mm: no ratio from this pair
    rec = L.pose_records(Tp, Tg)
    valid = np.ones((M, F), np.float32)
    valid[[2, 9], 0] = 0
    valid[5, 1] = 0
    rec[0, 7, 6] = np.nan                                     # bad
    rec[1, 11, 8] = np.inf                                    # bad
    rec[1, 5, 7] = np.nan                                     # missing AND non-finite: missing
    out = L.metrics(rec, valid, [-1, 1])
    assert set(out) == {-1, 1, "all"}
    assert (out[-1]["pairs"], out[-1]["missing"], out[-1]["bad"]) == (M - 3, 2, 1)
    assert (out[1]["pairs"], out[1]["missing"], out[1]["bad"]) == (M - 2, 1, 1)
    assert (out["all"]["pairs"], out["all"]["missing"], out["all"]["bad"]) == (2 * M - 5, 3, 2)
    keep = [np.array([i for i in range(M) if i not in (2, 9, 7)]), np.array([i for i in range(M) if i not in (5, 11)])]
    for f, fid in ((0, -1), (1, 1), (None, "all")):
        r = rec[f][keep[f]] if f is not None else np.concatenate([rec[0][keep[0]], rec[1][keep[1]]])
        deg, mm = np.degrees(r[:, 6]), 1000.0 * r[:, 7]
        for name, x in (("rot_deg", deg), ("trans_mm", mm)):
            got = out[fid][name]
            np.testing.assert_allclose([got["mean"], got["median"], got["rmse"], got["max"]],
                                       [x.mean(), np.median(x), np.sqrt(np.mean(x ** 2)), x.max()], rtol=1e-12)
        big = r[:, 9] >= 1e-3
        np.testing.assert_allclose(out[fid]["scale_ratio_median"], np.median(r[big, 8] / r[big, 9]), rtol=1e-12)
    assert not (rec[0][keep[0]][:, 9] >= 1e-3).all()
    # records: the geodesic angle is the angle between the two rotations
    Rp, Rg = Tp[1][:, :3, :3].astype(np.float64), Tg[1][:, :3, :3].astype(np.float64)
    ang = np.linalg.norm(Rotation.from_matrix(np.einsum("nki,nkj->nij", Rp, Rg)).as_rotvec(), axis=1)
    np.testing.assert_allclose(rec[1][keep[1]][:, 6], ang[keep[1]], rtol=0, atol=5e-7)
    empty = L.metrics(rec, np.zeros((M, F)), [-1, 1])["all"]
    assert empty["pairs"] == 0 and empty["missing"] == 2 * M and np.isnan(empty["rot_deg"]["mean"])
