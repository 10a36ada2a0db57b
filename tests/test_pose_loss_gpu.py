"""pd_pose_loss_fwd / _bwd and ops.pose_supervision on the device against tests/pose_loss_ref.py (float64): records, vals,
the gradient, bit-reproducibility, the missing-frame mask, and the chain behind ops.pose_matrix against autograd in float64.
The inputs are the float32 matrices the pose head produces; the device takes its branch decisions from the same float32
values with the same exactly stated float64 expressions, so no case is excluded."""
import numpy as np
import pytest
import torch

import pose_loss_ref as L
import pose_ref as P

pytestmark = pytest.mark.gpu


def _cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def make_case(N, F, first_branch=0):
    """F frames of N predicted / ground-truth matrices (float32).  N >= 65: every frame holds all four branches, a
    small-angle item and an exact identity.  N == 1: frame f holds an item of branch (first_branch + f) % 4."""
    rng = np.random.default_rng(1000 * N + 10 * F + first_branch)
    Tp, Tg = [], []
    for f in range(F):
        pool = L.head_matrices(rng, max(N, 64), 3.0)
        c = L.rotvec(pool[:, :3, :3])[1]
        if N == 1:
            pool = pool[np.flatnonzero(c == (first_branch + f) % 4)[:1]]
        else:
            pool[0] = L.head_matrices(rng, 1, 5e-4)[0]
            pool[1] = np.eye(4, dtype=np.float32)
            pool[2, :3, 3] = 0                                # |t| = 0
            assert (np.bincount(L.rotvec(pool[:, :3, :3])[1], minlength=4) > 0).all()
            assert L.small_angle(pool[:, :3, :3])[:2].all() and not L.small_angle(pool[:, :3, :3])[3:].all()
        Tp.append(pool)
        Tg.append(L.head_matrices(rng, N, 3.0, invert=bool(f & 1)))
    return Tp, Tg


def make_valid(N, F, seed=0):
    v = (np.random.default_rng(seed).random((N, F)) < 0.7).astype(np.float32)
    v[0, 0] = 1.0
    if F > 1:
        v[:, F - 1] = 0                                       # a frame without a valid item
    if N > 1:
        v[1, 0] = 0
    return v


def raw_fwd(Tp, Tg, valid, weights, records=True):
    import ctypes
    from polardepth._lib import lib, check, ptr, stream_ptr
    F, N = len(Tp), Tp[0].shape[0]
    vals = torch.full((3 + 2 * F,), float("nan"), device="cuda")
    rec = torch.full((F, N, 10), float("nan"), dtype=torch.float64, device="cuda") if records else None
    arr = lambda ts: (ctypes.c_void_p * F)(*[t.data_ptr() for t in ts])
    check(lib.pd_pose_loss_fwd(arr(Tp), arr(Tg), F, (ctypes.c_float * F)(*weights), ptr(valid), ptr(rec), ptr(vals), N,
                               stream_ptr()), "pd_pose_loss_fwd")
    return vals, rec


def raw_bwd(gvals, Tp, Tg, valid, weights):
    import ctypes
    from polardepth._lib import lib, check, ptr, stream_ptr
    F, N = len(Tp), Tp[0].shape[0]
    gT = [torch.full((N, 4, 4), float("nan"), device="cuda") for _ in range(F)]
    arr = lambda ts: (ctypes.c_void_p * F)(*[t.data_ptr() for t in ts])
    check(lib.pd_pose_loss_bwd(ptr(gvals), arr(Tp), arr(Tg), F, (ctypes.c_float * F)(*weights), ptr(valid), arr(gT), N,
                               stream_ptr()), "pd_pose_loss_bwd")
    return gT


CASES = [(N, F, 0) for N in (65, 257) for F in (1, 2, 8)] + [(1, 1, b) for b in range(4)] + [(1, 2, 1), (1, 8, 0)]


@pytest.mark.parametrize("N,F,first", CASES)
@pytest.mark.parametrize("masked", [False, True])
def test_forward_and_backward_against_the_statement(N, F, first, masked):
    Tp, Tg = make_case(N, F, first)
    valid = make_valid(N, F, N + F) if masked else None
    weights = L.default_weights(F) if not masked else [0.5 + 0.25 * f for f in range(F)]
    dTp, dTg = [_cu(t) for t in Tp], [_cu(t) for t in Tg]
    dvalid = None if valid is None else _cu(valid)

    vals, rec = raw_fwd(dTp, dTg, dvalid, weights)
    ref_rec = L.pose_records(Tp, Tg)
    err = np.abs(rec.cpu().numpy() - ref_rec).max()
    print("records: max err", err)
    assert err <= 1e-12
    ref_vals = L.pose_loss(Tp, Tg, valid, weights)
    want = ref_vals.astype(np.float32)
    got = vals.cpu().numpy()
    print("vals", got[:3], "err / ulp", (np.abs(got.astype(np.float64) - ref_vals) / np.spacing(np.abs(want)).clip(1e-45)).max())
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert np.isfinite(got).all() and (got[0] > 0 and got[1] > 0)
    if masked and F > 1:
        assert got[3 + 2 * (F - 1)] == 0 and got[4 + 2 * (F - 1)] == 0
    vals2, rec2 = raw_fwd(dTp, dTg, dvalid, weights)
    assert torch.equal(vals2, vals) and torch.equal(rec2, rec)
    vals3, _ = raw_fwd(dTp, dTg, dvalid, weights, records=False)       # the records change nothing in vals
    assert torch.equal(vals3, vals)

    gv = np.array([0.75, -1.25, 1.5], np.float32)
    gT = raw_bwd(_cu(gv), dTp, dTg, dvalid, weights)
    ref_g = L.pose_loss_grad(gv, Tp, Tg, valid, weights)
    for f in range(F):
        got_g, want_g = gT[f].cpu().numpy(), ref_g[f]
        assert (got_g[:, 3] == 0).all()
        big = np.abs(want_g).reshape(N, -1).max(1)[:, None, None]
        e = np.abs(got_g.astype(np.float64) - want_g)
        print("frame", f, "gT: max err / tol", (e / (2.0 ** -22 * np.abs(want_g) + 1e-12 * big + 1e-300)).max())
        assert (e <= 2.0 ** -22 * np.abs(want_g) + 1e-12 * big).all(), f
        if valid is not None:
            assert (got_g[valid[:, f] == 0] == 0).all()
            if (valid[:, f] != 0).any():
                assert np.abs(got_g[valid[:, f] != 0]).max() > 0
    gT2 = raw_bwd(_cu(gv), dTp, dTg, dvalid, weights)
    assert all(torch.equal(a, b) for a, b in zip(gT, gT2))


def test_valid_of_ones_is_no_mask():
    Tp, Tg = make_case(65, 2)
    dTp, dTg = [_cu(t) for t in Tp], [_cu(t) for t in Tg]
    w = L.default_weights(2)
    ones = torch.ones(65, 2, device="cuda")
    a, ra = raw_fwd(dTp, dTg, None, w)
    b, rb = raw_fwd(dTp, dTg, ones, w)
    assert torch.equal(a, b) and torch.equal(ra, rb)
    gv = _cu(np.array([1, 1, 1], np.float32))
    assert all(torch.equal(x, y) for x, y in zip(raw_bwd(gv, dTp, dTg, None, w), raw_bwd(gv, dTp, dTg, ones, w)))


def test_empty_batch_writes_zeros():
    from polardepth import ops
    e = torch.empty(0, 4, 4, device="cuda")
    vals, _ = raw_fwd([e, e], [e, e], None, [2.0, 1.0], records=False)
    assert (vals == 0).all() and vals.numel() == 7
    Tp = e.clone().requires_grad_(True)
    r, t, tot, rec = ops.pose_supervision([Tp], [e], details=True)
    assert r.item() == 0 and t.item() == 0 and tot.item() == 0 and tuple(rec.shape) == (1, 0, 10)
    tot.backward()
    assert tuple(Tp.grad.shape) == (0, 4, 4)


def test_non_finite_input_propagates():
    Tp, Tg = make_case(65, 1)
    Tp[0][5, 0, 0] = np.nan
    Tp[0][6, 1, 3] = np.inf
    vals, rec = raw_fwd([_cu(Tp[0])], [_cu(Tg[0])], None, [1.0])
    rec = rec.cpu().numpy()
    assert np.isnan(rec[0, 5, :3]).all() and np.isnan(rec[0, 5, 6]) and np.isinf(rec[0, 6, 7])
    assert np.isfinite(np.delete(rec[0], (5, 6), 0)).all() and not np.isfinite(vals.cpu().numpy()[:2]).any()
    valid = np.ones((65, 1), np.float32)
    valid[[5, 6]] = 0                                         # masked out: the loss is finite again
    vals, _ = raw_fwd([_cu(Tp[0])], [_cu(Tg[0])], _cu(valid), [1.0])
    assert np.isfinite(vals.cpu().numpy()).all()


def test_pose_supervision_behind_pose_matrix_against_autograd_fp64():
    """axisangle / translation -> ops.pose_matrix -> ops.pose_supervision on the device against pose_ref.torch_matrix ->
    torch_pose_loss in float64 on the CPU: the gradient is rounded to float32 twice on the way (gT, then gaxisangle)."""
    from polardepth import ops
    rng = np.random.default_rng(21)
    N, F = 12, 2
    aa = [rng.uniform(-1.2, 1.2, (N, 1, 3)).astype(np.float32) for _ in range(F)]
    tr = [rng.uniform(-0.2, 0.2, (N, 1, 3)).astype(np.float32) for _ in range(F)]
    Tg = [L.head_matrices(rng, N, 2.0, 0.1) for _ in range(F)]
    valid = np.ones((N, F), np.float32)
    valid[3, 0] = valid[7, 1] = 0
    keep = [valid[:, f] != 0 for f in range(F)]

    da = [_cu(a).requires_grad_(True) for a in aa]
    dt = [_cu(t).requires_grad_(True) for t in tr]
    T = [ops.pose_matrix(da[f], dt[f], invert=bool(f == 0)) for f in range(F)]
    r, t, tot, rec = ops.pose_supervision(T, [_cu(x) for x in Tg], valid=_cu(valid), details=True)
    assert tuple(rec.shape) == (F, N, 10) and not rec.requires_grad and tot.requires_grad
    tot.backward()

    ca = [torch.from_numpy(a).double().requires_grad_(True) for a in aa]
    ct = [torch.from_numpy(x).double().requires_grad_(True) for x in tr]
    cT = [P.torch_matrix(ca[f], ct[f], f == 0)[keep[f]] for f in range(F)]
    # the sub-batch of every frame: the mean over the present items, as the mask gives it
    rr, tt, total = L.torch_pose_loss(cT, [torch.from_numpy(Tg[f][keep[f]]).double() for f in range(F)])
    total.backward()
    np.testing.assert_allclose([r.item(), t.item(), tot.item()], [rr.item(), tt.item(), total.item()], rtol=1e-6)
    for f in range(F):
        for got, want, name in ((da[f].grad, ca[f].grad, "axisangle"), (dt[f].grad, ct[f].grad, "translation")):
            got, want = got.cpu().numpy().astype(np.float64), want.numpy()
            err = np.abs(got - want).max() / np.abs(want).max()
            print("frame", f, name, "relative error", err)
            assert err <= 1e-5, (f, name)
        assert (da[f].grad[~torch.from_numpy(keep[f])] == 0).all()
    # the defaults: no mask, weights [F .. 1]
    with torch.no_grad():
        r2, t2, tot2 = ops.pose_supervision([x.detach() for x in T], [_cu(x) for x in Tg])
    want = L.pose_loss([x.detach().cpu().numpy() for x in T], Tg)
    np.testing.assert_allclose([r2.item(), t2.item(), tot2.item()], want[:3], rtol=2.0 ** -23)
