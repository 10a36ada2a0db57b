"""tests/pose_chain_ref.py (the statement of pd_pose_chain) against what the reference's own Trainer.predict_poses computed
(tests/golden/g16_pose_chain.npz, make_golden_pose_chain.py), against its own definition, and against geometry.  CPU only."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import pose_chain_ref as C
import pose_ref as P

U32 = 2.0 ** -24                     # unit roundoff of float32
F64, F32 = np.float64, np.float32
CASES = ("a", "b")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "g16_pose_chain.npz")))


def _chains(g, case):
    """[(direction, [frame ids of the chain, nearest first])] of a case."""
    ids = [int(i) for i in g[f"{case}_ids"]]
    out = []
    for s in (-1, 1):
        chain = sorted([f for f in ids if f * s > 0], key=abs)
        if chain:
            out.append((s, chain))
    return out


def _present(g, chain):
    return np.stack([g[f"frame_{f}"].reshape(g[f"frame_{f}"].shape[0], -1).sum(1) != 0 for f in chain]).astype(F32)


def _tau(aa, tr, inv):
    """The one-matrix bound of tests/test_pose_ref.py::test_matrices_against_the_reference_float32_ones, per item."""
    t = np.abs(tr.astype(F64))
    M = P.pose_matrix(aa, tr, inv)
    Rt = np.einsum("nki,nk->ni", np.abs(M[:, :3, :3]), t)
    return 12 * U32 * np.maximum(1.0, t.sum(1)) + 4 * U32 * Rt.max(1)


def test_the_fixture_meets_its_conditions(g):
    n_abs, f_abs = (int(v) for v in g["absent"])
    assert not g[f"frame_{f_abs}"][n_abs].any()
    for f in (-3, -2, -1, 0, 1):
        fr = g[f"frame_{f}"]
        assert fr.shape == (4, 3, 8, 12) and fr.dtype == F32
        assert [bool(fr[n].any()) for n in range(4)] == [(n, f) != (n_abs, f_abs) for n in range(4)]
    assert [int(i) for i in g["a_ids"]] == [0, -1, -2, -3] and [int(i) for i in g["b_ids"]] == [0, 1, -1, -2]
    assert f_abs in [int(i) for i in g["a_ids"]][1:-1]                         # absent in mid-chain
    for case in CASES:
        for f in [int(i) for i in g[f"{case}_ids"]][1:]:
            angle = np.linalg.norm(g[f"{case}_aa_{f}"].astype(F64), axis=1)
            assert (angle > 0.05).all() and (angle <= 1.1).all(), (case, f, angle)
            assert (np.linalg.norm(g[f"{case}_tr_{f}"].astype(F64), axis=1) > 1e-2).all(), (case, f)
            # slot 0 of the stub is the stored linear map of the stored means
            o = g[f"{case}_means_{f}"] @ g["map_w"].T + g["map_b"]
            np.testing.assert_allclose(np.concatenate([g[f"{case}_aa_{f}"], g[f"{case}_tr_{f}"]], 1), o, rtol=0, atol=1e-6)


@pytest.mark.parametrize("case", CASES)
def test_chain_against_the_reference_float32_chain(g, case):
    """E_0 = tau_0;  E_k = tau_k |A_{k-1}|_inf + |M_k|_inf E_{k-1} + 5 u max(|M_k| |A_{k-1}|): the link's own matrix error
    against the inherited pose, the inherited error through the link, a four-term float32 dot product (4 u) and our one
    rounding (1 u).  tau_k is the one-matrix bound of tests/test_pose_ref.py; norms are maximum row sums."""
    n_abs, f_abs = (int(v) for v in g["absent"])
    for s, chain in _chains(g, case):
        aa = np.stack([g[f"{case}_aa_{f}"] for f in chain])
        tr = np.stack([g[f"{case}_tr_{f}"] for f in chain])
        present = _present(g, chain)
        rel, rel_inv = C.pose_chain(aa, tr, present, None, s)
        M, _ = C.link_matrices(aa, tr, s)
        E = None
        for k, f in enumerate(chain):
            ref = g[f"{case}_rel_{f}"].astype(F64)
            tau = _tau(aa[k], tr[k], s < 0)
            if k == 0:
                E = tau
            else:
                Aprev = np.abs(rel[k - 1].astype(F64))
                Mk = np.abs(M[k].astype(F64))
                E = tau * Aprev.sum(2).max(1) + Mk.sum(2).max(1) * E + 5 * U32 * (Mk @ Aprev).reshape(-1, 16).max(1)
            err = np.abs(rel[k].astype(F64) - ref).reshape(-1, 16).max(1)
            print(case, "direction", s, "frame", f, "err", err, "bound", E)
            assert (err <= E).all()
            # zeros are zeros exactly where the reference has them, and nowhere else
            zero_ref = ~ref.reshape(-1, 16).any(1)
            zero = ~rel[k].reshape(-1, 16).any(1)
            assert zero.tolist() == zero_ref.tolist() == [s < 0 and n == n_abs and f <= f_abs for n in range(4)]
            E = np.where(zero, 0.0, E)                                          # an exact zero carries no error on
            # relative_pose_inv: the link's own inverse -- one matrix, neither chained nor zeroed
            ref_inv = g[f"{case}_relinv_{f}"].astype(F64)
            Minv = P.pose_matrix(aa[k], tr[k], s > 0)                          # before its rounding, as in that test
            err_inv = np.abs(Minv - ref_inv).reshape(-1, 16).max(1)
            print(case, "frame", f, "err_inv", err_inv, "tau", _tau(aa[k], tr[k], s > 0))
            assert (err_inv <= _tau(aa[k], tr[k], s > 0)).all()
            np.testing.assert_array_equal(rel_inv[k], Minv.astype(F32))        # ... and ours is that matrix rounded once
            assert ref_inv.reshape(-1, 16).any(1).all() and rel_inv[k].reshape(-1, 16).any(1).all()
    assert g[f"{case}_dev"] <= 1e-6


@pytest.mark.parametrize("case", CASES)
def test_recorded_pairing_is_what_matching_poses_documents(g, case):
    """The pose stub saw the six channel means of (fi, fi + 1) for a negative id and of (fi - 1, fi) for a positive one: the
    temporal order polardepth.matching.chain_pairs states and matching_poses uses."""
    from polardepth import matching
    ids = [int(i) for i in g[f"{case}_ids"]]
    pairs = matching.chain_pairs(ids)
    assert list(pairs) == ids[1:]
    for f in ids[1:]:
        first, second = pairs[f]
        assert (first, second) == ((f, f + 1) if f < 0 else (f - 1, f))
        want = np.concatenate([g[f"frame_{first}"].astype(F64).mean((2, 3)), g[f"frame_{second}"].astype(F64).mean((2, 3))], 1)
        np.testing.assert_allclose(g[f"{case}_means_{f}"], want, rtol=0, atol=1e-6)
        swapped = np.concatenate([want[:, 3:], want[:, :3]], 1)
        assert np.abs(g[f"{case}_means_{f}"] - swapped).max() > 1e-2
    for bad in ([0, -2], [0, -1, -3], [0, 2], [0, 1, 3], [-1, 0], [0, -1, -1], [0]):
        with pytest.raises(ValueError):
            matching.chain_pairs(bad)


def _random_links(rng, L, N):
    aa = rng.uniform(-0.4, 0.4, (L, N, 3)).astype(F32)
    tr = rng.uniform(-0.3, 0.3, (L, N, 3)).astype(F32)
    return aa, tr


@pytest.mark.parametrize("direction", [-1, 1])
def test_one_link_without_init_is_the_rounded_pose_matrix(direction):
    aa, tr = _random_links(np.random.default_rng(1), 1, 5)
    rel, rel_inv = C.pose_chain(aa, tr, None, None, direction)
    np.testing.assert_array_equal(rel[0], P.pose_matrix(aa[0], tr[0], direction < 0).astype(F32))
    np.testing.assert_array_equal(rel_inv[0], P.pose_matrix(aa[0], tr[0], direction > 0).astype(F32))


@pytest.mark.parametrize("direction", [-1, 1])
def test_one_call_of_L_links_equals_L_calls_of_one_link(direction):
    rng = np.random.default_rng(2)
    L, N = 4, 6
    aa, tr = _random_links(rng, L, N)
    present = (rng.random((L, N)) > 0.25).astype(F32)
    assert (present == 0).any() and present[-1].any()
    init = P.pose_matrix(*(a[0] for a in _random_links(rng, 1, N)), False).astype(F32)
    for ini in (None, init):
        rel, rel_inv = C.pose_chain(aa, tr, present, ini, direction)
        A = ini
        for k in range(L):
            r1, i1 = C.pose_chain(aa[k:k + 1], tr[k:k + 1], present[k:k + 1], A, direction)
            np.testing.assert_array_equal(r1[0], rel[k])
            np.testing.assert_array_equal(i1[0], rel_inv[k])
            A = r1[0]
        # a zero travels down the chain by arithmetic alone
        gone = np.cumsum(present == 0, 0) > 0
        assert (~rel.reshape(L, N, 16).any(2) == gone).all()


def test_the_chain_returns_the_poses_it_was_derived_from():
    """Random rigid poses P_i (0 -> i) for i = -1 .. -3 and +1; every link's parameters from P_i P_{i -+ 1}^-1: for a past
    link the network's matrix is inverted, M = R(a)^T Trans(-t), so a = -rotvec(R_link) and t = -R_link^T t_link; for a future
    link M = Trans(t) R(a) directly.  The chain gives P_i back to 1e-6, the bound tests/test_pose_ref.py uses for a product
    of two fp32-rounded matrices (the 1e-7 of the axis normalisation dominates): this pins the multiplication order and the
    inversion to geometry, in both directions."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    N = 5

    def rigid():
        T = np.tile(np.eye(4), (N, 1, 1))
        T[:, :3, :3] = Rotation.from_rotvec(rng.uniform(-0.3, 0.3, (N, 3))).as_matrix()
        T[:, :3, 3] = rng.uniform(-0.2, 0.2, (N, 3))
        return T

    pose = {0: np.tile(np.eye(4), (N, 1, 1)), -1: rigid(), -2: rigid(), -3: rigid(), 1: rigid()}
    for s, chain in ((-1, [-1, -2, -3]), (1, [1])):
        aa, tr = [], []
        for f in chain:
            link = pose[f] @ np.linalg.inv(pose[f - s])
            Rl, tl = link[:, :3, :3], link[:, :3, 3]
            rv = Rotation.from_matrix(Rl).as_rotvec()
            if s < 0:
                aa.append(-rv)
                tr.append(-np.einsum("nki,nk->ni", Rl, tl))
            else:
                aa.append(rv)
                tr.append(tl)
        rel, rel_inv = C.pose_chain(np.stack(aa).astype(F32), np.stack(tr).astype(F32), None, None, s)
        for k, f in enumerate(chain):
            err = np.abs(rel[k].astype(F64) - pose[f]).max()
            print("direction", s, "frame", f, "err", err)
            assert err <= 1e-6
            link = pose[f] @ np.linalg.inv(pose[f - s])
            assert np.abs(rel_inv[k].astype(F64) - np.linalg.inv(link)).max() <= 1e-6
