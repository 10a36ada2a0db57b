"""The NumPy statement of pd_depth_consistency (tests/consistency_ref.py) against independent statements (no GPU): its forward
leg against reproj_ref.project (pinned to the reference by g12_reproj.npz), its return leg against a dense fp64 inverse, two
views of an analytic plane, the counter identity, and what `visible` and `frame_valid` move."""
import numpy as np

import consistency_ref as C
import reproj_ref

N, F, H, W = 2, 2, 21, 34
CLASSES = [(1, 0), (20, 160), (40, 40), (500, 600)]


def _scene(seed=3, big_last=True):
    return C.plane_pair(N, F, H, W, seed, big_last=big_last)


def _mask(seed=5):
    return (np.random.default_rng(seed).integers(0, 11, (N, H, W)) * 20).astype(np.int32)


def test_forward_leg_agrees_with_the_reprojection_statement():
    depth0, _, T, K, inv_K = _scene()
    for f in range(F):
        uv, hz, _ = reproj_ref.project(depth0[:, None], K, inv_K, T[:, f])
        for n in range(N):
            u, v, z = C.forward_leg(depth0[n], K[n], inv_K[n], T[n, f])
            assert np.abs(u - uv[n, ..., 0]).max() <= 1e-9 and np.abs(v - uv[n, ..., 1]).max() <= 1e-9
            assert np.abs(z - hz[n]).max() <= 1e-9


def test_return_leg_agrees_with_a_dense_inverse():
    """On motions that are rigid to fp64 precision (the statement widens whatever it is given): the rigid inverse is then the
    inverse, and the two statements differ by rounding alone.  A T stored in fp32 is a rotation only to 6e-8; its rigid
    inverse differs from its dense inverse by that much (the last assertion), about 1e-6 px after the projection -- a
    property of the definition, which the device shares."""
    depth0, depths, T32, K, inv_K = _scene()
    rng = np.random.default_rng(11)
    for n in range(N):
        for f in range(F):
            uf = rng.uniform(0, W - 1, (H, W)).astype(np.float32)
            vf = rng.uniform(0, H - 1, (H, W)).astype(np.float32)
            d1 = rng.uniform(0.3, 1.8, (H, W)).astype(np.float32)
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = C.rot(rng.uniform(-0.2, 0.2, 3)), rng.uniform(-0.1, 0.1, 3)
            u2, v2, hz2 = C.return_leg(uf, vf, d1, K[n], inv_K[n], T)
            K64, iK64, Ti = K[n].astype(np.float64), inv_K[n].astype(np.float64), np.linalg.inv(T)
            pix = np.stack([uf.astype(np.float64), vf.astype(np.float64), np.ones((H, W))], -1)
            X = d1.astype(np.float64)[..., None] * np.einsum("ij,hwj->hwi", iK64[:3, :3], pix)
            Xh = np.concatenate([X, np.ones((H, W, 1))], -1)
            h = np.einsum("ij,hwj->hwi", (K64 @ Ti)[:3], Xh)
            z = h[..., 2] + 1e-7
            assert np.abs(u2 - h[..., 0] / z).max() <= 1e-9 and np.abs(v2 - h[..., 1] / z).max() <= 1e-9
            assert np.abs(hz2 - z).max() <= 1e-9
            assert np.abs(C.rigid_inverse(T) - Ti).max() <= 1e-12
            d32 = np.abs(C.rigid_inverse(T32[n, f]) - np.linalg.inv(T32[n, f].astype(np.float64))).max()
            assert d32 <= 1e-6, d32


def test_two_views_of_a_plane_are_tight():
    depth0, depths, T, K, inv_K = _scene(big_last=False)
    r = C.consistency(depth0, depths, T, K, inv_K)
    cmp_ = r["outcome"] == C.COMPARED
    assert cmp_.sum() > 0.8 * cmp_.size
    assert (r["level"][cmp_] == 4).all()
    assert r["e_rel"][cmp_].max() < 1e-4
    assert (r["outcome"][~cmp_] == C.OUTSIDE).all()                         # nothing else can happen to a clean plane
    assert (r["counters"][:, 0, 0] == r["n"][:, 0]).all() and (r["counters"][:, 0, 2] == r["n"][:, 0]).all()
    # every view is tight: fused averages F + 1 depths of the same surface
    full = r["n_cons"] == F
    assert full.any() and np.abs(r["fused"][full] - depth0[full]).max() < 1e-4


def _noisy():
    depth0, depths, T, K, inv_K = _scene()
    rng = np.random.default_rng(17)
    depths = depths * rng.choice(np.float32([1, 1.005, 0.985, 1.03, 0.9, 1.3]), depths.shape).astype(np.float32)
    depth0 = depth0.copy()
    depth0[rng.random(depth0.shape) < 0.05] = 0
    depths[rng.random(depths.shape) < 0.05] = 0
    depth0[0, 1, 1], depth0[1, 2, 2], depths[0, 0, 3, 3] = np.nan, 2.5, np.inf
    return depth0, depths, T, K, inv_K


def test_the_counter_identity_holds_for_every_class():
    depth0, depths, T, K, inv_K = _noisy()
    mask = _mask()
    fv = np.float32([[1, 0], [1, 1]])
    r = C.consistency(depth0, depths, T, K, inv_K, frame_valid=fv, mask=mask, classes=CLASSES)
    assert (r["n"] + r["counters"][..., 3:].sum(-1) == r["pixels"] * F).all()
    assert (r["pixels"][:, 0] == H * W).all() and (r["pixels"][:, 3] == 0).all() and (r["n"][:, 1] > 0).all()
    assert (r["hist"].sum(-1) == r["n"]).all()
    c = r["counters"]
    assert (c[..., 0] >= c[..., 1]).all() and (c[..., 1] >= c[..., 2]).all() and (r["n"] >= c[..., 0]).all()
    for name in ("invalid", "absent", "outside", "hole"):
        assert c[:, 0, C.COUNTERS.index(name)].sum() > 0, name
    assert set(np.unique(r["level"])) == {0, 1, 2, 3, 4}
    assert (r["n_cons"][~C.in_range(depth0, 0.1, 2.0)] == 0).all() and (r["fused"][~C.in_range(depth0, 0.1, 2.0)] == 0).all()


def test_a_visible_mask_from_the_call_itself_moves_exactly_the_other_pairs_to_filtered():
    depth0, depths, T, K, inv_K = _noisy()
    a = C.consistency(depth0, depths, T, K, inv_K)
    vis = a["level"] >= 3
    b = C.consistency(depth0, depths, T, K, inv_K, visible=vis.astype(np.uint8))
    kept = vis                                                               # compared before, and compared now
    assert (b["outcome"][kept] == C.COMPARED).all() and np.array_equal(b["level"][kept], a["level"][kept])
    inv = a["outcome"] == C.INVALID
    assert (b["outcome"][inv] == C.INVALID).all()                            # invalid is tested first
    moved = ~kept & ~inv
    assert (b["outcome"][moved] == C.FILTERED).all() and (b["level"][moved] == 0).all()
    assert b["counters"][:, 0, 5].sum() == moved.sum() and a["counters"][:, 0, 5].sum() == 0
    assert (b["n"] == b["counters"][..., 1]).all()                          # everyone left meets the mid level


def test_frame_valid_zero_moves_a_whole_view_to_absent():
    depth0, depths, T, K, inv_K = _noisy()
    fv = np.float32([[1, 1], [0, 1]])
    a = C.consistency(depth0, depths, T, K, inv_K)
    b = C.consistency(depth0, depths, T, K, inv_K, frame_valid=fv)
    inv = a["outcome"][1, 0] == C.INVALID
    assert (b["outcome"][1, 0][~inv] == C.ABSENT).all() and (b["outcome"][1, 0][inv] == C.INVALID).all()
    assert (b["level"][1, 0] == 0).all()
    for n, f in ((0, 0), (0, 1), (1, 1)):
        assert np.array_equal(a["outcome"][n, f], b["outcome"][n, f]) and np.array_equal(a["level"][n, f], b["level"][n, f])
    assert b["counters"][1, 0, 4] == (~inv).sum() and b["counters"][0, 0, 4] == 0
