"""pd_backproject / pd_cloud_nn / pd_cloud_stats on the GPU against the NumPy statement (tests/pointcloud_ref.py, pinned by
tests/test_pointcloud_ref.py).

Back-projection: x and y within 4 * 2^-24 relative of the fp64 pinhole model (a subtraction, a division and a product, each
within 2^-24, with half an ulp to spare), z and the w pattern equal, boxes exactly the min / max / count of the kernel's own
points.  Nearest neighbour: np.array_equal with the statement on the kernel's own clouds, NaN and inf patterns included -- a
minimum of float32 terms has one value, whatever the tiles and whatever is pruned.  Records: integer fields and patterns
equal; sum_d / sum_d2 rtol 1e-11 (any order of n exactly converted terms errs by at most (n - 1) 2^-53 of the sum, 7e-13 at
the 6144 pixels of the largest image here, and both sides take a correctly rounded fp64 square root: the bound argued in
tests/test_normals_stats_gpu.py); dist within one float32 ulp."""
import functools

import numpy as np
import pytest
import torch

import pointcloud_ref as R

pytestmark = pytest.mark.gpu

# one partial tile, less than a wave of points | 3 x 5 tiles, partial on both edges | 4 x 6 full tiles
SHAPES = [(2, 5, 7), (3, 33, 70), (4, 64, 96)]
MIN_D, MAX_D = 0.1, 2.0
EPS = 2.0 ** -24


def PC():
    from polardepth import pointcloud
    return pointcloud


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a writable C-ordered copy: the scene arrays are read-only


def _classes(K):
    pc = PC()
    if K == 1:
        return [("all", None)]
    if K == 12:
        return list(pc.DEFAULT_CLASSES)
    assert K == 16
    return list(pc.DEFAULT_CLASSES) + [("a", (40, 60)), ("b", (0, 0)), ("none", (500, 600)), ("every", (-5, 1000))]


def _lohi(classes):
    return [(1, 0) if r is None else tuple(r) for _, r in classes]


@functools.lru_cache(maxsize=None)
def scene(N, H, W):
    """Host arrays (never modified): a smooth true depth with holes, NaN, zero and out-of-range values, a prediction = the
    truth with 1 % noise, depth spikes and its own zero / NaN / negative / infinite values, intrinsics with fx != fy, a mask
    of grey values.  From three images on, the last image's prediction is NaN everywhere (an empty predicted cloud); the
    largest shape has a whole 16x16 tile of holes."""
    rng = np.random.default_rng(2000 * N + H + W)
    ys, xs = np.mgrid[0:H, 0:W]
    gt = (1.0 + 0.3 * np.sin(xs / 9.0 + np.arange(N)[:, None, None]) + 0.2 * np.cos(ys / 7.0)).astype(np.float32)
    gt[:, 1, 2] = 0.0
    gt[0, 0, 0] = 0.0
    gt[-1, H - 1, W - 2] = np.nan
    gt[0, 3, 4] = 2.5
    if H > 8:
        gt[:, H // 2, ::9] = 0.0                     # a dotted line of holes
        gt[:, :, W - 1][:, ::7] = 3.0                # out of range on the right border
    if H >= 32 and W >= 48:
        gt[1, 16:32, 32:48] = 0.0                    # a whole tile of holes
    pred = (gt * (1.0 + 0.01 * rng.normal(size=gt.shape))).astype(np.float32)
    spikes = rng.uniform(size=gt.shape) < 0.01
    pred[spikes] *= np.float32(1.5)
    pred[0, 2, 3], pred[0, 4, 5], pred[0, 4, 6], pred[-1, 0, 1] = 0.0, np.nan, np.inf, -0.5
    if N >= 3:
        pred[-1] = np.nan
    Kmat = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    Kmat[:, 0, 0], Kmat[:, 1, 1], Kmat[:, 0, 2], Kmat[:, 1, 2] = 0.58 * W, 1.92 * H, 0.5 * W - 0.25, 0.5 * H + 0.125
    mask = (rng.integers(0, 11, (N, H, W)) * 20).astype(np.int32)
    for a in (gt, pred, Kmat, mask):
        a.setflags(write=False)
    return gt, pred, Kmat, mask


def _host(cloud):
    torch.cuda.synchronize()
    return cloud.points.cpu().numpy(), cloud.boxes.cpu().numpy()


@functools.lru_cache(maxsize=None)
def clouds(N, H, W):
    """The kernel's own clouds of the scene, both gated by the truth, and the statement's distances both ways (computed
    once, never modified)."""
    pc = PC()
    gt, pred, Kmat, _ = scene(N, H, W)
    p = pc.backproject(_dev(pred), _dev(Kmat), gate=_dev(gt), min_depth=MIN_D, max_depth=MAX_D)
    t = pc.backproject(_dev(gt), _dev(Kmat), min_depth=MIN_D, max_depth=MAX_D)
    pp, _ = _host(p)
    tp, _ = _host(t)
    acc, comp = R.nn_d2(pp, tp), R.nn_d2(tp, pp)
    for a in (pp, tp, acc, comp):
        a.setflags(write=False)
    return p, t, pp, tp, acc, comp


def cloud_from_host(points, H=None, W=None):
    """A device ``Cloud`` of host points [N, T*256, 4], with the statement's boxes."""
    lo, hi, n = R.boxes_of(points)
    return PC().Cloud(_dev(points), _dev(R.pack_boxes(lo, hi, n)), H, W)


def nn(query, target, prune):
    d2, seen = PC().nearest(query, target, prune=prune, visited=True)
    torch.cuda.synchronize()
    return d2.cpu().numpy(), seen.cpu().numpy()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_backprojection_against_fp64(shape, gated):
    pc = PC()
    gt, pred, Kmat, _ = scene(*shape)
    N, H, W = shape
    cloud = pc.backproject(_dev(pred), _dev(Kmat), gate=_dev(gt) if gated else None, min_depth=MIN_D, max_depth=MAX_D)
    pts, boxes = _host(cloud)
    T = R.tiles_of(H, W)
    assert pts.shape == (N, T * 256, 4) and boxes.shape == (N, T, 8) and cloud.tiles == T
    ref = R.backproject(pred, Kmat, gt if gated else None, MIN_D, MAX_D, dtype=np.float64)
    assert np.array_equal(pts[..., 3], ref[..., 3])
    assert set(np.unique(pts[..., 3])) <= {-1.0, 0.0, 1.0} and (pts[..., 3] == 1).any()
    if gated:
        assert (pts[..., 3] == -1).any()
    else:
        assert not (pts[..., 3] == -1).any()             # its own gate never passes a depth that is not a point
    assert (pts[pts[..., 3] != 1] == np.array([0, 0, 0, 1], np.float32) * pts[pts[..., 3] != 1]).all()      # x = y = z = 0
    is_pt = pts[..., 3] == 1
    assert np.array_equal(pts[..., 2][is_pt], ref[..., 2][is_pt].astype(np.float32))      # z: copied
    for c in (0, 1):
        err = np.abs(pts[..., c][is_pt].astype(np.float64) - ref[..., c][is_pt])
        rel = err / np.maximum(np.abs(ref[..., c][is_pt]), 1e-300)
        print(shape, "gated" if gated else "own gate", "xy"[c], "max rel err", rel.max(), "bound", 4 * EPS)
        assert (err <= 4 * EPS * np.abs(ref[..., c][is_pt])).all()
    lo, hi, n = R.boxes_of(pts)
    assert np.array_equal(boxes[..., 0:3], lo) and np.array_equal(boxes[..., 3:6], hi)
    assert np.array_equal(boxes.view(np.int32)[..., 6], n) and (boxes.view(np.int32)[..., 7] == 0).all()
    assert np.array_equal(cloud.counts.cpu().numpy(), n)
    # the float32 statement repeats the kernel's three operations: the same bits
    assert np.array_equal(pts, R.backproject(pred, Kmat, gt if gated else None, MIN_D, MAX_D), equal_nan=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_nearest_neighbour_equals_the_statement_pruned_and_brute(shape):
    p, t, pp, tp, acc, comp = clouds(*shape)
    T = p.tiles
    for what, q, tg, ref in (("accuracy", p, t, acc), ("completeness", t, p, comp)):
        pruned, seen_p = nn(q, tg, True)
        brute, seen_b = nn(q, tg, False)
        assert same(pruned, brute), what
        assert same(pruned, ref), what
        assert (seen_b == T).all() and (seen_p <= T).all(), what
        qp = pp if q is p else tp
        assert np.array_equal(np.isnan(pruned), qp[..., 3] != 1), what
    if shape[0] >= 3:                                     # the last image's predicted cloud is empty
        assert (pp[-1, :, 3] != 1).all() and np.isposinf(comp[-1][tp[-1, :, 3] == 1]).all()
        assert np.isnan(acc[-1]).all()


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_any_partition_into_tiles_gives_the_same_distances(shape):
    """The same clouds with their slots permuted at random: the boxes are loose (each covers most of the cloud), little can
    be pruned, and every point keeps its distance."""
    p, t, pp, tp, acc, comp = clouds(*shape)
    rng = np.random.default_rng(5)
    S = pp.shape[1]
    perm_q, perm_t = rng.permutation(S), rng.permutation(S)
    q2, t2 = cloud_from_host(pp[:, perm_q]), cloud_from_host(tp[:, perm_t])
    for prune in (True, False):
        got, _ = nn(q2, t2, prune)
        assert same(got, acc[:, perm_q]), prune
        got, _ = nn(q2, t, prune)                         # loose queries against tight targets, and the reverse
        assert same(got, acc[:, perm_q]), prune
        got, _ = nn(p, t2, prune)
        assert same(got, acc), prune


def test_query_and_target_of_different_tile_counts():
    N, H, W = SHAPES[1]
    p, t, pp, tp, acc, comp = clouds(N, H, W)
    rng = np.random.default_rng(6)
    T = p.tiles
    extra = np.zeros((N, 3 * 256, 4), np.float32)         # an empty tile, a sparse tile near the cloud, a full tile far off
    extra[:, 256:256 + 40, :3] = tp[:, 100:140, :3] + np.float32(0.002)
    extra[:, 256:256 + 40, 3] = (tp[:, 100:140, 3] == 1)
    extra[:, 256:256 + 40, :3] *= extra[:, 256:256 + 40, 3:4]
    extra[:, 512:, :3] = rng.uniform(5, 6, (N, 256, 3)).astype(np.float32)
    extra[:, 512:, 3] = 1
    big = np.concatenate([tp[:, :5 * 256], extra, tp[:, 5 * 256:]], 1)      # the same-index tiles no longer correspond
    small = pp[:, 4 * 256:9 * 256]
    cb, cs = cloud_from_host(big), cloud_from_host(small)
    assert cb.tiles == T + 3 and cs.tiles == 5
    for q, tg, qh, th in ((cs, cb, small, big), (cb, cs, big, small), (p, cb, pp, big), (cb, p, big, pp)):
        ref = R.nn_d2(qh, th)
        pruned, seen_p = nn(q, tg, True)
        brute, seen_b = nn(q, tg, False)
        assert same(pruned, ref) and same(brute, ref)
        assert (seen_b == tg.tiles).all() and seen_p.shape == (N, q.tiles)
        assert (seen_p >= R.necessary_tiles(qh, th, ref)).all()


def test_degenerate_clouds():
    pc = PC()
    N, H, W = SHAPES[2]
    p, t, pp, tp, acc, comp = clouds(N, H, W)
    T = t.tiles
    # identical clouds: every point is its own neighbour
    for prune in (True, False):
        got, _ = nn(t, t, prune)
        assert (got[tp[..., 3] == 1] == 0).all() and np.isnan(got[tp[..., 3] != 1]).all()
    # a whole tile of holes: no point in either cloud, NaN for its 256 slots, and as a target it is never scanned
    hole = 1 * 6 + 2
    assert (tp[1, hole * 256:(hole + 1) * 256, 3] == 0).all() and (pp[1, hole * 256:(hole + 1) * 256, 3] == 0).all()
    got, seen = nn(p, t, True)
    assert np.isnan(got[1, hole * 256:(hole + 1) * 256]).all() and seen[1, hole] == 0
    assert (seen[1] <= T - 1).all()
    # image 0 of the target empty: +inf for every query point of that image, the other images as before
    empty = tp.copy()
    empty[0] = 0
    ce = cloud_from_host(empty)
    for prune in (True, False):
        got, seen = nn(p, ce, prune)
        assert np.isposinf(got[0][pp[0, :, 3] == 1]).all() and np.isnan(got[0][pp[0, :, 3] != 1]).all()
        assert same(got[1:], acc[1:])
        assert (seen[0] == (0 if prune else T)).all()
    # an image with no query point: NaN everywhere; the pruned route scans nothing for it
    for prune in (True, False):
        got, seen = nn(ce, p, prune)
        assert np.isnan(got[0]).all() and (seen[0] == (0 if prune else T)).all()
        assert same(got[1:], comp[1:])
    # the empty depth map through the whole Python layer
    gt, pred, Kmat, mask = scene(N, H, W)
    none = pc.backproject(_dev(np.zeros_like(gt)), _dev(Kmat))
    pts, boxes = _host(none)
    assert (pts == 0).all() and np.isposinf(boxes[..., 0:3]).all() and np.isneginf(boxes[..., 3:6]).all()
    assert (boxes.view(np.int32)[..., 6:8] == 0).all()


def _plane(depth):
    N, H, W = 1, 64, 96
    Kmat = np.eye(4, dtype=np.float32)[None].copy()
    Kmat[0, 0, 0] = Kmat[0, 1, 1] = 60.0
    Kmat[0, 0, 2], Kmat[0, 1, 2] = 48.0, 32.0
    return PC().backproject(_dev(np.full((N, H, W), depth, np.float32)), _dev(Kmat), min_depth=MIN_D, max_depth=MAX_D)


def test_visited_tiles():
    """The brute route reports Tt; the pruned route at least the tiles it cannot avoid (boxd2 <= the final R), and on a plane
    -- neighbouring tile boxes about 16 mm apart, R about 1.3 mm -- at most two, the necessary count being one."""
    for shape in SHAPES:
        p, t, pp, tp, acc, comp = clouds(*shape)
        for q, tg, qh, th, ref in ((p, t, pp, tp, acc), (t, p, tp, pp, comp)):
            _, seen_p = nn(q, tg, True)
            _, seen_b = nn(q, tg, False)
            need = R.necessary_tiles(qh, th, ref)
            print(shape, "visited mean", seen_p.mean(), "necessary mean", need.mean(), "of", tg.tiles)
            assert (seen_b == tg.tiles).all()
            assert (seen_p >= need).all() and (seen_p <= tg.tiles).all()
    true, pred = _plane(1.0), _plane(1.001)
    th, _ = _host(true)
    ph, _ = _host(pred)
    assert true.tiles == 24 and (th[..., 3] == 1).all()
    got, seen = nn(pred, true, True)
    ref = R.nn_d2(ph, th)
    assert same(got, ref)
    print("plane: R (mm)", np.sqrt(ref.reshape(24, 256).max(1)) * 1e3)
    need = R.necessary_tiles(ph, th, ref)
    assert (need == 1).all() and need.shape == (1, 24)
    print("plane: visited", seen)
    assert (seen >= 1).all() and (seen <= 2).all()
    # two clouds 100 m apart, the target's slots shuffled: every target box spans the cloud, boxd2 = 100^2 <= every d2, and
    # nothing can be pruned
    rng = np.random.default_rng(7)
    far = th[:, rng.permutation(th.shape[1])].copy()
    far[..., 2] += np.float32(100.0)
    cf = cloud_from_host(far)
    ref = R.nn_d2(th, far)
    assert (R.necessary_tiles(th, far, ref) == 24).all()
    for prune in (True, False):
        got, seen = nn(true, cf, prune)
        assert same(got, ref) and (seen == 24).all()


def _fields(records, dist):
    torch.cuda.synchronize()
    pc = PC()
    d = pc._Direction(records)
    return {"n": d.n.cpu().numpy(), "bad": d.bad.cpu().numpy(), "unmatched": d.unmatched.cpu().numpy(),
            "sum_d": d.sum_d.cpu().numpy(), "sum_d2": d.sum_d2.cpu().numpy(), "hist": d.hist.cpu().numpy().astype(np.int64),
            "dist": None if dist is None else dist.cpu().numpy(), "zero": records.view(torch.int64)[..., 5].cpu().numpy()}


def _compare(got, ref, what):
    for k in ("n", "bad", "unmatched", "hist"):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k] if k != "hist" else None, ref[k] if k != "hist" else None)
    assert np.array_equal(got["n"], got["hist"].sum(-1)) and (got["zero"] == 0).all(), what
    for k in ("sum_d", "sum_d2"):
        rel = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300)
        print(what, k, "max rel err", rel.max())
        assert np.allclose(got[k], ref[k], rtol=1e-11, atol=0.0), (what, k, rel.max())
    if got["dist"] is not None:
        assert np.array_equal(np.isnan(got["dist"]), np.isnan(ref["dist"])), what
        assert np.array_equal(np.isposinf(got["dist"]), np.isposinf(ref["dist"])), what
        ok = np.isfinite(ref["dist"])
        r32 = ref["dist"][ok].astype(np.float32)
        d = np.abs(got["dist"][ok].astype(np.float64) - ref["dist"][ok])
        print(what, "dist max err in ulp", (d / np.spacing(r32)).max() if d.size else 0.0)
        assert (d <= np.spacing(r32)).all(), what


@pytest.mark.parametrize("K,with_mask", [(1, True), (12, True), (16, True), (1, False), (16, False)])
@pytest.mark.parametrize("shape", SHAPES)
def test_records_equal_the_statement(shape, K, with_mask):
    pc = PC()
    N, H, W = shape
    gt, pred, Kmat, mask = scene(*shape)
    p, t, pp, tp, acc, comp = clouds(*shape)
    classes = _classes(K) if with_mask else [(f"c{k}", None) for k in range(K)]
    m = _dev(mask) if with_mask else None
    edges = pc.edges2_numpy()
    for what, q, tg, qh in (("accuracy", p, t, pp), ("completeness", t, p, tp)):
        d2 = pc.nearest(q, tg)
        rec, dist = pc.direction_stats(d2, q, m, classes, dist_map=True)
        got = _fields(rec, dist)
        ref = R.stats(d2.cpu().numpy(), qh, mask if with_mask else None, _lohi(classes), edges, H, W)
        _compare(got, ref, (shape, K, with_mask, what))
        assert got["n"][:, 0].sum() > 0
        rec2, none = pc.direction_stats(d2, q, m, classes)
        torch.cuda.synchronize()
        assert none is None and torch.equal(rec, rec2)                     # two calls: identical record bytes
    if shape[0] >= 3 and K != 12:
        assert got["unmatched"][-1, 0] > 0                                 # completeness of the image without a prediction


def test_cloud_stats_wires_both_directions():
    pc = PC()
    shape = SHAPES[2]
    N, H, W = shape
    gt, pred, Kmat, mask = scene(*shape)
    p, t, pp, tp, acc, comp = clouds(*shape)
    st = pc.cloud_stats(_dev(pred)[:, None], _dev(gt)[:, None], _dev(Kmat), mask=_dev(mask)[:, None], dist_map=True)
    slow = pc.cloud_stats(_dev(pred), _dev(gt), _dev(Kmat), mask=_dev(mask), prune=False)
    torch.cuda.synchronize()
    assert torch.equal(st.acc.records, slow.acc.records) and torch.equal(st.comp.records, slow.comp.records)
    lohi, edges = _lohi(pc.DEFAULT_CLASSES), pc.edges2_numpy()
    _compare(_fields(st.acc.records, st.dist_acc), R.stats(acc, pp, mask, lohi, edges, H, W), "cloud_stats accuracy")
    _compare(_fields(st.comp.records, st.dist_comp), R.stats(comp, tp, mask, lohi, edges, H, W), "cloud_stats completeness")
    m = st.metrics().cpu().numpy()
    assert m.shape == (N, 12, 9) and st.names[0] == "all"
    assert np.allclose(m[:3, 0, 2], m[:3, 0, 0] + m[:3, 0, 1]) and (m[:3, 0, 5:8] > 0).all() and (m[:3, 0, 5:8] <= 1).all()
    assert np.isnan(m[3, 0, 0]) and m[3, 0, 8] == 0                        # the image without a prediction
    assert (m[3, 0, 5:8] == 0).all() or np.isnan(m[3, 0, 5:8]).all()
    P, Rc = st.shares()
    assert P.shape == (N, 12, 3) and (Rc[3, 0] == 0).all()                 # nothing of that image's truth is recalled
    pooled = st.pooled().cpu().numpy()
    st += slow
    twice = st.pooled().cpu().numpy()
    assert pooled.shape == (12, 9) and np.allclose(twice[:, :8], pooled[:, :8], rtol=1e-12, equal_nan=True)
    assert np.array_equal(twice[:, 8], 2 * pooled[:, 8])
    assert int(st.pooled_bad()[0]) == 2 * int(slow.acc.bad[:, 0].sum()) > 0
    assert int(st.pooled_unmatched()[0]) == 2 * int(slow.comp.unmatched[:, 0].sum()) > 0
