"""Pins the NumPy statement of the point-cloud kernels (tests/pointcloud_ref.py) and the host formulas of
polardepth.pointcloud (no GPU): the float32 nearest-neighbour distance against fp64, the box lower bound that makes the
pruning exact, the report's formulas against plain NumPy, the PLY writer and the edge table."""
import numpy as np
import torch

import pointcloud_ref as R
from polardepth import pointcloud as PC

EPS = 2.0 ** -24


def _cloud(rng, n_slots, scale=1.0, holes=0.2):
    p = np.zeros((1, n_slots, 4), np.float32)
    p[0, :, :3] = (rng.uniform(-1, 1, (n_slots, 3)) * scale).astype(np.float32)
    p[0, :, 3] = np.where(rng.uniform(size=n_slots) < holes, rng.choice([0.0, -1.0], n_slots), 1.0)
    p[0, p[0, :, 3] != 1, :3] = 0
    return p


def test_nn_d2_is_within_six_roundings_of_fp64():
    """Three subtractions, three squares and two additions of non-negative terms, each within 2^-24: the float32 minimum is
    within 6 * 2^-24 (relative) of the fp64 minimum over the same float32 points."""
    rng = np.random.default_rng(0)
    for n_q, n_t, scale in ((256, 512, 1.0), (512, 256, 1e-2), (256, 768, 50.0)):
        q, t = _cloud(rng, n_q, scale), _cloud(rng, n_t, scale)
        got = R.nn_d2(q, t, chunk=100)
        isq, ist = q[0, :, 3] == 1, t[0, :, 3] == 1
        assert np.array_equal(np.isnan(got[0]), ~isq)
        d = q[0][isq][:, None, :3].astype(np.float64) - t[0][ist][None, :, :3].astype(np.float64)
        want = (d * d).sum(-1).min(1)
        rel = np.abs(got[0, isq].astype(np.float64) - want) / want
        print("max rel err", rel.max(), "bound", 6 * EPS)
        assert (rel <= 6 * EPS).all()
    empty = _cloud(rng, 256)
    empty[0, :, 3] = 0
    got = R.nn_d2(q, empty)
    assert np.array_equal(np.isposinf(got[0]), isq) and np.array_equal(np.isnan(got[0]), ~isq)


def _box_pairs(rng):
    """(points_a [m,3], points_b [m,3]) float32 pairs of point sets; the boxes are their bounding boxes."""
    for scale in (1e-3, 1.0, 1e3):
        for _ in range(40):                       # random boxes: apart, overlapping, nested
            ca, cb = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
            ra, rb = rng.uniform(0, 0.7, 3), rng.uniform(0, 0.7, 3)
            a = ((ca + rng.uniform(-1, 1, (24, 3)) * ra) * scale).astype(np.float32)
            b = ((cb + rng.uniform(-1, 1, (24, 3)) * rb) * scale).astype(np.float32)
            yield a, b
        # touching: b starts exactly where a ends; and one ulp apart / one ulp inside, per axis
        a = (rng.uniform(0, 1, (24, 3)) * scale).astype(np.float32)
        edge = a.max(0)
        for shift in (edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))):
            b = (shift + rng.uniform(0, 1, (24, 3)).astype(np.float32) * np.float32(scale)).astype(np.float32)
            b[0] = shift                          # a corner of b sits on the shifted edge itself
            yield a, b
            for ax in range(3):                   # apart along one axis only, overlapping along the others
                b2 = a.copy()
                b2[:, ax] = b[:, ax]
                yield a, b2
        # values that differ in the last bit only
        base = (rng.uniform(0.5, 1, (24, 3)) * scale).astype(np.float32)
        up = np.nextafter(base, np.float32(np.inf))
        yield base, up
        yield base, np.nextafter(up, np.float32(np.inf))
        yield base[:1], up[:1]                    # two single points one ulp apart: the boxes ARE the points


def test_box_distance_is_a_lower_bound_of_the_computed_distance():
    """float32 boxd2 <= the float32 d2 of EVERY pair drawn from the two boxes, with no exception: rounding is monotone, and
    boxd2 repeats the operation order of the point distance.  This is what lets the pruned route equal the brute one bit for
    bit."""
    rng = np.random.default_rng(1)
    n = 0
    for a, b in _box_pairs(rng):
        for q, t in ((a, b), (b, a)):
            bd = R.boxd2(q.min(0), q.max(0), t.min(0), t.max(0))
            d2 = R.pair_d2(q[:, None, :], t[None, :, :])
            assert bd <= d2.min(), (bd, d2.min(), q.min(0), q.max(0), t.min(0), t.max(0))
            n += 1
    assert n > 300
    # overlapping boxes bound nothing (0); an empty box (lo = +inf, hi = -inf) gives +inf, never NaN <= R
    z = np.zeros(3, np.float32)
    assert R.boxd2(z, z + 1, z + 0.5, z + 2) == 0
    inf = np.full(3, np.inf, np.float32)
    assert np.isposinf(R.boxd2(z, z + 1, inf, -inf))


def test_tiling_boxes_and_necessary_tiles():
    rng = np.random.default_rng(2)
    H, W = 20, 37
    assert R.tiles_of(H, W) == 2 * 3 == PC.tiles_of(H, W) and R.tiles_of(320, 480) == 600 and R.tiles_of(512, 640) == 1280
    depth = rng.uniform(0.3, 1.8, (1, H, W)).astype(np.float32)
    depth[0, 0, 0], depth[0, 1, 1], depth[0, 2, 2], depth[0, 3, 3] = 0.0, np.nan, 2.5, 0.05
    gate = np.full((1, H, W), 1.0, np.float32)
    gate[0, 5, 5] = 0.0
    Km = np.eye(4, dtype=np.float32)[None].copy()
    Km[0, 0, 0], Km[0, 1, 1], Km[0, 0, 2], Km[0, 1, 2] = 30.0, 40.0, 18.0, 10.0
    own = R.backproject(depth, Km, None, 0.1, 2.0)
    v, u, inside = R.slot_pixels(H, W)
    w = np.zeros((H, W))
    w[v[inside], u[inside]] = own[0, inside, 3]
    assert (own[0, ~inside] == 0).all() and inside.sum() == H * W
    assert w[0, 0] == 0 and w[1, 1] == 0 and w[2, 2] == 0 and w[3, 3] == 0 and w[4, 4] == 1      # own gate: never bad
    gated = R.backproject(depth, Km, gate, 0.1, 2.0)
    w[v[inside], u[inside]] = gated[0, inside, 3]
    assert w[0, 0] == -1 and w[1, 1] == -1 and w[2, 2] == 1 and w[3, 3] == 1 and w[5, 5] == 0
    s = int(np.flatnonzero((v == 7) & (u == 20))[0])                                         # tile 1, row 7, column 4
    assert s == 256 + 7 * 16 + 4
    assert gated[0, s, 2] == depth[0, 7, 20] and gated[0, s, 0] == np.float32((np.float32(20) - np.float32(18)) / np.float32(30)) * depth[0, 7, 20]
    lo, hi, n = R.boxes_of(gated)
    assert n.sum() == (gated[..., 3] == 1).sum() and lo.shape == (1, 6, 3)
    rec = R.pack_boxes(lo, hi, n)
    assert rec.shape == (1, 6, 8) and rec.view(np.int32)[0, 0, 6] == n[0, 0] and rec.view(np.int32)[..., 7].max() == 0
    d2 = R.nn_d2(gated, own)
    need = R.necessary_tiles(gated, own, d2)
    assert need.shape == (1, 6) and (need >= 1).all() and (need <= 6).all()
    # the definition, once by hand
    lo_t, hi_t, n_t = R.boxes_of(own)
    Rmax = d2[0, :256][gated[0, :256, 3] == 1].max()
    by_hand = sum(1 for t in range(6) if n_t[0, t] > 0 and R.boxd2(lo[0, 0], hi[0, 0], lo_t[0, t], hi_t[0, t]) <= Rmax)
    assert need[0, 0] == by_hand


def _fields(dist_m):
    d2 = (np.asarray(dist_m, np.float64) ** 2).astype(np.float32)
    hist = np.bincount(np.searchsorted(R.edges2(), d2, side="right"), minlength=R.BINS)
    n = torch.tensor(d2.size)
    return n, torch.tensor(0), torch.tensor(float(np.sqrt(d2.astype(np.float64)).sum()), dtype=torch.float64), torch.from_numpy(hist)


def test_report_formulas_against_plain_numpy():
    """Means and shares are exact (to the last bits of a float64 mean), medians within one 0.5 mm bin."""
    rng = np.random.default_rng(3)
    for n_a, n_c, s_a, s_c in ((1000, 900, 0.004, 0.009), (17, 4000, 0.02, 0.001), (501, 499, 0.05, 0.3)):
        acc, comp = np.abs(rng.normal(0, s_a, n_a)), np.abs(rng.normal(0, s_c, n_c))
        acc[:3] = (0.005, 0.01, 0.02)                                   # exactly on the thresholds: not "within"
        # the lists as the kernel would see them: square roots of float32 squared distances
        acc = np.sqrt((acc ** 2).astype(np.float32).astype(np.float64))
        comp = np.sqrt((comp ** 2).astype(np.float32).astype(np.float64))
        m = PC.metrics_from_fields(_fields(acc), _fields(comp)).numpy()
        ref = R.metrics_from_distances(acc, comp)
        assert np.allclose(m[0], ref["acc"], rtol=1e-12) and np.allclose(m[1], ref["comp"], rtol=1e-12)
        assert np.allclose(m[2], ref["chamfer"], rtol=1e-12)
        assert abs(m[3] - ref["acc_med"]) <= 0.5 and abs(m[4] - ref["comp_med"]) <= 0.5
        assert np.array_equal(m[5:8], ref["F"]) and m[8] == n_a
        fa, fc = _fields(acc), _fields(comp)
        P, Rc = PC.shares_from_fields(fa[0], fa[1], fa[3]).numpy(), PC.shares_from_fields(fc[0], fc[1], fc[3]).numpy()
        assert np.array_equal(P, ref["P"]) and np.array_equal(Rc, ref["R"])
    # unmatched points miss; an empty direction gives NaN
    n, _, s, h = _fields([0.001, 0.002])
    assert np.array_equal(PC.shares_from_fields(n, torch.tensor(2), h).numpy(), [0.5, 0.5, 0.5])
    zero = (torch.tensor(0), torch.tensor(0), torch.tensor(0.0, dtype=torch.float64), torch.zeros(R.BINS, dtype=torch.int64))
    assert np.isnan(PC.metrics_from_fields(zero, (n, torch.tensor(0), s, h)).numpy()[[0, 2, 3, 5]]).all()


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    pts = np.zeros((50, 4), np.float32)
    pts[:, :3] = rng.normal(size=(50, 3))
    pts[:, 3] = rng.choice([1.0, 0.0, -1.0], 50)
    rgb = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    keep = pts[:, 3] == 1
    for flip in (True, False):
        for colours in (rgb, None):
            path = tmp_path / "c.ply"
            n = PC.write_ply(str(path), torch.from_numpy(pts), colours, flip=flip)
            raw = path.read_bytes()
            head, payload = raw.split(b"end_header\n", 1)
            lines = head.decode("ascii").splitlines()
            assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
            assert lines[2] == f"element vertex {keep.sum()}" and n == keep.sum()
            props = [l for l in lines if l.startswith("property")]
            assert props[:3] == ["property float x", "property float y", "property float z"]
            assert len(props) == (6 if colours is not None else 3)
            dt = [("xyz", "<f4", 3)] + ([("rgb", "u1", 3)] if colours is not None else [])
            rows = np.frombuffer(payload, dtype=dt)
            assert rows.shape == (keep.sum(),) and len(payload) == keep.sum() * (15 if colours is not None else 12)
            sign = np.array([1, -1, -1], np.float32) if flip else np.ones(3, np.float32)
            assert np.array_equal(rows["xyz"], pts[keep, :3] * sign)
            if colours is not None:
                assert np.array_equal(rows["rgb"], rgb[keep])
    assert PC.write_ply(str(tmp_path / "d.ply"), pts[:, :3]) == 50        # [n,3]: every row


def test_edge_table():
    e = PC.edges2_numpy()
    assert e.dtype == np.float32 and e.shape == (511,) and np.array_equal(e, R.edges2())
    assert (np.diff(e) > 0).all()
    for j, mm in ((10, 5.0), (20, 10.0), (40, 20.0)):
        assert e[j - 1] == np.float32((mm * 1e-3) ** 2) and PC.THRESHOLD_BINS[(10, 20, 40).index(j)] == j
    assert e[0] == np.float32(0.0005 ** 2) and PC.BINS == R.BINS == 512 and PC.TILE == R.TILE == 256


def test_default_classes_are_the_normals_ones():
    from polardepth import normals_eval
    assert PC.DEFAULT_CLASSES is normals_eval.DEFAULT_CLASSES
