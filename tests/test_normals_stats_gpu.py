"""pd_normals_stats / polardepth.normals_eval on the GPU against the NumPy statement (tests/normals_stats_ref.py, pinned by
tests/test_normals_stats_ref.py) applied to the very tensors handed to the kernel: the prediction, the kernel's own gtn
(pd_gt_normals), depth, mask and the 719-entry cosine table.

n, bad, hist and the NaN pattern of err_deg must be equal.  sum_deg / sum_deg2: rtol 1e-11 -- any order of n exactly
converted terms errs by at most (n - 1) 2^-53 of the sum, 7e-13 at the 6144 pixels of the largest image here; the device acos
adds a few ulp per term; 1e-11 leaves an order of magnitude over both.  err_deg: atol 1e-5 degrees (it is stored as fp32:
half an ulp at 180 degrees is 7.6e-6)."""
import functools

import numpy as np
import pytest
import torch

import normals_stats_ref as R

pytestmark = pytest.mark.gpu

# less than a wave, odd width | several workgroups per image, W % 4 == 2 | the evaluation test's size
SHAPES = [(2, 5, 7), (3, 33, 70), (4, 64, 96)]
MIN_D, MAX_D = 0.1, 2.0


def NE():
    from polardepth import normals_eval
    return normals_eval


def _classes(K):
    ne = NE()
    if K == 1:
        return [("all", None)]
    if K == 12:
        return list(ne.DEFAULT_CLASSES)
    assert K == 16
    return list(ne.DEFAULT_CLASSES) + [("a", (40, 60)), ("b", (0, 0)), ("none", (500, 600)), ("every", (-5, 1000))]


def _lohi(classes):
    return [(1, 0) if r is None else tuple(r) for _, r in classes]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a writable copy: the scene arrays are read-only


@functools.lru_cache(maxsize=None)
def scene(N, H, W):
    """Host arrays (never modified): depth with holes, NaN and out-of-range values, intrinsics, mask, a prediction in an
    8-float pixel (x, y, z first, junk behind) with zero and NaN normals, and the kernel's own gtn."""
    from polardepth._lib import lib, check, ptr, stream_ptr
    rng = np.random.default_rng(1000 * N + H + W)
    gt = rng.uniform(0.3, 1.8, (N, H, W)).astype(np.float32)
    gt[:, 1, 2] = 0.0
    gt[0, 0, 0] = 0.0
    gt[-1, H - 1, W - 2] = np.nan
    gt[0, 3, 4] = 2.5
    if H > 8:
        gt[:, H // 2, ::9] = 0.0                     # a dotted line of holes
        gt[:, :, W - 1][:, ::7] = 3.0                # out of range on the right border
    Kmat = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    Kmat[:, 0, 0], Kmat[:, 1, 1], Kmat[:, 0, 2], Kmat[:, 1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    mask = (rng.integers(0, 11, (N, H, W)) * 20).astype(np.int32)
    gt_t, K_t = _dev(gt), _dev(Kmat)                 # held until the kernel has read them
    gtn_t = torch.empty((N, H, W, 4), dtype=torch.float32, device="cuda")
    check(lib.pd_gt_normals(ptr(gt_t), ptr(K_t), ptr(gtn_t), N, H, W, MIN_D, MAX_D, stream_ptr()), "pd_gt_normals")
    gtn = gtn_t.cpu().numpy()
    pred8 = rng.normal(size=(N, H, W, 8)).astype(np.float32)
    pred8[..., :3] = gtn[..., :3] + 0.4 * pred8[..., :3]      # around the truth: the low bins are populated, like a real run's
    pred8[0, 3, 0, :3] = 0.0
    pred8[-1, 4, 0, 1] = np.nan
    pred8[0, 4, 1, 0] = np.inf
    for a in (gt, Kmat, mask, gtn, pred8):
        a.setflags(write=False)
    return gt, Kmat, mask, gtn, pred8


def pred_tensor(pred8, ld):
    """An [N,3,H,W] view with pixel stride ld on the device: ld = 3 channels-last, 4 / 8 the head of a wider pixel."""
    t = _dev(pred8[..., :max(ld, 3)])
    return t.permute(0, 3, 1, 2)[:, :3]


def fields(st):
    torch.cuda.synchronize()
    return {"n": st.n.cpu().numpy(), "bad": st.bad.cpu().numpy(), "sum_deg": st.sum_deg.cpu().numpy(),
            "sum_deg2": st.sum_deg2.cpu().numpy(), "hist": st.hist.cpu().numpy().astype(np.int64),
            "err_deg": None if st.err_deg is None else st.err_deg.cpu().numpy()}


def compare(got, ref, what):
    for k in ("n", "bad", "hist"):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k] if k != "hist" else None, ref[k] if k != "hist" else None)
    for k in ("sum_deg", "sum_deg2"):
        rel = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300)
        print(what, k, "max rel err", rel.max())
        assert np.allclose(got[k], ref[k], rtol=1e-11, atol=0.0), (what, k, rel.max())
    if got["err_deg"] is not None:
        assert np.array_equal(np.isnan(got["err_deg"]), np.isnan(ref["err_deg"])), what
        ok = ~np.isnan(ref["err_deg"])
        d = np.abs(got["err_deg"][ok].astype(np.float64) - ref["err_deg"][ok])
        print(what, "err_deg max abs err", d.max() if d.size else 0.0)
        assert (d <= 1e-5).all(), (what, d.max())


@pytest.mark.parametrize("gate", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_records_equal_the_statement(shape, gate):
    ne = NE()
    gt, Kmat, mask, gtn, pred8 = scene(*shape)
    edges = ne.cos_edges_numpy()
    gt_t, K_t, mask_t = _dev(gt)[:, None], _dev(Kmat), _dev(mask)[:, None]
    for K in (1, 12, 16):
        classes = _classes(K)
        ref = R.stats(pred8, gtn, gt, mask, _lohi(classes), edges, gate, MIN_D, MAX_D)
        assert ref["n"][:, 0].sum() > 0 and ref["bad"][:, 0].sum() >= (1 if gate else 2)
        for ld in (3, 4, 8):
            pred = pred_tensor(pred8, ld)
            got_pred, got_ld = ne.pixel_major(pred)
            assert got_ld == ld and got_pred.data_ptr() == pred.data_ptr()
            st = ne.normals_stats(pred, gt_t, K_t, mask=mask_t, classes=classes, gate=bool(gate), min_depth=MIN_D,
                                  max_depth=MAX_D, err_map=True)
            assert st.names == [n for n, _ in classes] and tuple(st.records.shape) == (shape[0], K, ne.RECORD_BYTES)
            compare(fields(st), ref, (shape, gate, K, ld))


@pytest.mark.parametrize("gate", [0, 1])
def test_no_mask_one_unranged_class(gate):
    ne = NE()
    gt, Kmat, mask, gtn, pred8 = scene(3, 33, 70)
    ref = R.stats(pred8, gtn, gt, None, [(1, 0)], ne.cos_edges_numpy(), gate, MIN_D, MAX_D)
    st = ne.normals_stats(pred_tensor(pred8, 3), _dev(gt), _dev(Kmat), mask=None, classes=[("all", None)], gate=bool(gate),
                          min_depth=MIN_D, max_depth=MAX_D, err_map=True)
    compare(fields(st), ref, ("no mask", gate))
    from polardepth._lib import PolarDepthError
    with pytest.raises(PolarDepthError, match="mask is null"):
        ne.normals_stats(pred_tensor(pred8, 3), _dev(gt), _dev(Kmat), mask=None)      # the default classes need the mask


def test_metrics_and_pool_follow_the_fields():
    ne = NE()
    gt, Kmat, mask, gtn, pred8 = scene(4, 64, 96)
    ref = R.stats(pred8, gtn, gt, mask, _lohi(ne.DEFAULT_CLASSES), ne.cos_edges_numpy(), 1, MIN_D, MAX_D)
    args = (pred_tensor(pred8, 3), _dev(gt)[:, None], _dev(Kmat))
    st = ne.normals_stats(*args, mask=_dev(mask)[:, None])
    m = st.metrics()
    assert m.is_cuda and m.dtype == torch.float64 and tuple(m.shape) == (4, 12, 7)
    want = ne.metrics_from_fields(*(torch.from_numpy(ref[k]) for k in ("n", "sum_deg", "sum_deg2", "hist"))).numpy()
    assert np.allclose(m.cpu().numpy(), want, rtol=1e-9, atol=0.0, equal_nan=True)
    theta = ref["err_deg"][0][~np.isnan(ref["err_deg"][0])]                 # class "all" of image 0
    assert want[0, 0, 6] == theta.size and abs(want[0, 0, 1] - np.median(theta)) <= 0.25
    assert want[0, 0, 3] == (theta < 11.25).sum() / theta.size
    # the pool: this call's images, then a second call's on top
    pooled = st.pooled()
    tot = ne.metrics_from_fields(*(torch.from_numpy(ref[k].sum(0)) for k in ("n", "sum_deg", "sum_deg2", "hist"))).numpy()
    assert pooled.is_cuda and tuple(pooled.shape) == (12, 7)
    assert np.allclose(pooled.cpu().numpy(), tot, rtol=1e-9, atol=0.0, equal_nan=True)
    st += ne.normals_stats(*args, mask=_dev(mask)[:, None])
    twice = st.pooled().cpu().numpy()
    assert np.array_equal(twice[:, 6], 2 * tot[:, 6]) and np.allclose(twice[:, :6], tot[:, :6], rtol=1e-9, equal_nan=True)
    assert np.array_equal(st.pooled_bad().cpu().numpy(), 2 * ref["bad"].sum(0))


# ------------------------------------------------------------------------------------------------ constructed cases
def _flat(H=12, W=18, N=1):
    """A fronto-parallel plane at depth 1 seen by a camera with fx = fy = 1, cx = cy = 0: the unprojected points are integers,
    every Sobel sum is exact, and the ground-truth normal is (0, 0, z) with z > 0 at every pixel."""
    gt = torch.ones((N, 1, H, W), device="cuda")
    return gt, torch.eye(4, device="cuda")[None].repeat(N, 1, 1)


def _const_pred(v, N, H, W):
    return torch.tensor(v, dtype=torch.float32, device="cuda").view(1, 3, 1, 1).expand(N, 3, H, W).contiguous(
        memory_format=torch.channels_last)


def test_parallel_orthogonal_antiparallel_and_bad():
    ne = NE()
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, H, W = 1, 12, 18
    gt, K = _flat(H, W, N)
    gtn = torch.empty((N, H, W, 4), device="cuda")
    check(lib.pd_gt_normals(ptr(gt), ptr(K), ptr(gtn), N, H, W, MIN_D, MAX_D, stream_ptr()), "pd_gt_normals")
    g = gtn.cpu().numpy()
    assert (g[..., 0] == 0).all() and (g[..., 1] == 0).all() and (g[..., 2] > 0.99).all()      # the construction holds
    for gate in (False, True):                               # no hole: the replicate border keeps every pixel under gate 1
        # (prediction, bin, angle): the last bin is [179.75, 180], antiparallel normals are its upper end
        for v, bin_, deg in (((0.0, 0.0, 2.5), 0, 0.0), ((1.0, 0.0, 0.0), 360, 90.0), ((0.0, -3.0, 0.0), 360, 90.0),
                             ((0.0, 0.0, -0.5), 719, 180.0)):
            f = fields(ne.normals_stats(_const_pred(v, N, H, W), gt, K, gate=gate, classes=[("all", None)], err_map=True))
            assert f["n"][0, 0] == H * W and f["bad"][0, 0] == 0 and f["hist"][0, 0, bin_] == H * W, (gate, v)
            assert np.abs(f["err_deg"] - deg).max() <= 1e-5 and f["sum_deg"][0, 0] == pytest.approx(H * W * deg, rel=1e-11)
            assert f["sum_deg2"][0, 0] == pytest.approx(H * W * deg * deg, rel=1e-11)
        # prediction equal to ground truth (the kernel's own gtn, ld = 4): everything in bin 0
        f = fields(ne.normals_stats(gtn.permute(0, 3, 1, 2)[:, :3], gt, K, gate=gate, classes=[("all", None)]))
        assert f["n"][0, 0] == f["hist"][0, 0, 0] == H * W
        # zero and NaN normals are counted, not averaged
        pred = _const_pred((0.0, 0.0, 1.0), N, H, W)
        pred[0, :, 2, 3] = 0.0
        pred[0, 1, 5, 7] = float("nan")
        pred[0, 0, 9, 1] = float("inf")
        f = fields(ne.normals_stats(pred, gt, K, gate=gate, classes=[("all", None)], err_map=True))
        assert f["n"][0, 0] == H * W - 3 and f["bad"][0, 0] == 3 and f["hist"][0, 0, 0] == H * W - 3
        assert f["sum_deg"][0, 0] == 0.0 and np.isnan(f["err_deg"]).sum() == 3
        assert np.isnan(f["err_deg"][0, 2, 3]) and np.isnan(f["err_deg"][0, 5, 7]) and np.isnan(f["err_deg"][0, 9, 1])


def test_a_hole_its_neighbours_and_the_borders():
    ne = NE()
    N, H, W = 1, 12, 18
    gt, K = _flat(H, W, N)
    pred = _const_pred((0.0, 0.3, 1.0), N, H, W)
    for (y, x), lost in (((5, 6), 9), ((0, 0), 4), ((H - 1, 7), 6), ((4, W - 1), 6), ((H - 1, W - 1), 4)):
        d = gt.clone()
        d[0, 0, y, x] = 0.0
        f0 = fields(ne.normals_stats(pred, d, K, gate=False, classes=[("all", None)], err_map=True))
        f1 = fields(ne.normals_stats(pred, d, K, gate=True, classes=[("all", None)], err_map=True))
        assert f0["n"][0, 0] + f0["bad"][0, 0] == H * W - 1 and np.isnan(f0["err_deg"][0, y, x])
        assert f1["n"][0, 0] + f1["bad"][0, 0] == H * W - lost, (y, x)
        want = np.zeros((H, W), bool)
        want[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True          # the hole and its neighbours, nothing else
        assert np.array_equal(np.isnan(f1["err_deg"][0]), want), (y, x)
        assert f1["bad"][0, 0] == 0 and f0["n"][0, 0] >= f1["n"][0, 0]      # gate 0 keeps the neighbours, whatever their normals are


def test_a_pixel_in_three_classes():
    ne = NE()
    N, H, W = 1, 12, 18
    gt, K = _flat(H, W, N)
    mask = torch.zeros((N, 1, H, W), dtype=torch.int32, device="cuda")
    mask[0, 0, 7, 11] = 40
    classes = [("all", None), ("objects", (20, 160)), ("bottle", (40, 40)), ("can", (60, 60))]
    pred = _const_pred((0.0, 0.0, 1.0), N, H, W)
    pred[0, :, 7, 11] = torch.tensor([0.0, 1.0, 1.0])                   # 45 degrees: bin 180 (or 179: the fp32 normal's z is ~1)
    f = fields(ne.normals_stats(pred, gt, K, mask=mask, classes=classes, err_map=True))
    assert f["n"][0].tolist() == [H * W, 1, 1, 0] and f["bad"][0].tolist() == [0, 0, 0, 0]
    b = int(np.flatnonzero(f["hist"][0, 1])[0])
    assert b in (179, 180) and f["hist"][0, 2, b] == 1 and f["hist"][0, 0, b] == 1 and f["hist"][0, 0, 0] == H * W - 1
    assert f["sum_deg"][0, 1] == f["sum_deg"][0, 2] == f["sum_deg"][0, 0] == pytest.approx(45.0, abs=1e-4)
    assert f["sum_deg"][0, 3] == 0.0 and f["hist"][0, 3].sum() == 0


# ------------------------------------------------------------------------------------------------ other checks
def test_a_depth_map_scores_as_its_own_normals():
    ne = NE()
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, H, W = 3, 33, 70
    gt, Kmat, mask, gtn, pred8 = scene(N, H, W)
    rng = np.random.default_rng(5)
    depth = (np.nan_to_num(gt, nan=1.0) + rng.normal(scale=0.02, size=gt.shape)).astype(np.float32)
    depth[1, 10, 10] = np.nan                                           # a non-finite predicted depth: zero normal, `bad`
    depth_t, gt_t, K_t, mask_t = _dev(depth)[:, None], _dev(gt)[:, None], _dev(Kmat), _dev(mask)[:, None]
    a = ne.normals_stats(depth_t, gt_t, K_t, mask=mask_t)
    pn = torch.empty((N, H, W, 4), device="cuda")
    big = float(np.finfo(np.float32).max)
    check(lib.pd_gt_normals(ptr(depth_t), ptr(K_t), ptr(pn), N, H, W, -big, big, stream_ptr()), "pd_gt_normals")
    assert (pn[1, 10, 10] == 0).all()
    b = ne.normals_stats(pn.permute(0, 3, 1, 2)[:, :3], gt_t, K_t, mask=mask_t)
    assert torch.equal(a.records, b.records)
    assert int(a.bad[1, 0]) >= 1 and int(a.n.sum()) > 0
    ref = R.stats(pn.cpu().numpy(), gtn, gt, mask, _lohi(ne.DEFAULT_CLASSES), ne.cos_edges_numpy(), 1, MIN_D, MAX_D)
    compare(fields(a), ref, "depth map")


def test_channels_last_is_read_in_place_and_nchw_gives_the_same_record():
    ne = NE()
    gt, Kmat, mask, gtn, pred8 = scene(3, 33, 70)
    cl = pred_tensor(pred8, 3)
    assert cl.is_contiguous(memory_format=torch.channels_last)
    same, ld = ne.pixel_major(cl)
    assert same is cl and same.data_ptr() == cl.data_ptr() and ld == 3
    nchw = cl.contiguous()
    copy, ld2 = ne.pixel_major(nchw)
    assert ld2 == 3 and copy.data_ptr() != nchw.data_ptr()
    args = (_dev(gt)[:, None], _dev(Kmat))
    a = ne.normals_stats(cl, *args, mask=_dev(mask)[:, None])
    b = ne.normals_stats(nchw, *args, mask=_dev(mask)[:, None])
    assert torch.equal(a.records, b.records)


def test_two_calls_give_identical_bytes():
    ne = NE()
    gt, Kmat, mask, gtn, pred8 = scene(4, 64, 96)
    args = (pred_tensor(pred8, 3), _dev(gt)[:, None], _dev(Kmat))
    a = ne.normals_stats(*args, mask=_dev(mask)[:, None], err_map=True)
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")      # whatever the allocator hands out next is dirty
    del junk
    b = ne.normals_stats(*args, mask=_dev(mask)[:, None], err_map=True)
    torch.cuda.synchronize()
    assert a.records.cpu().numpy().tobytes() == b.records.cpu().numpy().tobytes()
    assert a.err_deg.cpu().numpy().tobytes() == b.err_deg.cpu().numpy().tobytes()


def test_captured_call_replays_the_eager_record():
    ne = NE()
    gt, Kmat, mask, gtn, pred8 = scene(3, 33, 70)
    pred, gt_t, K_t, mask_t = pred_tensor(pred8, 3), _dev(gt)[:, None], _dev(Kmat), _dev(mask)[:, None]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires (builds the table)
        eager = ne.normals_stats(pred, gt_t, K_t, mask=mask_t, err_map=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        st = ne.normals_stats(pred, gt_t, K_t, mask=mask_t, err_map=True)
    st.records.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.records, eager.records)
    assert st.err_deg.cpu().numpy().tobytes() == eager.err_deg.cpu().numpy().tobytes()
    # the replay reads the tensors of its capture: new data, new record
    pred.copy_(pred.flip(0))
    graph.replay()
    again = ne.normals_stats(pred, gt_t, K_t, mask=mask_t)
    torch.cuda.synchronize()
    assert torch.equal(st.records, again.records) and not torch.equal(st.records, eager.records)
