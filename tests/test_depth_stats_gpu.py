"""pd_depth_medians / pd_depth_stats / polardepth.depth_eval on the GPU against the NumPy statement (tests/depth_stats_ref.py,
pinned to the reference by tests/test_depth_stats_ref.py) applied to the very arrays handed to the kernels.

The medians must be bit-equal.  n, a1..a3, bad, hist and the NaN pattern of err must be equal.  The four sums: rtol 1e-11,
the convention of tests/test_normals_stats_gpu.py and for the same reason -- any order of n exactly converted non-negative
terms errs by at most (n - 1) 2^-53 of the sum, 2.2e-13 at the 1961 pixels of the largest image here; the device's division
and log1p add a few ulp per term; 1e-11 leaves more than an order of magnitude over both.  err: atol 1e-7 m (it is stored as
fp32, and with gt and the clamped prediction inside (0.1, 2.0) it stays below 2 m, where half an fp32 ulp is at most 6e-8)."""
import functools

import numpy as np
import pytest
import torch

import depth_stats_ref as R

pytestmark = pytest.mark.gpu

# more than one workgroup per image (1961 pixels), W % 4 == 1 | less than two waves
SHAPES = [(3, 37, 53), (3, 8, 12)]
MIN_D, MAX_D = 0.1, 2.0


def DE():
    from polardepth import depth_eval
    return depth_eval


def _classes(K):
    de = DE()
    if K == 1:
        return [("all", None)]
    if K == 12:
        return list(de.DEFAULT_CLASSES)
    assert K == 16
    return list(de.DEFAULT_CLASSES) + [("a", (40, 60)), ("b", (0, 0)), ("none", (500, 600)), ("every", (-5, 1000))]


def _lohi(classes):
    return [(1, 0) if r is None else tuple(r) for _, r in classes]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a writable copy: the scene arrays are read-only


@functools.lru_cache(maxsize=None)
def scene(N, H, W):
    """Host arrays (never modified): depth with holes, NaN and out-of-range values; a prediction around 1.2 x the truth with
    values beyond both clamps, NaN and both infinities; the instance mask."""
    rng = np.random.default_rng(1000 * N + H + W)
    gt = rng.uniform(0.3, 1.8, (N, H, W)).astype(np.float32)
    gt[:, 1, 2] = 0.0
    gt[0, 0, 0] = 0.0
    gt[-1, H - 1, W - 2] = np.nan
    gt[0, 3, 4] = 2.5
    gt[1, 2, 3] = MIN_D                                   # exactly on the gate: out
    gt[1, 2, 4] = MAX_D
    gt[:, H // 2, ::9] = 0.0                              # a dotted line of holes
    pred = (gt * rng.normal(1.2, 0.08, (N, H, W)) + rng.normal(0, 0.01, (N, H, W))).astype(np.float32)
    pred[rng.random((N, H, W)) < 0.03] = 0.02             # below the lower clamp
    pred[rng.random((N, H, W)) < 0.03] = 3.5              # above the upper clamp
    pred[0, 4, 1] = np.nan
    pred[-1, 4, 0] = np.inf
    pred[0, 5, 5] = -np.inf
    pred[:, 1, 2] = np.nan                                # on a hole of the ground truth: gated out, not bad
    mask = (rng.integers(0, 11, (N, H, W)) * 20).astype(np.int32)
    for a in (gt, pred, mask):
        a.setflags(write=False)
    return gt, pred, mask


@functools.lru_cache(maxsize=None)
def ref_stats(shape, K, how=None, masked=True):
    """The statement's records for a scene, computed once; with ``how`` the statement's own medians and scale go in."""
    gt, pred, mask = scene(*shape)
    classes = _lohi(_classes(K))
    m = mask if masked else None
    scale = None
    if how is not None:
        scale = R.scale_of(R.medians(pred, gt, m, classes, MIN_D, MAX_D)[1], how)
    return R.stats(pred, gt, m, classes, R.edges_numpy(), MIN_D, MAX_D, scale=scale), scale


def fields(st):
    torch.cuda.synchronize()
    return {"n": st.n.cpu().numpy(), "bad": st.bad.cpu().numpy(), "a": st.a.cpu().numpy(), "sums": st.sums.cpu().numpy(),
            "hist": st.hist.cpu().numpy().astype(np.int64), "err": None if st.err is None else st.err.cpu().numpy()}


def compare(got, ref, what):
    for k in ("n", "bad", "a", "hist"):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k] if k != "hist" else None, ref[k] if k != "hist" else None)
    rel = np.abs(got["sums"] - ref["sums"]) / np.maximum(np.abs(ref["sums"]), 1e-300)
    print(what, "sums: max rel err", rel.max())
    assert np.allclose(got["sums"], ref["sums"], rtol=1e-11, atol=0.0), (what, rel.max())
    if got["err"] is not None:
        assert np.array_equal(np.isnan(got["err"]), np.isnan(ref["err"])), what
        ok = ~np.isnan(ref["err"])
        d = np.abs(got["err"][ok].astype(np.float64) - ref["err"][ok])
        print(what, "err: max abs err", d.max() if d.size else 0.0)
        assert (d <= 1e-7).all(), (what, d.max())


def same_floats(got, ref, what):
    """bit-equal, NaN where and only where the reference has NaN"""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    assert np.array_equal(got.view(np.uint32)[ok], ref.view(np.uint32)[ok]), (what, got[ok], ref[ok])


def medians_equal(pred, gt, mask, classes, lo=MIN_D, hi=MAX_D, what=""):
    n, med = DE().depth_medians(_dev(pred), _dev(gt), mask=None if mask is None else _dev(mask), classes=classes,
                                min_depth=lo, max_depth=hi)
    torch.cuda.synchronize()
    rn, rmed = R.medians(pred, gt, mask, _lohi(classes), lo, hi)
    assert n.dtype == torch.int64 and med.dtype == torch.float32 and tuple(med.shape) == rmed.shape
    assert np.array_equal(n.cpu().numpy(), rn), (what, n.cpu().numpy(), rn)
    same_floats(med.cpu().numpy(), rmed, what)
    return rn, rmed


# ------------------------------------------------------------------------------------------------ the medians
@pytest.mark.parametrize("K", [1, 12, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_medians_are_bit_equal_to_the_sorted_values(shape, K):
    gt, pred, mask = scene(*shape)
    n, med = medians_equal(pred, gt, mask if K > 1 else None, _classes(K), what=(shape, K))
    assert n[:, 0].min() > 0 and not np.isnan(med[:, 0]).any()
    if K == 16:
        assert (n[:, 14] == 0).all() and np.isnan(med[:, 14]).all()          # the class nobody is in


def test_medians_of_classes_of_zero_one_two_and_three_pixels():
    H, W = 8, 12
    rng = np.random.default_rng(7)
    gt = rng.uniform(0.3, 1.8, (2, H, W)).astype(np.float32)
    pred = rng.uniform(0.3, 1.8, (2, H, W)).astype(np.float32)
    mask = np.zeros((2, H, W), np.int32)
    mask[0, 0, 0] = 1
    mask[0, 1, 1:3] = 2
    mask[0, 2, 3], mask[0, 7, 11], mask[0, 4, 5] = 3, 3, 3
    mask[1, 5, 5:7] = 1                                    # two pixels, one of them with a NaN prediction: a class of one
    pred[1, 5, 5] = np.nan
    mask[1, 6, 6] = 2                                      # one pixel, outside the gate: a class of none
    gt[1, 6, 6] = 0.0
    classes = [("none", (9, 9)), ("one", (1, 1)), ("two", (2, 2)), ("three", (3, 3)), ("all", None)]
    n, med = medians_equal(pred, gt, mask, classes, what="tiny classes")
    assert n[0].tolist() == [0, 1, 2, 3, H * W] and n[1].tolist() == [0, 1, 0, 0, H * W - 2]
    assert med[0, 1, 0] == med[0, 1, 1] == gt[0, 0, 0] and med[0, 2, 0] != med[0, 2, 1]
    assert med[0, 3, 2] == med[0, 3, 3] == np.sort(pred[0][mask[0] == 3])[1]


def test_medians_under_heavy_ties_and_at_both_clamps():
    N, H, W = 3, 37, 53
    rng = np.random.default_rng(8)
    gt = rng.choice(np.array([0.5, 0.75, 1.0], np.float32), (N, H, W))            # three values only
    pred = np.where(rng.random((N, H, W)) < 0.5, np.float32(0.01), np.float32(7.0)).astype(np.float32)      # both clamps
    pred[0] = 0.01                                         # image 0: everything at the lower clamp
    pred[1, :, : W // 2] = 1.0                             # image 1: a third value between them
    mask = (rng.integers(0, 11, (N, H, W)) * 20).astype(np.int32)
    n, med = medians_equal(pred, gt, mask, _classes(12), what="ties")
    assert set(np.unique(med[:, :, 2:])) <= {np.float32(MIN_D), np.float32(1.0), np.float32(MAX_D)}
    assert (med[0, :, 2:] == np.float32(MIN_D)).all()


def test_medians_of_values_that_differ_in_one_byte_only():
    N, H, W = 2, 37, 53
    rng = np.random.default_rng(9)
    base = np.float32(0.7).view(np.uint32)
    low = (base & np.uint32(0xFFFFFF00)) + rng.integers(0, 256, (N, H, W)).astype(np.uint32)
    gt = low.view(np.float32)                              # only the lowest mantissa byte differs: decided in the last pass
    pred = (2.0 ** rng.integers(-3, 1, (N, H, W))).astype(np.float32)            # 0.125 .. 1: only the exponent differs
    assert len(np.unique(gt.view(np.uint32) >> 8)) == 1 and len(np.unique(pred.view(np.uint32) & 0x007FFFFF)) == 1
    n, med = medians_equal(pred, gt, None, [("all", None)], what="one byte")
    assert n[0, 0] == H * W
    medians_equal(gt, pred + np.float32(0.25), None, [("all", None)], what="one byte, swapped")


def test_medians_with_an_open_range_and_non_finite_predictions():
    N, H, W = 2, 8, 12
    rng = np.random.default_rng(10)
    gt = np.exp(rng.uniform(-2, 60, (N, H, W))).astype(np.float32)               # up to 1e26
    gt[0, 0, 0] = np.inf                                   # not below +inf: gated out
    pred = np.exp(rng.uniform(-4, 80, (N, H, W))).astype(np.float32)
    pred[0, 1, 1], pred[1, 2, 2], pred[1, 3, 3] = np.nan, np.inf, -np.inf
    n, med = medians_equal(pred, gt, None, [("all", None)], lo=0.5, hi=float("inf"), what="open range")
    assert n[0, 0] <= H * W - 2 and n[1, 0] <= H * W - 2              # the infinite gt, the three non-finite predictions
    assert np.isfinite(med).all() and med[..., 2:].min() >= 0.5 and med.max() > 1e6
    # the same inputs through depth_stats: the excluded predictions are counted
    st = fields(DE().depth_stats(_dev(pred), _dev(gt), classes=[("all", None)], min_depth=0.5, max_depth=float("inf")))
    ref = R.stats(pred, gt, None, [(1, 0)], R.edges_numpy(), 0.5, float("inf"))
    assert np.array_equal(st["n"], n) and np.array_equal(st["bad"], ref["bad"]) and ref["bad"].sum() >= 2
    assert np.array_equal(st["hist"], ref["hist"]) and np.array_equal(st["a"], ref["a"])


# ------------------------------------------------------------------------------------------------ the records
@pytest.mark.parametrize("K", [1, 12, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_records_equal_the_statement(shape, K):
    de = DE()
    gt, pred, mask = scene(*shape)
    classes = _classes(K)
    ref, _ = ref_stats(shape, K, None, K > 1)
    assert ref["n"][:, 0].sum() > 0 and ref["bad"][:, 0].sum() >= 2 and ref["hist"][:, 0, -1].sum() > 0
    st = de.depth_stats(_dev(pred)[:, None], _dev(gt)[:, None], mask=_dev(mask)[:, None] if K > 1 else None, classes=classes,
                        min_depth=MIN_D, max_depth=MAX_D, out_err=True)
    assert st.names == [n for n, _ in classes] and tuple(st.records.shape) == (shape[0], K, de.RECORD_BYTES)
    assert st.scale is None and tuple(st.err.shape) == shape
    compare(fields(st), ref, (shape, K))
    assert np.array_equal(st.records.view(torch.int64)[..., 9].cpu().numpy(), np.zeros((shape[0], K), np.int64))      # the padding


@pytest.mark.parametrize("how", ["numpy", "torch"])
@pytest.mark.parametrize("K", [1, 12, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_median_scaled_records_equal_the_statement_run_with_its_own_scale(shape, K, how):
    de = DE()
    gt, pred, mask = scene(*shape)
    classes = _classes(K)
    ref, scale = ref_stats(shape, K, how, K > 1)
    st = de.depth_stats(_dev(pred), _dev(gt), mask=_dev(mask) if K > 1 else None, classes=classes, min_depth=MIN_D,
                        max_depth=MAX_D, median_scaling=how)
    assert st.err is None and st.scale.dtype == torch.float32 and tuple(st.scale.shape) == (shape[0], K)
    same_floats(st.scale.cpu().numpy(), scale, (shape, K, how))
    compare(fields(st), ref, (shape, K, how))
    unscaled, _ = ref_stats(shape, K, None, K > 1)
    assert not np.array_equal(ref["hist"], unscaled["hist"]) and np.array_equal(ref["n"], unscaled["n"])
    if K == 16:                                            # the empty class has no scale; nothing of it is counted
        assert np.isnan(scale[:, 14]).all() and (ref["n"][:, 14] == 0).all() and (ref["bad"][:, 14] == 0).all()


def test_no_mask_needs_unranged_classes():
    from polardepth._lib import PolarDepthError
    gt, pred, mask = scene(3, 8, 12)
    with pytest.raises(PolarDepthError, match="mask is null"):
        DE().depth_stats(_dev(pred), _dev(gt))             # the default classes need the mask
    with pytest.raises(PolarDepthError, match="mask is null"):
        DE().depth_medians(_dev(pred), _dev(gt))


# ------------------------------------------------------------------------------------------------ one case per rule
def _one(gt_row, pred_row, **kw):
    gt = np.array([[gt_row]], np.float32)
    pred = np.array([[pred_row]], np.float32)
    st = DE().depth_stats(_dev(pred), _dev(gt), classes=[("all", None)], out_err=True, **kw)
    return fields(st)


def test_bin_edges_last_bin_ratio_threshold_and_the_strict_gate():
    e = R.edges_numpy()
    assert e[249] == 0.125 and abs(e[510] - 0.2555) < 1e-15
    # |d| exactly on edge 250 belongs to bin 250; one fp32 step less to bin 249
    below = np.nextafter(np.float32(1.0), np.float32(0))                         # 1 - 2^-24: |d| = 0.125 - 2^-24 exactly
    f = _one([1.0, below], [0.875, 0.875])
    assert f["hist"][0, 0, 250] == 1 and f["hist"][0, 0, 249] == 1 and f["n"][0, 0] == 2 and f["hist"][0, 0].sum() == 2
    assert f["err"][0, 0, 0] == 0.125
    # |d| >= 255.5 mm lands in the last bin, just below it in bin 510
    f = _one([1.0, 1.0, 1.0, 1.0], [0.25, 1.75, 0.7444, 0.7446])
    assert 1.0 - np.float64(np.float32(0.7444)) > e[510] > 1.0 - np.float64(np.float32(0.7446)) > e[509]
    assert f["hist"][0, 0, 511] == 3 and f["hist"][0, 0, 510] == 1
    # the ratio exactly 1.25 (1 / 0.8f rounds to it in fp32; 1.25 / 1) is not below 1.25; 1.5625 and 1.953125 likewise
    assert np.float32(1.0) / np.float32(0.8) == np.float32(1.25)
    f = _one([1.0, 1.25, 1.0, 1.5625, 1.0, 1.0], [0.8, 1.0, 1.5625, 1.0, 1.953125, 1.0])
    assert f["a"][0, 0].tolist() == [1, 3, 5] and f["n"][0, 0] == 6
    # gt exactly at min_depth and at max_depth is gated out, one step inside counts
    lo, hi = np.float32(MIN_D), np.float32(MAX_D)
    f = _one([lo, hi, np.nextafter(lo, hi), np.nextafter(hi, lo)], [1.0, 1.0, 1.0, 1.0], min_depth=MIN_D, max_depth=MAX_D)
    assert f["n"][0, 0] == 2 and f["bad"][0, 0] == 0 and np.isnan(f["err"][0, 0]).tolist() == [True, True, False, False]
    # the four sums of one pixel, by hand: g = 1, p = 0.5
    f = _one([1.0], [0.5])
    assert f["sums"][0, 0].tolist() == pytest.approx([0.5, 0.25, 0.25, np.log(2.0) ** 2], rel=1e-14)


def test_a_pixel_in_three_classes():
    H, W = 8, 12
    gt = np.ones((1, H, W), np.float32)
    pred = np.ones((1, H, W), np.float32)
    pred[0, 5, 7] = 0.984375                               # |d| = 2^-6 m = 15.625 mm exactly: bin 31
    mask = np.zeros((1, H, W), np.int32)
    mask[0, 5, 7] = 40
    classes = [("all", None), ("objects", (20, 160)), ("bottle", (40, 40)), ("can", (60, 60))]
    f = fields(DE().depth_stats(_dev(pred), _dev(gt), mask=_dev(mask), classes=classes))
    assert f["n"][0].tolist() == [H * W, 1, 1, 0] and f["bad"][0].tolist() == [0, 0, 0, 0]
    assert f["hist"][0, 0, 0] == H * W - 1 and f["hist"][0, 0, 31] == f["hist"][0, 1, 31] == f["hist"][0, 2, 31] == 1
    assert f["sums"][0, 1].tolist() == f["sums"][0, 2].tolist() == f["sums"][0, 0].tolist() and f["sums"][0, 0, 0] > 0
    assert f["sums"][0, 3].tolist() == [0, 0, 0, 0] and f["a"][0].tolist() == [[H * W] * 3, [1] * 3, [1] * 3, [0] * 3]


def test_a_non_finite_scale_makes_the_class_bad():
    """through the C ABI: the Python layer only ever hands over the scale of its own medians"""
    from polardepth._lib import lib, check, ptr, stream_ptr
    de = DE()
    gt, pred, mask = scene(3, 8, 12)
    N, H, W = gt.shape
    classes = [("all", None), ("objects", (20, 160)), ("box", (20, 20))]
    names, table = de.class_table(classes)
    scale = np.array([[1.0, np.nan, 0.5], [np.inf, 2.0, 1.0], [1.0, 1.0, -np.inf]], np.float32)
    gt_t, pred_t, mask_t, scale_t = _dev(gt), _dev(pred), _dev(mask), _dev(scale)
    rec = torch.empty((N, 3, de.RECORD_BYTES), dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(lib.pd_depth_stats_workspace(N, H, W, 3)), dtype=torch.uint8, device="cuda")
    check(lib.pd_depth_stats(ptr(gt_t), ptr(pred_t), ptr(mask_t), table, 3, ptr(scale_t), ptr(de.edges("cuda")), None, ptr(rec),
                             ptr(ws), ws.numel(), N, H, W, MIN_D, MAX_D, stream_ptr()), "pd_depth_stats")
    ref = R.stats(pred, gt, mask, _lohi(classes), R.edges_numpy(), MIN_D, MAX_D, scale=scale)
    got = fields(de.DepthStats(rec, names))
    compare(got, ref, "non-finite scale")
    plain = R.stats(pred, gt, mask, _lohi(classes), R.edges_numpy(), MIN_D, MAX_D)
    for i, k in ((0, 1), (1, 0), (2, 2)):
        assert got["n"][i, k] == 0 and got["hist"][i, k].sum() == 0 and (got["sums"][i, k] == 0).all()
        assert got["bad"][i, k] == plain["n"][i, k] + plain["bad"][i, k] > 0


# ------------------------------------------------------------------------------------------------ metrics, pool, replay
def test_metrics_and_pool_follow_the_fields():
    de = DE()
    shape = SHAPES[0]
    gt, pred, mask = scene(*shape)
    ref, _ = ref_stats(shape, 12)
    args = dict(mask=_dev(mask), min_depth=MIN_D, max_depth=MAX_D)
    st = de.depth_stats(_dev(pred), _dev(gt), **args)
    m = st.metrics()
    assert m.is_cuda and m.dtype == torch.float64 and tuple(m.shape) == (3, 12, 13) and len(de.METRIC_NAMES) == 13
    t = lambda r: (torch.from_numpy(r[k]) for k in ("n", "a", "sums", "hist"))
    want = de.metrics_from_fields(*t(ref)).numpy()
    assert np.allclose(m.cpu().numpy(), want, rtol=1e-9, atol=0.0, equal_nan=True)
    # class "all" of image 0 by hand: the reference's seven figures, the error distribution in millimetres
    em = ref["err"][0][~np.isnan(ref["err"][0])]
    e, edge = em * 1e3, R.edges_numpy()                    # edge[9], [19], [39]: 5, 10, 20 mm
    assert np.allclose(want[0, 0, :7], R.errors_from(ref, 0, 0), rtol=1e-12) and want[0, 0, 12] == e.size
    assert want[0, 0, 9] == (em < edge[9]).sum() / e.size and want[0, 0, 10] == (em < edge[19]).sum() / e.size
    assert want[0, 0, 11] == (em < edge[39]).sum() / e.size and abs(want[0, 0, 8] - np.median(e)) <= 0.5
    assert abs(want[0, 0, 7] - np.minimum(e, 255.75).mean()) <= 0.25
    # the pool: this call's images, then a second call's on top
    tot = de.metrics_from_fields(*(torch.from_numpy(ref[k].sum(0)) for k in ("n", "a", "sums", "hist"))).numpy()
    pooled = st.pooled()
    assert pooled.is_cuda and tuple(pooled.shape) == (12, 13)
    assert np.allclose(pooled.cpu().numpy(), tot, rtol=1e-9, atol=0.0, equal_nan=True)
    st += de.depth_stats(_dev(pred), _dev(gt), **args)
    twice = st.pooled().cpu().numpy()
    assert np.array_equal(twice[:, 12], 2 * tot[:, 12]) and np.allclose(twice[:, :12], tot[:, :12], rtol=1e-9, equal_nan=True)
    assert np.array_equal(st.pooled_bad().cpu().numpy(), 2 * ref["bad"].sum(0))
    with pytest.raises(ValueError, match="cannot pool"):
        st += de.depth_stats(_dev(pred), _dev(gt), classes=[("all", None)])


def test_two_calls_give_identical_bytes():
    de = DE()
    gt, pred, mask = scene(*SHAPES[0])
    args = (_dev(pred), _dev(gt))
    a = de.depth_stats(*args, mask=_dev(mask), out_err=True)
    s = de.depth_stats(*args, mask=_dev(mask), median_scaling="numpy")
    junk = torch.full((1 << 22,), 0x5A, dtype=torch.uint8, device="cuda")      # whatever the allocator hands out next is dirty
    del junk
    b = de.depth_stats(*args, mask=_dev(mask), out_err=True)
    t = de.depth_stats(*args, mask=_dev(mask), median_scaling="numpy")
    torch.cuda.synchronize()
    assert a.records.cpu().numpy().tobytes() == b.records.cpu().numpy().tobytes()
    assert a.err.cpu().numpy().tobytes() == b.err.cpu().numpy().tobytes()
    assert s.records.cpu().numpy().tobytes() == t.records.cpu().numpy().tobytes()
    assert s.scale.cpu().numpy().tobytes() == t.scale.cpu().numpy().tobytes()
    assert a.records.cpu().numpy().tobytes() != s.records.cpu().numpy().tobytes()


def test_captured_calls_replay_the_eager_records():
    de = DE()
    gt, pred, mask = scene(*SHAPES[0])
    pred_t, gt_t, mask_t = _dev(pred), _dev(gt), _dev(mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires (builds the table)
        eager = de.depth_stats(pred_t, gt_t, mask=mask_t, out_err=True)
        eager_s = de.depth_stats(pred_t, gt_t, mask=mask_t, median_scaling="numpy")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        st = de.depth_stats(pred_t, gt_t, mask=mask_t, out_err=True)
        ss = de.depth_stats(pred_t, gt_t, mask=mask_t, median_scaling="numpy")      # the medians are captured with it
    st.records.zero_()
    ss.records.zero_()
    ss.scale.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.records, eager.records) and torch.equal(ss.records, eager_s.records)
    assert st.err.cpu().numpy().tobytes() == eager.err.cpu().numpy().tobytes()
    assert ss.scale.cpu().numpy().tobytes() == eager_s.scale.cpu().numpy().tobytes()
    # the replay reads the tensors of its capture: new data, new records
    pred_t.copy_(pred_t.flip(0))
    graph.replay()
    again = de.depth_stats(pred_t, gt_t, mask=mask_t)
    again_s = de.depth_stats(pred_t, gt_t, mask=mask_t, median_scaling="numpy")
    torch.cuda.synchronize()
    assert torch.equal(st.records, again.records) and not torch.equal(st.records, eager.records)
    assert torch.equal(ss.records, again_s.records) and not torch.equal(ss.records, eager_s.records)


def test_the_other_evaluators_still_repeat_themselves():
    """normals_stats and cloud_stats go through the same reducer, now with its `Sums` parameter: a second call returns the
    same bytes (their own suites compare them with their statements)."""
    from polardepth import normals_eval, pointcloud
    N, H, W = 3, 37, 53
    gt, pred, mask = scene(N, H, W)
    depth = np.nan_to_num(pred, nan=1.0, posinf=1.0, neginf=1.0).clip(MIN_D, MAX_D)
    Kmat = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    Kmat[:, 0, 0], Kmat[:, 1, 1], Kmat[:, 0, 2], Kmat[:, 1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    args = (_dev(depth)[:, None], _dev(gt)[:, None], _dev(Kmat))
    a = normals_eval.normals_stats(*args, mask=_dev(mask)[:, None])
    b = normals_eval.normals_stats(*args, mask=_dev(mask)[:, None])
    c = pointcloud.cloud_stats(*args, mask=_dev(mask)[:, None])
    d = pointcloud.cloud_stats(*args, mask=_dev(mask)[:, None])
    torch.cuda.synchronize()
    assert torch.equal(a.records, b.records) and int(a.n.sum()) > 0
    assert torch.equal(c.acc.records, d.acc.records) and torch.equal(c.comp.records, d.comp.records) and int(c.acc.n.sum()) > 0
