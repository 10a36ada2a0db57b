"""pd_unc_stats / polardepth.uncertainty_eval on the GPU against the NumPy statement (tests/unc_stats_ref.py) applied to the
very arrays handed to the kernel.

n, bad, cover50, cover90, hist and the three tables must be equal (tests/test_unc_stats_ref.py shows that no coverage
decision of these cases is within reach of an ulp of exp).  The three fp64 sums: the summation-order bound
(n - 1) 2^-53 sum|term| plus the allowance for the device's exp and division of tests/test_unc_loss_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import depth_stats_ref as D
import unc_cases as C
import unc_stats_ref as R
from test_unc_loss_gpu import EPS, EXP_ULP

pytestmark = pytest.mark.gpu


def UE():
    from polardepth import uncertainty_eval
    return uncertainty_eval


def _classes(K):
    return list(UE().DEFAULT_CLASSES) if K == 12 else C.CLASSES[K]


def _lohi(classes):
    return [(1, 0) if r is None else tuple(r) for _, r in classes]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def ref_stats(shape, K):
    gt, pred, unc, mask = C.stats_case(*shape)
    return R.stats(pred, gt, unc, mask if K > 1 else None, _lohi(_classes(K)), C.B_RANGE, C.MIN_D, C.MAX_D)


def call(shape, K):
    gt, pred, unc, mask = C.stats_case(*shape)
    return UE().uncertainty_stats(_dev(pred)[:, None], _dev(gt)[:, None], _dev(unc)[:, None], mask=_dev(mask) if K > 1 else None,
                                  classes=_classes(K), b_range=C.B_RANGE, min_depth=C.MIN_D, max_depth=C.MAX_D)


def fields(st):
    torch.cuda.synchronize()
    f = lambda t: t.cpu().numpy()
    return {"n": f(st.n), "bad": f(st.bad), "cover": f(st.cover), "sums": f(st.sums), "hist": f(st.hist).astype(np.int64),
            "tables": f(st.tables)}


def sum_bounds(shape, K):
    """[N,K,3]: what the device's nll, b and e sums may differ from the exactly rounded ones."""
    gt, pred, unc, mask = C.stats_case(*shape)
    ok, good, e, b, logb, *_ = R.pixels(pred, gt, unc, C.B_RANGE, C.MIN_D, C.MAX_D)
    m = np.zeros(gt.shape, np.int64) if (mask is None or K == 1) else mask.astype(np.int64)
    out = np.zeros((shape[0], K, 3))
    for i in range(shape[0]):
        for k, (lo, hi) in enumerate(_lohi(_classes(K))):
            v = D.in_class(m[i], lo, hi) & ok[i] & good[i]
            n = int(v.sum())
            order = max(n - 1, 0) * EPS
            ratio, l2b = (e[i] / b[i])[v], np.abs(logb[i] + R.LN2)[v]
            # per term: e / b carries the exp (twice the measured distance, an ulp = 2 EPS at most) and one IEEE division, the
            # addition of log 2b one rounding more
            out[i, k] = ((order + EPS) * (ratio + l2b).sum() + (2 * EXP_ULP * 2 * EPS + EPS) * ratio.sum(),
                         (order + 2 * EXP_ULP * 2 * EPS) * b[i][v].sum(), order * e[i][v].sum())
    return out


@pytest.mark.parametrize("K", [1, 3, 12])
@pytest.mark.parametrize("shape", C.STATS_SHAPES)
def test_records_and_tables_equal_the_statement(shape, K):
    ue = UE()
    ref = ref_stats(shape, K)
    st = call(shape, K)
    assert st.names == [n for n, _ in _classes(K)] and tuple(st.records.shape) == (shape[0], K, ue.RECORD_BYTES)
    assert tuple(st.tables.shape) == (shape[0], K, 3, 512)
    got = fields(st)
    for key in ("n", "bad", "cover", "hist", "tables"):
        assert np.array_equal(got[key], ref[key]), (shape, K, key)
    err, bound = np.abs(got["sums"] - ref["sums"]), sum_bounds(shape, K)
    print(shape, K, "sums: largest error / bound", (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (shape, K, err, bound)
    assert not st.records.view(torch.int64)[..., 7].any()                     # the padding
    assert ref["n"].sum() > 0 and ref["bad"].sum() >= 2
    if K == 12:
        assert (ref["n"][:, 8] == 0).all() and not got["tables"][:, 8].any()  # "cutlery": the class nobody is in
    if K == 3:                                                                # overlapping ranges: a pixel in three classes
        assert (ref["n"][:, 2] > 0).any() and (ref["n"][:, 2] <= ref["n"][:, 1]).all() and (ref["n"][:, 1] <= ref["n"][:, 0]).all()
    if shape == (3, 1, 40):                                                   # the image without a pixel inside the gate
        assert not got["n"][0].any() and not got["bad"][0].any() and not got["tables"][0].any()


@pytest.mark.parametrize("K", [1, 12])
@pytest.mark.parametrize("shape", C.STATS_SHAPES)
def test_n_bad_and_the_error_histogram_are_those_of_depth_stats(shape, K):
    """On inputs without an unusable u, n, bad and table row 1 equal pd_depth_stats' n, bad and hist."""
    from polardepth import depth_eval
    gt, pred, unc, mask = C.stats_case(*shape)
    u = np.clip(np.nan_to_num(np.array(unc), nan=0.5), 0.0, 1.0).astype(np.float32)
    args = dict(mask=_dev(mask) if K > 1 else None, classes=_classes(K), min_depth=C.MIN_D, max_depth=C.MAX_D)
    us = UE().uncertainty_stats(_dev(pred), _dev(gt), _dev(u), b_range=C.B_RANGE, **args)
    ds = depth_eval.depth_stats(_dev(pred), _dev(gt), **args)
    torch.cuda.synchronize()
    assert torch.equal(us.n, ds.n) and torch.equal(us.bad, ds.bad) and int(ds.bad.sum()) >= 1
    assert torch.equal(us.tables[:, :, 1], ds.hist.long())


def test_one_case_per_rule():
    """u exactly 0 and 1 and just inside; the coverage thresholds; a finite u beyond [0, 1] and a NaN are bad."""
    ue = UE()
    one = np.float32(1)
    u = np.array([[[0.0, 1.0, np.nextafter(one, 0), 0.5, 0.5, 0.5, -0.25, 1.5, np.nan, 0.5]]], np.float32)
    b_half = float(np.exp(R.fma64(np.array([0.5]), np.log(1000.0), np.log(0.0005))[0]))      # 15.8 mm
    gt = np.ones((1, 1, 10), np.float32)
    pred = gt.copy()
    pred[0, 0, 3] = 1 - np.float32(0.5 * b_half)          # inside the central 50 %
    pred[0, 0, 4] = 1 - np.float32(1.5 * b_half)          # inside the central 90 % only
    pred[0, 0, 5] = 1 - np.float32(3.0 * b_half)          # outside both
    pred[0, 0, 9] = np.nan
    st = ue.uncertainty_stats(_dev(pred), _dev(gt), _dev(u), classes=[("all", None)], b_range=C.B_RANGE)
    f = fields(st)
    assert f["n"][0, 0] == 6 and f["bad"][0, 0] == 4 and f["cover"][0, 0].tolist() == [4, 5]
    assert f["hist"][0, 0, 0] == 1 and f["hist"][0, 0, 511] == 2 and f["hist"][0, 0, 256] == 3 and f["hist"][0, 0].sum() == 6
    ref = R.stats(pred, gt, u, None, [(1, 0)], C.B_RANGE, 0.1, 2.0)
    assert np.array_equal(f["tables"], ref["tables"]) and f["tables"][0, 0, 1, 0] == 3       # three pixels without error
    e_um = [int(round((1.0 - float(pred[0, 0, i])) * 1e6)) for i in (3, 4, 5)]
    assert f["tables"][0, 0, 0, 256] == sum(e_um) == f["tables"][0, 0, 2].sum()


def test_metrics_pool_and_report():
    ue = UE()
    shape = C.STATS_SHAPES[3]
    ref = ref_stats(shape, 12)
    st = call(shape, 12)
    m = st.metrics()
    want = ue.metrics_from_fields(ref["n"], ref["cover"], ref["sums"], ref["hist"], ref["tables"])
    assert m.shape == (2, 12, 10) and np.allclose(m, want, rtol=1e-9, atol=0.0, equal_nan=True)
    assert np.array_equal(m[..., 5:9], want[..., 5:9], equal_nan=True)       # AUSE / AURG come from integers: equal
    st += call(shape, 12)
    pooled = st.pooled()
    tabs = st.pooled_tables()
    assert isinstance(tabs[0, 0, 0], int) and np.array_equal(tabs, 2 * ref["tables"].astype(object).sum(0))
    tot = ue.metrics_from_fields(2 * ref["n"].sum(0), 2 * ref["cover"].sum(0), 2 * ref["sums"].sum(0), 2 * ref["hist"].sum(0), tabs)
    assert np.allclose(pooled, tot, rtol=1e-9, atol=0.0, equal_nan=True) and np.array_equal(pooled[:, 5:9], tot[:, 5:9], equal_nan=True)
    assert np.array_equal(st.pooled_bad().cpu().numpy(), 2 * ref["bad"].sum(0))
    text = ue.format_report(st.names, np.nanmean(m, 0), pooled, st.pooled_bad().cpu().numpy())
    assert "ause_mm" in text and "glass" in text and "cutlery" not in text
    with pytest.raises(ValueError, match="cannot pool"):
        st += call(shape, 1)
    b = ue.scale_of(_dev(np.array([0.0, 0.5, 1.0], np.float32)), C.B_RANGE).cpu().numpy()
    assert b[0] == np.float32(0.0005) and b[2] == np.float32(0.5) and abs(b[1] - 0.0158113883) < 1e-8


def test_two_calls_give_identical_bytes():
    shape = C.STATS_SHAPES[3]
    a = call(shape, 12)
    junk = torch.full((1 << 22,), 0x5A, dtype=torch.uint8, device="cuda")      # whatever the allocator hands out next is dirty
    del junk
    b = call(shape, 12)
    torch.cuda.synchronize()
    assert a.records.cpu().numpy().tobytes() == b.records.cpu().numpy().tobytes()
    assert torch.equal(a.tables, b.tables) and int(a.n.sum()) > 0


def test_a_captured_call_replays_the_eager_records():
    ue = UE()
    gt, pred, unc, mask = C.stats_case(*C.STATS_SHAPES[3])
    pred_t, gt_t, unc_t, mask_t = _dev(pred), _dev(gt), _dev(unc), _dev(mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires (builds the table)
        eager = ue.uncertainty_stats(pred_t, gt_t, unc_t, mask=mask_t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        st = ue.uncertainty_stats(pred_t, gt_t, unc_t, mask=mask_t)
    st.records.zero_()
    st.tables.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.records, eager.records) and torch.equal(st.tables, eager.tables)
    pred_t.copy_(pred_t.flip(0))                        # the replay reads the tensors of its capture: new data, new records
    graph.replay()
    again = ue.uncertainty_stats(pred_t, gt_t, unc_t, mask=mask_t)
    torch.cuda.synchronize()
    assert torch.equal(st.records, again.records) and torch.equal(st.tables, again.tables)
    assert not torch.equal(st.tables, eager.tables)
