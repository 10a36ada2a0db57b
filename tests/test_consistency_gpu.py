"""pd_depth_consistency / polardepth.consistency_eval on the GPU against the NumPy statement (tests/consistency_ref.py, checked
by tests/test_consistency_ref.py) applied to the very arrays handed to the kernel.

n, the eight counters, hist, level and n_cons must be equal, fused bit-equal.  The four sums: rtol 1e-11, the convention of
tests/test_depth_stats_gpu.py and for the same reason -- any order of n non-negative terms errs by at most (n - 1) 2^-53 of
the sum, 7.5e-12 at the 67584 pairs of the largest image here and 4.4e-13 at the next largest; the device's division and
square root add at most an ulp per term.  The observed figure is printed.  No case is left out of any comparison."""
import functools
import itertools

import numpy as np
import pytest
import torch

import consistency_ref as R

pytestmark = pytest.mark.gpu

# (N, F, H, W): more than one workgroup per image, W % 4 == 1 | less than two waves | three views | beyond the cap of 64
# workgroups per image (66 x 1024 pixels)
SHAPES = [(2, 2, 37, 53), (2, 1, 8, 12), (1, 3, 24, 40), (1, 1, 264, 256)]
SMALL = SHAPES[:3]
MIN_D, MAX_D = 0.1, 2.0
SCALES = np.float32([1.0, 1.005, 0.995, 1.015, 0.985, 1.03, 0.97, 1.1, 0.9, 1.3, 0.7])


def CE():
    from polardepth import consistency_eval
    return consistency_eval


def _classes(K):
    ce = CE()
    if K == 1:
        return [("all", None)]
    if K == 12:
        return list(ce.DEFAULT_CLASSES)
    assert K == 16
    return list(ce.DEFAULT_CLASSES) + [("a", (40, 60)), ("b", (0, 0)), ("none", (500, 600)), ("every", (-5, 1000))]


def _lohi(classes):
    return [(1, 0) if r is None else tuple(r) for _, r in classes]


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a writable copy: the scene arrays are read-only


@functools.lru_cache(maxsize=None)
def scene(N, F, H, W):
    """Host arrays (never modified): the analytic plane pair with small poses, the last view of the last item moved far
    enough for pixels to leave the frame; the source depths scaled in 4 x 4 blocks by 1 +- {0, 0.5, 1.5, 3, 10, 30} %; 3 %
    holes in either map; NaN, inf and 2.5 m entries; at F > 1 view 0 of item 0 absent; the instance mask."""
    rng = np.random.default_rng(1000 * N + 100 * F + H + W)
    depth0, depths, T, K, inv_K = R.plane_pair(N, F, H, W, seed=H * W + F, big_last=True)
    blocks = rng.integers(0, len(SCALES), (N, F, (H + 3) // 4, (W + 3) // 4))
    depths = (depths * SCALES[np.repeat(np.repeat(blocks, 4, 2), 4, 3)[:, :, :H, :W]]).astype(np.float32)
    depth0 = depth0.copy()
    depth0[rng.random(depth0.shape) < 0.03] = 0.0
    depths[rng.random(depths.shape) < 0.03] = 0.0
    depth0[0, 1, 2], depth0[-1, 2, 3], depth0[0, 3, 4] = np.nan, np.inf, 2.5
    depths[0, 0, 2, 5], depths[-1, -1, 4, 4], depths[0, 0, 5, 7] = np.nan, np.inf, 2.5
    frame_valid = np.ones((N, F), np.float32)
    if F > 1:
        frame_valid[0, 0] = 0.0
    mask = (rng.integers(0, 11, (N, H, W)) * 20).astype(np.int32)
    out = (depth0, depths, T, K, inv_K, frame_valid, mask)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_pairs(shape, fuse_level=4, vis_level=None):
    """The statement's per-pair figures for a scene, computed once; with ``vis_level`` a `visible` mask made of the
    statement's own first call (level >= vis_level) goes in."""
    depth0, depths, T, K, inv_K, fv, _ = scene(*shape)
    visible = None
    if vis_level is not None:
        visible = (ref_pairs(shape)["level"] >= vis_level).astype(np.uint8)
    pr = R.pairs(depth0, depths, T, K, inv_K, frame_valid=fv, visible=visible, min_depth=MIN_D, max_depth=MAX_D,
                 fuse_level=fuse_level)
    pr["visible"] = visible
    return pr


@functools.lru_cache(maxsize=None)
def ref_records(shape, K, masked, fuse_level=4, vis_level=None):
    mask = scene(*shape)[6] if masked else None
    return R.records(ref_pairs(shape, fuse_level, vis_level), mask, _lohi(_classes(K)))


def run(shape, K=1, masked=False, fuse_level=4, visible=None, want=("level", "n_cons", "fused"), tensors=None):
    depth0, depths, T, Km, inv_K, fv, mask = tensors if tensors is not None else [_dev(a) for a in scene(*shape)]
    return CE().consistency(depth0, depths, T, Km, inv_K, frame_valid=fv, mask=mask if masked else None, classes=_classes(K),
                            visible=_dev(visible), min_depth=MIN_D, max_depth=MAX_D, fuse_level=fuse_level, want=want)


def compare(st, pr, rec, what):
    torch.cuda.synchronize()
    got = {"n": st.n.cpu().numpy(), "counters": st.counters.cpu().numpy(), "hist": st.hist.cpu().numpy().astype(np.int64)}
    for k in ("n", "counters", "hist"):
        assert np.array_equal(got[k], rec[k]), (what, k, got[k] if k != "hist" else None, rec[k] if k != "hist" else None)
    sums = st.sums.cpu().numpy()
    rel = np.abs(sums - rec["sums"]) / np.maximum(np.abs(rec["sums"]), 1e-300)
    print(what, "sums: max rel err", rel.max())
    assert np.allclose(sums, rec["sums"], rtol=1e-11, atol=0.0), (what, rel.max())
    assert np.array_equal(st.records.view(torch.int64)[..., 13].cpu().numpy(), np.zeros_like(rec["n"])), what      # the padding
    if st.level is not None:
        lv = st.level.cpu().numpy()
        assert lv.dtype == np.uint8 and np.array_equal(lv, pr["level"]), (what, np.argwhere(lv != pr["level"])[:5])
    if st.n_cons is not None:
        nc = st.n_cons.cpu().numpy()
        assert nc.dtype == np.uint8 and np.array_equal(nc, pr["n_cons"]), (what, np.argwhere(nc != pr["n_cons"])[:5])
    if st.fused is not None:
        fu = st.fused.cpu().numpy()
        assert fu.dtype == np.float32 and not np.isnan(pr["fused"]).any()
        assert np.array_equal(fu.view(np.uint32), pr["fused"].view(np.uint32)), (what, np.argwhere(fu != pr["fused"])[:5])


# ------------------------------------------------------------------------------------------------ the scenes
@pytest.mark.parametrize("shape", SMALL)
def test_the_scenes_exercise_every_outcome_and_level(shape):
    """On the STATEMENT's records alone: every outcome and level has at least 10 members (1 at the 8 x 12 shape)."""
    pr, rec = ref_pairs(shape), ref_records(shape, 1, False)
    floor = 1 if shape[2:] == (8, 12) else 10
    c = rec["counters"][:, 0].sum(0)
    names = ["invalid", "outside", "hole"] + (["absent"] if shape[1] > 1 else [])
    print(shape, "compared", rec["n"].sum(), dict(zip(R.COUNTERS, c)), "levels", np.bincount(pr["level"].ravel(), minlength=5),
          "open bin", rec["hist"][..., -1].sum())
    for name in names:
        assert c[R.COUNTERS.index(name)] >= floor, (shape, name, c)
    levels = np.bincount(pr["level"].ravel(), minlength=5)
    assert (levels[1:] >= floor).all(), (shape, levels)
    assert rec["hist"][..., -1].sum() >= floor                               # the open bin
    assert (rec["n"] + rec["counters"][..., 3:].sum(-1) == rec["pixels"] * shape[1]).all()
    assert 0 < pr["n_cons"].max() <= shape[1] and (pr["fused"] > 0).any()


# ------------------------------------------------------------------------------------------------ against the statement
@pytest.mark.parametrize("K,masked", [(1, False), (1, True), (12, True), (16, True)])
@pytest.mark.parametrize("shape", SHAPES)
def test_records_and_maps_equal_the_statement(shape, K, masked):
    st = run(shape, K, masked)
    assert tuple(st.records.shape) == (shape[0], K, CE().RECORD_BYTES)
    compare(st, ref_pairs(shape), ref_records(shape, K, masked), (shape, K, masked))
    if K == 16:
        assert (st.n[:, 14] == 0).all() and (st.counters[:, 14] == 0).all()       # the class nobody is in
        assert torch.equal(st.records[:, 15], st.records[:, 0])                    # the range that holds every mask value


@pytest.mark.parametrize("fuse_level", [2, 3])
def test_the_other_fuse_levels(fuse_level):
    shape = SHAPES[0]
    st = run(shape, 12, True, fuse_level=fuse_level)
    pr = ref_pairs(shape, fuse_level)
    assert (pr["n_cons"] != ref_pairs(shape)["n_cons"]).any()
    compare(st, pr, ref_records(shape, 12, True, fuse_level), (shape, "fuse", fuse_level))


@pytest.mark.parametrize("shape", SMALL)
def test_visible_built_from_a_first_call(shape):
    first = run(shape, 1, False, want=("level",))
    vis = first.level >= 3
    pr = ref_pairs(shape, 4, 3)
    assert np.array_equal(vis.cpu().numpy().astype(np.uint8), pr["visible"])
    depth0, depths, T, K, inv_K, fv, mask = [_dev(a) for a in scene(*shape)]
    st = CE().consistency(depth0, depths, T, K, inv_K, frame_valid=fv, mask=mask, classes=_classes(12), visible=vis,
                          min_depth=MIN_D, max_depth=MAX_D, want=("level", "n_cons", "fused"))
    rec = ref_records(shape, 12, True, 4, 3)
    assert rec["counters"][:, 0, 5].sum() >= (1 if shape[2:] == (8, 12) else 10)      # `filtered`, on the statement alone
    compare(st, pr, rec, (shape, "visible"))
    assert (st.n == st.counters[..., 1]).all()                              # whoever is left meets the mid level


def test_visibility_is_the_tight_level_of_the_same_call():
    shape = SHAPES[0]
    depth0, depths, T, K, inv_K, fv, _ = [_dev(a) for a in scene(*shape)]
    vis = CE().visibility(depth0, depths, T, K, inv_K, frame_valid=fv, min_depth=MIN_D, max_depth=MAX_D)
    assert vis.dtype == torch.bool and np.array_equal(vis.cpu().numpy(), ref_pairs(shape)["level"] >= 4)


@pytest.mark.parametrize("want", [c for r in range(4) for c in itertools.combinations(("level", "n_cons", "fused"), r)])
def test_each_want_combination(want):
    shape = SHAPES[0]
    st = run(shape, 12, True, want=want)
    assert (st.level is not None) == ("level" in want) and (st.n_cons is not None) == ("n_cons" in want)
    assert (st.fused is not None) == ("fused" in want)
    compare(st, ref_pairs(shape), ref_records(shape, 12, True), (shape, want))


# ------------------------------------------------------------------------------------------------ reproducibility, capture
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]])
def test_two_calls_give_identical_bytes(shape):
    tensors = [_dev(a) for a in scene(*shape)]
    a, b = run(shape, 12, True, tensors=tensors), run(shape, 12, True, tensors=tensors)
    torch.cuda.synchronize()
    assert a.records.data_ptr() != b.records.data_ptr() and torch.equal(a.records, b.records)
    assert torch.equal(a.level, b.level) and torch.equal(a.n_cons, b.n_cons)
    assert a.fused.cpu().numpy().tobytes() == b.fused.cpu().numpy().tobytes()


def test_captured_call_replays_the_eager_records():
    shape = SHAPES[0]
    tensors = [_dev(a) for a in scene(*shape)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires
        eager = run(shape, 12, True, tensors=tensors)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        st = run(shape, 12, True, tensors=tensors)
    st.records.zero_()
    st.level.zero_()
    st.fused.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.records, eager.records) and torch.equal(st.level, eager.level)
    assert torch.equal(st.n_cons, eager.n_cons) and st.fused.cpu().numpy().tobytes() == eager.fused.cpu().numpy().tobytes()
    # the replay reads the tensors of its capture: new data, new records
    tensors[1].copy_(tensors[1].flip(1))
    graph.replay()
    again = run(shape, 12, True, tensors=tensors)
    torch.cuda.synchronize()
    assert torch.equal(st.records, again.records) and not torch.equal(st.records, eager.records)


# ------------------------------------------------------------------------------------------------ the report
def test_metrics_and_the_pool():
    ce = CE()
    shape = SHAPES[0]
    st = run(shape, 12, True)
    rec = ref_records(shape, 12, True)
    m = st.metrics().cpu().numpy()
    assert m.shape == (shape[0], 12, len(ce.METRIC_NAMES))
    n = rec["n"].astype(np.float64)
    total = (rec["pixels"] * shape[1]).astype(np.float64)
    col = {name: m[..., j] for j, name in enumerate(ce.METRIC_NAMES)}
    ok = n > 0
    assert ok[:, 0].all()
    np.testing.assert_array_equal(col["n"], n)
    np.testing.assert_allclose(col["compared"][ok], (n / total)[ok], rtol=1e-14)
    for j, name in enumerate(("loose", "mid", "tight")):
        np.testing.assert_allclose(col[name][ok], (rec["counters"][..., j] / n)[ok], rtol=1e-14)
    for j, name in enumerate(("invalid", "absent", "filtered", "outside", "hole")):
        np.testing.assert_allclose(col[name][ok], (rec["counters"][..., 3 + j] / total)[ok], rtol=1e-14)
    np.testing.assert_allclose(col["mean_rel%"][ok], (100 * rec["sums"][..., 1] / n)[ok], rtol=1e-10)
    np.testing.assert_allclose(col["mean_px"][ok], (rec["sums"][..., 0] / n)[ok], rtol=1e-10)
    np.testing.assert_allclose(col["rms_px"][ok], np.sqrt(rec["sums"][..., 2] / n)[ok], rtol=1e-10)
    # the median lies in the bin that holds the n/2-th value
    pr = ref_pairs(shape)
    for i in range(shape[0]):
        e = np.sort(pr["e_rel"][i][pr["outcome"][i] == R.COMPARED])
        true = 100 * e[(len(e) - 1) // 2]
        assert abs(col["median_rel%"][i, 0] - min(true, 25.0)) <= ce.BIN_PERCENT, (col["median_rel%"][i, 0], true)
    # the pool: two calls added on the device
    other = run(shape, 12, True)
    st += other
    p = st.pooled().cpu().numpy()
    assert p.shape == (12, len(ce.METRIC_NAMES))
    np.testing.assert_array_equal(p[:, -1], 2 * n.sum(0))
    np.testing.assert_allclose(p[0, 1:4], rec["counters"][:, 0, :3].sum(0) / n[:, 0].sum(), rtol=1e-14)
    with pytest.raises(ValueError, match="cannot pool"):
        st += run(shape, 1, False)
