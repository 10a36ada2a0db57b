"""Evaluation.test_depth on the GPU: its per-image figures are those of ``test`` (eleven pd_depth_metrics launches per batch)
for the classes both report; "objects" is the union of its materials; and median scaling undoes a constant factor on the
prediction.

``test`` accumulates in fp32 and takes log g - log p in fp32; 1e-5 is the tolerance tests/test_loss_gpu.py uses for its
figures.  The integer fields must be equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=2)
MATERIALS_OF_OBJECTS = ("box", "bottle", "can", "cup", "remote", "teapot", "cutlery", "glass")      # grey 20 .. 160


@pytest.fixture(scope="module")
def ev():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    return Evaluation(**KW)


def test_per_image_figures_are_those_of_test(ev, capsys):
    from polardepth import depth_eval
    old = ev.test()
    res = ev.test_depth()
    text = capsys.readouterr().out
    assert "depth (unscaled)" in text and "pooled" in text and "per-image" in text and "glass" in text and "abs_rel" in text
    assert list(res) == [n for n, _ in depth_eval.DEFAULT_CLASSES] and len(res) == 12
    assert set(old) <= set(res) and "all" in old and len(old) == 11 and "objects" not in old
    for name, want in old.items():
        r = res[name]
        assert set(r) == {"per_image", "pooled", "bad"} and r["per_image"].shape == (13,) and r["pooled"].shape == (13,)
        print(name, "test_depth", r["per_image"][:7], "test", want, "max diff", np.abs(r["per_image"][:7] - want).max())
        assert np.allclose(r["per_image"][:7], want, rtol=1e-5, atol=1e-5), name
        assert r["bad"] == 0 and r["pooled"][12] > 0          # predict() clamps: every prediction is finite


def test_objects_is_the_union_of_its_materials(ev):
    res = ev.test_depth()
    counts = lambda r: np.rint(np.concatenate([[r["pooled"][12]], r["pooled"][[4, 5, 6, 9, 10, 11]] * r["pooled"][12]]))
    union = sum(counts(res[m]) for m in MATERIALS_OF_OBJECTS)
    assert np.array_equal(counts(res["objects"]), union) and union[0] > 0
    assert res["objects"]["bad"] == sum(res[m]["bad"] for m in MATERIALS_OF_OBJECTS)
    everything = sum(counts(res[m]) for m in MATERIALS_OF_OBJECTS + ("table", "wall"))
    assert (counts(res["all"]) >= everything).all() and counts(res["all"])[0] > everything[0]      # mask value 0 is in no material


def _batches(n_batches=2, N=2, H=64, W=96):
    """Ground truth in (0.3, 1.0) with holes, and a prediction in (0.3, 1.0) that moves every pixel without moving it across
    any class median: between the smallest and the largest class median it equals the truth, above and below it is pulled
    towards or pushed away from that band.  The medians of every class are then those of the truth and np.median's factor is
    exactly 1."""
    from polardepth import depth_eval
    rng = np.random.default_rng(17)
    out = []
    for _ in range(n_batches):
        gt = rng.uniform(0.32, 0.98, (N, 1, H, W)).astype(np.float32)
        mask = (rng.integers(0, 11, (N, 1, H, W)) * 20).astype(np.int32)
        hole = rng.random((N, 1, H, W)) < 0.1
        pred = gt.copy()
        for i in range(N):
            meds = []
            for _, r in depth_eval.DEFAULT_CLASSES:
                sel = ~hole[i] & (np.ones_like(hole[i]) if r is None else (mask[i] >= r[0]) & (mask[i] <= r[1]))
                v = np.sort(gt[i][sel])
                meds += [v[(v.size - 1) // 2], v[v.size // 2]]
            lo, hi = min(meds), max(meds)
            eta = rng.uniform(-0.5, 0.5, gt[i].shape).astype(np.float32)
            p = np.where(gt[i] > hi, gt[i] + eta * (gt[i] - hi), np.where(gt[i] < lo, gt[i] - eta * (lo - gt[i]), gt[i]))
            pred[i] = np.clip(p, 0.31, 0.99)
            assert ((pred[i] > hi) == (gt[i] > hi)).all() and ((pred[i] < lo) == (gt[i] < lo)).all()
        gt[hole] = 0.0
        out.append({"depth_gt": torch.from_numpy(gt), ("mask", 0, 0): torch.from_numpy(mask),
                    "pred": torch.from_numpy(pred.astype(np.float32))})
    return out


def test_median_scaling_undoes_a_constant_factor(ev, monkeypatch):
    batches = _batches()
    factor = {"f": 1.0}
    monkeypatch.setattr(ev, "test_loader", batches)
    monkeypatch.setattr(ev, "predict", lambda inputs: inputs["pred"] * factor["f"])
    for b in batches:                                      # the clamps do not bite: neither on 1.7 x the prediction ...
        p = b["pred"]
        assert 0.3 < p.min() and p.max() < 1.0 and ev.min_depth < 1.7 * p.min() and 1.7 * p.max() < ev.max_depth
        g = b["depth_gt"][b["depth_gt"] > 0]
        assert 0.3 < g.min() and g.max() < 1.0
    plain = ev.test_depth()
    same = ev.test_depth(median_scaling="numpy")           # the factor is exactly 1: the same records, bit for bit
    for name in plain:
        assert np.array_equal(plain[name]["per_image"], same[name]["per_image"], equal_nan=True), name
        assert np.array_equal(plain[name]["pooled"], same[name]["pooled"], equal_nan=True), name
    factor["f"] = 1.7
    off = ev.test_depth()
    scaled = ev.test_depth(median_scaling="numpy")
    # ... nor on the rescaled one: it is the original within a few fp32 roundings (1.7 p, the two medians, their ratio, the
    # product: under 4 x 2^-24 = 2.4e-7 relative), so abs_rel, sq_rel, rmse and rmse_log move by less than 1e-6 and a
    # threshold count by the rare pixel whose ratio lies that close to its threshold
    for name in plain:
        a, b, n = plain[name]["per_image"], scaled[name]["per_image"], plain[name]["pooled"][12]
        assert n > 0 and scaled[name]["pooled"][12] == n and scaled[name]["bad"] == 0, name
        print(name, "unscaled original", a[:7], "scaled 1.7x", b[:7], "unscaled 1.7x", off[name]["per_image"][:7])
        assert np.allclose(a[:4], b[:4], rtol=0.0, atol=1e-5), name
        images = len(batches) * KW["batch_size"]           # two such pixels on an image of the class's average size
        assert np.allclose(a[4:7], b[4:7], rtol=0.0, atol=1e-5 + 2.0 * images / n), name
        assert off[name]["per_image"][0] > a[0] + 0.3, name   # without the scaling the factor is all there is to see
