"""Evaluation.test_consistency on the GPU: finite tables, pooled records equal to the NumPy statement (tests/consistency_ref.py)
applied to the very depths ``predict`` returned for the same batches, both settings of ``visible``, per-view tables that pool
to the all-views table, and ``test`` undisturbed."""
import numpy as np
import pytest
import torch

import consistency_ref as R

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=2)
IDS = (-1, 1)


@pytest.fixture(scope="module")
def ev():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    return Evaluation(**KW)


def _lohi():
    from polardepth import consistency_eval
    return [(1, 0) if r is None else tuple(r) for _, r in consistency_eval.DEFAULT_CLASSES]


def _statement(ev, depths_seen, visible):
    """The statement over the loader's batches, with the depths ``predict`` returned (frame 0, then the neighbours)."""
    total = None
    loader = ev._consistency_loaders[IDS]
    assert len(depths_seen) == len(loader) * (1 + len(IDS))
    for b, inputs in enumerate(loader):
        d0, dn = depths_seen[3 * b][:, 0], np.stack([depths_seen[3 * b + 1 + f][:, 0] for f in range(len(IDS))], 1)
        T = np.stack([inputs[("poses", i)].numpy() for i in IDS], 1)
        fv = np.stack([inputs[("frame_valid", i)].numpy() for i in IDS], 1)
        K, inv_K = inputs[("K", 0)].numpy(), inputs[("inv_K", 0)].numpy()
        vis = None
        if visible == "auto":
            gt0 = inputs["depth_gt"][:, 0].numpy()
            gts = np.stack([inputs[("neighbour", i)]["depth_gt"][:, 0].numpy() for i in IDS], 1)
            vis = (R.pairs(gt0, gts, T, K, inv_K, frame_valid=fv, min_depth=ev.min_depth, max_depth=ev.max_depth)["level"] >= 4)
            vis = vis.astype(np.uint8)
        r = R.consistency(d0, dn, T, K, inv_K, frame_valid=fv, visible=vis, mask=inputs[("mask", 0, 0)][:, 0].numpy(),
                          classes=_lohi(), min_depth=ev.min_depth, max_depth=ev.max_depth)
        part = {k: r[k].sum(0) for k in ("n", "counters", "sums", "hist")}
        total = part if total is None else {k: total[k] + part[k] for k in part}
    return total


@pytest.mark.parametrize("visible", ["auto", None])
def test_tables_are_finite_and_equal_the_statement(ev, monkeypatch, capsys, visible):
    from polardepth import consistency_eval
    seen = []
    predict = ev.predict

    def recording(inputs):
        d = predict(inputs)
        seen.append(d.cpu().numpy())
        return d
    monkeypatch.setattr(ev, "predict", recording)
    res = ev.test_consistency(ids=IDS, visible=visible)
    text = capsys.readouterr().out
    assert "consistency (views [-1, 1]" in text and "glass" in text and "median_rel%" in text
    assert ("mutually visible" in text) == (visible == "auto")
    assert list(res) == [n for n, _ in consistency_eval.DEFAULT_CLASSES]
    want = _statement(ev, seen, visible)
    for k, name in enumerate(res):
        r = res[name]
        assert r["pooled"].shape == (len(consistency_eval.METRIC_NAMES),)
        assert r["n"] == want["n"][k], (name, r["n"], want["n"][k])
        assert np.array_equal(r["counters"], want["counters"][k]), (name, r["counters"], want["counters"][k])
        assert np.array_equal(r["hist"], want["hist"][k]), name
        assert np.allclose(r["sums"], want["sums"][k], rtol=1e-11, atol=0.0), (name, r["sums"], want["sums"][k])
        if r["n"] > 0:
            assert np.isfinite(r["pooled"]).all(), (name, r["pooled"])
    assert res["all"]["n"] > 0 and res["objects"]["n"] > 0
    c = dict(zip(consistency_eval.COUNTER_NAMES, res["all"]["counters"]))
    assert c["absent"] == 0 and (c["filtered"] > 0) == (visible == "auto")
    pixels = len(ev._consistency_loaders[IDS]) * KW["batch_size"] * KW["height"] * KW["width"]
    assert res["all"]["n"] + sum(res["all"]["counters"][3:]) == pixels * len(IDS)


def test_the_ground_truth_is_consistent_with_itself(ev, monkeypatch):
    """The synthetic neighbours show frame 0's surface from the moved camera: scored on the ground truth, every compared
    pair is tight."""
    monkeypatch.setattr(ev, "predict", lambda inputs: inputs["depth_gt"])
    res = ev.test_consistency(ids=IDS, visible=None)
    a = res["all"]
    assert a["n"] > 0 and a["counters"][2] == a["n"] and a["pooled"][5] < 0.2      # median e_rel below 0.2 %


def test_export_keeps_the_confirmed_points_at_the_fused_depth(ev, monkeypatch):
    """tools/export_pointcloud.py --consistent M, on the ground truth as the prediction: the gate keeps the pixels that M
    views confirm and the depth there is the fused one, within the tight threshold of the single one."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_pointcloud as E
    monkeypatch.setattr(ev, "predict", lambda inputs: inputs["depth_gt"])
    gt = ev.test_loader.dataset[0]["depth_gt"][None].to(ev.device)
    kept = {}
    for M in (1, 2):
        depth, gate = E.consistent_depth(ev, 0, gt, gt, M)
        assert depth.shape == gt.shape and gate.shape == gt.shape
        keep = gate > 0
        kept[M] = int(keep.sum())
        assert torch.equal(gate[keep], gt[keep]) and ((depth[keep] - gt[keep]).abs() <= 0.01 * gt[keep]).all()
    assert 0 < kept[2] < kept[1] < int((gt > 0).sum())
    with pytest.raises(ValueError, match="neighbouring frames"):
        E.consistent_depth(ev, 0, gt, gt, 3)


def test_per_view_tables_pool_to_the_all_views_table(ev, capsys):
    res = ev.test_consistency(ids=IDS, visible="auto", per_view=True)
    text = capsys.readouterr().out
    assert "consistency (view -1," in text and "consistency (view 1," in text
    views = res.pop("views")
    assert list(views) == list(IDS)
    for name, r in res.items():
        assert r["n"] == sum(views[i][name]["n"] for i in IDS), name
        assert np.array_equal(r["counters"], sum(views[i][name]["counters"] for i in IDS)), name
        assert np.array_equal(r["hist"], sum(views[i][name]["hist"] for i in IDS)), name
        assert np.allclose(r["sums"], sum(views[i][name]["sums"] for i in IDS), rtol=1e-11, atol=0.0), name


def test_bad_arguments_and_test_is_undisturbed(ev, capsys):
    with pytest.raises(ValueError, match="visible"):
        ev.test_consistency(visible="gt")
    with pytest.raises(ValueError, match="ids"):
        ev.test_consistency(ids=(0, 1))
    capsys.readouterr()
    before = ev.test()
    text_before = capsys.readouterr().out
    ev.test_consistency()
    capsys.readouterr()
    after = ev.test()
    text_after = capsys.readouterr().out
    assert text_before == text_after and text_before.startswith("all ") and set(before) == set(after)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
