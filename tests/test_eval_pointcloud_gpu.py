"""Evaluation.test_pointcloud on the GPU: the report equals the NumPy statement (tests/pointcloud_ref.py) applied per image
to what ``predict`` returns; the brute-force route gives the same bits; and nothing else moves -- test() and predict() give
the bits they give without it.

Integer fields (point counts, `bad`, `unmatched`, hence the precision / recall shares under the F-scores) must be equal; the
other figures agree to rtol 1e-9 (the kernel's fp64 sums are within 1e-11 of the statement's,
tests/test_pointcloud_gpu.py; the metrics divide them by equal integers)."""
import os

import numpy as np
import pytest
import torch

import pointcloud_ref as R

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=4)


@pytest.fixture(scope="module")
def ev():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    return Evaluation(**KW)


def _statement(ev):
    """Per batch: the statement's clouds of the predicted and the true depth (both gated by the truth), its distances both
    ways and its records; then the two conventions with the Python layer's formulas on host tensors (pinned against plain
    NumPy in tests/test_pointcloud_ref.py -- this file checks the wiring: which depth, which gate, which direction is which,
    the classes, the two ways of averaging)."""
    from polardepth import pointcloud as pc
    lohi = [(1, 0) if r is None else r for _, r in pc.DEFAULT_CLASSES]
    edges = pc.edges2_numpy()
    acc, comp = [], []
    for inputs in ev.test_loader:
        inputs = {k: v.cuda() for k, v in inputs.items()}
        depth = ev.predict(inputs)[:, 0].cpu().numpy()
        gt, K = inputs["depth_gt"][:, 0].cpu().numpy(), inputs[("K", 0)].cpu().numpy()
        mask = inputs[("mask", 0, 0)][:, 0].cpu().numpy()
        H, W = gt.shape[1:]
        p, t = R.backproject(depth, K, gt, 0.1, 2.0), R.backproject(gt, K, None, 0.1, 2.0)
        acc.append(R.stats(R.nn_d2(p, t), p, mask, lohi, edges, H, W))
        comp.append(R.stats(R.nn_d2(t, p), t, mask, lohi, edges, H, W))
    keys = ("n", "bad", "unmatched", "sum_d", "hist")
    fa = {k: torch.from_numpy(np.concatenate([x[k] for x in acc])) for k in keys}
    fc = {k: torch.from_numpy(np.concatenate([x[k] for x in comp])) for k in keys}
    four = lambda f, red: tuple(red(f[k]) for k in ("n", "unmatched", "sum_d", "hist"))
    m = pc.metrics_from_fields(four(fa, lambda x: x), four(fc, lambda x: x))                       # [images, K, 9]
    valid = (fa["n"] > 0) & (fc["n"] > 0)
    per_image = torch.where(valid[..., None], m, torch.zeros_like(m)).sum(0) / valid.sum(0)[:, None].double()
    pooled = pc.metrics_from_fields(four(fa, lambda x: x.sum(0)), four(fc, lambda x: x.sum(0)))
    P = pc.shares_from_fields(fa["n"].sum(0), fa["unmatched"].sum(0), fa["hist"].sum(0))
    Rc = pc.shares_from_fields(fc["n"].sum(0), fc["unmatched"].sum(0), fc["hist"].sum(0))
    return ([n for n, _ in pc.DEFAULT_CLASSES], per_image.numpy(), pooled.numpy(), fa["bad"].sum(0).numpy(),
            (fa["unmatched"].sum(0) + fc["unmatched"].sum(0)).numpy(), P.numpy(), Rc.numpy())


def test_report_equals_the_statement(ev, capsys):
    res = ev.test_pointcloud()
    text = capsys.readouterr().out
    assert "pointcloud " in text and "pooled" in text and "per-image" in text and "glass" in text and "chamfer" in text
    names, per_image, pooled, bad, unmatched, P, Rc = _statement(ev)
    assert list(res) == names and len(names) == 12
    assert pooled[0, 8] > 0 and pooled[1, 8] > 0                          # the frame and the objects class hold points
    for k, name in enumerate(names):
        r = res[name]
        print(name, "pooled", r["pooled"], "per image", r["per_image"], "bad", r["bad"], "unmatched", r["unmatched"])
        assert set(r) == {"per_image", "pooled", "bad", "unmatched"}
        assert r["per_image"].shape == (9,) and r["pooled"].shape == (9,)
        assert r["bad"] == int(bad[k]) and r["unmatched"] == int(unmatched[k]) and r["pooled"][8] == pooled[k, 8], name
        with np.errstate(invalid="ignore", divide="ignore"):
            F = np.where(P[k] + Rc[k] > 0, 2 * P[k] * Rc[k] / (P[k] + Rc[k]), P[k] + Rc[k])        # from exact integer shares
        assert np.array_equal(r["pooled"][5:8], F, equal_nan=True), name
        assert np.allclose(r["pooled"], pooled[k], rtol=1e-9, atol=0.0, equal_nan=True), name
        assert np.allclose(r["per_image"], per_image[k], rtol=1e-9, atol=0.0, equal_nan=True), name
        assert np.isclose(r["pooled"][2], r["pooled"][0] + r["pooled"][1], rtol=1e-12), name
    # the brute-force route: the same bits
    brute = ev.test_pointcloud(prune=False)
    for name in names:
        for f in ("per_image", "pooled"):
            assert np.array_equal(res[name][f], brute[name][f], equal_nan=True), (name, f)
        assert res[name]["bad"] == brute[name]["bad"] and res[name]["unmatched"] == brute[name]["unmatched"]


def test_nothing_else_moves(ev):
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    fresh = Evaluation(**KW)                               # never asked for a point cloud
    a = fresh.test()
    ev.test_pointcloud()
    b = ev.test()
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for inputs in ev.test_loader:
        batch = lambda: {k: v.cuda() for k, v in inputs.items()}
        assert torch.equal(fresh.predict(batch()), ev.predict(batch()))
        break


def test_the_environment_switch_is_read_by_evaluation_main_only(monkeypatch, capsys):
    import manydepth
    from manydepth import evaluation_main
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(manydepth.__file__)))
    holders = []
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and "PD_EVAL_POINTCLOUD" in open(os.path.join(root, f), errors="ignore").read():
                holders.append(os.path.relpath(os.path.join(root, f), pkg))
    assert holders == [os.path.join("manydepth", "evaluation_main.py")]

    calls = []

    class Fake:
        def load_mono_model(self):
            calls.append("load")

        def test(self):
            calls.append("test")

        def test_normals(self):
            calls.append("normals")

        def test_pointcloud(self):
            calls.append("pointcloud")

    monkeypatch.setattr(evaluation_main, "Evaluation", Fake)
    monkeypatch.delenv("PD_EVAL_NORMALS", raising=False)
    monkeypatch.delenv("PD_EVAL_POINTCLOUD", raising=False)
    evaluation_main.main()
    assert calls == ["load", "test"]
    del calls[:]
    monkeypatch.setenv("PD_EVAL_POINTCLOUD", "1")
    evaluation_main.main()
    assert calls == ["load", "test", "pointcloud"]
    del calls[:]
    monkeypatch.setenv("PD_EVAL_POINTCLOUD", "0")
    evaluation_main.main()
    assert calls == ["load", "test"]
