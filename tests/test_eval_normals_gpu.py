"""Evaluation.test_normals / predict_all on the GPU: the report equals the NumPy statement (tests/normals_stats_ref.py) applied
per image to what the networks return, for both sources; and nothing else moves -- test() and predict() give the bits they
gave before the normals decoder could be asked for.

Integer fields (pixel counts, `bad`, hence the three pooled shares) must be equal; the other figures agree to rtol 1e-9 (the
kernel's fp64 sums are within 1e-11 of the statement's, tests/test_normals_stats_gpu.py; the metrics divide them by equal
integers)."""
import numpy as np
import pytest
import torch

import normals_stats_ref as R

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=4)


def _evaluation(**kw):
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)                                  # the same initialisation for every instance: the decoder is built last
    return Evaluation(**KW, **kw)


@pytest.fixture(scope="module")
def plain():
    import os
    assert os.environ.get("PD_NORMALS_DECODER") != "1"
    return _evaluation()


@pytest.fixture(scope="module")
def with_decoder():
    return _evaluation(normals_decoder=True)


def _statement(ev, source):
    """The report from the statement: per batch the kernel's own gtn, the scored normal map as the device holds it, and
    R.stats per image; then the two conventions with the Python layer's formulas on host tensors."""
    from polardepth import normals_eval as ne
    from polardepth._lib import lib, check, ptr, stream_ptr
    big = float(np.finfo(np.float32).max)
    lohi = [(1, 0) if r is None else r for _, r in ne.DEFAULT_CLASSES]
    parts = []
    for inputs in ev.test_loader:
        inputs = {k: v.cuda() for k, v in inputs.items()}
        out = ev.predict_all(inputs)
        gt, K = inputs["depth_gt"].float().contiguous(), inputs[("K", 0)].float().contiguous()
        N, _, H, W = gt.shape
        gtn = torch.empty((N, H, W, 4), device="cuda")
        check(lib.pd_gt_normals(ptr(gt), ptr(K), ptr(gtn), N, H, W, 0.1, 2.0, stream_ptr()), "pd_gt_normals")
        if source == "depth":
            depth, pn = out["depth"].contiguous(), torch.empty((N, H, W, 4), device="cuda")
            check(lib.pd_gt_normals(ptr(depth), ptr(K), ptr(pn), N, H, W, -big, big, stream_ptr()), "pd_gt_normals")
        else:
            pn = out["normals_pred"].permute(0, 2, 3, 1).contiguous()
        parts.append(R.stats(pn.cpu().numpy(), gtn.cpu().numpy(), gt[:, 0].cpu().numpy(), inputs[("mask", 0, 0)][:, 0].cpu().numpy(),
                             lohi, ne.cos_edges_numpy(), 1, 0.1, 2.0))
    f = {k: torch.from_numpy(np.concatenate([p[k] for p in parts])) for k in ("n", "bad", "sum_deg", "sum_deg2", "hist")}
    # The seven figures come from the Python layer's own formulas here, so a wrong formula would cancel out in THIS file: they
    # are pinned against NumPy (mean, rmse and the shares exactly, the median within one bin) in tests/test_normals_stats_ref.py.
    # What this file checks is the wiring: which tensor is scored, the gate, the classes, the two ways of averaging.
    m = ne.metrics_from_fields(f["n"], f["sum_deg"], f["sum_deg2"], f["hist"])                     # [images, K, 7]
    valid = f["n"] > 0
    per_image = torch.where(valid[..., None], m, torch.zeros_like(m)).sum(0) / valid.sum(0)[:, None].double()
    pooled = ne.metrics_from_fields(f["n"].sum(0), f["sum_deg"].sum(0), f["sum_deg2"].sum(0), f["hist"].sum(0))
    return [n for n, _ in ne.DEFAULT_CLASSES], per_image.numpy(), pooled.numpy(), f["bad"].sum(0).numpy()


def _check(res, statement, what):
    names, per_image, pooled, bad = statement
    assert list(res) == names and len(names) == 12
    assert pooled[0, 6] > 0 and pooled[1, 6] > 0                          # the frame and the objects class hold pixels
    for k, name in enumerate(names):
        r = res[name]
        print(what, name, "pooled", r["pooled"], "per image", r["per_image"], "bad", r["bad"])
        assert r["per_image"].shape == (7,) and r["pooled"].shape == (7,)
        assert r["bad"] == int(bad[k]) and r["pooled"][6] == pooled[k, 6], (what, name)
        assert np.array_equal(r["pooled"][3:6], pooled[k, 3:6], equal_nan=True), (what, name)      # integer ratios: exact
        assert np.allclose(r["pooled"], pooled[k], rtol=1e-9, atol=0.0, equal_nan=True), (what, name)
        assert np.allclose(r["per_image"], per_image[k], rtol=1e-9, atol=0.0, equal_nan=True), (what, name)


def test_depth_source_equals_the_statement(plain, capsys):
    res = plain.test_normals()
    text = capsys.readouterr().out
    assert "normals (depth)" in text and "pooled" in text and "per-image" in text and "glass" in text
    _check(res, _statement(plain, "depth"), "depth")
    same = plain.test_normals(source="depth")
    assert all(np.array_equal(res[k]["pooled"], same[k]["pooled"], equal_nan=True) for k in res)
    with pytest.raises(ValueError, match="normals_decoder=True"):
        plain.test_normals(source="decoder")
    with pytest.raises(ValueError, match="source must be"):
        plain.test_normals(source="xolp")


def test_decoder_source_scores_the_decoder(with_decoder, capsys):
    assert "normals_decoder" in with_decoder.models
    res = with_decoder.test_normals(source="decoder")
    assert "normals (decoder)" in capsys.readouterr().out
    _check(res, _statement(with_decoder, "decoder"), "decoder")
    auto = with_decoder.test_normals()
    assert "normals (decoder)" in capsys.readouterr().out
    for k in res:
        assert np.array_equal(res[k]["pooled"], auto[k]["pooled"], equal_nan=True) and res[k]["bad"] == auto[k]["bad"]
    depth = with_decoder.test_normals(source="depth")
    _check(depth, _statement(with_decoder, "depth"), "depth behind a decoder")
    assert not np.array_equal(depth["all"]["pooled"], res["all"]["pooled"], equal_nan=True)


def test_nothing_else_moves(plain, with_decoder, monkeypatch):
    from manydepth.evaluation import Evaluation
    a, b = plain.test(), with_decoder.test()
    off = _evaluation(normals_decoder=False)
    c = off.test()
    assert list(a) == list(b) == list(c)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    for inputs in plain.test_loader:
        batch = lambda: {k: v.cuda() for k, v in inputs.items()}
        d = plain.predict(batch())
        both = with_decoder.predict_all(batch())
        assert set(both) == {"depth", "normals_pred"} and tuple(both["normals_pred"].shape) == (4, 3, 64, 96)
        assert set(plain.predict_all(batch())) == {"depth"}
        assert torch.equal(d, both["depth"]) and torch.equal(d, with_decoder.predict(batch()))
        assert torch.equal(d, off.predict(batch())) and torch.equal(d, plain.predict_all(batch())["depth"])
        break
    # the environment switch is the Trainer's
    monkeypatch.setenv("PD_NORMALS_DECODER", "1")
    assert "normals_decoder" in Evaluation(**KW).models and "normals_decoder" not in Evaluation(normals_decoder=False, **KW).models
    monkeypatch.delenv("PD_NORMALS_DECODER")
    assert "normals_decoder" not in Evaluation(**KW).models
    with pytest.raises(ValueError, match="augment_normals"):
        Evaluation(normals_decoder=True, augment_normals=False, **KW)
