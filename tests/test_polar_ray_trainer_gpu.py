"""The ray frame in the Trainer (opt.polar_ray_frame) and in Evaluation(polar_ray_frame=True).test_polar_normals, on the
synthetic loader at the size of tests/test_polar_loss_trainer_gpu.py / tests/test_eval_polar_normals_gpu.py.  With the option
unset not a bit of a step changes; with it the polarimetric entries differ from the orthographic run's, ``loss`` is composed
as before and the flag travels in opt.json.  That the terms and their gradient are right in the ray frame is checked in
tests/test_polar_ray_gpu.py: the synthetic loader's depth and polarisation are unrelated fields."""
import json
import os

import numpy as np
import pytest
import torch

import polar_normals_ref as R
from test_polar_loss_trainer_gpu import _opts, _step, _trainer

pytestmark = pytest.mark.gpu


def test_unset_nothing_changes_and_set_the_terms_move(tmp_path):
    from polardepth import functional as PF
    base = _trainer(tmp_path / "a", polar_loss=(0.5, 0.5))
    assert not hasattr(base.opt, "polar_ray_frame") and base.polar_ray_frame is False
    off = _trainer(tmp_path / "b", like=base, polar_loss=(0.5, 0.5), polar_ray_frame=False)
    on = _trainer(tmp_path / "c", like=base, polar_loss=(0.5, 0.5), polar_ray_frame=True)
    assert on.polar_ray_frame is True and off.polar_ray_frame is False
    batch = next(iter(base.train_loader))
    lb, gb, pb, _ = _step(base, batch)
    lo, go, po, _ = _step(off, batch)
    assert lb.keys() == lo.keys() and all(torch.equal(lb[k], lo[k]) for k in lb)
    assert all(torch.equal(a, b) for a, b in zip(gb, go)) and torch.equal(pb, po)
    # a Trainer that never heard of the attribute and no term at all: the plain run, as before
    plain = _trainer(tmp_path / "d", like=base)
    assert plain.polar_loss is None and plain.polar_ray_frame is False

    scales = list(on.opt.scales)
    ln, gn, pn, outputs = _step(on, batch)
    assert ln.keys() == lb.keys()
    for s in scales:
        for t in ("normal", "azimuth"):
            k = f"polar_{t}_loss/{s}"
            assert torch.isfinite(ln[k]) and 0.0 < ln[k].item() < 2.0 and not torch.equal(ln[k], lb[k]), (k, ln[k], lb[k])
    # `loss` is composed as before: the supervised loss on the same disparities plus the mean of the weighted terms
    dev_batch = {k: v.to(on.device) for k, v in batch.items()}
    vals, _ = PF.multiscale_loss(on.loss_cfg, dev_batch["depth"], dev_batch[("K", 0)],
                                 [outputs[("disp", s)].detach() for s in scales], [dev_batch[("color", 0, s)] for s in scales])
    term = [0.5 * ln[f"polar_normal_loss/{s}"].item() + 0.5 * ln[f"polar_azimuth_loss/{s}"].item() for s in scales]
    want = vals[0].item() + sum(term) / len(term)
    assert abs(ln["loss"].item() - want) <= 1e-6 * abs(want), (ln["loss"].item(), want)
    assert torch.equal(ln["supervised_depth_loss/0"], lb["supervised_depth_loss/0"])
    for s, a, b in zip(scales, gn, gb):
        assert torch.isfinite(a).all() and not torch.equal(a, b), s
    assert not torch.equal(pn, pb)
    saved = json.load(open(os.path.join(on.log_path, "models", "opt.json")))
    assert saved["polar_ray_frame"] is True and saved["polar_loss"] == [0.5, 0.5]
    assert "polar_ray_frame" not in json.load(open(os.path.join(base.log_path, "models", "opt.json")))


def test_refusals(tmp_path, monkeypatch):
    from manydepth.trainer import Trainer
    opts = _opts(tmp_path)
    opts.polar_ray_frame = True
    with pytest.raises(ValueError, match="polar_ray_frame is set without opt.polar_loss"):
        Trainer(opts)
    opts = _opts(tmp_path)
    opts.polar_loss, opts.polar_ray_frame = (0.5, 0.5), "on"
    with pytest.raises(ValueError, match="polar_ray_frame must be True or False"):
        Trainer(opts)
    monkeypatch.setenv("PD_STEP_GRAPH", "1")
    opts = _opts(tmp_path)
    opts.polar_loss, opts.polar_ray_frame = (0.5, 0.5), True
    with pytest.raises(NotImplementedError, match="not captured yet"):
        Trainer(opts)


# ------------------------------------------------------------------ Evaluation

KW = dict(data_path="synthetic", height=64, width=96, batch_size=4)


@pytest.fixture(scope="module")
def ev():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    return Evaluation(polar_ray_frame=True, **KW)


def _class_pixels(ev, source):
    from polardepth import normals_eval as ne
    import normals_stats_ref as NR
    tot = np.zeros(len(ne.DEFAULT_CLASSES), np.int64)
    for inputs in ev.test_loader:
        mask = inputs[("mask", 0, 0)][:, 0].numpy()
        live = np.ones(mask.shape, bool)
        if source == "gt":
            live = NR.window_ok(inputs["depth_gt"][:, 0].float().numpy(), np.float32(0.1), np.float32(2.0), 1)
        for k, (_, r) in enumerate(ne.DEFAULT_CLASSES):
            lo, hi = (1, 0) if r is None else r
            tot[k] += (R.in_class(mask, lo, hi) & live).sum()
    return tot


@pytest.mark.parametrize("source", ["depth", "gt"])
def test_the_report_names_the_frame_and_the_counts_add_up(ev, source, capsys):
    from polardepth import normals_eval as ne
    res = ev.test_polar_normals(source=source)
    text = capsys.readouterr().out
    assert f"polar normal ({source}, ray frame)" in text and f"polar azimuth ({source}, ray frame)" in text
    names = [n for n, _ in ne.DEFAULT_CLASSES]
    assert list(res) == names
    pixels = _class_pixels(ev, source)
    assert pixels[0] > 0 and pixels[1] > 0
    for k, name in enumerate(names):
        for sname in ("normal", "azimuth"):
            r = res[name][sname]
            n = int(r["pooled"][6])
            gates = r["bad"] + r["dolp_out"] + (r["frontal"] if sname == "azimuth" else 0)
            assert n + gates == pixels[k], (source, name, sname)
    assert res["all"]["normal"]["pooled"][6] > 0 and res["all"]["azimuth"]["pooled"][6] > 0


def test_the_frame_moves_the_report_and_nothing_else(ev, capsys, monkeypatch):
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    plain = Evaluation(**KW)
    assert plain.polar_ray_frame is False
    a = plain.test()
    before = capsys.readouterr().out
    b = ev.test()
    assert capsys.readouterr().out == before                      # test() prints what it printed before
    assert before.startswith("all ") and list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    ortho = plain.test_polar_normals(source="gt")
    text = capsys.readouterr().out
    assert "polar normal (gt)" in text and "ray frame" not in text
    ray = ev.test_polar_normals(source="gt")
    assert ray["all"]["normal"]["pooled"][0] != ortho["all"]["normal"]["pooled"][0]
    assert ray["all"]["azimuth"]["pooled"][0] != ortho["all"]["azimuth"]["pooled"][0]
    monkeypatch.setenv("PD_POLAR_RAY_FRAME", "1")
    torch.manual_seed(0)
    assert Evaluation(**KW).polar_ray_frame is True and Evaluation(polar_ray_frame=False, **KW).polar_ray_frame is False
