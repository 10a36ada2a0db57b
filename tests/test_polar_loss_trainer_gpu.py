"""The Trainer with the polarimetric normals loss (opt.polar_loss) on polardepth.synthetic items at the size of
tests/test_step_gpu.py: without the option not a bit changes; with it the new loss entries, their place in ``loss``, the
gradient at the disparity heads; "holes" on a ground truth without holes; the refusals.  That the term and its gradient are
right is checked in tests/test_polar_loss_gpu.py: the synthetic loader's depth and polarisation are unrelated fields."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _opts(tmp, mode="only", extra=()):
    from manydepth.options import MonodepthOptions
    flags = {"only": ["--depth_supervision_only", "True"], "poses": ["--pose_input", "True"], "posenet": []}[mode]
    opts = MonodepthOptions().parse([
        "--png", "--batch_size", "2", "--height", "64", "--width", "96", "--dataset", "HAMMER", "--split", "HAMMER",
        "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision", "True", *flags,
        "--normals_loss_weight", "0.35", "--augment_xolp", "--augment_normals", "--dropout_rate", "0.0",
        "--log_dir", str(tmp), "--data_path", "synthetic", "--data_path_val", "synthetic", "--num_workers", "0",
        "--weights_init", "scratch", "--learning_rate", "1e-4", *extra])
    if mode == "posenet":
        opts.pose_network = True
    return opts


def _trainer(tmp, like=None, mode="only", **attrs):
    from manydepth.trainer import Trainer
    opts = _opts(tmp, mode)
    for k, v in attrs.items():
        setattr(opts, k, v)
    tr = Trainer(opts)
    if like is not None:
        for name, m in like.models.items():
            tr.models[name].load_state_dict(m.state_dict())
    tr.set_train()
    return tr


def _step(tr, batch):
    """One training step -> (losses, the gradients at the disparity heads, a seeded sample of the updated parameters)."""
    tr.model_optimizer.zero_grad()
    outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    disps = [outputs[("disp", s)] for s in tr.opt.scales]
    gd = torch.autograd.grad(losses["loss"], disps, retain_graph=True)
    losses["loss"].backward()
    tr.model_optimizer.step()
    flat = tr.store.flat
    idx = torch.randint(0, flat.numel(), (4096,), generator=torch.Generator().manual_seed(11)).to(flat.device)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in losses.items()}, [g.clone() for g in gd], flat[idx].clone(), outputs


def test_without_the_option_nothing_changes_and_with_it_the_term_joins_the_loss(tmp_path):
    from polardepth import functional as PF
    base = _trainer(tmp_path / "a")
    assert not hasattr(base.opt, "polar_loss") and base.polar_loss is None
    off = _trainer(tmp_path / "b", like=base, polar_loss=None)
    on = _trainer(tmp_path / "c", like=base, polar_loss=(0.5, 0.5))
    batch = next(iter(base.train_loader))
    lb, gb, pb, _ = _step(base, batch)
    lo, go, po, _ = _step(off, batch)
    assert lb.keys() == lo.keys() and all(torch.equal(lb[k], lo[k]) for k in lb)
    assert all(torch.equal(a, b) for a, b in zip(gb, go)) and torch.equal(pb, po)
    assert not any(k.startswith("polar_") for k in lb)

    scales = list(on.opt.scales)
    ln, gn, pn, outputs = _step(on, batch)
    new = [f"polar_{t}_loss/{s}" for s in scales for t in ("normal", "azimuth")]
    assert len(new) == 8 and set(ln) - set(lb) == set(new)
    for k in new:
        assert torch.isfinite(ln[k]) and 0.0 < ln[k].item() < 2.0, (k, ln[k])
    # `loss` is the supervised loss of the unchanged path on the same disparities plus the mean of the weighted terms
    dev_batch = {k: v.to(on.device) for k, v in batch.items()}
    vals, _ = PF.multiscale_loss(on.loss_cfg, dev_batch["depth"], dev_batch[("K", 0)],
                                 [outputs[("disp", s)].detach() for s in scales], [dev_batch[("color", 0, s)] for s in scales])
    term = [0.5 * ln[f"polar_normal_loss/{s}"].item() + 0.5 * ln[f"polar_azimuth_loss/{s}"].item() for s in scales]
    want = vals[0].item() + sum(term) / len(term)
    assert abs(ln["loss"].item() - want) <= 1e-6 * abs(want), (ln["loss"].item(), want)
    for i, s in enumerate(scales):
        want_s = vals[1 + 3 * i].item() + term[i]
        assert abs(ln[f"loss/{s}"].item() - want_s) <= 1e-6 * abs(want_s)
    # same weights, same batch: the forward pass is the base run's, the gradient at every disparity head is not
    assert torch.equal(ln["supervised_depth_loss/0"], lb["supervised_depth_loss/0"])
    for s, a, b in zip(scales, gn, gb):
        assert torch.isfinite(a).all() and not torch.equal(a, b), s
    assert not torch.equal(pn, pb)
    saved = json.load(open(os.path.join(on.log_path, "models", "opt.json")))
    assert saved["polar_loss"] == [0.5, 0.5]


def test_holes_on_a_ground_truth_without_holes_is_the_base_run(tmp_path):
    base = _trainer(tmp_path / "a")
    holes = _trainer(tmp_path / "b", like=base, polar_loss=(0.5, 0.5), polar_loss_where="holes")
    batch = next(iter(base.train_loader))
    d = batch["depth"]
    batch["depth"] = torch.where((d >= 0.1) & (d <= 2.0), d, torch.full_like(d, 1.0))      # every pixel in range: no hole
    batch["depth_gt"] = batch["depth"]
    lb, gb, pb, _ = _step(base, batch)
    lh, gh, ph, _ = _step(holes, batch)
    for s in holes.opt.scales:
        assert lh[f"polar_normal_loss/{s}"].item() == 0.0 and lh[f"polar_azimuth_loss/{s}"].item() == 0.0
    assert all(torch.equal(lb[k], lh[k]) for k in lb)
    assert all(torch.equal(a, b) for a, b in zip(gb, gh)) and torch.equal(pb, ph)
    # and with holes the term sees them
    batch["depth"] = d
    batch["depth_gt"] = d
    lh2 = _step(holes, batch)[0]
    assert lh2["polar_normal_loss/0"].item() > 0.0


@pytest.mark.parametrize("mode", ["poses", "posenet"])
def test_the_photometric_modes_take_the_term(tmp_path, mode):
    tr = _trainer(tmp_path, mode=mode, polar_loss="0.25,0.75", pol_aolp_sign=-1)
    assert tr.photometric and tr.polar_loss == [0.25, 0.75] and tr.pol_aolp_sign == -1
    losses = _step(tr, next(iter(tr.train_loader)))[0]
    for s in tr.opt.scales:
        assert torch.isfinite(losses[f"polar_normal_loss/{s}"]) and torch.isfinite(losses[f"reproj_loss/{s}"])
    assert torch.isfinite(losses["loss"]) and torch.isfinite(tr.store.flat).all()


def test_refusals(tmp_path, monkeypatch):
    from manydepth.trainer import Trainer
    for bad in ((-0.1, 0.5), (0.5, float("nan")), (float("inf"), 0.0), (0.5,), "a,b"):
        opts = _opts(tmp_path)
        opts.polar_loss = bad
        with pytest.raises(ValueError, match="polar_loss"):
            Trainer(opts)
    opts = _opts(tmp_path)
    opts.polar_loss, opts.polar_loss_where = (0.5, 0.5), "glass"
    with pytest.raises(ValueError, match="polar_loss_where"):
        Trainer(opts)
    opts = _opts(tmp_path)
    opts.polar_loss, opts.pol_aolp_sign = (0.5, 0.5), 0
    with pytest.raises(ValueError, match="pol_aolp_sign"):
        Trainer(opts)
    opts = _opts(tmp_path)
    opts.polar_loss, opts.step_graph = (0.5, 0.5), True
    with pytest.raises(NotImplementedError, match="not captured yet"):
        Trainer(opts)
    monkeypatch.setenv("PD_STEP_GRAPH", "1")
    opts = _opts(tmp_path)
    opts.polar_loss = (0.5, 0.5)
    with pytest.raises(NotImplementedError, match="not captured yet"):
        Trainer(opts)
