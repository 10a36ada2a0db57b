"""The Trainer with the depth-uncertainty term (opt.uncertainty_loss) on polardepth.synthetic items at the size of
tests/test_step_gpu.py: which weights a step moves, the logged entries and their place in ``loss``, the detached mode, a
checkpoint without heads, the range through save and load, the refusals.  That the term and its gradients are right is checked
in tests/test_unc_loss_gpu.py."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _opts(tmp, extra=()):
    from manydepth.options import MonodepthOptions
    return MonodepthOptions().parse([
        "--png", "--batch_size", "2", "--height", "64", "--width", "96", "--dataset", "HAMMER", "--split", "HAMMER",
        "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision", "True",
        "--depth_supervision_only", "True", "--normals_loss_weight", "0.35", "--augment_xolp", "--augment_normals",
        "--dropout_rate", "0.0", "--log_dir", str(tmp), "--data_path", "synthetic", "--data_path_val", "synthetic",
        "--num_workers", "0", "--weights_init", "scratch", "--learning_rate", "1e-4", *extra])


def _trainer(tmp, like=None, extra=(), **attrs):
    from manydepth.trainer import Trainer
    opts = _opts(tmp, extra)
    for k, v in attrs.items():
        setattr(opts, k, v)
    tr = Trainer(opts)
    if like is not None:
        for name, m in like.models.items():
            tr.models[name].load_state_dict(m.state_dict())
    tr.set_train()
    return tr


def _heads(tr, kind):
    dec = tr.models["mono_depth"]
    return {f"{kind}{key[1:]}.{n}": p for key, m in dec.convs.items() if key[0] == kind for n, p in m.named_parameters()}


def _step(tr, batch, update=True):
    tr.model_optimizer.zero_grad()
    outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    losses["loss"].backward()
    torch.cuda.synchronize()
    grads = {f"{mn}.{pn}": p.grad.detach().clone() for mn, m in tr.models.items() for pn, p in m.named_parameters()}
    if update:
        tr.model_optimizer.step()
        torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in losses.items()}, grads, outputs


def test_a_step_trains_the_unc_conv_heads_and_logs_the_term(tmp_path):
    from polardepth import functional as PF
    tr = _trainer(tmp_path, uncertainty_loss=0.1)
    assert tr.models["mono_depth"].uncertainty and tr.uncertainty_range == (0.0005, 0.5) and not tr.uncertainty_detach
    names = [n for n, _ in tr.store.entries[tr.store.n_used_params:]]
    assert sum("mono_depth" in n for n in names) == 8                        # four unc_conv_color heads, weight and bias, idle
    before = {k: p.detach().clone() for kind in ("unc_conv", "unc_conv_color", "dispconv") for k, p in _heads(tr, kind).items()}
    batch = next(iter(tr.train_loader))
    losses, grads, outputs = _step(tr, batch)
    scales = list(tr.opt.scales)
    for s in scales:
        assert torch.isfinite(losses[f"uncertainty_loss/{s}"]), s
        assert tuple(outputs[("uncertainty", s)].shape) == tuple(outputs[("disp", s)].shape)
    for kind, moves in (("unc_conv", True), ("unc_conv_color", False), ("dispconv", True)):
        for k, p in _heads(tr, kind).items():
            assert torch.equal(p, before[k]) != moves, (k, moves)
    # `loss` is the supervised loss of the unchanged path on the same disparities plus the mean of the weighted terms
    dev_batch = {k: v.to(tr.device) for k, v in batch.items()}
    vals, _ = PF.multiscale_loss(tr.loss_cfg, dev_batch["depth"], dev_batch[("K", 0)],
                                 [outputs[("disp", s)].detach() for s in scales], [dev_batch[("color", 0, s)] for s in scales])
    term = [0.1 * losses[f"uncertainty_loss/{s}"].item() for s in scales]
    want = vals[0].item() + sum(term) / len(term)
    assert abs(losses["loss"].item() - want) <= 1e-6 * abs(want), (losses["loss"].item(), want)
    for i, s in enumerate(scales):
        want_s = vals[1 + 3 * i].item() + term[i]
        assert abs(losses[f"loss/{s}"].item() - want_s) <= 1e-6 * abs(want_s)
    saved = json.load(open(os.path.join(tr.log_path, "models", "opt.json")))
    assert saved["uncertainty_loss"] == 0.1 and saved["uncertainty_range"] == [0.0005, 0.5] and saved["uncertainty_detach"] is False


def test_detached_the_rest_of_the_network_gets_the_gradient_of_weight_zero(tmp_path):
    zero = _trainer(tmp_path / "a", uncertainty_loss=0.0)
    det = _trainer(tmp_path / "b", like=zero, uncertainty_loss=0.3, uncertainty_detach=True)
    att = _trainer(tmp_path / "c", like=zero, uncertainty_loss=0.3)
    batch = next(iter(zero.train_loader))
    _, gz, _ = _step(zero, batch, update=False)
    _, gd, _ = _step(det, batch, update=False)
    _, ga, _ = _step(att, batch, update=False)
    assert gz.keys() == gd.keys()
    unc = {f"mono_depth.{n}" for n, p in det.models["mono_depth"].named_parameters()
           if any(p is q for q in _heads(det, "unc_conv").values())}
    assert len(unc) == 8
    for k in gz:
        if k in unc:
            assert gd[k].abs().sum() > 0 and not gz[k].any(), k
        else:
            assert torch.equal(gd[k], gz[k]), k
    # attached, the term reaches the network through the depth maps and the heads' input
    assert any(not torch.equal(ga[k], gz[k]) for k in gz if k not in unc and k.startswith("rgb_encoder"))


def test_a_checkpoint_without_heads_loads_and_the_range_survives_save_and_load(tmp_path):
    plain = _trainer(tmp_path / "a")
    assert not plain.models["mono_depth"].uncertainty and plain.uncertainty_loss is None
    plain.save_model()
    folder = os.path.join(plain.log_path, "models", "weights_0")
    assert "uncertainty_range" not in torch.load(os.path.join(folder, "trainer_state.pth"))
    with_heads = _trainer(tmp_path / "b", extra=("--load_weights_folder", folder), uncertainty_loss=0.1,
                          uncertainty_range="0.001,0.25")
    assert with_heads.uncertainty_range == (0.001, 0.25)
    for k, p in plain.models["mono_depth"].state_dict().items():
        assert torch.equal(with_heads.models["mono_depth"].state_dict()[k], p), k
    fresh = _trainer(tmp_path / "c", uncertainty_loss=0.1)
    w = _heads(with_heads, "unc_conv")
    assert all(torch.isfinite(p).all() and p.abs().sum() > 0 for k, p in w.items() if k.endswith("weight"))
    assert len(w) == len(_heads(fresh, "unc_conv")) == 8
    losses, _, _ = _step(with_heads, next(iter(with_heads.train_loader)))
    assert torch.isfinite(losses["loss"])
    with_heads.save_model()
    folder2 = os.path.join(with_heads.log_path, "models", "weights_0")
    assert torch.load(os.path.join(folder2, "trainer_state.pth"))["uncertainty_range"] == [0.001, 0.25]
    again = _trainer(tmp_path / "d", extra=("--load_weights_folder", folder2), uncertainty_loss=0.1)
    assert again.uncertainty_range == (0.001, 0.25) and again.opt.uncertainty_range == [0.001, 0.25]
    for k, p in with_heads.models["mono_depth"].state_dict().items():
        assert torch.equal(again.models["mono_depth"].state_dict()[k], p), k
    with pytest.raises(ValueError, match="were trained with"):
        _trainer(tmp_path / "e", extra=("--load_weights_folder", folder2), uncertainty_loss=0.1, uncertainty_range=(0.0005, 0.5))


def test_refusals(tmp_path, monkeypatch):
    from manydepth.trainer import Trainer
    for bad in (-0.1, float("nan"), float("inf"), "a", (0.1, 0.2)):
        opts = _opts(tmp_path)
        opts.uncertainty_loss = bad
        with pytest.raises(ValueError, match="uncertainty_loss"):
            Trainer(opts)
    for bad in ((0.0, 0.5), (0.5, 0.5), (0.5, 0.1), (0.1,), "a,b", (0.1, float("inf")), 3.0):
        opts = _opts(tmp_path)
        opts.uncertainty_loss, opts.uncertainty_range = 0.1, bad
        with pytest.raises(ValueError, match="uncertainty_range|uncertainty range"):
            Trainer(opts)
    opts = _opts(tmp_path)
    opts.uncertainty_range = (0.001, 0.1)
    with pytest.raises(ValueError, match="without opt.uncertainty_loss"):
        Trainer(opts)
    opts = _opts(tmp_path)
    opts.uncertainty_loss, opts.uncertainty_detach = 0.1, "yes"
    with pytest.raises(ValueError, match="uncertainty_detach"):
        Trainer(opts)
    opts = _opts(tmp_path)
    opts.uncertainty_loss, opts.bf16 = 0.1, True
    with pytest.raises(NotImplementedError, match="bf16"):
        Trainer(opts)
    opts = _opts(tmp_path)
    opts.uncertainty_loss, opts.step_graph = 0.1, True
    with pytest.raises(NotImplementedError, match="not captured"):
        Trainer(opts)
    monkeypatch.setenv("PD_STEP_GRAPH", "1")
    opts = _opts(tmp_path)
    opts.uncertainty_loss = 0.1
    with pytest.raises(NotImplementedError, match="not captured"):
        Trainer(opts)
    monkeypatch.delenv("PD_STEP_GRAPH")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)      # a stub: no process group is created
    opts = _opts(tmp_path)
    opts.uncertainty_loss = 0.1
    with pytest.raises(NotImplementedError, match="torch.distributed"):
        Trainer(opts)
