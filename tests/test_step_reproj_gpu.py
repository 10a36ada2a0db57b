"""The Trainer in the photometric mode (--depth_supervision True --pose_input True, without --depth_supervision_only) on
synthetic items, at the size of tests/test_step_gpu.py: two training steps, the new loss entries, the gradient the term sends
to every disparity scale, its place in ``loss``, and the configurations the constructor still refuses.  The synthetic loader's
frame 0 is white noise, so nothing here says the numbers are right: that the term, its gradient and the weight gradients of the
step equal a reference's is checked in tests/test_step_reproj_oracle_gpu.py, against the CPU oracle on a consistent batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _opts(tmp, extra=(), only=False):
    from manydepth.options import MonodepthOptions
    mode = ["--depth_supervision_only", "True"] if only else ["--pose_input", "True"]
    return MonodepthOptions().parse([
        "--png", "--batch_size", "2", "--height", "64", "--width", "96", "--dataset", "HAMMER", "--split", "HAMMER",
        "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision", "True", *mode,
        "--normals_loss_weight", "0.35", "--augment_xolp", "--augment_normals", "--dropout_rate", "0.0",
        "--log_dir", str(tmp), "--data_path", "synthetic", "--data_path_val", "synthetic", "--num_workers", "0",
        "--weights_init", "scratch", "--learning_rate", "1e-4", *extra])


def test_two_steps_loss_entries_gradients_and_composition(tmp_path):
    from manydepth.trainer import Trainer
    from polardepth import functional as PF
    tr = Trainer(_opts(tmp_path))
    assert tr.photometric and tr.frame_ids == [0, -1, 1]
    tr.set_train()
    batch = next(iter(tr.train_loader))
    assert ("poses", -1) in batch and ("color", 1, 0) in batch and batch[("frame_valid", 1)].shape == (2,)
    scales = list(tr.opt.scales)
    for step in range(2):
        tr.model_optimizer.zero_grad()
        outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
        losses["loss"].backward()
        tr.model_optimizer.step()
        for k, v in losses.items():
            assert torch.isfinite(v).all(), (step, k)
        assert all(f"reproj_loss/{s}" in losses and losses[f"reproj_loss/{s}"].item() > 0 for s in scales)
    assert torch.isfinite(tr.store.flat).all()

    # the term's own gradient reaches every disparity scale, and `loss` is the supervised loss of the unchanged path on the
    # same disparities plus the mean of the reprojection terms
    tr.model_optimizer.zero_grad()
    outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    disps = [outputs[("disp", s)] for s in scales]
    term = sum(losses[f"reproj_loss/{s}"] for s in scales)
    grads = torch.autograd.grad(term, disps, retain_graph=True)
    for s, g in zip(scales, grads):
        assert torch.isfinite(g).all() and g.abs().max().item() > 0, s
    dev_batch = {k: v.to(tr.device) for k, v in batch.items()}
    vals, _ = PF.multiscale_loss(tr.loss_cfg, dev_batch["depth"], dev_batch[("K", 0)], [d.detach() for d in disps],
                                 [dev_batch[("color", 0, s)] for s in scales])
    want = vals[0].item() + sum(losses[f"reproj_loss/{s}"].item() for s in scales) / len(scales)
    assert abs(losses["loss"].item() - want) <= 1e-6 * abs(want), (losses["loss"].item(), want)
    for i, s in enumerate(scales):
        want_s = vals[1 + 3 * i].item() + losses[f"reproj_loss/{s}"].item()
        assert abs(losses[f"loss/{s}"].item() - want_s) <= 1e-6 * abs(want_s)
    losses["loss"].backward()


def test_supervised_only_trainer_reports_the_same_supervised_loss_and_draws_nothing(tmp_path):
    """The unchanged mode on the same weights and batch: its `loss` is the photometric mode's `loss` minus the mean of the
    reprojection terms (1e-6 relative), it has no reproj entries, and it leaves torch's device RNG stream where it was."""
    from manydepth.trainer import Trainer
    new = Trainer(_opts(tmp_path / "a"))
    old = Trainer(_opts(tmp_path / "b", only=True))
    assert not old.photometric and old.frame_ids == [0]
    for name, m in new.models.items():
        old.models[name].load_state_dict(m.state_dict())
    batch = next(iter(new.train_loader))
    new.set_train(); old.set_train()
    _, ln, _ = new.process_batch(dict(batch), is_train=True)
    state = torch.cuda.get_rng_state()
    _, lo, _ = old.process_batch({k: v for k, v in batch.items()}, is_train=True)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    assert not any(k.startswith("reproj_loss") for k in lo)
    scales = list(new.opt.scales)
    want = lo["loss"].item() + sum(ln[f"reproj_loss/{s}"].item() for s in scales) / len(scales)
    assert abs(ln["loss"].item() - want) <= 1e-6 * abs(want), (ln["loss"].item(), want)


def test_options_change_the_term(tmp_path):
    from manydepth.trainer import Trainer
    tr = Trainer(_opts(tmp_path, ["--no_ssim", "--disable_automasking", "--avg_reprojection"]))
    assert tr.opt.no_ssim and tr.opt.disable_automasking and tr.opt.avg_reprojection       # the switches parse
    batch = next(iter(tr.train_loader))
    tr.set_eval()
    vals = {}
    for name, (no_ssim, no_mask, avg) in (("base", (False, False, False)), ("no_ssim", (True, False, False)),
                                          ("no_automask", (False, True, False)), ("avg", (False, False, True))):
        tr.opt.no_ssim, tr.opt.disable_automasking, tr.opt.avg_reprojection = no_ssim, no_mask, avg      # read at every step
        with torch.no_grad():
            _, losses, _ = tr.process_batch(dict(batch))
        vals[name] = losses["reproj_loss/0"].item()
    assert len(set(vals.values())) == 4 and all(v > 0 for v in vals.values()), vals


def test_constructor_refusals(tmp_path, monkeypatch):
    from manydepth.trainer import Trainer
    with pytest.raises(NotImplementedError, match="train_student"):
        Trainer(_opts(tmp_path, ["--train_student", "True"]))
    with pytest.raises(NotImplementedError, match="only --depth_supervision_only True --depth_supervision True"):
        Trainer(_opts(tmp_path, ["--v1_multiscale"]))
    opts = _opts(tmp_path)
    opts.pose_input = False
    with pytest.raises(NotImplementedError, match="only --depth_supervision_only True --depth_supervision True"):
        Trainer(opts)
    monkeypatch.setenv("PD_STEP_GRAPH", "1")
    with pytest.raises(NotImplementedError, match="PD_STEP_GRAPH"):
        Trainer(_opts(tmp_path))
    monkeypatch.delenv("PD_STEP_GRAPH")
    opts = _opts(tmp_path)
    opts.step_graph = True
    with pytest.raises(NotImplementedError, match="PD_STEP_GRAPH"):
        Trainer(opts)
