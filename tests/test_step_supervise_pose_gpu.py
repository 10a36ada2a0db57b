"""The Trainer's pose-network mode with ``--supervise_pose True`` on synthetic items, at the size of
tests/test_step_posenet_gpu.py: what the constructor accepts and refuses, the terms of one step against
ops.pose_supervision on the step's own matrices, their place in ``loss``, the gradients that reach the pose decoder, and two
optimiser steps.  The kernels are checked in tests/test_pose_loss_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _opts(tmp, extra=()):
    from manydepth.options import MonodepthOptions
    opts = MonodepthOptions().parse([
        "--png", "--batch_size", "2", "--height", "64", "--width", "96", "--dataset", "HAMMER", "--split", "HAMMER",
        "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision", "True",
        "--normals_loss_weight", "0.35", "--augment_xolp", "--augment_normals", "--dropout_rate", "0.0",
        "--log_dir", str(tmp), "--data_path", "synthetic", "--data_path_val", "synthetic", "--num_workers", "0",
        "--weights_init", "scratch", "--learning_rate", "1e-4", *extra])
    opts.pose_input = False
    return opts


@pytest.fixture(scope="module")
def trainer(tmp_path_factory):
    from manydepth.trainer import Trainer
    opts = _opts(tmp_path_factory.mktemp("supervise_pose"), ["--supervise_pose", "True"])
    opts.pose_network = True
    tr = Trainer(opts)
    tr.set_train()
    return tr, next(iter(tr.train_loader))


def test_constructor(trainer, tmp_path):
    from manydepth.trainer import Trainer
    tr, batch = trainer
    assert tr.pose_network and tr.supervise_pose and tr.photometric and tr.frame_ids == [0, -1, 1]
    for loader in (tr.train_loader, tr.val_loader, tr.test_loader):
        assert loader.dataset.need_poses is True and loader.dataset.lookup_aug is True
    assert ("poses", -1) in batch and ("frame_valid", 1) in batch
    with pytest.raises(NotImplementedError, match="supervise_pose"):
        Trainer(_opts(tmp_path, ["--supervise_pose", "True"]))            # no pose network: nothing to supervise
    opts = _opts(tmp_path, ["--supervise_pose", "True", "--res_pose", "True"])
    opts.pose_network = True
    with pytest.raises(NotImplementedError, match="res_pose"):
        Trainer(opts)


def _step(tr, batch, supervise):
    tr.supervise_pose = supervise
    try:
        tr.model_optimizer.zero_grad()
        torch.manual_seed(77)                                          # the automask noise is the step's only draw
        outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
        losses["loss"].backward()
        torch.cuda.synchronize()
    finally:
        tr.supervise_pose = True
    named = dict(tr.models["pose"].named_parameters())
    return outputs, losses, named["net.3.weight"].grad.detach().clone()


def test_one_step_terms_total_and_gradients(trainer):
    from polardepth import ops
    tr, batch = trainer
    out0, losses0, g_off = _step(tr, batch, False)
    out1, losses1, g_on = _step(tr, batch, True)
    assert "r_loss" not in losses0 and "t_loss" not in losses0
    for f in (-1, 1):                                                  # the same seed, the same forward
        assert torch.equal(out0[("cam_T_cam", 0, f)].detach(), out1[("cam_T_cam", 0, f)].detach())
    r, t = losses1["r_loss"], losses1["t_loss"]
    assert torch.isfinite(r) and torch.isfinite(t) and r.item() > 0 and t.item() > 0
    dev = {k: v.to(tr.device) for k, v in batch.items()}
    with torch.no_grad():
        r2, t2, total = ops.pose_supervision([out1[("cam_T_cam", 0, i)].detach() for i in (-1, 1)],
                                             [dev[("poses", i)] for i in (-1, 1)],
                                             valid=torch.stack([dev[("frame_valid", i)] for i in (-1, 1)], 1).float())
    assert torch.equal(r.detach(), r2) and torch.equal(t.detach(), t2)
    # the reference's cumulative weights: the first neighbour counts twice
    _, _, flat = ops.pose_supervision([out1[("cam_T_cam", 0, i)].detach() for i in (-1, 1)],
                                      [dev[("poses", i)] for i in (-1, 1)], frame_weight=[1.0, 1.0])
    assert total.item() > flat.item() and abs(flat.item() - (r.item() + t.item())) <= 1e-6 * flat.item()
    want = np.float32(losses0["loss"].item()) + np.float32(total.item())
    got = np.float32(losses1["loss"].item())
    print("loss", got, "off + total", want)
    assert abs(np.float64(got) - np.float64(want)) <= np.spacing(np.abs(want))
    assert torch.isfinite(g_on).all() and not torch.equal(g_on[:6], g_off[:6])
    assert (g_on[6:] == 0).all() and (g_off[6:] == 0).all()


def test_two_optimiser_steps_stay_finite(trainer):
    tr, batch = trainer
    for step in range(2):
        tr.model_optimizer.zero_grad()
        outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
        losses["loss"].backward()
        tr.model_optimizer.step()
        for k, v in losses.items():
            assert torch.isfinite(v).all(), (step, k)
    assert torch.isfinite(tr.store.flat).all()


def test_freeze_teacher_and_pose_computes_the_terms_without_a_tape(trainer):
    tr, batch = trainer
    tr.train_teacher_and_pose = False
    try:
        outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    finally:
        tr.train_teacher_and_pose = True
    assert not losses["r_loss"].requires_grad and not losses["t_loss"].requires_grad
    assert torch.isfinite(losses["loss"]).all() and losses["r_loss"].item() > 0
