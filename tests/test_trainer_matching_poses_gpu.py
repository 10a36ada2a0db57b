"""The Trainer's ``opt.matching_poses`` on synthetic items (64 x 96, B = 2, frame_ids 0 -1 1, two matching frames, the pose
network): what the loaders serve, the relative poses process_batch leaves in ``inputs``, and that the first step's losses and
parameter gradients are, bit for bit, those of the Trainer without the option."""
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
        "--weights_init", "scratch", "--learning_rate", "1e-4", "--frame_ids", "0", "-1", "1", "--num_matching_frames", "2",
        *extra])
    opts.pose_input = False
    return opts


def _trainer(tmp, matching):
    from manydepth.trainer import Trainer
    opts = _opts(tmp)
    opts.pose_network = True
    if matching:
        opts.matching_poses = True
    torch.manual_seed(5)                                       # the same initialisation for both
    tr = Trainer(opts)
    tr.set_train()
    torch.manual_seed(3)                                       # the same shuffle for both
    return tr, next(iter(tr.train_loader))


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    return _trainer(tmp_path_factory.mktemp("matching_on"), True), _trainer(tmp_path_factory.mktemp("matching_off"), False)


def _step(tr, batch):
    tr.model_optimizer.zero_grad()
    torch.manual_seed(77)                                      # the automask noise is the step's only draw
    inputs = dict(batch)
    outputs, losses, _ = tr.process_batch(inputs, is_train=True)
    losses["loss"].backward()
    torch.cuda.synchronize()
    grads = {f"{n}.{k}": (None if p.grad is None else p.grad.detach().clone())
             for n, m in tr.models.items() for k, p in m.named_parameters()}
    return inputs, outputs, losses, grads


def test_loaders_and_option(pair, tmp_path):
    from manydepth.trainer import Trainer
    (on, batch_on), (off, batch_off) = pair
    assert on.matching_poses and on.matching_ids == [0, -1, -2] and on.frame_ids == [0, -1, 1]
    assert on.frames_to_load == [0, -1, 1, -2] and off.frames_to_load == off.frame_ids == [0, -1, 1]
    assert not off.matching_poses
    for loader in (on.train_loader, on.val_loader, on.test_loader):
        assert loader.dataset.frame_idxs == [0, -1, 1, -2]
    # the new neighbour is drawn last: everything else is what the loader without the option serves
    assert set(batch_on) - set(batch_off) == {("color", -2, 0), ("color_aug", -2, 0), ("poses", -2), ("frame_valid", -2)}
    assert set(batch_off) <= set(batch_on) and all(torch.equal(batch_on[k], batch_off[k]) for k in batch_off)
    opts = _opts(tmp_path)
    opts.pose_input = True
    opts.matching_poses = True
    with pytest.raises(ValueError, match="matching_poses"):
        Trainer(opts)                                          # no pose network: nobody predicts the links
    opts = _opts(tmp_path, ["--use_future_frame"])
    opts.pose_network = opts.matching_poses = True
    assert Trainer(opts).matching_ids == [0, 1, -1, -2]


def test_first_step_relative_poses_and_bit_equal_losses_and_gradients(pair):
    from polardepth import matching
    (on, batch_on), (off, batch_off) = pair
    inputs, out_on, losses_on, grads_on = _step(on, batch_on)
    inputs_off, out_off, losses_off, grads_off = _step(off, batch_off)
    for fi in (-1, -2):
        for key in ("relative_pose", "relative_pose_inv"):
            T = inputs[(key, fi)]
            assert tuple(T.shape) == (2, 4, 4) and torch.isfinite(T).all() and T.reshape(2, 16).any(1).all()
            assert not T.requires_grad and T.grad_fn is None
    assert not any(isinstance(k, tuple) and k[0].startswith("relative_pose") for k in inputs_off)
    # ... equal to matching_poses recomputed from the same batch (training mode: batch statistics, so a further pass gives
    # the same poses; it moves the running statistics once more, which no figure below reads)
    rel, rel_inv = matching.matching_poses(on.models["pose_encoder"], on.models["pose"],
                                           {i: inputs[("color_aug", i, 0)] for i in (0, -1, -2)}, [0, -1, -2],
                                           {i: inputs[("frame_valid", i)] for i in (-1, -2)})
    for fi in (-1, -2):
        assert torch.equal(rel[fi], inputs[("relative_pose", fi)]) and torch.equal(rel_inv[fi], inputs[("relative_pose_inv", fi)])
    # the first link of the chain is the first half's pose for the neighbour -1: the same pair, the same batch statistics
    assert torch.equal(inputs[("relative_pose", -1)], out_on[("cam_T_cam", 0, -1)].detach())
    # every loss and every parameter gradient: the Trainer without the option
    assert set(losses_on) == set(losses_off)
    for k in losses_off:
        assert torch.equal(losses_on[k].detach(), losses_off[k].detach()), k
    assert set(grads_on) == set(grads_off) and any(g is not None for g in grads_off.values())
    for k, g in grads_off.items():
        assert (g is None) == (grads_on[k] is None), k
        assert g is None or torch.equal(grads_on[k], g), k
