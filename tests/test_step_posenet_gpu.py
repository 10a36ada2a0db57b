"""The Trainer with a pose network (``opt.pose_network = True``: --depth_supervision True, no --pose_input) on synthetic items,
at the size of tests/test_step_reproj_gpu.py: two training steps, the predicted matrices, the photometric term formed from
them, the gradients that reach both pose modules, and what the constructor refuses.  The synthetic frames are white noise, so
nothing here says the poses are right: the kernels are checked in tests/test_pose_gpu.py, the modules in
tests/test_pose_modules_gpu.py."""
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
    opts = _opts(tmp_path_factory.mktemp("posenet"))
    opts.pose_network = True
    tr = Trainer(opts)
    tr.set_train()
    return tr, next(iter(tr.train_loader))


def test_two_steps_matrices_term_and_gradients(trainer):
    from polardepth import functional as PF
    tr, batch = trainer
    assert tr.pose_network and tr.photometric and tr.frame_ids == [0, -1, 1]
    for loader in (tr.train_loader, tr.val_loader, tr.test_loader):    # neighbours need no pose files here (tests/test_pose_loader.py)
        assert loader.dataset.need_poses is False and loader.dataset.lookup_aug is True
    assert set(tr.models) >= {"pose_encoder", "pose"} and ("color_aug", -1, 0) in batch and ("color_aug", 1, 0) in batch
    named = {f"{m}.{k}": p for m in ("pose_encoder", "pose") for k, p in tr.models[m].named_parameters()}
    assert all(f"{m}.{k}" in tr.store.offsets for m in ("pose_encoder", "pose") for k, _ in tr.models[m].named_parameters())
    scales = list(tr.opt.scales)
    for step in range(2):
        tr.model_optimizer.zero_grad()
        outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
        losses["loss"].backward()
        tr.model_optimizer.step()
        for k, v in losses.items():
            assert torch.isfinite(v).all(), (step, k)
        assert all(losses[f"reproj_loss/{s}"].item() > 0 for s in scales)
    assert torch.isfinite(tr.store.flat).all()

    before = {k: p.detach().clone() for k, p in named.items()}
    tr.model_optimizer.zero_grad()
    torch.manual_seed(77)                                              # the automask noise is the step's only draw
    outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    for f in (-1, 1):
        assert tuple(outputs[("axisangle", 0, f)].shape) == tuple(outputs[("translation", 0, f)].shape) == (2, 2, 1, 3)
        T, Ti = outputs[("cam_T_cam", 0, f)], outputs[("cam_T_cam_inv", 0, f)]
        assert T.requires_grad and tuple(T.shape) == (2, 4, 4)
        eye = torch.eye(4, device=T.device).expand(2, 4, 4)
        assert (T.detach() @ Ti.detach() - eye).abs().max().item() <= 1e-5, f
        # cam_T_cam is the inverted matrix for the earlier frame, the plain one for the later frame
        plain = Ti if f < 0 else T
        assert torch.equal(plain.detach()[:, :3, 3], outputs[("translation", 0, f)].detach()[:, 0, 0])

    # the term is PF.photometric_loss of the predicted matrices, bit for bit
    dev = {k: v.to(tr.device) for k, v in batch.items()}
    depths = [outputs[("depth", 0, s)].detach() for s in scales]
    torch.manual_seed(77)
    noise = [torch.randn(depths[0].shape, device=tr.device).mul_(1e-5) for _ in scales]
    with torch.no_grad():
        want = PF.photometric_loss(tr.loss_cfg, None, depths, dev[("color", 0, 0)], [dev[("color", i, 0)] for i in (-1, 1)],
                                   dev[("K", 0)], dev[("inv_K", 0)], [outputs[("cam_T_cam", 0, i)].detach() for i in (-1, 1)],
                                   torch.stack([dev[("frame_valid", i)] for i in (-1, 1)], 1).float(), noise=noise,
                                   no_ssim=tr.opt.no_ssim, automask=True, avg=tr.opt.avg_reprojection)
    for i, s in enumerate(scales):
        assert torch.equal(losses[f"reproj_loss/{s}"].detach(), want[i]), s

    losses["loss"].backward()
    torch.cuda.synchronize()
    g3 = named["pose.net.3.weight"].grad
    assert (g3[:6] != 0).any() and (g3[6:] == 0).all() and torch.isfinite(g3).all()
    gb = named["pose.net.3.bias"].grad
    assert (gb[:6] != 0).all() and (gb[6:] == 0).all()
    g1 = named["pose_encoder.encoder.conv1.weight"].grad
    assert torch.isfinite(g1).all() and g1.abs().max().item() > 0
    tr.model_optimizer.step()
    torch.cuda.synchronize()
    for m in ("pose_encoder", "pose"):
        changed = [k for k, p in named.items() if k.startswith(m + ".") and not torch.equal(p.detach(), before[k])]
        assert changed, m
    assert not torch.equal(named["pose.net.0.weight"].detach(), before["pose.net.0.weight"])
    assert torch.equal(named["pose_encoder.encoder.fc.weight"].detach(), before["pose_encoder.encoder.fc.weight"])   # never run


def test_freeze_teacher_and_pose_runs_the_pose_pass_without_a_tape(trainer):
    tr, batch = trainer
    tr.train_teacher_and_pose = False
    try:
        outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    finally:
        tr.train_teacher_and_pose = True
    assert not outputs[("cam_T_cam", 0, -1)].requires_grad and not outputs[("disp", 0)].requires_grad
    assert torch.isfinite(losses["loss"]).all()


def test_checkpoints_hold_both_pose_models_and_load_back(trainer):
    """save_model writes pose_encoder.pth / pose.pth under the reference's key names; load_model copies them back into the
    parameters the optimiser holds.  --models_to_load is at the parser's preset, which names both pose models and none of
    the depth networks: load_model reads the preset as "nothing named" and loads EVERY model of the run, so a parameter of
    ``mono_depth`` and one of ``rgb_encoder`` come back as well (the whole resume: tests/test_resume_gpu.py)."""
    import os
    from manydepth.options import MODELS_TO_LOAD_DEFAULT
    tr, _ = trainer
    assert "pose_encoder" in tr.opt.models_to_load and "pose" in tr.opt.models_to_load
    assert list(tr.opt.models_to_load) == list(MODELS_TO_LOAD_DEFAULT)
    depth = {f"{m}.{k}": dict(tr.models[m].named_parameters())[k]
             for m, k in (("mono_depth", "decoder.0.conv.conv.weight"), ("rgb_encoder", "encoder.conv1.weight"))}
    depth_before = {k: p.detach().clone() for k, p in depth.items()}
    assert all(v.abs().max().item() > 0 for v in depth_before.values())
    tr.save_model()
    folder = os.path.join(tr.log_path, "models", "weights_{}".format(tr.epoch))
    saved = {m: torch.load(os.path.join(folder, m + ".pth"), map_location="cpu") for m in ("pose_encoder", "pose")}
    assert list(saved["pose"]) == [f"net.{i}.{p}" for i in range(4) for p in ("weight", "bias")]
    assert "encoder.conv1.weight" in saved["pose_encoder"] and tuple(saved["pose_encoder"]["encoder.conv1.weight"].shape) == (64, 6, 7, 7)
    named = {f"{m}.{k}": p for m in ("pose_encoder", "pose") for k, p in tr.models[m].named_parameters()}
    ptrs = {k: p.data_ptr() for k, p in named.items()}
    for m in ("pose_encoder", "pose"):
        for k, v in tr.models[m].state_dict().items():
            assert torch.equal(saved[m][k], v.detach().cpu()), (m, k)
    with torch.no_grad():
        for p in list(named.values()) + list(depth.values()):
            p.zero_()
    tr.opt.load_weights_folder = folder
    tr.load_model()
    for k, p in depth.items():
        assert torch.equal(p.detach(), depth_before[k]), k
    for k, p in named.items():
        m, key = k.split(".", 1)
        assert torch.equal(p.detach().cpu(), saved[m][key]), k
        assert p.data_ptr() == ptrs[k], k                              # still the views of the flat parameter store


def test_data_parallel_is_refused(tmp_path):
    """The pose modules run once per neighbour, the gradient reducer expects one backward pass per module: refused."""
    import torch.distributed as dist
    from manydepth.trainer import Trainer
    opts = _opts(tmp_path)
    opts.pose_network = True
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "rendezvous"), 1), rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="torch.distributed"):
            Trainer(opts)
    finally:
        dist.destroy_process_group()


def test_constructor_refusals(tmp_path, monkeypatch):
    from manydepth.trainer import Trainer
    with pytest.raises(NotImplementedError, match="only --depth_supervision_only True --depth_supervision True"):
        Trainer(_opts(tmp_path))                                       # without the opt-in: as before
    opts = _opts(tmp_path)
    opts.pose_network = True
    opts.bf16 = True
    with pytest.raises(NotImplementedError, match="bf16"):
        Trainer(opts)
    opts = _opts(tmp_path)
    opts.pose_network = True
    opts.pose_input = True
    with pytest.raises(ValueError, match="pose_network"):
        Trainer(opts)
    opts = _opts(tmp_path, ["--depth_supervision_only", "True"])
    opts.pose_network = True
    with pytest.raises(ValueError, match="pose_network"):
        Trainer(opts)
    monkeypatch.setenv("PD_STEP_GRAPH", "1")
    opts = _opts(tmp_path)
    opts.pose_network = True
    with pytest.raises(NotImplementedError, match="PD_STEP_GRAPH"):
        Trainer(opts)
    monkeypatch.delenv("PD_STEP_GRAPH")
    from manydepth.train import options_from_environment
    assert options_from_environment(_opts(tmp_path), {"PD_POSE_NETWORK": "1"}).pose_network is True
    assert not hasattr(options_from_environment(_opts(tmp_path), {}), "pose_network")
