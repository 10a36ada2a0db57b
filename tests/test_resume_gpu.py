"""A checkpoint resumes every training mode bit for bit: Trainer.save_model after two steps, a NEW Trainer built with
``--load_weights_folder`` alone (no ``--models_to_load``), two more steps -- against the run that was never interrupted.

Per mode, run A (``torch.manual_seed(1)``, construct, steps on b0 b1, checkpoint, steps on b2 b3) and run B (the process-wide
state -- dropout seed and step counter, torch's generator -- moved elsewhere first, construct with the folder, steps on b2 b3).
Every step is ``torch.manual_seed(seed_i)`` (the automask noise of the photometric modes is the step's only draw),
``zero_grad``, ``process_batch``, ``backward``, ``step``; or one replay of a GraphedTrainStep.  Compared with ``torch.equal`` /
``==``: the bits of ``loss`` of steps three and four; then the flat parameter buffer, both Adam moment buffers, Adam's step
count (and its device word when the step is replayed from a graph), the learning rate, every module buffer (BatchNorm
running statistics, num_batches_tracked) and the dropout stream's seed and step counter -- right after B's construction
against A's snapshot at checkpoint time, and after the last step against A's end.

The bound is equality: both sides run the same kernels on the same inputs in the same order, and every reduction of this
build has a fixed order (tests/test_graph_gpu.py relies on the same for eager against replay); the control test shows that
two uninterrupted runs are equal, so a difference here is the checkpoint's.

Two checkpoint positions: "mid" -- ``save_model(epoch_complete=False, batch_idx=1)`` behind the second step, as run_epoch
writes it on a logging step -- and "lr" -- ``--scheduler_step_size 1``, ``model_lr_scheduler.step()`` then
``save_model(epoch_complete=True)``, as train() writes it behind an epoch: B must come up with the decayed learning rate.
The batches are fixed device tensors, so what a checkpoint does not hold (the loader's permutation and augmentation draws,
torch's generator: see save_model) plays no part.  Size of tests/test_step_gpu.py: batch 2, 64x96, dropout at its default
0.1 in every mode -- the mask stream has to continue."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS = (101, 102, 103, 104)            # torch.manual_seed in front of step i
DROPOUT_SEED, OTHER_DROPOUT_SEED = 4242, 777

MODES = {
    # 1: supervised only, three encoders
    "supervised": dict(kind="only", ckpt="mid"),
    # 2: ... in the bf16 training mode
    "bf16": dict(kind="only", ckpt="lr", attrs={"bf16": True}),
    # 3: photometric term from pose files (tests/test_step_reproj_gpu.py)
    "pose_input": dict(kind="poses", ckpt="mid"),
    # 4: ... from the pose network (tests/test_step_posenet_gpu.py): pose_encoder / pose are among the --models_to_load preset
    "posenet": dict(kind="posenet", ckpt="lr"),
    "posenet_supervise_pose": dict(kind="posenet", ckpt="mid", extra=("--supervise_pose", "True")),
    # 5: uncertainty heads (more parameters, some of them idle: another adam.pth order) and the polarimetric term
    "uncertainty_polar": dict(kind="only", ckpt="mid", attrs={"uncertainty_loss": 0.1, "polar_loss": (0.5, 0.5)}),
    # 6: the step replayed from a graph: Adam's t and the learning rate are device words of the optimizer
    "graph": dict(kind="only", ckpt="lr", graph=True),
}
assert {m["ckpt"] for m in MODES.values()} == {"mid", "lr"}


def _opts(tmp, mode, extra=()):
    from manydepth.options import MonodepthOptions
    m = MODES[mode]
    flags = {"only": ["--depth_supervision_only", "True"], "poses": ["--pose_input", "True"], "posenet": []}[m["kind"]]
    if m["ckpt"] == "lr":
        flags = flags + ["--scheduler_step_size", "1"]
    opts = MonodepthOptions().parse([
        "--png", "--batch_size", "2", "--height", "64", "--width", "96", "--dataset", "HAMMER", "--split", "HAMMER",
        "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision", "True", *flags,
        "--normals_loss_weight", "0.35", "--augment_xolp", "--augment_normals",
        "--log_dir", str(tmp), "--data_path", "synthetic", "--data_path_val", "synthetic", "--num_workers", "0",
        "--weights_init", "scratch", "--learning_rate", "1e-4", *m.get("extra", ()), *extra])
    if m["kind"] == "posenet":
        opts.pose_input = False
        opts.pose_network = True
    for k, v in m.get("attrs", {}).items():
        setattr(opts, k, v)
    assert opts.dropout_rate == 0.1
    return opts


def _batches(tr, mode):
    """Four distinct device batches.  The modes that need neighbouring frames (and the polarimetric term) take the items of
    the Trainer's own synthetic loader, in the dataset's order rather than the loader's shuffled one."""
    from polardepth import synthetic
    m = MODES[mode]
    if m["kind"] == "only" and "polar_loss" not in m.get("attrs", {}):
        return [synthetic.make_batch(2, 64, 96, frame_w=92, device="cuda", seed=20 + i) for i in range(4)]
    ds = tr.train_loader.dataset
    assert len(ds) >= 8
    out = []
    for i in range(4):
        b = torch.utils.data.default_collate([ds[2 * i], ds[2 * i + 1]])
        out.append({k: v.to(tr.device) for k, v in b.items()})
    return out


def _bits(loss):
    return int(loss.detach().float().reshape(1).view(torch.int32).item())


def _steps(tr, batches, seeds, gs=None):
    bits = []
    for b, s in zip(batches, seeds):
        torch.manual_seed(s)
        if gs is not None:
            loss = gs.step(b)
        else:
            tr.model_optimizer.zero_grad()
            _, losses, _ = tr.process_batch(dict(b), is_train=True)
            losses["loss"].backward()
            tr.model_optimizer.step()
            loss = losses["loss"]
        bits.append(_bits(loss))
    torch.cuda.synchronize()
    return bits


def _state(tr):
    from polardepth import functional as PF
    opt = tr.model_optimizer
    torch.cuda.synchronize()
    return {
        "store.flat": tr.store.flat.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
        "step_count": opt.step_count, "lr": opt.param_groups[0]["lr"], "last_lr": list(tr.model_lr_scheduler.get_last_lr()),
        "scheduler.last_epoch": tr.model_lr_scheduler.last_epoch,
        "dropout_seed": PF.DropoutState.seed, "dropout_step": PF.DropoutState.get_step(tr.device),
        "buffers": {f"{mn}.{k}": b.detach().clone() for mn, mod in tr.models.items() for k, b in mod.named_buffers()},
        # Adam's t as the captured step reads it
        "dev_t": int(opt.dev_state[1].item()) if opt.device_step else None,
    }


def _assert_same(want, got, what, skip=()):
    assert want.keys() == got.keys()
    for k, a in want.items():
        if k in skip:
            continue
        b = got[k]
        if k == "buffers":
            assert list(a) == list(b), what
            assert any(n.endswith("running_var") for n in a) and any(n.endswith("num_batches_tracked") for n in a)
            for n in a:
                assert torch.equal(a[n], b[n]), f"{what}: buffer {n}"
        elif torch.is_tensor(a):
            if not torch.equal(a, b):
                first = int((a != b).nonzero()[0])
                raise AssertionError(f"{what}: {k} differs in {int((a != b).sum())} of {a.numel()} elements, first at {first}: "
                                     f"{a[first].item()!r} != {b[first].item()!r}")
        else:
            assert a == b, f"{what}: {k}: {a!r} != {b!r}"


class _RunA:
    pass


def _run_a(mode, tmp):
    """The uninterrupted run, with the checkpoint written behind its second step."""
    from manydepth.trainer import Trainer
    from polardepth import functional as PF
    from polardepth.graph import GraphedTrainStep
    m = MODES[mode]
    PF.DropoutState.manual_seed(DROPOUT_SEED)               # (also puts the device step counter to 0)
    torch.manual_seed(1)
    a = _RunA()
    a.tr = tr = Trainer(_opts(tmp, mode))
    tr.set_train()
    a.batches = _batches(tr, mode)
    a.lr0 = tr.model_optimizer.param_groups[0]["lr"]
    a.gs = GraphedTrainStep(tr, a.batches[0], warmup=1, restore_state=True) if m.get("graph") else None
    a.bits = _steps(tr, a.batches[:2], SEEDS[:2], a.gs)
    tr.epoch = 0
    if m["ckpt"] == "lr":                                   # train(): run_epoch ends with the scheduler's step, then the checkpoint
        tr.step = 2
        tr.model_lr_scheduler.step()
        tr.save_model(epoch_complete=True)
        a.resume = (1, 2, 0)
    else:                                                   # run_epoch on a logging step: before `self.step += 1`
        tr.step = 1
        tr.save_model(epoch_complete=False, batch_idx=1)
        a.resume = (0, 2, 2)
    a.folder = os.path.join(tr.log_path, "models", "weights_0")
    a.at_ckpt = _state(tr)
    a.bits += _steps(tr, a.batches[2:], SEEDS[2:], a.gs)
    a.end = _state(tr)
    return a


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """Run A of a mode, made once per module: the resume case and the in-process reload of a mode share it."""
    runs = {}

    def get(mode):
        if mode not in runs:
            runs[mode] = _run_a(mode, tmp_path_factory.mktemp("a_" + mode))
        return runs[mode]
    yield get
    runs.clear()


@pytest.fixture(autouse=True)
def _dropout_stream_put_back():
    """The dropout stream is process-wide: leave it to the other modules as it was found."""
    from polardepth import functional as PF
    dev = torch.device("cuda", torch.cuda.current_device())
    seed, site, step = PF.DropoutState.seed, PF.DropoutState.site, PF.DropoutState.get_step(dev)
    yield
    PF.DropoutState.seed, PF.DropoutState.site = seed, site
    PF.DropoutState.set_step(dev, step)


def _elsewhere(device):
    """Process-wide state where a new process would not have it by accident: whatever the checkpoint fails to restore
    differs from run A afterwards."""
    from polardepth import functional as PF
    PF.DropoutState.manual_seed(OTHER_DROPOUT_SEED)
    PF.DropoutState.set_step(device, 0)
    torch.manual_seed(2)


def _check_run_a(mode, a):
    m = MODES[mode]
    assert len(set(a.bits)) == 4, a.bits                    # four different batches, four different losses
    assert a.end["step_count"] == 4 and a.at_ckpt["step_count"] == 2
    assert a.at_ckpt["dropout_step"] == 2 and a.end["dropout_step"] == 4 and a.end["dropout_seed"] == DROPOUT_SEED
    assert not torch.equal(a.at_ckpt["store.flat"], a.end["store.flat"])
    assert not torch.equal(a.at_ckpt["exp_avg_sq"], a.end["exp_avg_sq"])
    if m["ckpt"] == "lr":                                   # the checkpoint lies behind a StepLR boundary
        assert a.lr0 == 1e-4 and abs(a.at_ckpt["lr"] - 1e-5) < 1e-12 and a.end["lr"] == a.at_ckpt["lr"]
    else:
        assert a.at_ckpt["lr"] == a.end["lr"] == a.lr0 == 1e-4
    if m.get("graph"):
        assert a.at_ckpt["dev_t"] == 2 and a.end["dev_t"] == 4


@pytest.mark.parametrize("mode", list(MODES))
def test_resumed_run_equals_the_uninterrupted_run(mode, run_a, tmp_path):
    from manydepth.options import MODELS_TO_LOAD_DEFAULT
    from manydepth.trainer import Trainer
    from polardepth.graph import GraphedTrainStep
    m = MODES[mode]
    a = run_a(mode)
    _check_run_a(mode, a)
    if m["kind"] == "posenet":
        assert {"pose_encoder", "pose", "rgb_encoder", "mono_depth"} <= set(a.tr.models)
    if "uncertainty_loss" in m.get("attrs", {}):            # the extra heads are in the flat buffer and in adam.pth
        assert a.tr.uncertainty_loss == 0.1 and a.tr.polar_loss == [0.5, 0.5]
        assert a.tr.store.numel > run_a("supervised").tr.store.numel
    assert sorted(os.listdir(a.folder)) == sorted([n + ".pth" for n in a.tr.models] + ["adam.pth", "trainer_state.pth"])

    _elsewhere(a.tr.device)
    tr = Trainer(_opts(tmp_path, mode, ["--load_weights_folder", a.folder]))
    assert list(tr.opt.models_to_load) == list(MODELS_TO_LOAD_DEFAULT)       # nothing was named
    tr.set_train()
    assert (tr.resume_epoch, tr.resume_step, tr.resume_batch) == a.resume
    _assert_same(a.at_ckpt, _state(tr), f"{mode}: after load", skip=("dev_t",))
    gs = GraphedTrainStep(tr, a.batches[2], warmup=1, restore_state=True) if m.get("graph") else None
    if gs is not None:                                      # built behind the load: t starts from the loaded count
        assert int(tr.model_optimizer.dev_state[1].item()) == 2
        _assert_same(a.at_ckpt, _state(tr), f"{mode}: after building the graph")
    bits = _steps(tr, a.batches[2:], SEEDS[2:], gs)
    assert bits == a.bits[2:], f"{mode}: loss bits of steps 3, 4: resumed {bits}, uninterrupted {a.bits[2:]}"
    _assert_same(a.end, _state(tr), f"{mode}: after step 4")


def test_control_two_uninterrupted_runs_are_equal(run_a, tmp_path):
    """Without this a failing resume comparison could not be told from run-to-run noise."""
    a = run_a("supervised")
    b = _run_a("supervised", tmp_path)
    assert b.bits == a.bits
    _assert_same(a.at_ckpt, b.at_ckpt, "control: at the checkpoint")
    _assert_same(a.end, b.end, "control: after step 4")


@pytest.mark.parametrize("mode", ["supervised", "graph"])
def test_load_model_on_a_trainer_that_has_trained_goes_back_to_the_checkpoint(mode, run_a):
    """The same object, after its four steps: load_model puts parameters, moments, buffers, counters and the dropout stream
    back, and steps three and four repeat bit for bit -- nothing derived from the later weights survives (transposed
    data-gradient operands; in the graph mode the captured step's device words: Adam's t, the learning rate)."""
    a = run_a(mode)
    _check_run_a(mode, a)
    tr = a.tr
    # (the dropout stream is process-wide and has moved on with the tests in between: load_model must put it back too)
    _assert_same(a.end, _state(tr), f"{mode}: run A is where it ended", skip=("dropout_seed", "dropout_step"))
    _elsewhere(tr.device)
    tr.opt.load_weights_folder = a.folder
    tr.load_model()
    _assert_same(a.at_ckpt, _state(tr), f"{mode}: after the reload")
    bits = _steps(tr, a.batches[2:], SEEDS[2:], a.gs)
    assert bits == a.bits[2:], f"{mode}: loss bits of steps 3, 4: after the reload {bits}, first time {a.bits[2:]}"
    _assert_same(a.end, _state(tr), f"{mode}: after step 4 again")
