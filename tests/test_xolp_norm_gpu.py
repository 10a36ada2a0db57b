"""The configurable (mean, std) pair of the XOLP encoder on the GPU: the default is unchanged bit for bit, a pair of one's own
reaches the stem's gather (parity with the CPU oracle whose constants are patched to the pair), travels with the checkpoint
and reaches Evaluation, and the captured training step replays it."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
sys.path.insert(0, GOLDEN)
from synth_weights import fill_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
PAIR = (0.21, 0.17)          # far from the reference's (0.0869, 0.4443)
FWD_TOL, GRAD_TOL = 2e-5, 5e-4      # tests/test_modules_gpu.py


def _run(mod, x, seed=100):
    """Training-mode forward and backward through a fixed random objective: (output, parameter gradients)."""
    from polardepth import functional as PF
    mod.train()
    mod.zero_grad()
    y = mod(x)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed)).to(y.device)
    (y * w).sum().backward()
    PF.sync_wgrad_stream()           # the device modules produce weight gradients on a side stream
    return y.detach(), {k: p.grad.detach().clone() for k, p in mod.named_parameters() if p.grad is not None}


def test_the_default_pair_is_the_default_bit_for_bit():
    from manydepth import networks
    from manydepth.networks.pre_encoders import XOLP_MEAN, XOLP_STD
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "g4_nets.npz"))["xolp"]).cuda()
    outs = []
    # the first pass is a warm-up: the scratch buffer of the split weight-gradient reductions (polardepth.ops._workspace) grows
    # on first use, and the slice count of a reduction follows the size it is handed -- the two passes that are compared
    # run with the buffer at its final size
    for kw in ({}, {}, {"xolp_norm": (XOLP_MEAN, XOLP_STD)}):
        mod = fill_state_dict(networks.ShallowEncoder('XOLP', 2, 0.0, **kw), 0, prefix="xolp_encoder.").cuda()
        outs.append(_run(mod, x))
        mod.eval()
        with torch.no_grad():
            outs[-1] += (mod(x),)
    (y0, g0, e0), (y1, g1, e1) = outs[1:]
    assert torch.equal(y0, y1) and torch.equal(e0, e1)
    assert set(g0) == set(g1) and len(g0) > 10
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def _close(a, b, tol, what):
    a, b = torch.as_tensor(a).detach().cpu().float(), torch.as_tensor(b).detach().float()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _check_against_oracle(mod, ref, x):
    """The procedure and tolerances of tests/test_modules_gpu.py::_check_module, with the CPU oracle module in the place of the
    fixture (a fixture of the reference's modules exists for its own constants only)."""
    ref.eval(); mod.eval()
    with torch.no_grad():
        _close(mod(x.cuda()), ref(x), FWD_TOL, "eval")
    y, grads = _run(mod, x.cuda())
    yr, grads_r = _run(ref, x)
    _close(y, yr, FWD_TOL, "train")
    n = 0
    for k, g in grads_r.items():
        if k.endswith("conv.bias"):       # conv bias feeds BatchNorm: exact zero here, ~1e-7 noise in torch
            assert k not in grads or grads[k].abs().max().item() <= 1e-4 * (1 + g.abs().max().item())
            continue
        _close(grads[k], g, GRAD_TOL, "grad " + k); n += 1
    assert n > 10
    for (k, v), (_, vr) in zip(mod.state_dict().items(), ref.state_dict().items()):
        if "running" in k:
            _close(v, vr, 1e-5, "buffer " + k)


def test_a_pair_of_ones_own_matches_the_patched_oracle(monkeypatch):
    from manydepth import networks
    from oracle import nets as onets
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "g4_nets.npz"))["xolp"])

    def pair_of_modules():
        mod = fill_state_dict(networks.ShallowEncoder('XOLP', 2, 0.0, xolp_norm=PAIR), 0, prefix="xolp_encoder.").cuda()
        ref = fill_state_dict(onets.ShallowEncoder('XOLP', 2, 0.0), 0, prefix="xolp_encoder.")
        return mod, ref

    # against the oracle as it stands (the HAMMER constants) the same comparison must fail: the pair arrives in the kernel
    with pytest.raises(AssertionError, match="max err"):
        _check_against_oracle(*pair_of_modules(), x)
    monkeypatch.setattr(onets, "XOLP_MEAN", PAIR[0])
    monkeypatch.setattr(onets, "XOLP_STD", PAIR[1])
    _check_against_oracle(*pair_of_modules(), x)


def _step(tr, batch):
    tr.set_train()
    tr.model_optimizer.zero_grad()
    _, losses, _ = tr.process_batch(dict(batch), is_train=True)
    losses["loss"].backward()
    tr.model_optimizer.step()
    return losses["loss"].detach().clone()


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """One Trainer with opt.xolp_norm set: a step, save_model -> (weights folder, log path)."""
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    from polardepth import synthetic
    torch.manual_seed(0)
    opts = _opts(tmp_path_factory.mktemp("xolp_norm"), ["--dropout_rate", "0.0"])
    opts.xolp_norm = "0.21,0.17"
    tr = Trainer(opts)
    assert tr.xolp_norm == PAIR and tr.models["xolp_encoder"].Conv1.in_affine == PAIR
    _step(tr, synthetic.make_batch(2, 64, 96, frame_w=92, device="cuda", seed=0))
    tr.epoch = 0
    tr.save_model()
    return os.path.join(tr.log_path, "models", "weights_0"), tr.log_path


def test_the_pair_travels_with_the_checkpoint(checkpoint, tmp_path):
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    folder, log_path = checkpoint
    assert json.load(open(os.path.join(log_path, "models", "opt.json")))["xolp_norm"] == "0.21,0.17"
    assert tuple(torch.load(os.path.join(folder, "trainer_state.pth"))["xolp_norm"]) == PAIR
    assert not any("norm" in k for k in torch.load(os.path.join(folder, "xolp_encoder.pth")))
    # unset: the checkpoint's pair is adopted (and recorded in the new run's opt.json)
    tr = Trainer(_opts(tmp_path / "adopt", ["--load_weights_folder", folder]))
    assert tr.xolp_norm == PAIR and tr.models["xolp_encoder"].Conv1.in_affine == PAIR
    assert tuple(json.load(open(os.path.join(tr.log_path, "models", "opt.json")))["xolp_norm"]) == PAIR
    # the same pair again is fine; a different one raises and names both
    same = _opts(tmp_path / "same", ["--load_weights_folder", folder])
    same.xolp_norm = PAIR
    assert Trainer(same).xolp_norm == PAIR
    other = _opts(tmp_path / "other", ["--load_weights_folder", folder])
    other.xolp_norm = (0.3, 0.2)
    with pytest.raises(ValueError, match=r"\(0\.3, 0\.2\).*\(0\.21, 0\.17\)"):
        Trainer(other)


def test_evaluation_picks_the_pair_up(checkpoint, monkeypatch):
    from manydepth.evaluation import Evaluation
    from manydepth.networks.pre_encoders import XOLP_MEAN, XOLP_STD
    from polardepth import synthetic
    folder, _ = checkpoint
    monkeypatch.delenv("PD_XOLP_NORM", raising=False)
    kw = dict(load_weights_folder=folder, data_path="synthetic", height=64, width=96, batch_size=2)
    ev = Evaluation(**kw)
    assert ev.xolp_norm == PAIR and ev.models["xolp_encoder"].Conv1.in_affine == PAIR
    forced = Evaluation(xolp_norm=(XOLP_MEAN, XOLP_STD), **kw)          # the argument goes first
    assert forced.models["xolp_encoder"].Conv1.in_affine == (XOLP_MEAN, XOLP_STD)
    monkeypatch.setenv("PD_XOLP_NORM", "0.3,0.2")                       # then the environment, then the checkpoint
    assert Evaluation(**kw).xolp_norm == (0.3, 0.2) and Evaluation(xolp_norm=PAIR, **kw).xolp_norm == PAIR
    monkeypatch.delenv("PD_XOLP_NORM")
    assert Evaluation(data_path="synthetic", height=64, width=96, batch_size=2).xolp_norm is None      # the HAMMER constants
    depths = []
    for e in (ev, forced):
        e.load_mono_model()
        depths.append(e.predict(synthetic.make_batch(2, 64, 96, frame_w=92, device="cuda", seed=4)))
    assert bool(torch.isfinite(depths[0]).all()) and not torch.equal(depths[0], depths[1])


def test_the_captured_step_replays_the_pair(tmp_path):
    """PD_STEP_GRAPH's step object with opt.xolp_norm set: the first replayed step's loss equals the eager step's bit for bit
    (tests/test_graph_gpu.py asserts it for the default); the pair is a launch constant, nothing else is needed."""
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    from polardepth import functional as PF
    from polardepth import synthetic
    from polardepth.graph import GraphedTrainStep
    batch = synthetic.make_batch(2, 64, 96, frame_w=92, device="cuda", seed=0)

    def trainer(tag, pair):
        torch.manual_seed(0)
        PF.DropoutState.manual_seed(99)
        opts = _opts(tmp_path / tag, ["--dropout_rate", "0.1"])
        opts.xolp_norm = pair
        return Trainer(opts)

    eager = _step(trainer("eager", PAIR), batch)
    tr = trainer("graph", PAIR)
    gs = GraphedTrainStep(tr, batch, warmup=1, restore_state=True)
    graphed = gs.step(batch).detach().clone()
    torch.cuda.synchronize()
    assert torch.equal(eager, graphed), (eager.item(), graphed.item())


def test_the_tool_prints_a_pair_a_trainer_accepts(tmp_path, capsys, monkeypatch):
    """tools/xolp_stats.py on synthetic items (in process): the reference's six lines, a JSON file, and a PD_XOLP_NORM string
    that, fed back through the options, constructs a Trainer with that pair."""
    import importlib.util
    from conftest import ROOT
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    from polardepth import polar
    for var in ("PD_POL_ANGLES", "PD_POL_LAYOUT", "PD_POL_DEMOSAIC", "PD_POL_BAYER", "PD_POL_GAINS", "PD_POL_COLOR_SCALE"):
        monkeypatch.delenv(var, raising=False)
    spec = importlib.util.spec_from_file_location("xolp_stats_tool", os.path.join(ROOT, "tools", "xolp_stats.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out_json = tmp_path / "x.json"
    tool.main(["--data_path", "synthetic", "--batches", "2", "--height", "64", "--width", "96", "--hist", "--json", str(out_json)])
    lines = capsys.readouterr().out.splitlines()
    assert [l.split(":")[0] for l in lines[:6]] == ["DOLP MEAN", "DOLP STD", "AOLP MEAN", "AOLP STD", "XOLP MEAN", "XOLP STD"]
    res = json.load(open(out_json))
    assert res["n"] == res["items"] * 64 * 96 and res["items"] == 8 and res["nonfinite"] == 0
    assert len(res["hist_dolp"]) == 257 and sum(res["hist_dolp"]) == res["n"] == sum(res["hist_aolp"])
    assert float(lines[4].split(":")[1]) == res["xolp_mean"] == 0.5 * (res["dolp_mean"] + res["aolp_mean"])
    norm = [l for l in lines if l.startswith("PD_XOLP_NORM=")]
    assert len(norm) == 1
    pair = polar.parse_xolp_norm(norm[0].split("=", 1)[1])
    assert pair == (res["xolp_mean"], res["xolp_std"])
    opts = _opts(tmp_path / "fed_back")
    opts.xolp_norm = norm[0].split("=", 1)[1]          # what manydepth/train.py does with $PD_XOLP_NORM
    assert Trainer(opts).models["xolp_encoder"].Conv1.in_affine == pair
