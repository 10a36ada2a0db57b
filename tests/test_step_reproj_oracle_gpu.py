"""One training step of the photometric mode (--depth_supervision True --pose_input True) through the Trainer façade against
the CPU oracle in fp32 and fp64 (oracle/nets.py, oracle/losses.py, oracle/reproj.py through tests/oracle_step.py), from the
same weights and the same batch: B = 2, 64 x 96, dropout 0, BatchNorm in training mode, as tests/test_step_gpu.py.  The
batch is ``oracle_step.multiview_batch``: a textured plane seen from known poses, so the term measures something -- on it the
fp64 weight gradients with and without the term differ by 0.58 relative L2 at the 10th percentile of the tensors.

What is compared.  The device draws the automask noise from torch's device generator; the test re-seeds, draws the same maps
and re-evaluates ``PF.photometric_loss`` on the Trainer's own depth maps with ITS OWN wiring of the batch (frames, poses,
intrinsics of scale 0, ``frame_valid``): bit-equal losses prove the noise and give the device's selection maps ``sel``.  Both
oracles then run with that noise and with the device's two kinds of discrete choices: ``sel`` (winning frame / automask per
pixel) and the bilinear cell every warped pixel was sampled in (``coords``, the coordinates pd_view_synth_fwd stored;
oracle.reproj.sample_in_cells).  A pixel that picks another frame, or another cell, in another arithmetic is another function
there, not a rounding error; the fp64 oracle's own choices differ from the device's on the pixels counted below (cap 1 %).

Why the cells.  The bars below were set before anything was measured; run with ``sel`` alone, base missed the weight-gradient bar on the MI355X: median
e_hip / e_cpu32 10.6, worst mono_depth.decoder.12.conv.weight e_hip 2.2e-3 against e_cpu32 7.3e-5.  Rerunning the fp32 oracle
with its colour input perturbed by 1e-7 relative (8 seeds) moved its own gradients to at most 1.7e-4 on that tensor, so that
remedy did not apply.  The cause was located instead: the device's d loss / d disparity equals the fp64 one AT THE DEVICE'S
disparities to 9e-6 per scale, and the device's weight gradients equal the fp64 network's backward pass of that disparity
gradient to 1.2e-5 (median; decoder 7e-7 to 6e-6) -- the device is right.  The fp64 term gradient of scale 2 itself differs by
1.05e-3 between the oracle's disparities and the device's (2.8e-6 apart): 99.9 % of that is one pixel of frame +1 (item 0,
y 11, x 88) sampled at u = 34.99993 on one side and 35.00003 on the other.  With the device's cells given, that difference is
3.8e-5, the loss entries move by 2e-10 relative, and the fp32 oracle's own median distance drops from 6.6e-5 to 2.8e-5.  The
term's other kinks (an SSIM clamp, the sign of an L1 difference) are not pinned; none showed in these four cases.
Against the fp64 oracle:
  disparities        2e-5 (both oracles)
  loss entries       1e-4 relative: loss, loss/s, reproj_loss/s, supervised_depth_loss/s
  term, wiring only  the oracle term at the device's depth maps: |dev - ref64| <= 4 |ref32 - ref64| + 1e-6 |ref64|
  term gradient      d sum_s(reproj_loss/s) / d disp_s at the device's disparities as leaves, per scale:
                     relative L2 <= 4 x the fp32 oracle's relative L2 + 1e-6
  weight gradients   per tensor e_hip <= max(1e-4, 2 e_cpu32, 2 e_ctl): relative L2 distances from fp64 of the device, of the
                     fp32 oracle, and of the device on the SUPERVISED-ONLY step of the same weights and batch (the control:
                     code tests/test_step_gpu.py pins; it carries the tensors that are ill-conditioned at this size with or
                     without the term)
  power              >= 90 % of the tensors: the fp64 gradients without the term lie >= 10 x that tensor's bound away
  Adam               finite parameters, cleared gradient buffer, first-step rule on mono_depth.decoder.0.conv.conv.weight

Cases: base (automask + noise, minimum, SSIM), missing_avg (--avg_reprojection, item 1 lacks frame +1), plain (--no_ssim
--disable_automasking), three_frames (frames 0 -1 1 2, item 0 lacks frame -1, scales 0 2).  With scales 0 2 the encoders'
gradients are ill-conditioned at this size on every fp32 path, term or no term (fp32 oracle: median 1e-2 from fp64); the
decoder tensors, whose backward plumbing the new mode reorders, stay at 1e-5 and are held at the 1e-4 floor.

Measured on an MI355X (see the figures each case prints: STEPFIG lines):
case          loss (rel err)  reproj_loss/s (worst)  term at device depth, err / tol (worst scale)  tensors  median / largest e_hip / e_cpu32  power
base          6.5e-07         7.0e-06                1.43e-06 / 5.23e-06                           160      1.19 / 6.79                      160 of 160
missing_avg   6.1e-07         6.4e-06                1.42e-06 / 5.45e-06                           160      1.29 / 2.90                      160 of 160
plain         2.1e-08         2.5e-07                6.47e-09 / 1.78e-07                           160      1.23 / 2.72                      160 of 160
three_frames  2.8e-07         3.0e-06                6.94e-07 / 2.35e-06                           156      0.91 / 1.79                      156 of 156
term gradient per scale, rel L2 / bound:
  base          2.42e-05 / 1.02e-04   1.95e-05 / 7.41e-05   1.57e-05 / 6.63e-05   8.46e-06 / 3.47e-05
  missing_avg   2.57e-05 / 1.05e-04   1.71e-05 / 7.22e-05   1.36e-05 / 5.33e-05   8.78e-06 / 3.08e-05
  plain         2.37e-07 / 5.76e-06   2.03e-07 / 3.98e-06   2.64e-07 / 5.01e-06   2.40e-07 / 2.29e-06
  three_frames  2.66e-05 / 1.12e-04 (scale 0)   1.64e-05 / 6.97e-05 (scale 2)
worst tensor against its bound (e_hip, e_cpu32, e_ctl):
  base          mono_depth.decoder.12.conv.bias            2.52e-04  1.60e-04  7.69e-06
  missing_avg   normals_encoder.ResBlock1.conv1.bn.weight  1.66e-04  1.65e-04  1.72e-05
  plain         normals_encoder.Conv1.bn.weight            1.92e-04  1.86e-04  2.80e-05
  three_frames  normals_encoder.ResBlock1.conv1.bn.bias    5.34e-03  5.34e-03  6.96e-03
e_ctl of the three worst-conditioned tensors (normals_encoder ResBlock1.conv1.bn.bias, Conv1.bn.bias, Conv1.conv.weight):
  scales 0 1 2 3: 7.13e-05, 4.63e-05, 3.93e-05 (with the term their e_cpu32 is 9.3e-04, 5.5e-04, 4.1e-04 on base and
  3.1e-03, 2.0e-03, 1.2e-03 on missing_avg, the device's e_hip equal to it within 1 %);  scales 0 2: 6.96e-03, 4.94e-03, 5.45e-03
pixels where the fp64 oracle's own selection differs from the device's, per scale (of 12288), and pixels it samples in another cell
(of 12288 per neighbour):
  base 0 1 1 1 and 0 1 3 0;  missing_avg 0 1 0 0 and 0 1 3 0;  plain 0 0 0 0 and 0 1 3 0;  three_frames 1 0 and 1 0
each case takes 1.3 to 5 s (the first one pays the control's Trainer and its fp64 pass).
"""
import statistics
import sys

import pytest
import torch

from conftest import GOLDEN
sys.path.insert(0, GOLDEN)
from synth_weights import fill_state_dict  # noqa: E402

from oracle_step import multiview_batch, oracle_grads, oracle_term  # noqa: E402

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 96
SEED = 1234
LR = 1e-4

CASES = {
    #                extra options                                 frames          frame_valid overrides    scales
    "base":         ((),                                            (0, -1, 1),     {},                      (0, 1, 2, 3)),
    "missing_avg":  (("--avg_reprojection",),                       (0, -1, 1),     {1: (1.0, 0.0)},         (0, 1, 2, 3)),
    "plain":        (("--no_ssim", "--disable_automasking"),        (0, -1, 1),     {},                      (0, 1, 2, 3)),
    "three_frames": ((),                                            (0, -1, 1, 2),  {-1: (0.0, 1.0)},        (0, 2)),
}


def _opts(tmp, extra, frame_ids, scales, only=False):
    from manydepth.options import MonodepthOptions
    mode = ["--depth_supervision_only", "True"] if only else ["--pose_input", "True"]
    return MonodepthOptions().parse([
        "--png", "--batch_size", str(B), "--height", str(H), "--width", str(W), "--dataset", "HAMMER", "--split", "HAMMER",
        "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision", "True", *mode,
        "--normals_loss_weight", "0.35", "--augment_xolp", "--augment_normals", "--dropout_rate", "0.0",
        "--log_dir", str(tmp), "--data_path", "synthetic", "--data_path_val", "synthetic", "--num_workers", "0",
        "--weights_init", "scratch", "--learning_rate", str(LR), "--scales", *map(str, scales),
        "--frame_ids", *map(str, frame_ids), *extra])


def _trainer(tmp, extra, frame_ids, scales, only=False):
    """(Trainer, oracle modules) with the same synthetic weights, both in training mode."""
    from manydepth.trainer import Trainer
    from oracle import nets as onets
    tr = Trainer(_opts(tmp, extra, frame_ids, scales, only))
    ref = onets.build_models(True, True, 0.0, scales=scales)
    assert set(ref) == set(tr.models)
    for name, m in ref.items():
        fill_state_dict(m, 0, prefix=name + ".")
        tr.models[name].load_state_dict(m.state_dict())
        m.train()
    tr.set_train()
    return tr, ref


class _cpu_threads:
    """torch's CPU threads limited to min(n, 16) around the oracle passes (tests/test_prodsize_gpu.py)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(min(self.n, 16))

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def _device_grads(tr):
    return {f"{mn}.{k}": p.grad.detach().cpu().clone() for mn in tr.models for k, p in tr.models[mn].named_parameters()}


def _skipped(k):
    return k.endswith("conv.bias") and not k.startswith("mono_depth")      # bias in front of BatchNorm: exactly 0 here


def _rel_l2(got, ref):
    return ((got.double() - ref).norm() / (ref.norm() + 1e-30)).item()


@pytest.fixture(scope="module")
def control(tmp_path_factory):
    """Per (frames, scales): the supervised-only step on a Trainer of its own with the same weights and batch, once per
    module -- e_ctl per tensor (device vs the supervised-only fp64 oracle) and those fp64 gradients (the power check)."""
    from polardepth import functional as PF
    cache = {}

    def get(frame_ids, scales):
        key = (tuple(frame_ids), tuple(scales))
        if key not in cache:
            tr, ref = _trainer(tmp_path_factory.mktemp("control"), (), frame_ids, scales, only=True)
            assert not tr.photometric
            batch = multiview_batch(B, H, W, frame_ids)
            tr.model_optimizer.zero_grad()
            _, losses, _ = tr.process_batch(dict(batch), is_train=True)
            assert not any(k.startswith("reproj_loss") for k in losses)
            losses["loss"].backward()
            PF.sync_wgrad_stream()
            torch.cuda.synchronize()
            dev = _device_grads(tr)
            with _cpu_threads():
                g64, L64, _ = oracle_grads(ref, {k: v.cpu() for k, v in batch.items()}, H, W, torch.float64, scales=scales)
            assert abs(losses["loss"].item() - L64["loss"]) <= 1e-4 * abs(L64["loss"])
            cache[key] = {"e_ctl": {k: _rel_l2(dev[k], g) for k, g in g64.items() if not _skipped(k)}, "g64": g64}
            tr.model_optimizer.zero_grad()
        return cache[key]
    return get


@pytest.mark.parametrize("case", list(CASES))
def test_photometric_step_matches_the_fp64_oracle(case, tmp_path, control):
    from oracle import losses as ol, reproj as orp
    from polardepth import functional as PF, ops
    extra, frame_ids, invalid, scales = CASES[case]
    scales, ids = list(scales), list(frame_ids[1:])
    tr, ref = _trainer(tmp_path, extra, frame_ids, scales)
    assert tr.photometric and tr.frame_ids == list(frame_ids) and list(tr.opt.scales) == scales
    no_ssim, automask, avg = tr.opt.no_ssim, not tr.opt.disable_automasking, tr.opt.avg_reprojection
    batch = multiview_batch(B, H, W, frame_ids)
    for i, row in invalid.items():
        batch[("frame_valid", i)] = torch.tensor(row, device="cuda")
    cpu = {k: v.cpu() for k, v in batch.items()}
    valid = torch.stack([batch[("frame_valid", i)] for i in ids], 1)                       # [B, F]
    assert (valid.sum(1) > 0).all()

    # ---- the device step
    tr.model_optimizer.zero_grad()
    torch.cuda.manual_seed(SEED)
    outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    disps = [outputs[("disp", s)] for s in scales]
    gterm = torch.autograd.grad(sum(losses[f"reproj_loss/{s}"] for s in scales), disps, retain_graph=True)
    losses["loss"].backward()
    PF.sync_wgrad_stream()
    torch.cuda.synchronize()
    dev_grads = _device_grads(tr)
    before = tr.store.flat.clone()

    # ---- noise and selection: the same draws, the term once more on the Trainer's depth maps with the test's own wiring
    depths = [outputs[("depth", 0, s)].detach() for s in scales]
    noise = None
    if automask:
        torch.cuda.manual_seed(SEED)
        noise = [torch.randn(depths[0].shape, device=depths[0].device).mul_(1e-5) for _ in scales]
    with torch.no_grad():
        again, sels = PF.photometric_loss(tr.loss_cfg, None, depths, batch[("color", 0, 0)], [batch[("color", i, 0)] for i in ids],
                                          batch[("K", 0)], batch[("inv_K", 0)], [batch[("poses", i)] for i in ids], valid,
                                          noise=noise, no_ssim=no_ssim, automask=automask, avg=avg, details=True)
    for n, s in enumerate(scales):
        assert torch.equal(again[n], losses[f"reproj_loss/{s}"].detach()), (s, again[n].item(), losses[f"reproj_loss/{s}"].item())
    sels = [s.cpu() for s in sels]
    for n, s in enumerate(scales):
        for b in range(B):
            kept = sels[n][b] != 255
            share = kept.float().mean().item()
            if automask:
                assert 0.05 <= share <= 0.95, (s, b, share)
            else:
                assert share == 1.0
            if not avg:
                for f in range(len(ids)):
                    won = ((sels[n][b] == f).sum() / kept.sum()).item()
                    assert (won >= 0.02) if valid[b, f] else (won == 0.0), (s, b, f, won)
            else:
                assert set(sels[n][b].unique().tolist()) <= {0, 255}
    # the other discrete choice: the bilinear cell every warped pixel was sampled in (the coordinates pd_view_synth_fwd stored)
    with torch.no_grad():
        coords = [[ops.view_synthesis(d, batch[("color", i, 0)], batch[("K", 0)], batch[("inv_K", 0)], batch[("poses", i)])[1].cpu()
                   for i in ids] for d in depths]
    ph = dict(frame_ids=frame_ids, scales=scales, no_ssim=no_ssim, automask=automask, avg=avg,
              noise=None if noise is None else [z.cpu() for z in noise], sels=sels, coords=coords)

    # ---- the oracle passes
    dev_disps = {s: outputs[("disp", s)].detach().cpu() for s in scales}
    dev_depths = {s: d.cpu() for s, d in zip(scales, depths)}
    with _cpu_threads():
        g64, L64, d64, _ = oracle_grads(ref, cpu, H, W, torch.float64, ph)
        g32, L32, d32, _ = oracle_grads(ref, cpu, H, W, torch.float32, ph)
        own = oracle_term(cpu, H, W, torch.float64, dict(ph, sels=None, coords=None), depths=dev_depths)[1]
        t64, t32 = (oracle_term(cpu, H, W, dt, ph, depths=dev_depths)[0] for dt in (torch.float64, torch.float32))
        (_, gd64), (_, gd32) = (oracle_term(cpu, H, W, dt, ph, disps=dev_disps) for dt in (torch.float64, torch.float32))
    ctl = control(frame_ids, scales)

    # the fp64 oracle's own selection under the same noise, and its own cells at its own depth maps: near ties only
    size = torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)
    for n, s in enumerate(scales):
        differ = (own[s] != sels[n]).float().mean().item()
        depth64, cells = ol.upsample_disp_to_depth(d64[s], H, W, 0.1, 2.0), 0
        for f, i in enumerate(ids):
            px = (orp.warp(depth64, cpu[("color", i, 0)], cpu[("K", 0)], cpu[("inv_K", 0)], cpu[("poses", i)])[1] + 1) / 2 * size
            c = coords[n][f].double()
            inside = (px > 0) & (px < size) & (c > 0) & (c < size)
            cells += int(((torch.floor(px) != torch.floor(c)) & inside).any(-1).sum())
        print(f"STEPFIG | {case} | selection scale {s} | device vs fp64 oracle's own: {int((own[s] != sels[n]).sum())} of "
              f"{sels[n].numel()} pixels differ ({differ:.5f}) | kept {(sels[n] != 255).float().mean().item():.3f} | "
              f"sampled in another cell: {cells} of {len(ids) * sels[n].numel()}")
        assert differ <= 0.01 and cells <= 0.01 * len(ids) * sels[n].numel(), (s, differ, cells)

    # ---- disparities, loss entries
    for s in scales:
        assert (dev_disps[s] - d32[s]).abs().max().item() < 2e-5, f"disp {s} vs fp32 oracle"
        assert (dev_disps[s].double() - d64[s]).abs().max().item() < 2e-5, f"disp {s} vs fp64 oracle"
    keys = ["loss"] + [f"{k}/{s}" for s in scales for k in ("loss", "reproj_loss", "supervised_depth_loss")]
    for k in keys:
        err = abs(losses[k].item() - L64[k]) / abs(L64[k])
        print(f"STEPFIG | {case} | {k} | dev {losses[k].item():.8f} | fp64 {L64[k]:.10f} | rel err {err:.2e} | "
              f"fp32 oracle {abs(L32[k] - L64[k]) / abs(L64[k]):.2e}")
    for k in keys:
        assert abs(losses[k].item() - L64[k]) <= 1e-4 * abs(L64[k]), (k, losses[k].item(), L64[k])

    # ---- the forward wiring alone: the oracle term at the device's own depth maps
    for s in scales:
        dev, tol = losses[f"reproj_loss/{s}"].item(), 4.0 * abs(t32[s] - t64[s]) + 1e-6 * abs(t64[s])
        print(f"STEPFIG | {case} | term at the device's depth, scale {s} | err {abs(dev - t64[s]):.2e} | tol {tol:.2e}")
        assert abs(dev - t64[s]) <= tol, (s, dev, t64[s], t32[s])

    # ---- the term's gradient per scale, at the device's disparities as leaves
    for n, s in enumerate(scales):
        e_dev, e_cpu = _rel_l2(gterm[n].detach().cpu(), gd64[s]), _rel_l2(gd32[s], gd64[s])
        print(f"STEPFIG | {case} | term gradient scale {s} (zoom {2 ** s}) | rel L2 {e_dev:.2e} | bound {4 * e_cpu + 1e-6:.2e}")
        assert gd64[s].abs().max().item() > 0 and e_dev <= 4.0 * e_cpu + 1e-6, (s, e_dev, e_cpu)

    # ---- weight gradients of `loss`, per tensor; the power of that check
    rows, bad, strong = [], [], 0
    for k, g in g64.items():
        if _skipped(k):
            continue
        e_hip, e_cpu, e_ctl = _rel_l2(dev_grads[k], g), _rel_l2(g32[k], g), ctl["e_ctl"][k]
        bound = max(1e-4, 2.0 * e_cpu, 2.0 * e_ctl)
        rows.append((k, e_hip, e_cpu, e_ctl))
        if not e_hip <= bound:
            bad.append((k, e_hip, e_cpu, e_ctl))
        strong += _rel_l2(ctl["g64"][k], g) >= 10.0 * bound
    worst = max(rows, key=lambda r: r[1] / max(1e-4, 2 * r[2], 2 * r[3]))
    med = statistics.median(r[1] / r[2] for r in rows if r[2] > 1e-6)
    print(f"STEPFIG | {case} | weight gradients | {len(rows)} tensors | median e_hip / e_cpu32 {med:.2f} | worst against its "
          f"bound {worst[0]}: e_hip {worst[1]:.2e}, e_cpu32 {worst[2]:.2e}, e_ctl {worst[3]:.2e} | largest e_hip / e_cpu32 "
          f"{max(r[1] / r[2] for r in rows if r[2] > 1e-6):.2f} | power {strong} of {len(rows)}")
    for r in sorted(rows, key=lambda r: -r[2])[:3]:
        print(f"STEPFIG | {case} | ill-conditioned | {r[0]} | e_hip {r[1]:.2e} | e_cpu32 {r[2]:.2e} | e_ctl {r[3]:.2e}")
    assert len(rows) > (120 if case == "three_frames" else 150), len(rows)
    assert not bad, bad
    assert strong >= 0.9 * len(rows), (strong, len(rows))

    # ---- the optimizer step
    tr.model_optimizer.step()
    torch.cuda.synchronize()
    assert torch.isfinite(tr.store.flat).all()
    off, n = tr.store.offsets["mono_depth.decoder.0.conv.conv.weight"]
    assert tr.store.grad[off:off + n].abs().max().item() == 0 and tr.store.grad_is_zero
    delta = (tr.store.flat[off:off + n] - before[off:off + n]).cpu()
    g = dev_grads["mono_depth.decoder.0.conv.conv.weight"].permute(0, 2, 3, 1).reshape(-1)       # storage order of the flat buffer
    big = g.abs() > 1e-6
    assert big.any() and torch.allclose(delta[big], -LR * torch.sign(g[big]), atol=2e-6)
