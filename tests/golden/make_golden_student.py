#!/usr/bin/env python3
"""Generate tests/golden/g14_student.npz by RUNNING THE REFERENCE's own pieces of the --train_student branch on the CPU in
float32:

    manydepth/trainer.py                  Trainer.compute_matching_mask, Trainer.compute_losses (is_multi=True, with
                                          depth_supervision off: the reprojection and consistency terms and their masks),
                                          Trainer.compute_reprojection_loss, Trainer.compute_loss_masks,
                                          Trainer.update_adaptive_depth_bins
    manydepth/networks/resnet_encoder.py  ResnetEncoderMatching.compute_depth_bins
    manydepth/layers.py                   SSIM, get_smooth_loss                                   (imported)
    torch                                 F.interpolate(mode="nearest") of the lowest-cost / confidence maps, trainer.py:617-627

The method bodies are compiled from the checkout's source files at run time (the modules themselves need tensorboard, kornia
and roma to import).  Like make_golden_reproj.py it runs only where the reference checkout is available ($PD_REFERENCE); the
output is data only.  Re-run with:

    PD_REFERENCE=<reference checkout> python tests/golden/make_golden_student.py

The generator asserts that tests/student_ref.py gives the reference's masks exactly, and stores the observed relative
difference between the reference's float32 losses and student_ref's fp64 sums.

Inputs: N = 3, quarter resolution 3 x 5, full resolution 12 x 20, two warped frames; item 1 is augmented.  Key layout:
"lowest" / "confidence" [3,3,5], "mono_depth" / "multi_depth" [3,1,12,20], "target" / "warped0" / "warped1" [3,3,12,20], "aug"
[3], all float32.  Reference results: "lowest_up" / "conf_up" [3,12,20] (F.interpolate), "matching_mask" [3,12,20] bool,
"consistency_mask" [3,12,20], "reproj0" / "reproj1" [3,1,12,20] (compute_reprojection_loss), and per case C in ("mm", "nomm",
"avg"): "rmask_C" [3,1,12,20] (trainer.py:1203-1211 restated), "reproj_loss_C", "consistency_loss_C" (compute_losses).
Recorded figures: "dev_reproj_C" / "dev_consistency_C" = |reference fp32 - student_ref| / |student_ref|.
Tracker: "tracker_depths" [3,2,1,8,12] (three successive teacher depth batches), "tracker_floor", "tracker_init" [2], "tracker"
[3,2] (min, max after each update, the reference's Python floats), "bins_linear" / "bins_inverse" [3,96] and "bins2_linear" /
"bins2_inverse" [3,2] (compute_depth_bins after each update)."""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("PD_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
N, h, w = 3, 3, 5
H, W = 4 * h, 4 * w
SEED = 14


def methods_of(path, cls_name, want, ns):
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want]
    for f in fns:
        f.decorator_list = []                     # @staticmethod: the functions are called unbound below
    assert {f.name for f in fns} == set(want), ({f.name for f in fns}, want)
    exec(compile(ast.Module(body=fns, type_ignores=[]), os.path.basename(path), "exec"), ns)
    return [ns[k] for k in want]


def inputs(seed):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    d = {}
    depth_q = rng.uniform(0.4, 3.0, (N, h, w)).astype(f32)
    d["lowest"] = (f32(1) / depth_q).astype(f32)
    d["confidence"] = (rng.random((N, h, w)) > 0.25).astype(f32)
    md = (f32(1) / d["lowest"].repeat(4, 1).repeat(4, 2)).astype(f32)
    cls = rng.random((N, H, W))
    factor = np.where(cls < 0.55, rng.uniform(0.7, 1.4, (N, H, W)),
                      np.where(cls < 0.775, rng.uniform(0.2, 0.45, (N, H, W)), rng.uniform(2.2, 3.0, (N, H, W)))).astype(f32)
    mono = (md * factor).astype(f32)
    mono[0, 1, 2] = md[0, 1, 2] * f32(0.5)      # the ratios that are exactly 1
    mono[0, 2, 1] = md[0, 2, 1] * f32(2.0)
    d["mono_depth"] = mono[:, None]
    d["multi_depth"] = (d["mono_depth"] * rng.uniform(0.8, 1.2, d["mono_depth"].shape)).astype(f32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = lambda sx, sy, n: np.stack([0.5 + 0.25 * np.sin((xx + sx) / (2.1 + c) + 0.7 * c + n) * np.cos((yy + sy) / (2.9 - 0.4 * c))
                                      + 0.2 * np.sin((xx + 2 * yy) / (5.0 + c)) for c in range(3)])
    d["target"] = np.stack([img(0, 0, n) for n in range(N)]).astype(f32)
    d["warped0"] = np.stack([img(0.6, -0.3, n) for n in range(N)]).astype(f32)
    d["warped1"] = np.stack([img(-0.5, 0.4, n) for n in range(N)]).astype(f32)
    d["aug"] = np.array([0, 1, 0], f32)
    return d


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set PD_REFERENCE to the reference checkout")
    sys.path.insert(0, os.path.join(REF, "manydepth"))
    import layers
    import student_ref as S
    ns = {"torch": torch, "get_smooth_loss": layers.get_smooth_loss, "np": np}
    (compute_matching_mask, compute_losses, compute_reprojection_loss, compute_loss_masks, update_adaptive_depth_bins) = methods_of(
        os.path.join(REF, "manydepth", "trainer.py"), "Trainer",
        ["compute_matching_mask", "compute_losses", "compute_reprojection_loss", "compute_loss_masks",
         "update_adaptive_depth_bins"], ns)
    (compute_depth_bins,) = methods_of(os.path.join(REF, "manydepth", "networks", "resnet_encoder.py"), "ResnetEncoderMatching",
                                       ["compute_depth_bins"], {"torch": torch, "np": np})
    inp = inputs(SEED)
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    data = dict(inp)

    def opt(**kw):
        base = dict(scales=[0], v1_multiscale=False, train_dpt=False, depth_supervision_only=False, frame_ids=[0, -1, 1],
                    res_pose=False, disable_automasking=True, avg_reprojection=False, disable_motion_masking=False,
                    no_matching_augmentation=False, post_process_mono_while_training=False, depth_supervision=False,
                    disparity_smoothness=0.0, supervise_pose=False, no_ssim=False, min_depth=0.1, max_depth=10.0)
        base.update(kw)
        return types.SimpleNamespace(**base)

    def stub(o):
        s = types.SimpleNamespace(opt=o, device=torch.device("cpu"), num_scales=1, ssim=layers.SSIM())
        s.compute_reprojection_loss = lambda pred, target: compute_reprojection_loss(s, pred, target)
        s.compute_loss_masks = compute_loss_masks
        return s

    # trainer.py:617-627
    outputs = {("mono_depth", 0, 0): t["mono_depth"], ("depth", 0, 0): t["multi_depth"], ("disp", 0): 1 / t["multi_depth"],
               ("color", -1, 0): t["warped0"], ("color", 1, 0): t["warped1"],
               "augmentation_mask": t["aug"].view(N, 1, 1, 1)}
    outputs["lowest_cost"] = F.interpolate(t["lowest"].unsqueeze(1), [H, W], mode="nearest")[:, 0]
    conf_up = F.interpolate(t["confidence"].unsqueeze(1), [H, W], mode="nearest")[:, 0]
    matching_mask = compute_matching_mask(stub(opt()), outputs)
    data["lowest_up"], data["conf_up"] = outputs["lowest_cost"].numpy(), conf_up.numpy()
    data["matching_mask"] = matching_mask.numpy()
    data["consistency_mask"] = (conf_up * matching_mask).numpy()
    ins = {("color", 0, 0): t["target"]}
    st = stub(opt())
    data["reproj0"] = compute_reprojection_loss(st, t["warped0"], t["target"]).numpy()
    data["reproj1"] = compute_reprojection_loss(st, t["warped1"], t["target"]).numpy()

    for case, kw in (("mm", {}), ("nomm", {"disable_motion_masking": True}), ("avg", {"avg_reprojection": True})):
        o = opt(**kw)
        outs = dict(outputs)
        outs["consistency_mask"] = conf_up if o.disable_motion_masking else conf_up * matching_mask      # :622-627
        losses = compute_losses(stub(o), ins, outs, is_multi=True)
        # trainer.py:1203-1211, line by line
        reprojection_loss_mask = torch.ones(N, 1, H, W)
        if not o.disable_motion_masking:
            reprojection_loss_mask = reprojection_loss_mask * outs["consistency_mask"].unsqueeze(1)
        if not o.no_matching_augmentation:
            reprojection_loss_mask = reprojection_loss_mask * (1 - outs["augmentation_mask"])
        data[f"rmask_{case}"] = reprojection_loss_mask.numpy()
        data[f"reproj_loss_{case}"] = np.float32(losses["reproj_loss/0"].item())
        data[f"consistency_loss_{case}"] = np.float32(losses["consistency_loss/0"].item())

        # student_ref: the masks exactly, the losses to the recorded difference
        m = S.masks(inp["lowest"], inp["confidence"], inp["mono_depth"], inp["aug"], not o.disable_motion_masking)
        assert np.array_equal(m["lowest_up"], data["lowest_up"]) and np.array_equal(m["conf"], data["conf_up"] != 0)
        assert np.array_equal(m["mm"], data["matching_mask"])
        assert np.array_equal(m["cmask"], outs["consistency_mask"].numpy()), case
        assert np.array_equal(m["rmask"], data[f"rmask_{case}"][:, 0].astype(np.uint8)), case
        c = S.combine([data["reproj0"], data["reproj1"]], m["rmask"], inp["multi_depth"], inp["mono_depth"],
                      avg=o.avg_reprojection)
        want = (c["sums"][0] / (c["sums"][1] + 1e-7), c["sums"][2] / (N * H * W))
        data[f"dev_reproj_{case}"] = abs(float(data[f"reproj_loss_{case}"]) - want[0]) / abs(want[0])
        data[f"dev_consistency_{case}"] = abs(float(data[f"consistency_loss_{case}"]) - want[1]) / abs(want[1])
        print(case, "rmask share", m["rmask"].mean(), "reproj", data[f"reproj_loss_{case}"], want[0], "consistency",
              data[f"consistency_loss_{case}"], want[1], "dev", data[f"dev_reproj_{case}"], data[f"dev_consistency_{case}"])
        assert 0.05 < m["rmask"].mean() < 0.95

    # the tracker: three updates, the bins after each
    rng = np.random.default_rng(SEED + 1)
    depths = rng.uniform(0.05, 6.0, (3, 2, 1, 8, 12)).astype(np.float32)
    depths[1] *= 0.02                                  # minima below the floor
    tr = stub(opt())
    tr.min_depth_tracker, tr.max_depth_tracker = tr.opt.min_depth, tr.opt.max_depth
    data["tracker_depths"], data["tracker_floor"] = depths, np.float64(tr.opt.min_depth)
    data["tracker_init"] = np.array([tr.min_depth_tracker, tr.max_depth_tracker], np.float64)
    track, bins = [], {"bins_linear": [], "bins_inverse": [], "bins2_linear": [], "bins2_inverse": []}
    for k in range(3):
        update_adaptive_depth_bins(tr, {("mono_depth", 0, 0): torch.from_numpy(depths[k])})
        track.append([tr.min_depth_tracker, tr.max_depth_tracker])
        for binning in ("linear", "inverse"):
            for D, key in ((96, "bins_"), (2, "bins2_")):
                enc = types.SimpleNamespace(depth_binning=binning, num_depth_bins=D, matching_height=2, matching_width=2,
                                            is_cuda=False)
                compute_depth_bins(enc, tr.min_depth_tracker, tr.max_depth_tracker)
                bins[key + binning].append(enc.depth_bins.numpy())
    data["tracker"] = np.array(track, np.float64)
    data.update({k: np.stack(v).astype(np.float32) for k, v in bins.items()})
    path = os.path.join(OUT, "g14_student.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    print("tracker", data["tracker"])


if __name__ == "__main__":
    main()
