"""The two clouds of the reference's demo (pointcloud/eval_pointcloud.py:256-291) for one test item, without Open3D:
``pred.ply`` (the predicted depth, back-projected at the pixels that have a ground-truth depth) and ``gt.ply`` (the ground
truth), binary little-endian PLY coloured by ("color", 0, 0), y and z negated as the reference's viewer transform does.

    python tools/export_pointcloud.py --data_path /data/HAMMER --weights /runs/x/models/weights_19 --index 0 --out clouds/

``--data_path synthetic`` serves a seeded synthetic item; without ``--weights`` the networks keep their initialisation.
``--consistent M`` writes only the predicted points that at least M of the neighbouring frames -1 and 1 confirm (their
predicted depth maps agree with this one at MVSNet's thresholds under the loader's poses: ``n_cons >= M`` of
``polardepth.consistency_eval.consistency``), at the depth fused over the confirming views instead of the single prediction.
``--normals depth`` adds the properties nx ny nz to ``pred.ply``: the normals of the depth map that is exported
(pd_gt_normals).  ``--normals polar`` writes the polarisation normal instead wherever the measurement gives one: of the three
physical candidates of K1 and their pi flips, the one closest to the depth normal (``pol_normal`` where ``choice != 0`` of
``polardepth.polar_normals_eval.polar_normals_stats``), the depth normal elsewhere.  ``--ray_frame`` makes that choice in the
frame of each pixel's viewing ray; the normal written is still a camera-frame one.  ``--max_uncertainty_mm X`` writes only the
predicted points whose stated uncertainty -- the Laplace scale b of the decoder's uncertainty head, ``Evaluation(uncertainty=True)``
-- is at most X millimetres; it needs weights trained with ``opt.uncertainty_loss`` and combines with ``--consistent``.
``--refine`` exports the predicted depth refined with the polarisation normals it disambiguates
(``polardepth.refine.polar_refine``; ``--refine_lam X --refine_iters N`` replace the conventional 0.02 and 100): the fine relief
of ``--normals polar`` then lies in the points too, and every later option acts on the refined depth.
``--refine_uncertainty [TAU]`` weights the prior per pixel with the uncertainty the decoder states (``polar_refine``'s
``uncertainty=``, TAU = ``unc_ref``, 0.002 without a value; it needs weights trained with ``opt.uncertainty_loss``), and
``--refine_robust C`` adds a second, reweighted round with the Huber threshold C in log depth (``robust=``, ``rounds=2``).
``gt.ply`` is unchanged."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))


def export(data_path, weights, index, out, height=320, width=480, flip=True, consistent=None, normals=None, aolp_sign=None,
           ray_frame=None, max_uncertainty_mm=None, refine=False, refine_lam=None, refine_iters=None, refine_uncertainty=None,
           refine_robust=None):
    import torch
    from torch.utils.data.dataloader import default_collate
    from manydepth.evaluation import Evaluation
    from polardepth import pointcloud as pc
    if normals not in (None, "polar", "depth"):
        raise ValueError(f'--normals takes "polar" or "depth", got {normals!r}')
    if not refine and (refine_lam is not None or refine_iters is not None):
        raise ValueError("--refine_lam and --refine_iters are options of --refine")
    if not refine and (refine_uncertainty is not None or refine_robust is not None):
        raise ValueError("--refine_uncertainty and --refine_robust are options of --refine")
    more = {} if max_uncertainty_mm is None and refine_uncertainty is None else {"uncertainty": True}
    if refine:
        more["polar_refine"] = {k: v for k, v in (("lam", refine_lam), ("iters", refine_iters)) if v is not None}
        if refine_uncertainty is not None:          # True: the conventional unc_ref
            more["polar_refine"]["uncertainty"] = True
            if refine_uncertainty is not True:
                more["polar_refine"]["unc_ref"] = float(refine_uncertainty)
        if refine_robust is not None:
            more["polar_refine"].update(robust=float(refine_robust), rounds=2)
    ev = Evaluation(load_weights_folder=weights, data_path=data_path, height=height, width=width, batch_size=1,
                    aolp_sign=aolp_sign, polar_ray_frame=ray_frame, **more)
    ev.load_mono_model()
    ds = ev.test_loader.dataset
    if not 0 <= index < len(ds):
        raise IndexError(f"--index {index}: the test split holds {len(ds)} items")
    inputs = {k: v.to(ev.device) for k, v in default_collate([ds[index]]).items()}
    colour = inputs[("color", 0, 0)][0].float()                        # [3,H,W] in 0 .. 1, before predict expands the batch
    scale = None
    if max_uncertainty_mm is not None or refine:  # one pass gives the depth, the head's Laplace scale b, the refined depth
        both = ev.predict_all(inputs)
        depth, scale = both["depth_refined" if refine else "depth"], both.get("uncertainty")
    else:
        depth = ev.predict(inputs)
    gt, K = inputs["depth_gt"], inputs[("K", 0)]
    if consistent is not None:
        depth, gt_gate = consistent_depth(ev, index, depth, gt, int(consistent))
    else:
        gt_gate = gt
    if max_uncertainty_mm is not None:            # the head's own statement of where the prediction should not be trusted
        gt_gate = torch.where(scale * 1e3 <= float(max_uncertainty_mm), gt_gate, torch.zeros_like(gt_gate))
    clouds = {"pred": pc.backproject(depth, K, gate=gt_gate, min_depth=ev.min_depth, max_depth=ev.max_depth),
              "gt": pc.backproject(gt, K, min_depth=ev.min_depth, max_depth=ev.max_depth)}
    rgb = (colour.permute(1, 2, 0).reshape(-1, 3) * 255).round().clamp(0, 255).to(torch.uint8).cpu()
    os.makedirs(out, exist_ok=True)
    written = {}
    for name, cloud in clouds.items():
        pix = torch.from_numpy(cloud.slot_pixels())
        cols = rgb[pix.clamp(min=0)]                                   # slots outside the image hold no point: any colour
        path = os.path.join(out, f"{name}.ply")
        nrm = pixel_normals(ev, inputs, depth, normals)[pix.clamp(min=0)] if normals is not None and name == "pred" else None
        written[path] = pc.write_ply(path, cloud.points[0], cols, flip=flip, normals=nrm)
    return written


def pixel_normals(ev, inputs, depth, kind):
    """[H * W, 3] on the host: per pixel the normal of ``depth`` (pd_gt_normals without a range), or with kind "polar" the
    disambiguated polarisation normal where the measurement gives one."""
    import numpy as np
    import torch
    from polardepth import polar as pdpolar
    from polardepth import polar_normals_eval as pe
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, _, H, W = depth.shape
    big = float(np.finfo(np.float32).max)
    depth, K = depth.float().contiguous(), inputs[("K", 0)].float().contiguous()
    dn = torch.empty((N, H, W, 4), dtype=torch.float32, device=depth.device)
    check(lib.pd_gt_normals(ptr(depth), ptr(K), ptr(dn), N, H, W, -big, big, stream_ptr()), "pd_gt_normals")
    out = dn[0, ..., :3]
    if kind == "polar":
        pol = pdpolar.polar_inputs(inputs, (ev.height, ev.width), ("xolp", "normals"), ev.pol_angles, dofp=ev.pol_dofp,
                                   cdofp=ev.pol_cdofp, calibration=ev.pol_calibration)
        st = pe.polar_normals_stats(dn.permute(0, 3, 1, 2)[:, :3], pol, inputs["xolp", 0, 0], K=K, classes=(("all", None),),
                                    aolp_sign=ev.aolp_sign, maps=True, ray_frame=ev.polar_ray_frame)
        out = torch.where((st.choice[0] != 0)[..., None], st.pol_normal[0, ..., :3], out)
    return out.reshape(H * W, 3).cpu()


def consistent_depth(ev, index, depth, gt, M, ids=(-1, 1)):
    """(the fused depth [1,1,H,W], the ground-truth gate with the pixels of n_cons < M emptied) for test item ``index``."""
    import torch
    from torch.utils.data.dataloader import default_collate
    from manydepth import datasets
    from polardepth import consistency_eval as ce
    if not 1 <= M <= len(ids):
        raise ValueError(f"--consistent {M}: there are {len(ids)} neighbouring frames")
    data_path, files, _ = ev._loader_args
    ds = datasets.HAMMER_Dataset(data_path, files, ev.height, ev.width, [0] + list(ids), 4, is_train=False,
                                 supervised_depth_only=False, need_poses=True, neighbour_items=True)
    to_dev = lambda d: {k: to_dev(v) if isinstance(v, dict) else v.to(ev.device) for k, v in d.items()}
    item = to_dev(default_collate([ds[index]]))
    depths = torch.cat([ev.predict(item[("neighbour", i)]) for i in ids], 1)
    st = ce.consistency(depth, depths, torch.stack([item[("poses", i)] for i in ids], 1), item[("K", 0)], item[("inv_K", 0)],
                        frame_valid=torch.stack([item[("frame_valid", i)] for i in ids], 1), classes=(("all", None),),
                        min_depth=ev.min_depth, max_depth=ev.max_depth, fuse_level=4, want=("n_cons", "fused"))
    keep = (st.n_cons >= M)[:, None]
    return st.fused[:, None], torch.where(keep, gt, torch.zeros_like(gt))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_path", required=True)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--index", type=int, default=0)
    ap.add_argument("--out", required=True)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--no_flip", action="store_true", help="keep the camera frame (y down, z forward)")
    ap.add_argument("--consistent", type=int, default=None, metavar="M",
                    help="keep the predicted points that M neighbouring frames confirm, at the fused depth")
    ap.add_argument("--normals", choices=("polar", "depth"), default=None,
                    help="add nx ny nz to pred.ply: the depth map's normals, or the polarisation normal where there is one")
    ap.add_argument("--aolp_sign", type=int, choices=(1, -1), default=None, help="the AoLP handedness for --normals polar")
    ap.add_argument("--ray_frame", action="store_true", default=None,
                    help="--normals polar: choose the candidate in the frame of each pixel's viewing ray")
    ap.add_argument("--max_uncertainty_mm", type=float, default=None, metavar="X",
                    help="keep the predicted points whose stated uncertainty (Laplace scale b) is at most X mm")
    ap.add_argument("--refine", action="store_true", help="export the depth refined with the polarisation normals")
    ap.add_argument("--refine_lam", type=float, default=None, metavar="X", help="--refine: the weight of the prior (0.02)")
    ap.add_argument("--refine_iters", type=int, default=None, metavar="N", help="--refine: Chebyshev steps (100)")
    ap.add_argument("--refine_uncertainty", nargs="?", type=float, const=True, default=None, metavar="TAU",
                    help="--refine: weight the prior per pixel with the decoder's stated uncertainty (unc_ref = TAU, 0.002)")
    ap.add_argument("--refine_robust", type=float, default=None, metavar="C",
                    help="--refine: a second, reweighted round with the Huber threshold C in log depth")
    args = ap.parse_args()
    for path, n in export(args.data_path, args.weights, args.index, args.out, args.height, args.width, not args.no_flip,
                          args.consistent, args.normals, args.aolp_sign, args.ray_frame, args.max_uncertainty_mm, args.refine,
                          args.refine_lam, args.refine_iters, args.refine_uncertainty, args.refine_robust).items():
        print(f"{path}: {n} points")
