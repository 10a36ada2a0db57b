"""The two clouds of the reference's demo (pointcloud/eval_pointcloud.py:256-291) for one test item, without Open3D:
``pred.ply`` (the predicted depth, back-projected at the pixels that have a ground-truth depth) and ``gt.ply`` (the ground
truth), binary little-endian PLY coloured by ("color", 0, 0), y and z negated as the reference's viewer transform does.

    python tools/export_pointcloud.py --data_path /data/HAMMER --weights /runs/x/models/weights_19 --index 0 --out clouds/

``--data_path synthetic`` serves a seeded synthetic item; without ``--weights`` the networks keep their initialisation."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))


def export(data_path, weights, index, out, height=320, width=480, flip=True):
    import torch
    from torch.utils.data.dataloader import default_collate
    from manydepth.evaluation import Evaluation
    from polardepth import pointcloud as pc
    ev = Evaluation(load_weights_folder=weights, data_path=data_path, height=height, width=width, batch_size=1)
    ev.load_mono_model()
    ds = ev.test_loader.dataset
    if not 0 <= index < len(ds):
        raise IndexError(f"--index {index}: the test split holds {len(ds)} items")
    inputs = {k: v.to(ev.device) for k, v in default_collate([ds[index]]).items()}
    colour = inputs[("color", 0, 0)][0].float()                        # [3,H,W] in 0 .. 1, before predict expands the batch
    depth = ev.predict(inputs)
    gt, K = inputs["depth_gt"], inputs[("K", 0)]
    clouds = {"pred": pc.backproject(depth, K, gate=gt, min_depth=ev.min_depth, max_depth=ev.max_depth),
              "gt": pc.backproject(gt, K, min_depth=ev.min_depth, max_depth=ev.max_depth)}
    rgb = (colour.permute(1, 2, 0).reshape(-1, 3) * 255).round().clamp(0, 255).to(torch.uint8).cpu()
    os.makedirs(out, exist_ok=True)
    written = {}
    for name, cloud in clouds.items():
        pix = torch.from_numpy(cloud.slot_pixels())
        cols = rgb[pix.clamp(min=0)]                                   # slots outside the image hold no point: any colour
        path = os.path.join(out, f"{name}.ply")
        written[path] = pc.write_ply(path, cloud.points[0], cols, flip=flip)
    return written


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_path", required=True)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--index", type=int, default=0)
    ap.add_argument("--out", required=True)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--no_flip", action="store_true", help="keep the camera frame (y down, z forward)")
    args = ap.parse_args()
    for path, n in export(args.data_path, args.weights, args.index, args.out, args.height, args.width, not args.no_flip).items():
        print(f"{path}: {n} points")
