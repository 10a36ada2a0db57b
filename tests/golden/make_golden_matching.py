#!/usr/bin/env python3
"""Generate tests/golden/g13_matching.npz by RUNNING THE REFERENCE's own multi-frame matching on the CPU, once in float32 and
once in float64:

    manydepth/layers.py                    BackprojectDepth, Project3D                               (imported)
    manydepth/networks/resnet_encoder.py   ResnetEncoderMatching.compute_depth_bins, match_features, compute_confidence_mask,
                                           indices_to_disparity -- the four method bodies are compiled from the checkout's
                                           file at run time (the module itself needs torchvision to import) and bound to a stub
                                           that carries the attributes they read; the argmin over (0 -> 100) of :623-627 is
                                           restated here line by line

Like make_golden_reproj.py it runs only where the reference checkout is available ($PD_REFERENCE); the output is data only:

    PD_REFERENCE=<reference checkout> python tests/golden/make_golden_matching.py

Inputs: B = 2, F = 2, C = 64, 24 x 40 features, D = 16 bins over 0.3 .. 2 m, linear and inverse; a K per item as in g12; smooth
non-negative features (multiples of 1/256) whose lookup frames are the current frame's pattern shifted by the parallax of a
plane at 0.8 m, so the cost has a minimum; frame 0 of item 0 a small motion, the other two motions large enough that interior
pixels lose bins; item 1's second pose is all zeros (the reference's "missing frame").

Key layout: "cur" [2,64,24,40], "lookup" [2,2,64,24,40], "K" / "inv_K" [2,4,4], "poses" [2,2,4,4], float32.  Per binning
G in ("linear", "inverse"): "bins_G" [16] float32 (compute_depth_bins' tensor), "cost_G" [2,16,24,40] float64, "missing_G"
uint8, "confidence_G" [2,24,40] uint8, "argmin_G" int32, "lowest_G" float64 -- the float64 run -- and "tie_G" [2,24,40] bool
(the two smallest costs of the float64 run differ by less than 1e-5).  "near" [2,24,40] bool: some (bin, frame) coordinate of
the pixel, under either binning, lies within 1e-3 px of a threshold of the edge mask (2, w-2, h-2).  Recorded figures:
"dev_cost_max" / "dev_cost_mean" (|float32 run - float64 run| of the cost outside the near / tie pixels, both binnings),
"share_near", "share_tie_G" (of the interior), "share_confident_G" (of the interior), "share_frames_G" [3] (interior entries to
which 0 / 1 / 2 frames contributed).
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("PD_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
B, NF, C, H, W, D = 2, 2, 64, 24, 40, 16
MIN_BIN, MAX_BIN = 0.3, 2.0
PLANE = 0.8
SEED = 13
WANT = ("compute_depth_bins", "match_features", "compute_confidence_mask", "indices_to_disparity")


def reference_methods():
    tree = ast.parse(open(os.path.join(REF, "manydepth", "networks", "resnet_encoder.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ResnetEncoderMatching")
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert {f.name for f in fns} == set(WANT)
    ns = {"torch": torch, "np": np, "F": F}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "resnet_encoder.py", "exec"), ns)
    return {k: ns[k] for k in WANT}


def pose(rot, t):
    rx, ry, rz = rot
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = t
    return T


def pattern(n, sx, sy):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    xx, yy = xx - sx, yy - sy
    c = np.arange(C, dtype=np.float64)[:, None, None]
    v = 0.9 + 0.45 * np.sin(xx / (2.0 + 0.05 * c) + 0.37 * c + n) * np.cos(yy / (3.1 - 0.02 * c) + 0.11 * c) \
        + 0.3 * np.sin((xx + 2 * yy) / (5.0 + 0.1 * c) + 0.2 * c)
    return np.round(np.clip(v, 0.0, None) * 256) / 256


def inputs(seed):
    rng = np.random.default_rng(seed)
    K = np.tile(np.eye(4), (B, 1, 1))
    for n in range(B):
        K[n, 0, 0], K[n, 1, 1] = (0.62 + 0.05 * n) * W, (1.05 - 0.07 * n) * H
        K[n, 0, 2], K[n, 1, 2] = W / 2 - 0.4 + 0.9 * n, H / 2 + 0.3 - 0.5 * n
    # frame 0 of item 0: a small forward motion (every pixel keeps every bin); frame 1 of item 0: a large sideways motion;
    # frame 0 of item 1: sideways and forward, with a rotation that cancels the parallax of the farthest bin -- interior
    # pixels lose their near bins and keep the far ones, so entries without any frame arise without emptying whole pixels
    trans = [[np.array([0.03, -0.01, 0.08]), np.array([-0.45, 0.12, -0.05])],
             [np.array([0.70, 0.02, 0.10]), np.array([0.09, 0.02, 0.02])]]
    rots = [[np.zeros(3), np.zeros(3)], [np.array([0.0, -0.70 / (MAX_BIN + 0.10), 0.0]), np.zeros(3)]]
    poses = np.stack([np.stack([pose(rots[n][f] + rng.uniform(-0.01, 0.01, 3), trans[n][f] + rng.uniform(-0.005, 0.005, 3))
                                for f in range(NF)]) for n in range(B)])

    def shift(n, f):                       # where the point on the optical axis at PLANE moves, in pixels
        q = poses[n, f, :3, :3] @ np.array([0.0, 0.0, PLANE]) + poses[n, f, :3, 3]
        return K[n, 0, 0] * q[0] / q[2], K[n, 1, 1] * q[1] / q[2]
    cur = np.stack([pattern(n, 0, 0) for n in range(B)])
    lookup = np.stack([np.stack([pattern(n, *shift(n, f))
                                 for f in range(NF)]) for n in range(B)])
    poses[1, 1] = 0.0                                                         # the missing frame
    d = {"cur": cur, "lookup": lookup, "K": K, "poses": poses}
    d["inv_K"] = np.linalg.pinv(K.astype(np.float32)).astype(np.float64)      # the loader's: pinv of the float32 matrix
    return {k: v.astype(np.float32) for k, v in d.items()}


def run(inp, dtype, binning, layers, m):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    stub = types.SimpleNamespace(num_depth_bins=D, matching_height=H, matching_width=W, depth_binning=binning, is_cuda=False,
                                 set_missing_to_max=True, depth_bins=None, warp_depths=None,
                                 backprojector=layers.BackprojectDepth(D, H, W).to(dtype), projector=layers.Project3D(D, H, W))
    m["compute_depth_bins"](stub, MIN_BIN, MAX_BIN)
    out = {"bins": stub.depth_bins.numpy().copy()}
    stub.warp_depths = stub.warp_depths.to(dtype)
    with torch.no_grad():
        cost_volume, missing_mask = m["match_features"](stub, t["cur"], t["lookup"], t["poses"], t["K"], t["inv_K"])
        confidence_mask = m["compute_confidence_mask"](stub, cost_volume.detach() * (1 - missing_mask.detach()))
        # resnet_encoder.py:623-627
        viz_cost_vol = cost_volume.clone().detach()
        viz_cost_vol[viz_cost_vol == 0] = 100
        mins, argmin = torch.min(viz_cost_vol, 1)
        lowest_cost = m["indices_to_disparity"](stub, argmin)
        # the coordinates match_features compares with its thresholds (:455, :467, :475-477), and its masks (:479-486)
        near = torch.zeros(B, H, W, dtype=torch.bool)
        frames = torch.zeros(B, D, H, W, dtype=torch.long)
        for b in range(B):
            world_points = stub.backprojector(stub.warp_depths, t["inv_K"][b:b + 1])
            for f in range(NF):
                if t["poses"][b, f].sum() == 0:
                    continue
                pix_locs = stub.projector(world_points, t["K"][b:b + 1], t["poses"][b:b + 1, f])
                x_vals = (pix_locs[..., 0] / 2 + 0.5) * (W - 1)
                y_vals = (pix_locs[..., 1] / 2 + 0.5) * (H - 1)
                for vals, hi in ((x_vals, W - 2), (y_vals, H - 2)):
                    near[b] |= (((vals - 2.0).abs() < 1e-3) | ((vals - hi).abs() < 1e-3)).any(0)
                edge = (x_vals >= 2.0) & (x_vals <= W - 2) & (y_vals >= 2.0) & (y_vals <= H - 2)
                frames[b] += edge.long()
    two = torch.topk(viz_cost_vol, min(2, D), dim=1, largest=False)[0]
    out.update({"cost": cost_volume.numpy(), "missing": missing_mask.numpy().astype(np.uint8),
                "confidence": confidence_mask.numpy().astype(np.uint8), "argmin": argmin.numpy().astype(np.int32),
                "lowest": lowest_cost.numpy(), "near": near.numpy(), "frames": frames.numpy(),
                "tie": ((two[:, 1] - two[:, 0]).abs() < 1e-5).numpy()})
    return out


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set PD_REFERENCE to the reference checkout")
    sys.path.insert(0, os.path.join(REF, "manydepth"))
    import layers
    m = reference_methods()
    inp = inputs(SEED)
    data = dict(inp)
    runs = {(g, tag): run(inp, dt, g, layers, m) for g in ("linear", "inverse")
            for tag, dt in (("f32", torch.float32), ("f64", torch.float64))}
    near = runs[("linear", "f64")]["near"] | runs[("inverse", "f64")]["near"]
    inner = np.zeros((B, H, W), bool)
    inner[:, 2:-2, 2:-2] = True
    data["near"] = near
    fig = {"share_near": near[inner].mean()}
    dev = []
    for g in ("linear", "inverse"):
        r32, r64 = runs[(g, "f32")], runs[(g, "f64")]
        assert np.array_equal(r32["bins"], r64["bins"]) and r64["bins"].dtype == np.float32
        data[f"bins_{g}"] = r64["bins"]
        for k in ("cost", "missing", "confidence", "argmin", "lowest", "tie"):
            data[f"{k}_{g}"] = r64[k]
        keep = inner & ~near & ~r64["tie"]
        dev.append(np.abs(r32["cost"].astype(np.float64) - r64["cost"])[np.broadcast_to(keep[:, None], r64["cost"].shape)])
        fr = r64["frames"][np.broadcast_to(inner[:, None], r64["frames"].shape)]
        fig[f"share_tie_{g}"] = r64["tie"][inner].mean()
        fig[f"share_confident_{g}"] = r64["confidence"][inner].mean()
        fig[f"share_frames_{g}"] = np.array([(fr == k).mean() for k in range(3)])
        # the conditions the tests rely on, met by the float64 run alone
        assert fig[f"share_tie_{g}"] <= 0.02, fig
        assert 0.2 < fig[f"share_confident_{g}"] < 0.9, fig
        assert (fig[f"share_frames_{g}"] >= 0.1).all(), fig
    assert fig["share_near"] <= 0.05, fig
    dev = np.concatenate(dev)
    fig["dev_cost_max"], fig["dev_cost_mean"] = dev.max(), dev.mean()
    data.update({k: np.asarray(v, np.float64) for k, v in fig.items()})
    path = os.path.join(OUT, "g13_matching.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    for k, v in fig.items():
        print(k, v)


if __name__ == "__main__":
    main()
