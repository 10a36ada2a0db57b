#!/usr/bin/env python3
"""Generate tests/golden/g12_reproj.npz by RUNNING THE REFERENCE's own view-synthesis and photometric-loss pieces on the CPU,
once in float32 and once in float64:

    manydepth/layers.py   BackprojectDepth, Project3D, SSIM              (imported)
    torch                 F.grid_sample(..., padding_mode="border", align_corners=True)   (trainer.py:1041-1044)
    manydepth/trainer.py  Trainer.compute_reprojection_loss, Trainer.compute_loss_masks   (the two method bodies are
                          compiled from the checkout's trainer.py at run time -- the module itself needs tensorboard,
                          kornia and roma to import) and the minimum / identity + noise / masked mean of :1163-1215,
                          restated here line by line

and autograd for d loss / d depth and for d sum(gw * warped_f) / d depth.  Like make_golden_depth.py it runs only where the
reference checkout is available ($PD_REFERENCE); the output is data only.  Re-run with:

    PD_REFERENCE=<reference checkout> python tests/golden/make_golden_reproj.py

Inputs: N = 2, C = 3, 19 x 37 (both odd), a K per item, two source frames, pose 0 small, pose 1 a forward motion that sends
at least a fifth of the pixels past each of the four borders, smooth images, a stored 1e-5 * randn noise map.

Key layout: inputs "depth" [2,1,19,37], "target" / "src0" / "src1" [2,3,19,37], "K" / "inv_K" / "T0" / "T1" [2,4,4], "noise"
[2,1,19,37], "gw0" / "gw1" [2,3,19,37] (cotangents of the warped images), all float32.  Per run R in ("f32", "f64"):
"coords{f}_R" [2,19,37,2] source PIXEL coordinates (the grid handed to grid_sample, un-normalised with ((g + 1) / 2) * (size
- 1)), "warped{f}_R", "reproj{f}_R" / "ident{f}_R" [2,1,19,37], "mask_R" (compute_loss_masks), "argmin_R" (the frame of the
minimum), "loss_R", "gloss_depth_R" (d loss / d depth), "gdepth{f}_R" (d sum(gw_f * warped_f) / d depth).  Recorded figures:
"dev_warped_max" / "dev_warped_mean" / "dev_loss" / "dev_gdepth_rel" (|f32 - f64|; the gradient relative to max|g| of the
fp64 run, outside the near-boundary pixels), "share_near_boundary" (coordinates within 1e-3 px of a cell boundary or border),
"share_near_tie" (|reprojection - (identity + noise)| < 1e-5), "past_borders" (share of pixels pose 1 sends past the left,
right, top, bottom border).
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
sys.path.insert(0, os.path.dirname(OUT))
N, C, H, W = 2, 3, 19, 37
SEED = 12


def reference_methods():
    """compute_reprojection_loss / compute_loss_masks of the reference's Trainer, compiled from its source file."""
    tree = ast.parse(open(os.path.join(REF, "manydepth", "trainer.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Trainer")
    want = {"compute_reprojection_loss", "compute_loss_masks"}
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert {f.name for f in fns} == want
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "trainer.py", "exec"), ns)
    return ns["compute_reprojection_loss"], ns["compute_loss_masks"]


def smooth_image(rng, shift):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    xx, yy = xx + shift[0], yy + shift[1]
    img = np.stack([0.5 + 0.25 * np.sin(xx / (2.1 + c) + 0.7 * c + rng.uniform(0, 0.3)) * np.cos(yy / (2.9 - 0.4 * c))
                    + 0.2 * np.sin((xx + 2 * yy) / (5.0 + c)) for c in range(C)])
    return img


def inputs(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = {}
    d["depth"] = np.stack([0.9 + 0.25 * np.sin(xx / 9.0 + n) * np.cos(yy / 6.0) + 0.1 * xx / W for n in range(N)])[:, None]
    base = np.random.default_rng(seed + 1)
    d["target"] = np.stack([smooth_image(np.random.default_rng(seed + 10 + n), (0, 0)) for n in range(N)])
    d["src0"] = np.stack([smooth_image(np.random.default_rng(seed + 10 + n), (1.3, -0.6)) for n in range(N)]) \
        + 0.02 * base.standard_normal((N, C, 1, 1))
    d["src1"] = np.stack([smooth_image(np.random.default_rng(seed + 10 + n), (-2.2, 0.9)) for n in range(N)]) \
        + 0.02 * base.standard_normal((N, C, 1, 1))
    K = np.tile(np.eye(4), (N, 1, 1))
    for n in range(N):
        K[n, 0, 0], K[n, 1, 1] = (0.62 + 0.05 * n) * W, (1.05 - 0.07 * n) * H
        K[n, 0, 2], K[n, 1, 2] = W / 2 - 0.4 + 0.9 * n, H / 2 + 0.3 - 0.5 * n
    d["K"] = K
    d["inv_K"] = np.linalg.pinv(K.astype(np.float32)).astype(np.float64)      # the loader's: pinv of the float32 matrix

    def pose(rot, t):
        rx, ry, rz = rot
        Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
        Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
        Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
        T = np.eye(4)
        T[:3, :3] = Rx @ Ry @ Rz
        T[:3, 3] = t
        return T
    d["T0"] = np.stack([pose(rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.04, 0.04, 3)) for _ in range(N)])
    d["T1"] = np.stack([pose(rng.uniform(-0.01, 0.01, 3), np.array([0.01, -0.01, -0.5]) + rng.uniform(-0.01, 0.01, 3))
                        for _ in range(N)])
    d["noise"] = 1e-5 * rng.standard_normal((N, 1, H, W))
    d["gw0"] = rng.standard_normal((N, C, H, W))
    d["gw1"] = rng.standard_normal((N, C, H, W))
    return {k: v.astype(np.float32) for k, v in d.items()}


def run(inp, dtype, layers, methods):
    compute_reprojection_loss, compute_loss_masks = methods
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    depth = t["depth"].clone().requires_grad_(True)
    backproject, project = layers.BackprojectDepth(N, H, W).to(dtype), layers.Project3D(N, H, W)
    stub = types.SimpleNamespace(opt=types.SimpleNamespace(no_ssim=False), ssim=layers.SSIM().to(dtype))
    out, reproj, ident = {}, [], []
    for f in range(2):
        cam = backproject(depth, t["inv_K"])
        pix = project(cam, t["K"], t[f"T{f}"])
        warped = F.grid_sample(t[f"src{f}"], pix, padding_mode="border", align_corners=True)
        size = torch.tensor([W - 1, H - 1], dtype=dtype)
        out[f"coords{f}"] = ((pix.detach() + 1) / 2) * size
        out[f"warped{f}"] = warped.detach()
        out[f"gdepth{f}"] = torch.autograd.grad((t[f"gw{f}"] * warped).sum(), depth, retain_graph=True)[0]
        reproj.append(compute_reprojection_loss(stub, warped, t["target"]))
        ident.append(compute_reprojection_loss(stub, t[f"src{f}"], t["target"]))
        out[f"reproj{f}"], out[f"ident{f}"] = reproj[-1].detach(), ident[-1].detach()
    # trainer.py:1163-1215 with automasking, without avg_reprojection, with the stored noise in place of the randn draw
    reprojection_losses = torch.cat(reproj, 1)
    identity_reprojection_losses = torch.cat(ident, 1)
    identity_reprojection_loss, _ = torch.min(identity_reprojection_losses, dim=1, keepdim=True)
    reprojection_loss, argmin = torch.min(reprojection_losses, dim=1, keepdim=True)
    identity_reprojection_loss = identity_reprojection_loss + t["noise"]
    # (compute_loss_masks returns .float(): in the float64 run the count would be summed, and the 1e-7 absorbed, in float32)
    mask = compute_loss_masks(reprojection_loss, identity_reprojection_loss).to(dtype)
    out["near_tie"] = ((reprojection_loss - identity_reprojection_loss).abs() < 1e-5).detach()
    loss = (reprojection_loss * mask).sum() / (mask.sum() + 1e-7)
    out["gloss_depth"] = torch.autograd.grad(loss, depth)[0]
    out["mask"], out["argmin"], out["loss"] = mask.detach(), argmin, loss.detach()
    return {k: v.numpy() for k, v in out.items()}


def figures(inp, r32, r64):
    import reproj_ref as R
    fig = {}
    near = np.zeros((N, H, W), bool)
    for f in range(2):
        near |= R.near_boundary(r64[f"coords{f}"], H, W)
    fig["share_near_boundary"] = near.mean()
    fig["share_near_tie"] = r64["near_tie"].mean()
    dw = np.concatenate([np.abs(r32[f"warped{f}"].astype(np.float64) - r64[f"warped{f}"]).ravel() for f in range(2)])
    fig["dev_warped_max"], fig["dev_warped_mean"] = dw.max(), dw.mean()
    fig["dev_loss"] = abs(float(r32["loss"]) - float(r64["loss"]))
    dg = []
    for f in range(2):
        nb = R.near_boundary(r64[f"coords{f}"], H, W)[:, None]
        g64 = r64[f"gdepth{f}"]
        dg.append((np.abs(r32[f"gdepth{f}"].astype(np.float64) - g64)[~nb] / np.abs(g64).max()).max())
    fig["dev_gdepth_rel"] = max(dg)
    c1 = r64["coords1"]
    fig["past_borders"] = np.array([(c1[..., 0] < 0).mean(), (c1[..., 0] > W - 1).mean(), (c1[..., 1] < 0).mean(),
                                    (c1[..., 1] > H - 1).mean()])
    return fig


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set PD_REFERENCE to the reference checkout")
    sys.path.insert(0, os.path.join(REF, "manydepth"))
    import layers
    methods = reference_methods()
    inp = inputs(SEED)
    r32, r64 = run(inp, torch.float32, layers, methods), run(inp, torch.float64, layers, methods)
    fig = figures(inp, r32, r64)
    assert fig["share_near_boundary"] <= 0.03, fig
    assert fig["share_near_tie"] <= 0.01, fig
    assert (fig["past_borders"] >= 0.2).all(), fig
    assert 0.1 < r64["mask"].mean() < 0.9, r64["mask"].mean()        # automasking both keeps and drops pixels
    data = dict(inp)
    for tag, r in (("f32", r32), ("f64", r64)):
        for k, v in r.items():
            if k != "near_tie":
                data[f"{k}_{tag}"] = v
    data["near_tie"] = r64["near_tie"]
    data.update({k: np.asarray(v, np.float64) for k, v in fig.items()})
    path = os.path.join(OUT, "g12_reproj.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    for k, v in fig.items():
        print(k, v)
    print("loss", r32["loss"], r64["loss"], "mask share", r64["mask"].mean(), "argmin share of frame 1", r64["argmin"].mean())


if __name__ == "__main__":
    main()
