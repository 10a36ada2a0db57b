#!/usr/bin/env python3
"""Generate tests/golden/g15_pose.npz by RUNNING THE REFERENCE's own pose pieces on the CPU:

    manydepth/layers.py                  transformation_from_parameters, BackprojectDepth, Project3D        (imported)
    manydepth/networks/pose_decoder.py   PoseDecoder (loaded by file path: the package itself needs torchvision)
    torch                                F.grid_sample(..., padding_mode="border", align_corners=True) and autograd

Like make_golden_reproj.py it runs only where the reference checkout is available ($PD_REFERENCE); the output is data only:

    PD_REFERENCE=<reference checkout> python tests/golden/make_golden_pose.py

Poses.  "aa" / "tr" [3,1,3] float32: one small pose, one with a rotation near 1 rad, one with axisangle exactly 0;
"M_inv0" / "M_inv1" [3,4,4]: the reference's matrices for invert False / True.  The reference builds rot and the translation
matrix in float32 buffers whatever the input dtype, so these are its float32 results; tests/pose_ref.py is the fp64 yardstick.

Decoder tail.  "head_w" [12,256], "head_b" [12], "head_x" [3,2,3,256] and "head_x1" [3,1,1,256] (NHWC, float32 values,
non-negative like the ReLU output they stand for); "head_aa" / "head_tr" and "head1_aa" / "head1_tr" [3,2,1,3] float64: the
reference PoseDecoder(num_ch_enc, 1, 2).double() forward with its squeeze / ("pose", 0) / ("pose", 1) layers replaced by
identities, so that its own lines 41-50 run on exactly that input (ReLU of a non-negative input is the input).

Warp.  The inputs of g12_reproj.npz (N = 2, C = 3, 19 x 37: three workgroups per item, the last one partial) with both source
frames, its cotangents gw0 / gw1, and a 3 x 5 case "s_*" (one partial wavefront).  The poses "wT0" / "wT1" / "s_T" are g12's
(the small case: drawn) with a translation offset chosen by a seed search: seeds are tried until no coordinate of the fp64
run lies within 1e-3 px of a cell boundary or of a border it has not clearly crossed, so that no flipped bilinear cell can hide
in a sum ("share_near_boundary" = 0, "warp_seed").  "dT{f}_f32" / "dT{f}_f64" and "s_dT_f32" / "s_dT_f64" [N,4,4]: autograd's
d sum(gw * warped) / d T through the reference chain in float32 and float64; "dev_gT_rel" = max|f32 - f64| / max|f64| over
the three cases; "share_clamped": the share of coordinates past a border per case.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("PD_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))


def poses(layers):
    aa = np.array([[[0.011, -0.007, 0.004]], [[0.62, -0.55, 0.58]], [[0.0, 0.0, 0.0]]], np.float32)
    tr = np.array([[[0.02, -0.013, 0.031]], [[-0.41, 0.27, 0.9]], [[0.05, 0.02, -0.3]]], np.float32)
    out = {"aa": aa, "tr": tr}
    for inv in (False, True):
        out[f"M_inv{int(inv)}"] = layers.transformation_from_parameters(torch.from_numpy(aa), torch.from_numpy(tr), inv).numpy()
    return out


def decoder_tail():
    spec = importlib.util.spec_from_file_location("ref_pose_decoder", os.path.join(REF, "manydepth", "networks", "pose_decoder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(15)
    dec = mod.PoseDecoder(np.array([64, 64, 128, 256, 512]), 1, 2).double()
    rng = np.random.default_rng(15)
    w = (0.2 * rng.standard_normal((12, 256))).astype(np.float32)
    b = (0.5 * rng.standard_normal(12)).astype(np.float32)
    with torch.no_grad():
        dec.convs[("pose", 2)].weight.copy_(torch.from_numpy(w).double().view(12, 256, 1, 1))
        dec.convs[("pose", 2)].bias.copy_(torch.from_numpy(b).double())
    for k in ("squeeze", ("pose", 0), ("pose", 1)):
        dec.convs[k] = torch.nn.Identity()
    out = {"head_w": w, "head_b": b}
    for tag, shape in (("head", (3, 2, 3, 256)), ("head1", (3, 1, 1, 256))):
        x = np.maximum(rng.standard_normal(shape) + 0.3, 0.0).astype(np.float32)
        with torch.no_grad():
            aa, tr = dec([[torch.from_numpy(x).double().permute(0, 3, 1, 2)]])
        out[f"{tag}_x"], out[f"{tag}_aa"], out[f"{tag}_tr"] = x, aa.numpy(), tr.numpy()
    return out


def warp_dT(layers, dtype, depth, src, K, inv_K, T, gw):
    """d sum(gw * warped) / d T and the pixel coordinates, through the reference chain in ``dtype``."""
    N, C, H, W = src.shape
    t = [torch.from_numpy(a).to(dtype) for a in (depth, src, K, inv_K, T, gw)]
    Tt = t[4].clone().requires_grad_(True)
    cam = layers.BackprojectDepth(N, H, W).to(dtype)(t[0], t[3])
    pix = layers.Project3D(N, H, W)(cam, t[2], Tt)
    warped = F.grid_sample(t[1], pix, padding_mode="border", align_corners=True)
    g = torch.autograd.grad((t[5] * warped).sum(), Tt)[0]
    coords = ((pix.detach() + 1) / 2) * torch.tensor([W - 1, H - 1], dtype=dtype)
    return g.numpy(), coords.numpy()


def small_case(rng):
    H, W = 3, 5
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = {"s_depth": (1.0 + 0.2 * np.sin(xx + 0.5 * yy))[None, None],
         "s_src": rng.uniform(0.1, 0.9, (1, 2, H, W)), "s_gw": rng.standard_normal((1, 2, H, W))}
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 0.7 * W, 0.9 * H, W / 2 - 0.3, H / 2 + 0.2
    d["s_K"] = K[None]
    d["s_inv_K"] = np.linalg.pinv(K.astype(np.float32)).astype(np.float64)[None]
    T = np.eye(4)
    T[:3, 3] = (0.03, -0.02, 0.01)
    d["s_T"] = T[None]
    return {k: v.astype(np.float32) for k, v in d.items()}


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set PD_REFERENCE to the reference checkout")
    sys.path.insert(0, os.path.join(REF, "manydepth"))
    import layers
    import reproj_ref as R
    data = {}
    data.update(poses(layers))
    data.update(decoder_tail())
    g12 = np.load(os.path.join(OUT, "g12_reproj.npz"))
    for seed in range(1000):
        rng = np.random.default_rng(1500 + seed)
        case = small_case(rng)
        cases = {"0": [g12[k] for k in ("depth", "src0", "K", "inv_K", "T0", "gw0")],
                 "1": [g12[k] for k in ("depth", "src1", "K", "inv_K", "T1", "gw1")],
                 "s": [case[k] for k in ("s_depth", "s_src", "s_K", "s_inv_K", "s_T", "s_gw")]}
        res, near, clamped = {}, 0, {}
        for tag, a in cases.items():
            a[4] = a[4].copy()
            a[4][:, :3, 3] += rng.uniform(-0.004, 0.004, (a[4].shape[0], 3)).astype(np.float32)
            H, W = a[1].shape[2:]
            g32, _ = warp_dT(layers, torch.float32, *a)
            g64, c64 = warp_dT(layers, torch.float64, *a)
            near += int(R.near_boundary(c64, H, W).sum())
            clamped[tag] = float(((c64[..., 0] <= 0) | (c64[..., 0] >= W - 1) | (c64[..., 1] <= 0) | (c64[..., 1] >= H - 1)).mean())
            res[tag] = (a[4], g32, g64)
        if near == 0:
            break
    else:
        sys.exit("no seed without a coordinate near a boundary")
    dev = 0.0
    for tag, (T, g32, g64) in res.items():
        pre = "s_" if tag == "s" else ""
        data[("s_T" if tag == "s" else f"wT{tag}")] = T
        data[f"{pre}dT{'' if tag == 's' else tag}_f32"], data[f"{pre}dT{'' if tag == 's' else tag}_f64"] = g32, g64
        dev = max(dev, float(np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max()))
    data.update({k: v for k, v in case.items() if k != "s_T"})
    data["dev_gT_rel"] = np.float64(dev)
    data["share_near_boundary"] = np.float64(0.0)
    data["warp_seed"] = np.int64(seed)
    data["share_clamped"] = np.array([clamped[k] for k in ("0", "1", "s")])
    path = os.path.join(OUT, "g15_pose.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes; seed", seed, "dev_gT_rel", dev, "clamped", clamped)


if __name__ == "__main__":
    main()
