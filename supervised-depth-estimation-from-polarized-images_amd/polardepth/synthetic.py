"""Seeded synthetic "HAMMER-shaped" batches generated directly on the device.

Polarizer planes come from a physical model I_theta = Iun (1 + rho cos(2 theta - 2 phi)) + noise with
smooth low-DoLP fields (realistic, theta mostly inside the tables); RGB is uniform noise with a 2x2
averaged pyramid; GT depth is a smooth field in [0.3, 1.8] m with ~10 % invalid (zero) pixels and the
right ``pad_cols`` columns invalid (512x612 frames padded to 512x640, BASELINE.md shape note).
"""
import math

import torch


def _smooth(shape, gen, device, cutoff=24):
    """Low-pass noise in [0,1]: bilinear upsampling of a coarse random grid."""
    B, H, W = shape
    coarse = torch.rand((B, 1, max(H // cutoff, 2), max(W // cutoff, 2)), generator=gen, device=device)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[:, 0]


def _rigid(rot, t):
    """4x4 rigid motion from three small rotation angles (x, y, z order) and a translation (NumPy, fp64)."""
    import numpy as np
    rx, ry, rz = rot
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = t
    return T


def multiview_plane(B=2, H=32, W=48, frame_ids=(0, -1, 1), device="cuda", seed=0):
    """A textured slanted plane seen from ``len(frame_ids)`` cameras with known cam-to-world poses: depth and colour are
    analytic per view (ray-plane intersection; the texture is a smooth function of the in-plane coordinates), so the
    neighbours warped through the TRUE depth and relative poses reproduce frame 0 up to the bilinear interpolation error.
    Returns what the loader would: ("color", i, 0) [B,3,H,W] for every frame id, "depth" [B,1,H,W] of frame 0, ("K", 0) /
    ("inv_K", 0) [B,4,4], and per neighbour ("poses", i) [B,4,4] = inv(inv(T_0) T_i) (hammer_dataset.py:104-132: frame 0's
    camera coordinates -> the neighbour's) and ("frame_valid", i) [B] = 1.  It exists to check the conventions of the
    photometric term: pose direction, pixel-centre and intrinsics conventions."""
    import numpy as np
    rng = np.random.default_rng(seed)
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 0.65 * W
    K[0, 2], K[1, 2] = W / 2, H / 2
    inv_K = np.linalg.inv(K)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rays = np.einsum("ij,hwj->hwi", inv_K[:3, :3], np.stack([xx, yy, np.ones_like(xx)], -1))      # z component 1
    out = {k: [] for k in [("color", i, 0) for i in frame_ids] + [("poses", i) for i in frame_ids if i != 0] + ["depth"]}
    for _ in range(B):
        n = np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), 1.0])
        n /= np.linalg.norm(n)
        d0 = rng.uniform(1.0, 1.4)
        e1 = np.cross(n, [0.0, 1.0, 0.0]); e1 /= np.linalg.norm(e1)
        e2 = np.cross(n, e1)
        phase = rng.uniform(0, 2 * math.pi, 3)
        T0 = _rigid(rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.02, 0.02, 3))
        for i in frame_ids:
            Ti = T0 if i == 0 else T0 @ _rigid(rng.uniform(-0.02, 0.02, 3),
                                              np.array([0.15 * i, 0.04 * i, -0.03 * i]) + rng.uniform(-0.01, 0.01, 3))
            D = rays @ Ti[:3, :3].T                                                                # ray directions, world
            z = (d0 - n @ Ti[:3, 3]) / (D @ n)                                                     # camera depth (rays have z = 1)
            X = Ti[:3, 3] + z[..., None] * D
            a, b = X @ e1, X @ e2
            col = np.stack([0.5 + 0.22 * np.sin(10.0 * a + phase[c]) * np.cos(8.0 * b - phase[c])
                            + 0.2 * np.sin(6.0 * (a + b) + 2.0 * c) for c in range(3)])
            out[("color", i, 0)].append(col)
            if i == 0:
                out["depth"].append(z[None])
            else:
                out[("poses", i)].append(np.linalg.inv(np.linalg.inv(T0) @ Ti))
    dev = torch.device(device)
    res = {k: torch.from_numpy(np.stack(v).astype(np.float32)).to(dev) for k, v in out.items()}
    res[("K", 0)] = torch.from_numpy(np.tile(K.astype(np.float32), (B, 1, 1))).to(dev)
    res[("inv_K", 0)] = torch.from_numpy(np.tile(inv_K.astype(np.float32), (B, 1, 1))).to(dev)
    for i in frame_ids:
        if i != 0:
            res[("frame_valid", i)] = torch.ones(B, dtype=torch.float32, device=dev)
    return res


def make_batch(B, H=512, W=640, frame_w=612, device="cuda", seed=0, scales=(0, 1, 2, 3), with_pol=True,
               with_xolp=False):
    """Batch dict as IndoorDataset.__getitem__ + collate would deliver it (indoor_dataset.py:277-425),
    plus the optional raw planes ("pol",0,0) uint8 [B,4,H,W] for the fused on-device XOLP path."""
    dev = torch.device(device)
    gen = torch.Generator(device=dev).manual_seed(seed)
    inputs = {}
    color = torch.rand((B, 3, H, W), generator=gen, device=dev)
    inputs[("color", 0, 0)] = color
    inputs[("color_aug", 0, 0)] = color
    c = color
    for s in scales:
        if s == 0:
            continue
        c = torch.nn.functional.avg_pool2d(inputs[("color", 0, s - 1)] if ("color", 0, s - 1) in inputs else c, 2)
        inputs[("color", 0, s)] = c
        inputs[("color_aug", 0, s)] = c
    depth = 0.3 + 1.5 * _smooth((B, H, W), gen, dev)
    invalid = torch.rand((B, H, W), generator=gen, device=dev) < 0.10
    depth = torch.where(invalid, torch.zeros_like(depth), depth)
    if frame_w < W:
        depth[:, :, frame_w:] = 0.0
    inputs["depth"] = depth[:, None].contiguous()
    inputs["depth_gt"] = inputs["depth"]
    inputs[("mask", 0, 0)] = (torch.rand((B, 1, H, W), generator=gen, device=dev) * 11).int() * 20
    for s in scales:
        K = torch.eye(4, device=dev)[None].repeat(B, 1, 1)
        w_s, h_s = W // (2 ** s), H // (2 ** s)
        K[:, 0, 0] = 0.65 * w_s; K[:, 1, 1] = 0.65 * w_s; K[:, 0, 2] = w_s / 2; K[:, 1, 2] = h_s / 2
        inputs[("K", s)] = K
        inputs[("inv_K", s)] = torch.linalg.inv(K)
    if with_pol or with_xolp:
        iun = 20 + 200 * _smooth((B, H, W), gen, dev)
        rho = 0.6 * _smooth((B, H, W), gen, dev, cutoff=32) ** 3
        phi = math.pi * (_smooth((B, H, W), gen, dev, cutoff=40) - 0.5)
        planes = []
        for a in (0.0, math.pi / 4, math.pi / 2, 3 * math.pi / 4):
            planes.append(iun * (1 + rho * torch.cos(2 * a - 2 * phi)))
        pol = torch.stack(planes, 1) + 1.5 * torch.randn((B, 4, H, W), generator=gen, device=dev)
        pol = pol.round().clamp(0, 255).to(torch.uint8)
        inputs[("pol", 0, 0)] = pol
    return inputs
