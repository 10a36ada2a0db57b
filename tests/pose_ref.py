"""NumPy statement of the three definitions of the pose-network path (include/polardepth.h): transformation_from_parameters
and its gradient, the tail of PoseDecoder.forward and its gradient, and the gradient of the view synthesis w.r.t. the pose.
The fp64 parts are float64; gu / gv of the warp are float32 in the kernel's order; the large sums use math.fsum (exactly
rounded, so independent of any order).  Test infrastructure only; nothing here is fast."""
import math

import numpy as np

import reproj_ref

F64, F32 = np.float64, np.float32


# ------------------------------------------------------------------ transformation_from_parameters
def _rot(a):
    """a [N,3] fp64 -> dict of the reference's intermediates (layers.py:110-149), every product in its order."""
    angle = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    s = angle + 1e-7
    x, y, z = a[:, 0] / s, a[:, 1] / s, a[:, 2] / s
    ca, sa = np.cos(angle), np.sin(angle)
    C = 1.0 - ca
    xs, ys, zs = x * sa, y * sa, z * sa
    xC, yC, zC = x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    R = np.zeros((a.shape[0], 3, 3), F64)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = x * xC + ca, xyC - zs, zxC + ys
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = xyC + zs, y * yC + ca, yzC - xs
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = zxC - ys, yzC + xs, z * zC + ca
    return {"angle": angle, "s": s, "x": x, "y": y, "z": z, "ca": ca, "sa": sa, "C": C, "R": R}


def pose_matrix(axisangle, translation, invert):
    """pd_pose_matrix_fwd before its single rounding: [N,4,4] fp64 from the fp32 VALUES of the inputs."""
    a = np.asarray(axisangle, F32).reshape(-1, 3).astype(F64)
    t = np.asarray(translation, F32).reshape(-1, 3).astype(F64)
    R = _rot(a)["R"]
    M = np.zeros((a.shape[0], 4, 4), F64)
    M[:, 3, 3] = 1.0
    if invert:
        M[:, :3, :3] = R.transpose(0, 2, 1)
        for i in range(3):
            M[:, i, 3] = (R[:, 0, i] * -t[:, 0] + R[:, 1, i] * -t[:, 1]) + R[:, 2, i] * -t[:, 2]
    else:
        M[:, :3, :3] = R
        M[:, :3, 3] = t
    return M


def pose_matrix_grad(gT, axisangle, translation, invert):
    """pd_pose_matrix_bwd before rounding: (gaxisangle, gtranslation) [N,3] fp64 of sum(gT * T)."""
    a = np.asarray(axisangle, F32).reshape(-1, 3).astype(F64)
    t = np.asarray(translation, F32).reshape(-1, 3).astype(F64)
    gM = np.asarray(gT, F64).reshape(-1, 4, 4)
    r = _rot(a)
    R = r["R"]
    if invert:
        g = gM[:, :3, :3].transpose(0, 2, 1).copy()
        gt = -np.einsum("ni,nki->nk", gM[:, :3, 3], R)
        g -= t[:, :, None] * gM[:, None, :3, 3]                  # g[k][i] -= gM[i][3] t[k]
    else:
        g = gM[:, :3, :3].copy()
        gt = gM[:, :3, 3].copy()
    x, y, z, C, sa, ca, s, angle = (r[k] for k in ("x", "y", "z", "C", "sa", "ca", "s", "angle"))
    sxy, szx, syz = g[:, 0, 1] + g[:, 1, 0], g[:, 0, 2] + g[:, 2, 0], g[:, 1, 2] + g[:, 2, 1]
    dx, dy, dz = g[:, 2, 1] - g[:, 1, 2], g[:, 0, 2] - g[:, 2, 0], g[:, 1, 0] - g[:, 0, 1]
    gx = (2 * g[:, 0, 0] * x + sxy * y + szx * z) * C + dx * sa
    gy = (2 * g[:, 1, 1] * y + sxy * x + syz * z) * C + dy * sa
    gz = (2 * g[:, 2, 2] * z + szx * x + syz * y) * C + dz * sa
    gC = g[:, 0, 0] * x * x + g[:, 1, 1] * y * y + g[:, 2, 2] * z * z + sxy * x * y + szx * z * x + syz * y * z
    gsa = dx * x + dy * y + dz * z
    gca = g[:, 0, 0] + g[:, 1, 1] + g[:, 2, 2] - gC
    gangle = (gsa * ca - gca * sa) - (gx * a[:, 0] + gy * a[:, 1] + gz * a[:, 2]) / (s * s)
    k = np.where(angle > 0, gangle / np.where(angle > 0, angle, 1.0), 0.0)     # d norm / d a := 0 at angle == 0
    ga = np.stack([gx, gy, gz], 1) / s[:, None] + k[:, None] * a
    return ga, gt


def torch_matrix(aa, tr, invert):
    """transformation_from_parameters as torch expressions in the dtype of its inputs (the reference keeps float32 buffers
    whatever the input), for autograd in float64."""
    import torch
    v = aa.reshape(-1, 3)
    angle = v.norm(dim=1, keepdim=True)
    x, y, z = (v / (angle + 1e-7)).unbind(1)
    ca, sa = torch.cos(angle[:, 0]), torch.sin(angle[:, 0])
    C = 1 - ca
    Rm = torch.stack([x * x * C + ca, x * y * C - z * sa, z * x * C + y * sa,
                      x * y * C + z * sa, y * y * C + ca, y * z * C - x * sa,
                      z * x * C - y * sa, y * z * C + x * sa, z * z * C + ca], 1).reshape(-1, 3, 3)
    t = tr.reshape(-1, 3, 1)
    top = torch.cat([Rm.transpose(1, 2), -Rm.transpose(1, 2) @ t], 2) if invert else torch.cat([Rm, t], 2)
    last = torch.tensor([0, 0, 0, 1], dtype=aa.dtype).expand(top.shape[0], 1, 4)
    return torch.cat([top, last], 1)


# ------------------------------------------------------------------ PoseDecoder tail
def pose_head(x, w, b, invert):
    """pd_pose_head_fwd: x [N,h,w,Cin] NHWC, w [Co,Cin], b [Co].  mean and the unrounded o in fp64 (fsum), the fp32 outputs,
    and the fp64 matrices of slot 0 formed from the fp32 outputs."""
    x, w, b = np.asarray(x, F32), np.asarray(w, F32), np.asarray(b, F32)
    N, h, wd, Cin = x.shape
    Co = w.shape[0]
    nf = Co // 6
    xs = x.reshape(N, h * wd, Cin).astype(F64)
    mean = np.array([[math.fsum(xs[n, :, c]) for c in range(Cin)] for n in range(N)], F64) / float(h * wd)
    dot = np.array([[math.fsum(w[k].astype(F64) * mean[n]) for k in range(Co)] for n in range(N)], F64)
    o64 = 0.01 * (b.astype(F64)[None] + dot)
    o = o64.astype(F32).reshape(N, nf, 1, 6)
    aa, tr = o[..., :3].copy(), o[..., 3:].copy()
    return {"mean": mean, "o64": o64, "axisangle": aa, "translation": tr,
            "T": pose_matrix(aa[:, 0], tr[:, 0], invert), "T_inv": pose_matrix(aa[:, 0], tr[:, 0], not invert)}


def pose_head_grad(x_shape, w, mean, axisangle, translation, invert, gT=None, gT_inv=None, gaxisangle=None,
                   gtranslation=None):
    """pd_pose_head_bwd before rounding: gx [N,h,w,Cin], gw [Co,Cin], gb [Co] fp64; ``axisangle`` / ``translation`` are the
    forward's fp32 outputs, ``mean`` its fp64 means."""
    N, h, wd, Cin = x_shape
    w = np.asarray(w, F32).astype(F64)
    Co = w.shape[0]
    nf = Co // 6
    go = np.zeros((N, nf, 6), F64)
    if gaxisangle is not None:
        go[..., :3] += np.asarray(gaxisangle, F64).reshape(N, nf, 3)
    if gtranslation is not None:
        go[..., 3:] += np.asarray(gtranslation, F64).reshape(N, nf, 3)
    a0, t0 = np.asarray(axisangle)[:, 0], np.asarray(translation)[:, 0]
    for g, inv in ((gT, invert), (gT_inv, not invert)):
        if g is not None:
            ga, gt = pose_matrix_grad(g, a0, t0, inv)
            go[:, 0, :3] += ga
            go[:, 0, 3:] += gt
    gpre = 0.01 * go.reshape(N, Co)
    gmean = gpre @ w
    gx = np.broadcast_to((gmean / float(h * wd))[:, None, None, :], (N, h, wd, Cin)).copy()
    return gx, gpre.T @ np.asarray(mean, F64), gpre.sum(0)


# ------------------------------------------------------------------ d view synthesis / d pose
def _axis(c, size, dt):
    """axis_of of csrc/reproj.hip in ``dt`` (float32: the kernel): lower / upper cell, upper weight, free flag."""
    c = np.asarray(c, dt)
    hi = dt(size - 1)
    free = (c > 0) & (c < hi)
    cc = np.where(np.abs(c) <= dt(3.0e38), c, dt(0))
    cc = np.minimum(np.maximum(cc, dt(0)), hi).astype(dt)
    f = np.floor(cc)
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < size - 1)
    return i0, i1, (cc - f).astype(dt), free


def warp_grad_uv(gwarped, src, coords, dt=F32):
    """gu, gv [N,H,W] exactly as view_synth_bwd_kernel forms them (channel loop, float32, no fused multiply-add), and the
    free flags.  dt=float64: the same expressions in fp64 at fp64 coordinates (the formula, for comparison with autograd)."""
    gw, src, coords = np.asarray(gwarped, dt), np.asarray(src, dt), np.asarray(coords, dt)
    N, C, H, W = src.shape
    x0, x1, wx1, fx = _axis(coords[..., 0], W, dt)
    y0, y1, wy1, fy = _axis(coords[..., 1], H, dt)
    wx0, wy0 = (dt(1) - wx1).astype(dt), (dt(1) - wy1).astype(dt)
    n = np.arange(N)[:, None, None]
    gu, gv = np.zeros((N, H, W), dt), np.zeros((N, H, W), dt)
    for c in range(C):
        pc = src[:, c]
        v00, v10, v01, v11 = pc[n, y0, x0], pc[n, y0, x1], pc[n, y1, x0], pc[n, y1, x1]
        gu = gu + gw[:, c] * ((v10 - v00) * wy0 + (v11 - v01) * wy1)
        gv = gv + gw[:, c] * ((v01 - v00) * wx0 + (v11 - v10) * wx1)
        assert gu.dtype == dt and gv.dtype == dt
    return gu, gv, fx, fy


def view_synth_pose_grad(gwarped, src, coords, depth, K, inv_K, T, dt=F32):
    """pd_view_synth_bwd_pose: gP [N,12] (exactly rounded sums of the per-pixel fp64 terms), abs [N,12] (the sums of their
    absolute values: what the rounding of any summation order is relative to) and gT [N,4,4] = K[:3,:]^T gP, all fp64.
    ``coords`` are used as given (the kernel reads the forward's float32 ones); dt: see warp_grad_uv."""
    gu, gv, fx, fy = warp_grad_uv(gwarped, src, coords, dt)
    depth, K, inv_K, T = (np.asarray(a, F32).astype(F64) for a in (depth, K, inv_K, T))
    N, _, H, W = depth.shape
    # project() of the kernel: every sum left to right
    P = np.zeros((N, 3, 4), F64)
    for i in range(3):
        for j in range(4):
            P[:, i, j] = ((K[:, i, 0] * T[:, 0, j] + K[:, i, 1] * T[:, 1, j]) + K[:, i, 2] * T[:, 2, j]) + K[:, i, 3] * T[:, 3, j]
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    iK = inv_K[:, :3, :3]
    r = [(iK[:, i, 0, None, None] * xx + iK[:, i, 1, None, None] * yy) + iK[:, i, 2, None, None] for i in range(3)]
    with np.errstate(all="ignore"):
        p = [depth[:, 0] * r[i] for i in range(3)]
        h = [((P[:, i, 0, None, None] * p[0] + P[:, i, 1, None, None] * p[1]) + P[:, i, 2, None, None] * p[2]) +
             P[:, i, 3, None, None] for i in range(3)]
        hz = h[2] + 1e-7
        u, v = h[0] / hz, h[1] / hz
        a0 = gu.astype(F64) / hz
        a1 = gv.astype(F64) / hz
        a2 = -(np.where(fx, a0 * u, 0.0) + np.where(fy, a1 * v, 0.0))
        pj = p + [np.ones_like(p[0])]
        any_free = fx | fy
        terms = np.zeros((N, 12, H, W), F64)
        for j in range(4):
            terms[:, j] = np.where(fx, a0 * pj[j], 0.0)
            terms[:, 4 + j] = np.where(fy, a1 * pj[j], 0.0)
            terms[:, 8 + j] = np.where(any_free, a2 * pj[j], 0.0)
    gP = np.array([[math.fsum(terms[n, k].ravel()) for k in range(12)] for n in range(N)], F64)
    ab = np.array([[math.fsum(np.abs(terms[n, k]).ravel()) for k in range(12)] for n in range(N)], F64)
    return {"gP": gP, "abs": ab, "gT": gT_from_gP(gP, K), "gu": gu, "gv": gv, "free_x": fx, "free_y": fy}


def gT_from_gP(gP, K):
    """gT[k][j] = (K[0][k] gP[0][j] + K[1][k] gP[1][j]) + K[2][k] gP[2][j] in fp64: the finalize kernel's expression."""
    gP = np.asarray(gP, F64).reshape(-1, 3, 4)
    K = np.asarray(K, F32).astype(F64)
    gT = np.zeros((gP.shape[0], 4, 4), F64)
    for k in range(4):
        for j in range(4):
            gT[:, k, j] = (K[:, 0, k] * gP[:, 0, j] + K[:, 1, k] * gP[:, 1, j]) + K[:, 2, k] * gP[:, 2, j]
    return gT


near_boundary = reproj_ref.near_boundary
