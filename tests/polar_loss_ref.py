"""The statement of the polarimetric normals loss (pd_polar_loss_fwd / _bwd, include/polardepth.h) for the tests.

``terms`` is the NumPy statement of the forward pass from p on, vectorised; ``terms_loop`` the plain per-pixel loop it must
equal bit for bit.  p is the fp32 normal of the depth map (``depth_normals`` restates pd_gt_normals without a depth range in
fp32 NumPy; the GPU tests take p from pd_gt_normals on the device instead).  From p on, every fp32 value is converted to fp64
first and every decision is that of pd_polar_normals_stats (tests/polar_normals_ref.py), in its operation order:

GATES, in this order: valid == 0 (the pixel counts nowhere); dolp_out (rho not finite, < rho_min or > rho_max); bad (a2 not
finite or not > 0, a non-finite candidate component, or no candidate with b2 > 0).
ORIENTATION: p is negated when pz < 0; cy' = aolp_sign * cy.
NORMAL TERM: c+ = (m + q) / (sqrt(a2) sqrt(b2)), c- = (-m + q) / (sqrt(a2) sqrt(b2)) over (diff, spec1, spec2), the first strict
maximum c* wins;                       l_n = 1 - clamp(c*, -1, 1).
AZIMUTH TERM: frontal when t2 <= tilt2_min * a2 or no branch is usable; else branch s when c_s > c_d strictly, else d; with
m = (px cx) + (py cy'), u2 = cx cx + cy' cy' of that branch:      l_a = clamp(1 - (m m) / (t2 u2), 0, 1).
WEIGHT w = rho when dolp_weighted, else 1.  L_n = sum w l_n / sum w over the pixels with a winner, L_a likewise over the pixels
of the azimuth set; 0 when sum w is 0.  The sums here are math.fsum (exactly rounded, no order); the kernel's ordered fp64
sums may differ from them by the (n - 1) 2^-53 of any summation order.

STATE byte: bits 0-2 the winner (0 none, 1..6 = the evaluator's ``choice``), bit 3 p negated, bits 4-5 the azimuth branch
(0 none, 1 d, 2 s), bits 6-7 the gate (0 none, 1 valid == 0, 2 dolp_out, 3 bad).

``torch_loss`` restates the two values in torch, in any dtype, from the DEPTH (oracle.losses.depth_to_normals) with the
decisions of a given state map held fixed: autograd through it is the reference gradient."""
import math

import numpy as np
import torch

from oracle import losses as ol

WINNER, NEGATED, BRANCH_SHIFT, GATE_SHIFT = 7, 8, 4, 6
GATE_NONE, GATE_INVALID, GATE_DOLP_OUT, GATE_BAD = 0, 1, 2, 3
BR_NONE, BR_D, BR_S = 0, 1, 2
COUNTERS = ("n_normal", "n_azimuth", "dolp_out", "bad", "frontal", "spec", "flipped")
F32_MAX = np.float32(np.finfo(np.float32).max)


def depth_normals(depth, K):
    """depth [N,1,H,W] fp32, K [N,4,4] fp32 -> [N,H,W,4] fp32 (xyz, w = 0): sobel_xyz, cross, normalize12 of csrc/depth_normals.hpp
    in fp32, operation for operation; zero where the depth is not finite."""
    depth, K = np.asarray(depth, np.float32), np.asarray(K, np.float32)
    N, _, H, W = depth.shape
    f = np.float32
    out = np.zeros((N, H, W, 4), np.float32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for n in range(N):
            D = depth[n, 0]
            fx, fy, cx, cy = K[n, 0, 0], K[n, 1, 1], K[n, 0, 2], K[n, 1, 2]
            A = [np.zeros((H, W), np.float32) for _ in range(3)]
            B = [np.zeros((H, W), np.float32) for _ in range(3)]
            for dy in (-1, 0, 1):
                yy = np.clip(ys + dy, 0, H - 1)
                sy = f(2.0 if dy == 0 else 1.0)
                for dx in (-1, 0, 1):
                    xx = np.clip(xs + dx, 0, W - 1)
                    sx = f(2.0 if dx == 0 else 1.0)
                    d = D[yy, xx]
                    X = (xx.astype(np.float32) - cx) / fx * d
                    Y = (yy.astype(np.float32) - cy) / fy * d
                    kx, ky = sy * f(dx) * f(0.125), f(dy) * sx * f(0.125)
                    for v, t in zip(A, (X, Y, d)):
                        v += kx * t
                    for v, t in zip(B, (X, Y, d)):
                        v += ky * t
            v = [A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]]
            nv = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            inv = f(1.0) / np.maximum(nv, f(1e-12))
            fin = (D >= -F32_MAX) & (D <= F32_MAX)
            for i in range(3):
                out[n, ..., i] = np.where(fin, v[i] * inv, f(0.0))
    return out


def _pack(win, neg, branch, gate):
    return (win | np.where(neg, NEGATED, 0) | (branch << BRANCH_SHIFT) | (gate << GATE_SHIFT)).astype(np.uint8)


def _finish(out, rho, dolp_weighted):
    """The weights, the counters, the fsum sums and the two values from the per-pixel results."""
    st, ln, la = out["state"], out["l_n"], out["l_a"]
    gate, win, branch = st >> GATE_SHIFT, st & WINNER, (st >> BRANCH_SHIFT) & 3
    w = rho if dolp_weighted else np.ones_like(rho)
    cn, ca = win > 0, branch > 0
    passed = gate == GATE_NONE
    out["w"] = w
    out["counters"] = {"n_normal": int(cn.sum()), "n_azimuth": int(ca.sum()), "dolp_out": int((gate == GATE_DOLP_OUT).sum()),
                       "bad": int((gate == GATE_BAD).sum()), "frontal": int((passed & ~ca).sum()),
                       "spec": int((win >= 3).sum()), "flipped": int((cn & (win % 2 == 0)).sum())}
    out["sums"] = [math.fsum(w[cn] * ln[cn]), math.fsum(w[cn]), math.fsum(w[ca] * la[ca]), math.fsum(w[ca])]
    out["n_terms"] = (int(cn.sum()), int(ca.sum()))
    s = out["sums"]
    out["values"] = np.array([s[0] / s[1] if s[1] > 0 else 0.0, s[2] / s[3] if s[3] > 0 else 0.0], np.float64).astype(np.float32)
    return out


def terms(p, pol, xolp, valid=None, rho_min=0.05, rho_max=1.0, tilt2_min=0.0, aolp_sign=1, dolp_weighted=True):
    """p [N,H,W,>=3] fp32, pol [N,9,H,>=W] fp32, xolp [N,2,H,>=W] fp32, valid [N,H,W] or None -> dict(state uint8 [N,H,W],
    l_n, l_a float64 [N,H,W] with NaN where not counted, w, counters, sums (fsum), n_terms, values fp32 [2])."""
    assert p.dtype == np.float32 and pol.dtype == np.float32 and xolp.dtype == np.float32
    N, H, W = p.shape[:3]
    rmin, rmax, sign = np.float64(np.float32(rho_min)), np.float64(np.float32(rho_max)), np.float64(aolp_sign)
    rho = xolp[:, 0, :, :W].astype(np.float64)
    live = np.ones((N, H, W), bool) if valid is None else np.asarray(valid) != 0
    px, py, pz = (p[..., i].astype(np.float64) for i in range(3))
    C = pol[:, :, :, :W].astype(np.float64)
    cx, cy, cz = C[:, 0::3], sign * C[:, 1::3], C[:, 2::3]
    with np.errstate(all="ignore"):
        dolp_out = live & (~np.isfinite(rho) | (rho < rmin) | (rho > rmax))
        a2 = (px * px + py * py) + pz * pz
        b2 = (cx * cx + cy * cy) + cz * cz
        good = np.isfinite(a2) & (a2 > 0) & np.isfinite(C).all(1) & (b2 > 0).any(1)
        bad = live & ~dolp_out & ~good
        ok = live & ~dolp_out & good
        neg = ok & (pz < 0)
        px, py, pz = (np.where(neg, -v, v) for v in (px, py, pz))
        # ---- normal term
        best = np.full((N, H, W), -np.inf)
        win = np.full((N, H, W), -1, np.int64)
        sa = np.sqrt(a2)
        for b in range(3):
            m = px * cx[:, b] + py * cy[:, b]
            q = pz * cz[:, b]
            den = sa * np.sqrt(b2[:, b])
            for j, c in enumerate(((m + q) / den, (-m + q) / den)):
                better = ok & (b2[:, b] > 0) & np.isfinite(c) & (c > best)
                best = np.where(better, c, best)
                win = np.where(better, 2 * b + j, win)
        cn = ok & (win >= 0)
        l_n = np.where(cn, 1.0 - np.minimum(np.maximum(best, -1.0), 1.0), np.nan)
        # ---- azimuth term
        t2 = px * px + py * py
        md, ms = px * cx[:, 0] + py * cy[:, 0], px * cx[:, 1] + py * cy[:, 1]
        ud, us = cx[:, 0] * cx[:, 0] + cy[:, 0] * cy[:, 0], cx[:, 1] * cx[:, 1] + cy[:, 1] * cy[:, 1]
        frontal = ok & ((t2 <= np.float64(tilt2_min) * a2) | ~((ud > 0) | (us > 0)))
        ca = ok & ~frontal
        st = np.sqrt(t2)
        cd = np.where(ud > 0, np.minimum(np.abs(md) / (st * np.sqrt(ud)), 1.0), -1.0)
        cs = np.where(us > 0, np.minimum(np.abs(ms) / (st * np.sqrt(us)), 1.0), -1.0)
        spec = ca & (cs > cd)
        m, u2 = np.where(spec, ms, md), np.where(spec, us, ud)
        l_a = np.where(ca, np.minimum(np.maximum(1.0 - (m * m) / (t2 * u2), 0.0), 1.0), np.nan)
    gate = np.where(~live, GATE_INVALID, np.where(dolp_out, GATE_DOLP_OUT, np.where(bad, GATE_BAD, GATE_NONE)))
    branch = np.where(ca, np.where(spec, BR_S, BR_D), BR_NONE)
    out = {"state": _pack(np.where(cn, win + 1, 0), neg, branch, gate), "l_n": l_n, "l_a": l_a}
    return _finish(out, rho, dolp_weighted)


def terms_loop(p, pol, xolp, valid=None, rho_min=0.05, rho_max=1.0, tilt2_min=0.0, aolp_sign=1, dolp_weighted=True):
    """The same, one pixel at a time."""
    N, H, W = p.shape[:3]
    f64 = np.float64
    rmin, rmax, sign, tilt2 = f64(np.float32(rho_min)), f64(np.float32(rho_max)), f64(aolp_sign), f64(tilt2_min)
    state = np.zeros((N, H, W), np.uint8)
    l_n, l_a = np.full((N, H, W), np.nan), np.full((N, H, W), np.nan)
    for i in range(N):
        for y in range(H):
            for x in range(W):
                if valid is not None and not valid[i, y, x]:
                    state[i, y, x] = GATE_INVALID << GATE_SHIFT
                    continue
                rho = f64(xolp[i, 0, y, x])
                if not np.isfinite(rho) or rho < rmin or rho > rmax:
                    state[i, y, x] = GATE_DOLP_OUT << GATE_SHIFT
                    continue
                px, py, pz = (f64(p[i, y, x, j]) for j in range(3))
                cand = [(f64(pol[i, 3 * b, y, x]), sign * f64(pol[i, 3 * b + 1, y, x]), f64(pol[i, 3 * b + 2, y, x]))
                        for b in range(3)]
                with np.errstate(all="ignore"):
                    a2 = (px * px + py * py) + pz * pz
                    b2 = [(cx * cx + cy * cy) + cz * cz for cx, cy, cz in cand]
                    if not (np.isfinite(a2) and a2 > 0 and all(np.isfinite(v) for c3 in cand for v in c3) and any(b > 0 for b in b2)):
                        state[i, y, x] = GATE_BAD << GATE_SHIFT
                        continue
                    s = 0
                    if pz < 0:
                        px, py, pz = -px, -py, -pz
                        s |= NEGATED
                    best, win = -np.inf, -1
                    for b, (cx, cy, cz) in enumerate(cand):
                        if not b2[b] > 0:
                            continue
                        m = px * cx + py * cy
                        q = pz * cz
                        den = np.sqrt(a2) * np.sqrt(b2[b])
                        for j, c in enumerate(((m + q) / den, (-m + q) / den)):
                            if np.isfinite(c) and c > best:
                                best, win = c, 2 * b + j
                    if win >= 0:
                        s |= win + 1
                        l_n[i, y, x] = 1.0 - min(max(best, -1.0), 1.0)
                    t2 = px * px + py * py
                    u2 = [cand[b][0] * cand[b][0] + cand[b][1] * cand[b][1] for b in (0, 1)]
                    if not (t2 <= tilt2 * a2 or not (u2[0] > 0 or u2[1] > 0)):
                        mb = [px * cand[b][0] + py * cand[b][1] for b in (0, 1)]
                        cb = [min(abs(mb[b]) / (np.sqrt(t2) * np.sqrt(u2[b])), 1.0) if u2[b] > 0 else -1.0 for b in (0, 1)]
                        b = 1 if cb[1] > cb[0] else 0
                        s |= (BR_S if b else BR_D) << BRANCH_SHIFT
                        l_a[i, y, x] = min(max(1.0 - (mb[b] * mb[b]) / (t2 * u2[b]), 0.0), 1.0)
                    state[i, y, x] = s
    rho = xolp[:, 0, :, :W].astype(np.float64)
    return _finish({"state": state, "l_n": l_n, "l_a": l_a}, rho, dolp_weighted)


def torch_loss(depth, K, pol, xolp, state, dt, aolp_sign=1, dolp_weighted=True, diffuse_is_own_normal=False):
    """(L_n, L_a) in dtype ``dt`` from depth [N,1,H,W] (a tensor, possibly requiring grad), with the decisions of ``state``
    (uint8 [N,H,W], NumPy or torch) held fixed.  pol [N,9,H,>=W], xolp [N,2,H,>=W] fp32 (the padding is cut off here).
    diffuse_is_own_normal: the diffuse candidate is replaced by the detached normal itself, in ``dt``."""
    N, _, H, W = depth.shape
    st = torch.as_tensor(np.asarray(state)).long()
    win, neg, branch = st & WINNER, (st & NEGATED) != 0, (st >> BRANCH_SHIFT) & 3
    cn, ca = win > 0, branch > 0
    p = ol.depth_to_normals(depth.to(dt), torch.as_tensor(K).to(dt)[:, :3, :3]).permute(0, 2, 3, 1)      # [N,H,W,3]
    p = torch.where(neg[..., None], -p, p)
    C = torch.as_tensor(np.asarray(pol))[:, :, :, :W].to(dt).reshape(N, 3, 3, H, W).permute(0, 3, 4, 1, 2)   # [N,H,W,cand,xyz]
    C = C * torch.tensor([1.0, float(aolp_sign), 1.0], dtype=dt)
    if diffuse_is_own_normal:
        C = torch.cat([p.detach()[..., None, :], C[..., 1:, :]], -2)
    rho = torch.as_tensor(np.asarray(xolp))[:, 0, :, :W].to(dt)
    w = rho if dolp_weighted else torch.ones_like(rho)
    safe = torch.tensor([0.6, 0.0, 0.8], dtype=dt)

    def pick(index, mask):
        c = torch.gather(C, 3, index.clamp(0, 2)[..., None, None].expand(N, H, W, 1, 3))[..., 0, :]
        c = torch.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0)
        return torch.where(mask[..., None], c, safe), torch.where(mask[..., None], p, safe)

    # normal term
    c, q = pick((win - 1) // 2, cn)
    flip = torch.where((win % 2 == 0) & cn, -1.0, 1.0).to(dt)                      # a "-" candidate is (-cx, -cy', cz)
    c = c * torch.stack([flip, flip, torch.ones_like(flip)], -1)
    cos = (q * c).sum(-1) / (q.norm(dim=-1) * c.norm(dim=-1))
    l_n = 1.0 - cos.clamp(-1.0, 1.0)
    wn = torch.where(cn, w, torch.zeros_like(w))
    L_n = (wn * l_n).sum() / wn.sum() if float(wn.sum()) > 0 else (l_n * 0.0).sum()
    # azimuth term
    c, q = pick(branch - 1, ca)
    m = (q[..., :2] * c[..., :2]).sum(-1)
    l_a = (1.0 - m * m / ((q[..., :2] ** 2).sum(-1) * (c[..., :2] ** 2).sum(-1))).clamp(0.0, 1.0)
    wa = torch.where(ca, w, torch.zeros_like(w))
    L_a = (wa * l_a).sum() / wa.sum() if float(wa.sum()) > 0 else (l_a * 0.0).sum()
    return L_n, L_a


def torch_grad(depth, K, pol, xolp, state, dt, g=(1.0, 1.0), **kw):
    """d (g[0] L_n + g[1] L_a) / d depth [N,1,H,W] by autograd, and the two values."""
    d = torch.as_tensor(np.asarray(depth)).to(dt).clone().requires_grad_(True)
    L_n, L_a = torch_loss(d, K, pol, xolp, state, dt, **kw)
    gt = torch.tensor(g, dtype=torch.float32).to(dt)
    (gt[0] * L_n + gt[1] * L_a).backward()
    return d.grad, (L_n.detach(), L_a.detach())
