"""Shared by tests/test_polar_loss_ref.py (CPU) and tests/test_polar_loss_gpu.py: the named geometries and seeded inputs of the
polarimetric normals loss (csrc/polar_loss.hip).

Depth: the ``pred`` surfaces of loss_cases.sup_case (smooth surfaces with 2 % noise; the tall one a sawtooth).  Candidates: built
near the surface's own normals -- per pixel one of diff / spec1 / spec2 is picked at random and given the normal's azimuth
(plus pi at random, plus N(0, 0.15 rad)) and zenith (plus N(0, 0.1 rad)); the other branch lies at pi/2 in azimuth, as the
physics has it, with a random zenith; rho is uniform in [0, 1.1).  On top, the special populations of
polar_normals_ref.random_case: NaN / zero / infinite candidates, no diffuse candidate, no azimuth, NaN rho, rho exactly at
rho_min, candidates on the far side (cz < 0), and a ``valid`` map with about 10 % zeros.

GEOMS: the first two straddle the 8 x 64 tile of the backward kernel; (1,2,2) is smaller than a Sobel window; a W = 1 frame has
no normal at all (every pixel `bad`) and an H = 1 frame normals made of rounding noise (tests/test_polar_loss_ref.py);
(1,32808,17) has more pixels than one forward launch covers without a second
grid-stride trip (2048 x 256) and more tiles (4101) than one trip of the backward kernel (PD_PLOSS_BWD_TILES_PER_TRIP)."""
import functools
import math

import numpy as np
import torch

import loss_cases as LC
import polar_loss_ref as R

GEOMS = [(2, 9, 65), (1, 17, 129), (2, 21, 70), (1, 8, 130), (1, 2, 2), (3, 1, 40), (2, 40, 1), (1, 32808, 17)]
SMALL = [g for g in GEOMS if g[1] * g[2] * g[0] < 10000]        # the per-pixel Python loop runs on these
DISP_GEOM, ZOOMS = (2, 18, 130), (1, 2)                        # d loss / d disp through DispDepthFn
PITCHED = (2, 21, 70, 80)                                      # N, H, W, ldp: rows padded with NaN
RHO_MIN, RHO_MAX, TILT_DEG = 0.05, 1.0, 5.0
TILT2 = math.sin(math.radians(TILT_DEG)) ** 2
COND = 5e-4                                                    # cap on max|g32 - g64| / max|g64| of the reference gradients
FWD_CAP = 2048 * 256                                           # pixels of one forward launch without a second trip
BWD_TILE_CAP = 4096


@functools.lru_cache(maxsize=None)
def case(N, H, W, ldp=None, exact=False):
    """-> dict(depth [N,1,H,W], K [N,4,4], p [N,H,W,4] (polar_loss_ref.depth_normals), pol [N,9,H,ldp], xolp [N,2,H,ldp], valid
    [N,H,W] uint8), fp32 NumPy.  exact: the diffuse candidate IS the pixel's own oriented normal, no special populations."""
    c = LC.sup_case(N, H, W)
    return build(c["pred"].numpy(), c["K"].numpy(), 7000 * N + 13 * H + W + (1 if exact else 0), ldp, exact)


@functools.lru_cache(maxsize=None)
def disp_case(N, H, W, zoom):
    """A disparity map [N,1,H/zoom,W/zoom] (loss_cases.ms_case), the depth map the reference chain makes of it in fp32, and
    candidates near that depth map's normals: the case of ``case`` plus "disp", "zoom"."""
    m = LC.ms_case(N, H, W, [zoom])
    depth = LC.ol.upsample_disp_to_depth(m["disps"][0], H, W, LC.MIN_D, LC.MAX_D)
    c = build(depth.numpy(), m["K"].numpy(), 9000 * N + 17 * H + W + zoom, None, False)
    c.update(disp=m["disps"][0].numpy(), zoom=zoom)
    return c


def build(depth, K, seed, ldp=None, exact=False):
    N, _, H, W = depth.shape
    p = R.depth_normals(depth, K)
    rng = np.random.default_rng(seed)
    ldp = W if ldp is None else ldp
    P = N * H * W
    n = p[..., :3].reshape(P, 3).astype(np.float64)
    n[n[:, 2] < 0] *= -1.0
    n[(n * n).sum(1) == 0] = (0.0, 0.0, 1.0)
    theta, phi = np.arccos(np.clip(n[:, 2], -1.0, 1.0)), np.arctan2(n[:, 1], n[:, 0])
    pick, flip = rng.integers(0, 3, P), rng.integers(0, 2, P)
    phi_n = phi + np.pi * flip + rng.normal(0, 0.15, P)
    th = rng.uniform(0.05, 1.4, (3, P))
    th[pick, np.arange(P)] = np.clip(theta + rng.normal(0, 0.1, P), 0.02, 1.5)
    az_d = np.where(pick == 0, phi_n, phi_n - np.pi / 2)
    az = np.stack([az_d, az_d + np.pi / 2, az_d + np.pi / 2])
    cand = np.stack([np.cos(az) * np.sin(th), np.sin(az) * np.sin(th), np.cos(th)], 1)          # [3 bases, 3 comps, P]
    rho = rng.uniform(0.0, 1.1, P)
    valid = np.ones((N, H, W), np.uint8)
    if exact:
        o = p[..., :3].reshape(P, 3).copy()
        o[o[:, 2] < 0] *= -1.0
        cand = cand.astype(np.float32)
        cand[0] = o.T
    else:
        kind = rng.random(P)
        cand[1, 1, kind < 0.02] = np.nan                                                         # bad
        cand[:, :, (kind >= 0.02) & (kind < 0.04)] = 0.0                                         # no candidate: bad
        cand[2, 0, (kind >= 0.04) & (kind < 0.05)] = np.inf                                      # bad
        cand[0, :, (kind >= 0.05) & (kind < 0.08)] = 0.0                                         # no diffuse candidate
        cand[:2, :2, (kind >= 0.08) & (kind < 0.10)] = 0.0                                       # no azimuth: frontal
        rho[(kind >= 0.10) & (kind < 0.11)] = np.nan
        rho[(kind >= 0.11) & (kind < 0.12)] = RHO_MIN                                            # at the lower bound: counts
        cand[:, :, (kind >= 0.12) & (kind < 0.16)] *= -1.0                                       # on the far side
        valid = (rng.random((N, H, W)) > 0.1).astype(np.uint8)
    pol = np.full((N, 9, H, ldp), np.nan, np.float32)                                            # the padding is never read
    pol[..., :W] = np.moveaxis(cand.reshape(9, N, H, W), 0, 1)
    xolp = np.full((N, 2, H, ldp), np.nan, np.float32)
    xolp[:, 0, :, :W] = rho.reshape(N, H, W)
    xolp[:, 1, :, :W] = phi.reshape(N, H, W)
    return {"N": N, "H": H, "W": W, "ldp": ldp, "depth": np.ascontiguousarray(depth), "K": np.ascontiguousarray(K), "p": p,
            "pol": pol, "xolp": xolp, "valid": valid}


def terms_of(c, p=None, **kw):
    """polar_loss_ref.terms of a case with the cases' options; p: another normal map (the device's)."""
    opt = dict(rho_min=RHO_MIN, rho_max=RHO_MAX, tilt2_min=TILT2)
    opt.update(kw)
    return R.terms(c["p"] if p is None else p, c["pol"], c["xolp"], c["valid"], **opt)


def disp_grad(c, state, dt, g=(1.3, 0.7), **kw):
    """d (g[0] L_n + g[1] L_a) / d disp through the reference's upsample_disp_to_depth, decisions fixed."""
    d = torch.from_numpy(c["disp"]).to(dt).requires_grad_(True)
    depth = LC.ol.upsample_disp_to_depth(d, c["H"], c["W"], LC.MIN_D, LC.MAX_D)
    L_n, L_a = R.torch_loss(depth, c["K"], c["pol"], c["xolp"], state, dt, **kw)
    gt = torch.tensor(g, dtype=torch.float32).to(dt)
    (gt[0] * L_n + gt[1] * L_a).backward()
    return d.grad
