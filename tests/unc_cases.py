"""The inputs of the depth-uncertainty tests (pd_unc_loss_*, pd_unc_stats): seeded host arrays, built once and read-only.

Loss cases.  Frame and head sizes: a non-integer ratio (9 x 65 <- 5 x 33), the three pyramid heads of a 24 x 40 frame (whose
width also takes the four-pixel path of the kernels), the identity at one row, one column and at 37 x 70 (21 workgroups, no
four-pixel path), and a ground truth that is a view of a wider array (pitched).  Every case holds: holes and NaN in the
ground truth, values exactly on both ends of the depth range (inside: the supervised mask is inclusive) and beyond them, a
pixel with depth == gt under the mask, u exactly 0 and exactly 1, a NaN u under the mask (the pixels it reaches leave the
mask), a NaN depth on a hole (it must not reach a sum), and |g - d| / b up to about 160.

Evaluator cases.  The four frame shapes; u at full resolution with exact 0 and 1, a NaN, one value beyond 1; predictions
beyond both clamps, NaN and infinite; image 0 of the 3 x 1 x 40 case has no pixel inside the gate; the instance mask never
holds 140, so the material "cutlery" of the default classes is empty."""
import functools

import numpy as np

MIN_D, MAX_D = 0.1, 2.0
B_RANGE = (0.0005, 0.5)

# name -> (N, H, W), (hs, ws), pitch of gt (0 = contiguous), with a `valid` map
LOSS_CASES = {
    "ratio_1.8": ((2, 9, 65), (5, 33), 0, True),
    "head_1": ((2, 24, 40), (12, 20), 0, False),
    "head_2": ((2, 24, 40), (6, 10), 0, True),
    "head_3": ((2, 24, 40), (3, 5), 0, False),
    "row": ((3, 1, 40), (1, 40), 0, False),
    "column": ((2, 40, 1), (40, 1), 0, True),
    "identity": ((2, 37, 70), (37, 70), 0, False),
    "pitched": ((2, 24, 40), (12, 20), 48, True),
}
STATS_SHAPES = [(2, 9, 65), (3, 1, 40), (2, 40, 1), (2, 37, 70)]
CLASSES = {
    1: [("all", None)],
    3: [("all", None), ("objects", (20, 160)), ("some", (40, 100))],          # overlapping ranges
    12: None,                                                                 # the default classes, filled in by the tests
}


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _gt(rng, N, H, W):
    gt = rng.uniform(0.3, 1.8, (N, H, W)).astype(np.float32)
    flat = gt.reshape(N, -1)
    P = H * W
    flat[:, 1 % P] = 0.0                                   # holes
    flat[0, 3 % P] = np.nan
    flat[-1, 5 % P] = 2.5                                  # beyond the range
    flat[0, 7 % P] = np.float32(MIN_D)                     # exactly on both ends
    flat[-1, 9 % P] = np.float32(MAX_D)
    flat[:, (P // 2)::11] = 0.0                            # a dotted line of holes
    return gt


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """dict(depth, gt [N,H,W] fp32 (gt possibly a view with row pitch), unc [N,hs,ws] fp32, valid uint8 [N,H,W] or None)"""
    (N, H, W), (hs, ws), pitch, with_valid = LOSS_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    gt = _gt(rng, N, H, W)
    P = H * W
    depth = (gt + rng.laplace(0.0, 0.02, (N, H, W))).astype(np.float32)
    dflat, gflat = depth.reshape(N, -1), gt.reshape(N, -1)
    dflat[:, 12 % P] = gflat[:, 12 % P]                    # depth == gt under the mask
    dflat[:, 1 % P] = np.nan                               # on a hole
    unc = rng.uniform(0.25, 0.8, (N, hs, ws)).astype(np.float32)
    uflat = unc.reshape(N, -1)
    Q = hs * ws
    uflat[:, 2 % Q] = 0.0
    uflat[:, 4 % Q] = 1.0
    uflat[-1, (Q - 1) - (3 % Q)] = np.nan
    valid = (rng.random((N, H, W)) < 0.9).astype(np.uint8) if with_valid else None
    if valid is not None:                                  # the pixels the case is about stay usable
        vflat = valid.reshape(N, -1)
        vflat[:, [7 % P, 9 % P, 12 % P]] = 1
    if pitch:
        wide = np.full((N, H, pitch), 1.0, np.float32)     # the padding is inside the depth range: reading it would show
        wide[:, :, :W] = gt
        _freeze(wide)
        gt = wide[:, :, :W]
    _freeze(depth, gt, unc, valid)
    return {"depth": depth, "gt": gt, "unc": unc, "valid": valid, "shape": (N, H, W), "head": (hs, ws)}


@functools.lru_cache(maxsize=None)
def stats_case(N, H, W):
    """(gt, pred, unc fp32 [N,H,W], mask int32 [N,H,W])"""
    rng = np.random.default_rng(7000 + 100 * N + H + W)
    gt = _gt(rng, N, H, W)
    P = H * W
    if (N, H, W) == (3, 1, 40):
        gt[0] = 0.0                                        # an image without a pixel inside the gate
    unc = rng.uniform(0.0, 1.0, (N, H, W)).astype(np.float32)
    b = np.exp(np.log(B_RANGE[0]) + unc.astype(np.float64) * np.log(B_RANGE[1] / B_RANGE[0]))
    # errors drawn from the stated scale times 0.5 .. 2: the ranking carries information, the calibration is off
    pred = (gt + rng.laplace(0.0, 1.0, (N, H, W)) * b * rng.uniform(0.5, 2.0, (N, H, W))).astype(np.float32)
    pflat, uflat = pred.reshape(N, -1), unc.reshape(N, -1)
    pflat[:, 14 % P] = 0.02                                # below and above the clamps
    pflat[:, 16 % P] = 3.5
    pflat[0, 18 % P] = np.nan
    pflat[-1, 20 % P] = np.inf
    pflat[-1, 22 % P] = -np.inf
    pflat[:, 1 % P] = np.nan                               # on a hole: gated out, not bad
    uflat[:, 24 % P] = 0.0
    uflat[:, 26 % P] = 1.0
    uflat[-1, 28 % P] = np.nan
    uflat[0, 30 % P] = 1.5                                 # finite but not a sigmoid's value: bad
    mask = (rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 8, 9, 10]), (N, H, W)) * 20).astype(np.int32)      # never 140
    _freeze(gt, pred, unc, mask)
    return gt, pred, unc, mask
