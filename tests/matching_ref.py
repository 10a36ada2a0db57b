"""NumPy statement of pd_cost_volume (include/polardepth.h, "multi-frame cost volume"): the same operations in the same
order -- the projection in fp64, everything from the rounded coordinates on in fp32 (``dtype``), the channel sum as 16
partial sums and a binary tree.  This file is the definition the device is held to bit for bit; nothing here is fast.
``dtype=np.float64`` keeps the fp32 coordinates (the same mask, the same cells) and runs the arithmetic of steps 4-7 in fp64:
an oracle for the values, not the definition."""
import numpy as np

F64 = np.float64
F32 = np.float32


def frame_valid(T, valid=None):
    """[B,F] bool: polardepth.ops.cost_volume's rule -- a frame is skipped where ``valid`` is 0 or the 16 elements of its
    pose sum to 0 (resnet_encoder.py:463; the sum in fp32)."""
    T = np.asarray(T, F32)
    v = T.reshape(T.shape[0], T.shape[1], 16).sum(-1, dtype=F32) != 0
    if valid is not None:
        v &= np.asarray(valid) != 0
    return v


def project(T, K, inv_K, bins, h, w):
    """Steps 1-2: (u, v) [B,F,h,w,D] fp64, not yet rounded."""
    T, K, inv_K = (np.asarray(a, F32).astype(F64) for a in (T, K, inv_K))
    bins = np.asarray(bins, F32).astype(F64)
    B, Fr = T.shape[:2]
    P = np.empty((B, Fr, 3, 4), F64)
    for i in range(3):
        for j in range(4):
            P[:, :, i, j] = ((K[:, None, i, 0] * T[:, :, 0, j] + K[:, None, i, 1] * T[:, :, 1, j])
                             + K[:, None, i, 2] * T[:, :, 2, j]) + K[:, None, i, 3] * T[:, :, 3, j]
    yy, xx = np.mgrid[0:h, 0:w].astype(F64)
    r = [(inv_K[:, i, 0, None, None] * xx + inv_K[:, i, 1, None, None] * yy) + inv_K[:, i, 2, None, None] for i in range(3)]
    p = [bins[None, None, None, :] * ri[..., None] for ri in r]                       # [B,h,w,D]
    hh = []
    for i in range(3):
        c = lambda j: P[:, :, i, j, None, None, None]
        hh.append(((c(0) * p[0][:, None] + c(1) * p[1][:, None]) + c(2) * p[2][:, None]) + c(3))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hz = hh[2] + 1e-7
        return hh[0] / hz, hh[1] / hz


def channel_sum(a):
    """sum over the last axis (C, a multiple of 4) in the stated order: 16 partials, then a four-level binary tree."""
    C = a.shape[-1]
    assert C % 4 == 0
    part = np.zeros(a.shape[:-1] + (16,), a.dtype)
    for c0 in range(0, C, 64):
        for l in range(16):
            for k in range(4):
                c = c0 + 4 * l + k
                if c < C and 4 * l < C - c0:
                    part[..., l] = part[..., l] + a[..., c]
    for _ in range(4):
        part = part[..., 0::2] + part[..., 1::2]
    return part[..., 0]


def cost_volume(cur, lookup, T, K, inv_K, bins, valid=None, apply_confidence=False, dtype=F32):
    """cur [B,C,h,w], lookup [B,F,C,h,w], T [B,F,4,4], K / inv_K [B,4,4], bins [D], valid [B,F] (as the kernel sees it: apply
    frame_valid first for the Python layer's rule).  Returns a dict: cost [B,D,h,w], missing [B,D,h,w] uint8, confidence
    [B,h,w], argmin [B,h,w] int32, lowest [B,h,w]; and for the tests c (before the fill), nframes [B,D,h,w] (frames with
    m = 1), u / v [B,F,h,w,D] fp64 unrounded, mask [B,F,h,w,D]."""
    dt = dtype
    cur = np.asarray(cur, F32).astype(dt)
    B, C, h, w = cur.shape
    binsf = np.asarray(bins, F32)
    D = binsf.shape[0]
    Fr = 0 if lookup is None else np.asarray(lookup).shape[1]
    val = np.ones((B, Fr), bool) if valid is None else np.asarray(valid) != 0
    cur_l = np.moveaxis(cur, 1, -1)                                                   # [B,h,w,C]
    s = np.zeros((B, h, w, D), dt)
    n = np.zeros((B, h, w, D), np.int64)
    nframes = np.zeros((B, h, w, D), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    inner = ((xx >= 2) & (xx < w - 2) & (yy >= 2) & (yy < h - 2))[None, :, :, None]
    out = {}
    if Fr:
        lookup = np.asarray(lookup, F32).astype(dt)
        u64, v64 = project(T, K, inv_K, binsf, h, w)
        out["u"], out["v"] = u64, v64
        out["mask"] = np.zeros((B, Fr, h, w, D), bool)
    one = dt(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for f in range(Fr):
            u, v = u64[:, f].astype(F32).astype(dt), v64[:, f].astype(F32).astype(dt)
            m = (u >= 2) & (u <= w - 2) & (v >= 2) & (v <= h - 2) & inner & val[:, f][:, None, None, None]
            out["mask"][:, f] = m
            uc, vc = np.where(m, u, dt(2)), np.where(m, v, dt(2))
            fx, fy = np.floor(uc), np.floor(vc)
            wx1, wy1 = uc - fx, vc - fy
            wx0, wy0 = one - wx1, one - wy1
            x0, y0 = np.clip(fx.astype(np.int64), 0, max(w - 2, 0)), np.clip(fy.astype(np.int64), 0, max(h - 2, 0))
            x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
            L = np.moveaxis(lookup[:, f], 1, -1)                                      # [B,h,w,C]
            bi = np.arange(B)[:, None, None, None]
            w00, w10, w01, w11 = (wx0 * wy0)[..., None], (wx1 * wy0)[..., None], (wx0 * wy1)[..., None], (wx1 * wy1)[..., None]
            warped = ((L[bi, y0, x0] * w00 + L[bi, y0, x1] * w10) + L[bi, y1, x0] * w01) + L[bi, y1, x1] * w11  # [B,h,w,D,C]
            diff = channel_sum(np.abs(warped - cur_l[:, :, :, None, :])) / dt(C)
            s = np.where(m, s + diff, s)
            n = n + (m & (diff > 0))
            nframes += m
        c = s / (n.astype(dt) + dt(1e-7))
        missing = c == 0
        mx = c.max(-1, keepdims=True)                                                 # NaN if any bin is NaN
        filled = np.where(missing, mx, c)
        confidence = ((c > 0).sum(-1) == D).astype(dt)
        key = np.where(filled == 0, dt(100), filled)
        argmin = np.argmin(key, -1).astype(np.int32)                                  # first minimum; the first NaN wins
        lowest = one / binsf.astype(dt)[argmin]
        cost = filled * confidence[..., None] if apply_confidence else filled
    mv = lambda a: np.ascontiguousarray(np.moveaxis(a, -1, 1))
    out.update({"cost": mv(cost), "missing": mv(missing.astype(np.uint8)), "confidence": confidence, "argmin": argmin,
                "lowest": lowest, "c": mv(c), "nframes": mv(nframes)})
    return out
