"""NumPy statement of the pose supervision (include/polardepth.h, csrc/pose_loss.hip): rv(M) = roma.rotmat_to_rotvec and its
gradient, the loss of trainer.py:1267-1285 with the missing-frame mask and its gradient, the per-pair records and the
metrics of the pose evaluator.  Everything is float64 from the float32 VALUES of the matrices, every expression in the
header's order.  ``torch_rotvec`` / ``torch_pose_loss`` restate the same as torch ops for autograd in float64.  Test
infrastructure only; nothing here is fast."""
import numpy as np

F64, F32 = np.float64, np.float32


def _blocks(T):
    """[N,4,4] (or [N,3,3]) of float32 values -> R [N,3,3], t [N,3] in float64."""
    T = np.asarray(T)
    if T.dtype != F64:
        T = np.asarray(T, F32).astype(F64)
    T = T.reshape(-1, *T.shape[-2:])
    return T[:, :3, :3], (T[:, :3, 3] if T.shape[-1] == 4 else None)


# ------------------------------------------------------------------ rv(M)
def _rotvec_parts(M):
    """M [N,3,3] float64 -> dict of every intermediate of the header's definition."""
    M = np.asarray(M, F64).reshape(-1, 3, 3)
    N = M.shape[0]
    tr = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    d = np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], tr], 1)
    c = np.zeros(N, np.int64)
    n = np.arange(N)
    for i in range(1, 4):
        c = np.where(d[:, i] > d[n, c], i, c)                    # the first maximum
    qu = np.zeros((N, 4), F64)
    for b in range(3):
        i, j, k = b, (b + 1) % 3, (b + 2) % 3
        m = c == b
        qu[m, i] = 1.0 - tr[m] + 2.0 * M[m, i, i]
        qu[m, j] = M[m, j, i] + M[m, i, j]
        qu[m, k] = M[m, k, i] + M[m, i, k]
        qu[m, 3] = M[m, k, j] - M[m, j, k]
    m = c == 3
    qu[m, 0] = M[m, 2, 1] - M[m, 1, 2]
    qu[m, 1] = M[m, 0, 2] - M[m, 2, 0]
    qu[m, 2] = M[m, 1, 0] - M[m, 0, 1]
    qu[m, 3] = 1.0 + tr[m]
    with np.errstate(all="ignore"):
        nq = np.sqrt(((qu[:, 0] * qu[:, 0] + qu[:, 1] * qu[:, 1]) + qu[:, 2] * qu[:, 2]) + qu[:, 3] * qu[:, 3])
        q = qu / nq[:, None]
        sign = np.where(q[:, 3] < 0, -1.0, 1.0)
        q = np.where((q[:, 3] < 0)[:, None], -q, q)
        s = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        angle = 2.0 * np.arctan2(s, q[:, 3])
        small = angle <= 1e-3
        a2 = angle * angle
        scale = np.where(small, (2.0 + a2 / 12.0) + 7.0 * (a2 * a2) / 2880.0,
                         angle / np.where(small, 1.0, np.sin(angle / 2.0)))
    return {"c": c, "qu": qu, "nq": nq, "q": q, "sign": sign, "s": s, "angle": angle, "small": small, "scale": scale,
            "rv": scale[:, None] * q[:, :3]}


def rotvec(M):
    """rv(M) [N,3] float64 and the branch index c [N] (0..2: the largest diagonal entry, 3: the trace)."""
    p = _rotvec_parts(M)
    return p["rv"], p["c"]


def small_angle(M):
    """[N] bool: the item took the polynomial branch of the scale."""
    return _rotvec_parts(M)["small"]


def rotvec_grad(M, g):
    """J^T g [N,3,3] float64 for g [N,3]: J = d rv / d M with the branch fixed, the sign flip a constant, the polynomial
    differentiated in its own branch and d sqrt(x) / dx := 0 at x == 0."""
    p = _rotvec_parts(M)
    g = np.asarray(g, F64).reshape(-1, 3)
    N = g.shape[0]
    q, qu, nq, s, angle, scale = p["q"], p["qu"], p["nq"], p["s"], p["angle"], p["scale"]
    gq = np.zeros((N, 4), F64)
    gscale = (g[:, 0] * q[:, 0] + g[:, 1] * q[:, 1]) + g[:, 2] * q[:, 2]
    gq[:, :3] = scale[:, None] * g
    with np.errstate(all="ignore"):
        sh, ch = np.sin(angle / 2.0), np.cos(angle / 2.0)
        shs = np.where(p["small"], 1.0, sh)
        dscale = np.where(p["small"], angle / 6.0 + 7.0 * ((angle * angle) * angle) / 720.0,
                          1.0 / shs - (angle * ch * 0.5) / (shs * shs))
        gangle = gscale * dscale
        den = s * s + q[:, 3] * q[:, 3]
        gs = gangle * (2.0 * q[:, 3] / den)
        gq[:, 3] = gangle * (-2.0 * s / den)
        pos = s > 0
        gq[:, :3] += np.where(pos[:, None], gs[:, None] * (q[:, :3] / np.where(pos, s, 1.0)[:, None]), 0.0)
        gp = p["sign"][:, None] * gq
        dot = ((gp[:, 0] * qu[:, 0] + gp[:, 1] * qu[:, 1]) + gp[:, 2] * qu[:, 2]) + gp[:, 3] * qu[:, 3]
        gnq = -dot / (nq * nq)
        gqu = gp / nq[:, None] + np.where((nq > 0)[:, None], gnq[:, None] * (qu / nq[:, None]), 0.0)
    gM = np.zeros((N, 3, 3), F64)
    gtr = np.zeros(N, F64)
    for b in range(3):
        i, j, k = b, (b + 1) % 3, (b + 2) % 3
        m = p["c"] == b
        gtr[m] = -gqu[m, i]
        gM[m, i, i] += 2.0 * gqu[m, i]
        gM[m, j, i] += gqu[m, j]
        gM[m, i, j] += gqu[m, j]
        gM[m, k, i] += gqu[m, k]
        gM[m, i, k] += gqu[m, k]
        gM[m, k, j] += gqu[m, 3]
        gM[m, j, k] -= gqu[m, 3]
    m = p["c"] == 3
    gtr[m] = gqu[m, 3]
    for (r0, c0), idx in (((2, 1), 0), ((0, 2), 1), ((1, 0), 2)):
        gM[m, r0, c0] += gqu[m, idx]
        gM[m, c0, r0] -= gqu[m, idx]
    for i in range(3):
        gM[:, i, i] += gtr
    return gM


# ------------------------------------------------------------------ the loss
def default_weights(F):
    """[F, F-1, ..., 1]: the reference adds the running sums inside its loop over the frames."""
    return [float(F - f) for f in range(F)]


def _frame_terms(Tp, Tg, v):
    Rp, tp = _blocks(Tp)
    Rg, tg = _blocks(Tg)
    ok = np.ones(Rp.shape[0], bool) if v is None else np.asarray(v) != 0
    dr = rotvec(Rp)[0] - rotvec(Rg)[0]
    dt = tp - tg
    e_r = (dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2]
    e_t = (dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1]) + dt[:, 2] * dt[:, 2]
    return Rp, dr, dt, e_r, e_t, ok


def pose_loss(T_pred, T_gt, valid=None, frame_weight=None):
    """pd_pose_loss_fwd before its roundings: vals [3 + 2F] float64.  T_pred / T_gt: lists of F [N,4,4]; valid [N,F] or None."""
    F = len(T_pred)
    w = default_weights(F) if frame_weight is None else [float(F32(x)) for x in frame_weight]
    vals = np.zeros(3 + 2 * F, F64)
    for f in range(F):
        _, _, _, e_r, e_t, ok = _frame_terms(T_pred[f], T_gt[f], None if valid is None else np.asarray(valid)[:, f])
        cnt = int(ok.sum())
        rf = 0.1 * (e_r[ok].sum() / (3.0 * cnt)) if cnt else 0.0
        tf = e_t[ok].sum() / (3.0 * cnt) if cnt else 0.0
        vals[0] += rf
        vals[1] += tf
        vals[2] += w[f] * (rf + tf)
        vals[3 + 2 * f], vals[4 + 2 * f] = rf, tf
    return vals


def pose_loss_grad(gvals, T_pred, T_gt, valid=None, frame_weight=None):
    """pd_pose_loss_bwd before rounding: list of F [N,4,4] float64, the gradient of sum(gvals * vals[:3]) w.r.t. T_pred."""
    F = len(T_pred)
    w = default_weights(F) if frame_weight is None else [float(F32(x)) for x in frame_weight]
    gv = np.asarray(gvals, F32).astype(F64)
    out = []
    for f in range(F):
        Rp, dr, dt, _, _, ok = _frame_terms(T_pred[f], T_gt[f], None if valid is None else np.asarray(valid)[:, f])
        cnt = int(ok.sum())
        g = np.zeros((Rp.shape[0], 4, 4), F64)
        if cnt:
            a_r = gv[0] + w[f] * gv[2]
            a_t = gv[1] + w[f] * gv[2]
            g[:, :3, :3] = (a_r * 0.1 * 2.0 / (3.0 * cnt)) * rotvec_grad(Rp, dr)
            g[:, :3, 3] = (a_t * 2.0 / (3.0 * cnt)) * dt
            g[~ok] = 0.0
        out.append(g)
    return out


def pose_records(T_pred, T_gt):
    """records [F,N,10] float64: rv_pred, rv_gt, |rv(R_pred^T R_gt)|, |t_pred - t_gt|, |t_pred|, |t_gt|."""
    rec = []
    norm = lambda x: np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    for Tp, Tg in zip(T_pred, T_gt):
        Rp, tp = _blocks(Tp)
        Rg, tg = _blocks(Tg)
        D = np.zeros_like(Rp)
        for i in range(3):
            for j in range(3):
                D[:, i, j] = (Rp[:, 0, i] * Rg[:, 0, j] + Rp[:, 1, i] * Rg[:, 1, j]) + Rp[:, 2, i] * Rg[:, 2, j]
        rec.append(np.concatenate([rotvec(Rp)[0], rotvec(Rg)[0], norm(rotvec(D)[0])[:, None], norm(tp - tg)[:, None],
                                   norm(tp)[:, None], norm(tg)[:, None]], 1))
    return np.stack(rec)


# ------------------------------------------------------------------ the evaluator's figures
def _four(x, unit):
    x = np.asarray(x, F64) * unit
    if x.size == 0:
        return {"mean": float("nan"), "median": float("nan"), "rmse": float("nan"), "max": float("nan")}
    return {"mean": float(x.mean()), "median": float(np.median(x)), "rmse": float(np.sqrt((x * x).mean())),
            "max": float(x.max())}


def _group(rec, valid):
    rec = np.asarray(rec, F64).reshape(-1, 10)
    valid = np.asarray(valid).reshape(-1) != 0
    finite = np.isfinite(rec).all(1)
    use = valid & finite
    r = rec[use]
    big = r[:, 9] >= 1e-3
    return {"pairs": int(use.sum()), "missing": int((~valid).sum()), "bad": int((valid & ~finite).sum()),
            "rot_deg": _four(r[:, 6], 180.0 / np.pi), "trans_mm": _four(r[:, 7], 1000.0),
            "scale_ratio_median": float(np.median(r[big, 8] / r[big, 9])) if big.any() else float("nan")}


def metrics(records, valid, frame_ids):
    """records [F,M,10] float64, valid [M,F] (0: the pair does not exist), frame_ids: F labels.  Per frame id and under
    "all": pairs / missing / bad counts, rot_deg and trans_mm (mean, median, rmse, max) of the scored pairs, and the median of
    |t_pred| / |t_gt| over the scored pairs with |t_gt| >= 1 mm.  A pair with valid == 0 is ``missing``; a valid pair with a
    non-finite record is ``bad``; neither is averaged."""
    records, valid = np.asarray(records, F64), np.asarray(valid)
    out = {fid: _group(records[f], valid[:, f]) for f, fid in enumerate(frame_ids)}
    out["all"] = _group(records.reshape(-1, 10), valid.T.reshape(-1))
    return out


# ------------------------------------------------------------------ the same as torch ops (autograd in float64)
def torch_rotvec(M):
    """rv(M) for M [N,3,3] in the dtype of M: roma.rotmat_to_rotvec's expressions; the untaken branch of the scale is fed a
    harmless argument so that its zero cotangent stays zero."""
    import torch
    tr = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    c = torch.argmax(torch.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], tr], 1), 1)      # the first maximum
    cand = []
    for b in range(3):
        i, j, k = b, (b + 1) % 3, (b + 2) % 3
        q = [None] * 4
        q[i] = 1 - tr + 2 * M[:, i, i]
        q[j] = M[:, j, i] + M[:, i, j]
        q[k] = M[:, k, i] + M[:, i, k]
        q[3] = M[:, k, j] - M[:, j, k]
        cand.append(torch.stack(q, 1))
    cand.append(torch.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1], 1 + tr], 1))
    q = cand[3]
    for b in range(3):
        q = torch.where((c == b)[:, None], cand[b], q)
    q = q / torch.norm(q, dim=1, keepdim=True)
    q = torch.where((q[:, 3] < 0)[:, None], -q, q)
    angle = 2 * torch.atan2(torch.norm(q[:, :3], dim=1), q[:, 3])
    small = angle <= 1e-3
    safe = torch.where(small, torch.ones_like(angle), angle)
    scale = torch.where(small, 2 + angle ** 2 / 12 + 7 * angle ** 4 / 2880, safe / torch.sin(safe / 2))
    return scale[:, None] * q[:, :3]


def torch_pose_loss(T_pred, T_gt):
    """trainer.py:1267-1285 literally: the running sums r_loss / t_loss are added to the total INSIDE the loop over the
    frames.  Returns (r_loss, t_loss, what was added to total_loss)."""
    import torch
    t_loss = 0.
    r_loss = 0.
    total_loss = 0.
    for Tp, Tg in zip(T_pred, T_gt):
        R_pred = torch_rotvec(Tp[:, :3, :3])
        R_GT = torch_rotvec(Tg[:, :3, :3])
        t_pred = Tp[:, :3, 3]
        t_GT = Tg[:, :3, 3]
        r_loss = r_loss + 0.1 * torch.pow(R_pred - R_GT, 2).mean()
        t_loss = t_loss + 1.0 * torch.pow(t_pred - t_GT, 2).mean()
        total_loss = total_loss + (1.0 * r_loss + 1.0 * t_loss)
    return r_loss, t_loss, total_loss


# ------------------------------------------------------------------ inputs shared by the tests
def head_matrices(rng, n, max_angle=3.0, t_scale=0.05, invert=False):
    """The float32 matrices the pose head produces ([n,4,4] float32 values): a seeded axis-angle with angle uniform in
    [0, max_angle) and a translation, through pose_ref.pose_matrix, rounded once."""
    import pose_ref
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    aa = (v * rng.uniform(0.0, max_angle, (n, 1))).astype(F32)
    tr = (t_scale * rng.standard_normal((n, 3))).astype(F32)
    return pose_ref.pose_matrix(aa, tr, invert).astype(F32)
