"""Pose accuracy of the pose network against the ground-truth relative poses: the per-pair records come from the kernel of
the pose supervision (``polardepth.ops.pose_supervision(details=True)``: pd_pose_loss_fwd, csrc/pose_loss.hip), stay on the
device while the evaluator walks its loader, and are copied to the host once; the figures below are formed there in
float64 (a few numbers per pair: there is nothing for a kernel to do).

Record of a pair (10 float64): rv(R_pred) [0:3], rv(R_gt) [3:6], the geodesic angle |rv(R_pred^T R_gt)| in radians [6],
|t_pred - t_gt| [7], |t_pred| [8], |t_gt| [9] (metres)."""
import numpy as np
import torch

from . import ops

STAT_NAMES = ("mean", "median", "rmse", "max")
SCALE_MIN_T = 1e-3          # pairs whose ground-truth translation is shorter than 1 mm say nothing about the scale


def pair_records(T_pred, T_gt, valid=None):
    """records [F,N,10] float64 on the device for lists of F predicted / ground-truth [N,4,4] matrices (no gradient)."""
    with torch.no_grad():
        return ops.pose_supervision([t.detach() for t in T_pred], T_gt, valid=valid, details=True)[3]


def _four(x, unit):
    x = np.asarray(x, np.float64) * unit
    if x.size == 0:
        return {k: float("nan") for k in STAT_NAMES}
    return {"mean": float(x.mean()), "median": float(np.median(x)), "rmse": float(np.sqrt((x * x).mean())),
            "max": float(x.max())}


def _group(rec, valid):
    rec = np.asarray(rec, np.float64).reshape(-1, 10)
    valid = np.asarray(valid).reshape(-1) != 0
    finite = np.isfinite(rec).all(1)
    use = valid & finite
    r = rec[use]
    far = r[:, 9] >= SCALE_MIN_T
    return {"pairs": int(use.sum()), "missing": int((~valid).sum()), "bad": int((valid & ~finite).sum()),
            "rot_deg": _four(r[:, 6], 180.0 / np.pi), "trans_mm": _four(r[:, 7], 1000.0),
            "scale_ratio_median": float(np.median(r[far, 8] / r[far, 9])) if far.any() else float("nan")}


def metrics_from_records(records, valid, frame_ids):
    """``records`` [F,M,10], ``valid`` [M,F] (0: the pair does not exist), tensors or arrays; ``frame_ids``: the F labels.
    Returns {frame id: figures, ..., "all": figures} with
      pairs / missing / bad   scored pairs; pairs with valid == 0; valid pairs with a non-finite record (never averaged)
      rot_deg, trans_mm       mean, median, rmse, max of the geodesic angle (degrees) and of |t_pred - t_gt| (millimetres)
      scale_ratio_median      the median of |t_pred| / |t_gt| over the scored pairs with |t_gt| >= 1 mm: a scale drift at a glance
    An empty set gives NaN figures."""
    if isinstance(records, torch.Tensor):
        records = records.detach().cpu().numpy()
    if isinstance(valid, torch.Tensor):
        valid = valid.detach().cpu().numpy()
    records, valid = np.asarray(records, np.float64), np.asarray(valid)
    if records.ndim != 3 or records.shape[2] != 10 or records.shape[0] != len(frame_ids) \
            or valid.shape != (records.shape[1], records.shape[0]):
        raise ValueError(f"metrics_from_records: records [F,M,10] and valid [M,F] for {len(frame_ids)} frame ids expected, "
                         f"got {records.shape} / {valid.shape}")
    out = {fid: _group(records[f], valid[:, f]) for f, fid in enumerate(frame_ids)}
    out["all"] = _group(records.reshape(-1, 10), valid.T.reshape(-1))
    return out


def format_report(results):
    lines = ["pose " + "{:>7} {:>7} {:>4} ".format("pairs", "missing", "bad")
             + ("{:>10} " * 9).format(*[f"rot_{k}" for k in STAT_NAMES], *[f"t_{k}" for k in STAT_NAMES], "scale")]
    for fid, r in results.items():
        lines.append(f"{str(fid):>4} {r['pairs']:>7} {r['missing']:>7} {r['bad']:>4} "
                     + ("&{: 9.4f} " * 9).format(*[r["rot_deg"][k] for k in STAT_NAMES],
                                                 *[r["trans_mm"][k] for k in STAT_NAMES], r["scale_ratio_median"]))
    return "\n".join(lines)
