"""Point-cloud accuracy (csrc/pointcloud.hip) at the evaluation's sizes: B = 12 at 320x480 and B = 16 at 512x640.

The scene is synthetic: a smooth surface with a few raised boxes ("objects") and holes; the prediction is the truth with about
1 % relative noise and a handful of depth spikes per image.  Timed, warm, with HIP events (one event pair per call, median of
``--iters`` calls; ``--brute-iters`` for the brute route):
  cloud_stats   the whole measurement: two back-projections, nearest neighbours both ways (pruned), two record calls
  stats         the two record calls (pd_cloud_stats) alone, on distances found beforehand
  nn_pruned     the two pd_cloud_nn calls alone, pruned;  nn_brute: the same with PD_PCD_BRUTE
  copy          a device copy that moves the bytes the two pd_cloud_nn calls must touch once (both clouds' points and boxes
                read, d2 written, per direction)
  ckdtree       scipy.spatial.cKDTree on ONE core for ONE image, both directions (build + query), if scipy is there
and the mean and the maximum number of target tiles scanned per query tile (``visited``).  The brute route's arithmetic floor is
quoted beside its time: 2 directions x (H W)^2 pairs x 8 vector operations per image against the guide's fp32 vector rate of
157.3 TFLOP/s counted as 78.6 T operations/s (an FMA counts two) -- derived, not measured.  One JSON line per size, printed and
written to ``--out`` (default: profiles/pointcloud.log)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

SIZES = ((12, 320, 480), (16, 512, 640))
VECTOR_OPS_PER_S = 78.6e12


def _median_ms(call, iters):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in evs:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[iters // 2]


def make_scene(N, H, W, seed=0, spikes=6):
    """(gt, pred, K, mask) on the device."""
    import torch
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = np.stack([1.2 + 0.25 * np.sin(xx / (W / 5.0) + rng.uniform(0, 6)) * np.cos(yy / (H / 4.0) + rng.uniform(0, 6))
                   for _ in range(N)]).astype(np.float32)
    mask = np.full((N, H, W), 180, np.int32)
    for i in range(N):
        for k in range(6):                                 # objects: boxes standing 5 - 25 cm in front of the surface
            h, w = rng.integers(H // 10, H // 4), rng.integers(W // 10, W // 4)
            y0, x0 = rng.integers(0, H - h), rng.integers(0, W - w)
            gt[i, y0:y0 + h, x0:x0 + w] -= np.float32(rng.uniform(0.05, 0.25))
            mask[i, y0:y0 + h, x0:x0 + w] = 20 * (1 + k)
    gt[rng.random((N, H, W)) < 0.002] = 0.0
    pred = (gt * (1.0 + 0.01 * rng.normal(size=gt.shape))).astype(np.float32)
    for i in range(N):
        ys, xs = rng.integers(0, H, spikes), rng.integers(0, W, spikes)
        pred[i, ys, xs] *= np.float32(1.4)
    Kmat = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    Kmat[:, 0, 0], Kmat[:, 1, 1], Kmat[:, 0, 2], Kmat[:, 1, 2] = 0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H
    dev = lambda a: torch.from_numpy(a).cuda()
    return dev(gt), dev(pred), dev(Kmat), dev(mask)


def _ckdtree_ms(p, t):
    """One image, both directions, one core: build + query of the exact nearest neighbour."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    a, b = p[p[:, 3] == 1][:, :3].astype(np.float64), t[t[:, 3] == 1][:, :3].astype(np.float64)
    t0 = time.perf_counter()
    cKDTree(b).query(a, k=1, workers=1)
    cKDTree(a).query(b, k=1, workers=1)
    return (time.perf_counter() - t0) * 1e3


def bench(N, H, W, iters, brute_iters):
    import torch
    from polardepth import pointcloud as pc
    if not torch.cuda.is_available():
        raise RuntimeError("bench_pointcloud needs the GPU; there is no CPU fallback")
    gt, pred, K, mask = make_scene(N, H, W)
    p = pc.backproject(pred, K, gate=gt)
    t = pc.backproject(gt, K)
    T = p.tiles

    def both(prune):
        pc.nearest(p, t, prune)
        pc.nearest(t, p, prune)

    def whole():
        pc.cloud_stats(pred, gt, K, mask=mask)

    d2_acc, d2_comp = pc.nearest(p, t), pc.nearest(t, p)

    def stats():
        pc.direction_stats(d2_acc, p, mask)
        pc.direction_stats(d2_comp, t, mask)

    for f in (lambda: both(True), whole, stats):
        f()
    torch.cuda.synchronize()
    out = {"op": "pointcloud", "N": N, "H": H, "W": W, "tiles": T}
    out["cloud_stats_ms"] = round(_median_ms(whole, iters), 4)
    out["stats_ms"] = round(_median_ms(stats, iters), 4)
    out["nn_pruned_ms"] = round(_median_ms(lambda: both(True), iters), 4)
    both(False)
    torch.cuda.synchronize()
    out["nn_brute_ms"] = round(_median_ms(lambda: both(False), brute_iters), 3)
    pairs = 2.0 * N * (float(H) * W) ** 2
    out["brute_floor_ms"] = round(pairs * 8 / VECTOR_OPS_PER_S * 1e3, 3)
    moved = 2 * (p.points.numel() * 4 + t.points.numel() * 4 + p.boxes.numel() * 4 + t.boxes.numel() * 4) + 2 * N * T * 256 * 4
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    out["bytes"] = moved
    out["copy_ms"] = round(_median_ms(lambda: dst.copy_(src), iters), 4)
    _, seen_a = pc.nearest(p, t, True, visited=True)
    _, seen_c = pc.nearest(t, p, True, visited=True)
    torch.cuda.synchronize()
    out["visited_mean_acc"] = round(float(seen_a.float().mean()), 2)
    out["visited_mean_comp"] = round(float(seen_c.float().mean()), 2)
    out["visited_max"] = int(max(seen_a.max(), seen_c.max()))
    st = pc.cloud_stats(pred, gt, K, mask=mask)
    pooled = st.pooled().cpu().numpy()
    out.update({"acc_mm": round(float(pooled[0, 0]), 3), "comp_mm": round(float(pooled[0, 1]), 3),
                "f10": round(float(pooled[0, 6]), 4), "points": int(pooled[0, 8])})
    ms = _ckdtree_ms(p.points[0].cpu().numpy(), t.points[0].cpu().numpy())
    out["ckdtree_one_image_one_core_ms"] = None if ms is None else round(ms, 1)
    out["nn_pruned_ms_per_image"] = round(out["nn_pruned_ms"] / N, 4)
    out["nn_brute_ms_per_image"] = round(out["nn_brute_ms"] / N, 3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--brute-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud.log"), help="the log; '' = print only")
    args = ap.parse_args()
    log = open(args.out, "w") if args.out else None
    for N, H, W in SIZES:
        line = json.dumps(bench(N, H, W, args.iters, args.brute_iters))
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
    if log:
        log.close()
