"""pd_depth_stats / pd_depth_medians (csrc/depth_stats.hip) at the evaluation's sizes: B = 12 at 320x480 and B = 16 at
512x640, the twelve default classes, without and with median scaling.

ms per call with HIP events, warm: one event pair per call, median of ``--iters`` calls, every call on another of ``--sets``
rotating input sets (sized past the 256 MB Infinity Cache).  The unscaled call is the C entry point on preallocated records
and workspace; the scaled call is ``depth_eval.depth_stats(median_scaling="numpy")`` as the evaluation makes it (medians, the
ratio in torch ops, the records; its allocations come from torch's caching allocator).  GB/s from the algorithm's own byte
count -- 12 bytes per pixel unscaled (depth, prediction, mask), 60 scaled (the four selection passes read them again) -- next
to the rate of a device copy that moves the SAME number of bytes (half read, half written; rotating buffers, the same
timing).  The yardstick, in the same run on the same sets: the 11 ``ops.depth_metrics`` launch pairs ``Evaluation.test``
makes for one batch.  One JSON line per measurement, printed and written to ``--out`` (default: profiles/depth_stats.log)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

SIZES = ((12, 320, 480), (16, 512, 640))
BYTES_PER_PIXEL = {None: 12, "numpy": 60}


def _median_ms(call, iters):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (e0, e1) in enumerate(evs):
        e0.record()
        call(i)
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[iters // 2], ts[0], ts[-1]


def _copy_rate(moved, sets, iters):
    """GB/s of a device copy that moves ``moved`` bytes, half read and half written, over rotating buffers"""
    import torch
    half = moved // 2
    src = [torch.empty(half, dtype=torch.uint8, device="cuda").fill_(s + 1) for s in range(sets)]
    dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    copy = lambda i: dst[i % sets].copy_(src[i % sets])
    for i in range(sets):
        copy(i)
    torch.cuda.synchronize()
    ms, _, _ = _median_ms(copy, iters)
    return ms, 2 * half / (ms * 1e-3) / 1e9


def make_set(N, H, W, seed):
    """One input set on the device: a smooth depth map with a few holes, a prediction a few per cent off with some values
    beyond the clamps, the instance mask in 32x32 blocks of the eleven grey values."""
    import torch
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = np.stack([1.0 + 0.3 * np.sin(xx / 37.0 + rng.uniform(0, 6)) * np.cos(yy / 29.0 + rng.uniform(0, 6)) + 0.001 * xx
                   for _ in range(N)]).astype(np.float32)
    pred = (gt * rng.normal(1.05, 0.03, (N, H, W))).astype(np.float32)
    pred[rng.random((N, H, W)) < 0.01] = 2.5
    gt[rng.random((N, H, W)) < 0.002] = 0.0
    blocks = rng.integers(0, 11, (N, -(-H // 32), -(-W // 32))) * 20
    mask = np.repeat(np.repeat(blocks, 32, axis=1), 32, axis=2)[:, :H, :W].astype(np.int32)
    return torch.from_numpy(gt).cuda()[:, None], torch.from_numpy(pred).cuda()[:, None], torch.from_numpy(mask).cuda()[:, None]


def sets_for(N, H, W, sets=None):
    return sets if sets is not None else max(2, min(24, -(-int(2.5 * 256e6) // (N * H * W * 12))))


def time_stats(N, H, W, iters=24, sets=None):
    import torch
    from polardepth import depth_eval as de
    from polardepth import ops
    from polardepth._lib import lib, check, ptr, stream_ptr
    from manydepth.evaluation import _MATERIAL_GREY
    if not torch.cuda.is_available():
        raise RuntimeError("bench_depth_stats needs the GPU; there is no CPU fallback")
    sets = sets_for(N, H, W, sets)
    data = [make_set(N, H, W, s) for s in range(sets)]
    names, table = de.class_table(de.DEFAULT_CLASSES)
    K = len(names)
    edges = de.edges("cuda")
    rec = torch.empty((N, K, de.RECORD_BYTES), dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(lib.pd_depth_stats_workspace(N, H, W, K)), dtype=torch.uint8, device="cuda")

    def unscaled(i):
        gt, pred, mask = data[i % sets]
        check(lib.pd_depth_stats(ptr(gt), ptr(pred), ptr(mask), table, K, None, ptr(edges), None, ptr(rec), ptr(ws), ws.numel(),
                                 N, H, W, 0.1, 2.0, stream_ptr()), "pd_depth_stats")

    def scaled(i):
        gt, pred, mask = data[i % sets]
        de.depth_stats(pred, gt, mask=mask, median_scaling="numpy")

    def metrics(i):                  # the 11 launch pairs of Evaluation.test on one batch
        gt, pred, mask = data[i % sets]
        for o in ["all"] + list(_MATERIAL_GREY):
            ops.depth_metrics(gt, pred, 0.1, 2.0, mask=None if o == "all" else mask, mask_value=_MATERIAL_GREY.get(o, 0))

    out = []
    timed = {}
    for what, call in (("depth_metrics_x11", metrics), ("depth_stats", unscaled), ("depth_stats_median_scaled", scaled)):
        for i in range(sets):
            call(i)
        torch.cuda.synchronize()
        timed[what] = _median_ms(call, iters)
    pooled = de.DepthStats(rec, names).pooled().cpu().numpy()
    for what, how in (("depth_stats", None), ("depth_stats_median_scaled", "numpy")):
        ms, ms_min, ms_max = timed[what]
        moved = N * H * W * BYTES_PER_PIXEL[how]
        copy_ms, copy_gbps = _copy_rate(moved, sets, iters)
        gbps = moved / (ms * 1e-3) / 1e9
        dm = timed["depth_metrics_x11"]
        out.append({"op": what, "N": N, "H": H, "W": W, "K": K, "sets": sets, "bytes": moved, "ms": round(ms, 4),
                    "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4), "GBps": round(gbps, 1), "copy_ms": round(copy_ms, 4),
                    "copy_GBps": round(copy_gbps, 1), "fraction_of_copy": round(gbps / copy_gbps, 3),
                    "depth_metrics_x11_ms": round(dm[0], 4), "depth_metrics_x11_ms_min": round(dm[1], 4),
                    "ratio_to_depth_metrics_x11": round(ms / dm[0], 3), "abs_rel_all": round(float(pooled[0, 0]), 5),
                    "pixels_all": int(pooled[0, 12])})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--sets", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_stats.log"), help="the log; '' = print only")
    args = ap.parse_args()
    log = open(args.out, "w") if args.out else None
    for N, H, W in SIZES:
        for row in time_stats(N, H, W, args.iters, args.sets):
            line = json.dumps(row)
            print(line, flush=True)
            if log:
                log.write(line + "\n")
                log.flush()
    if log:
        log.close()
