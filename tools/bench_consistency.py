"""pd_depth_consistency (csrc/consistency.hip) at the evaluation's sizes: B = 12 at 320x480 and B = 16 at 512x640, F = 2 source
views, the twelve default classes, writing ``level`` and ``fused``.

ms per call with HIP events, warm: one event pair per call, median of ``--iters`` calls, every call on another of ``--sets``
rotating input sets (sized past the 256 MB Infinity Cache).  The call is the C entry point on preallocated records, outputs
and workspace.  GB/s from the algorithm's own byte count -- per pixel 4 (depth) + 4 (mask) + 4 F (every source map once) read
and F (level) + 4 (fused) written: 22 bytes at F = 2 -- next to the rate of a device copy that moves the SAME number of bytes
(half read, half written; rotating buffers, the same timing).  The yardstick, in the same run on the same sets: the same
figures written with torch ops (``torch_consistency``: two ``grid_sample`` calls per view, the levels, and masked reductions
and a ``bincount`` per class; fp32, on the device, records left there).  One JSON line per measurement, printed and written
to ``--out`` (default: profiles/consistency.log)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

from bench_depth_stats import _copy_rate, _median_ms      # noqa: E402  (tools/ is the script's directory)

SIZES = ((12, 320, 480), (16, 512, 640))
F = 2


def bytes_per_pixel(f):
    return 4 + 4 + 4 * f + f + 4


def make_set(N, H, W, seed):
    """One input set on the device: a smooth surface seen from F + 1 cameras a few centimetres apart (each source map is the
    current one plus a few per cent of block noise, which is all the timing needs), a few holes, the instance mask in 32x32
    blocks of the eleven grey values, the camera of the synthetic items."""
    import torch
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    d0 = np.stack([1.0 + 0.3 * np.sin(xx / 37.0 + rng.uniform(0, 6)) * np.cos(yy / 29.0 + rng.uniform(0, 6)) + 0.001 * xx
                   for _ in range(N)]).astype(np.float32)
    noise = rng.choice(np.float32([1, 1, 1.005, 0.99, 1.03]), (N, F, -(-H // 8), -(-W // 8)))
    ds = d0[:, None] * np.repeat(np.repeat(noise, 8, 2), 8, 3)[:, :, :H, :W]
    d0[rng.random(d0.shape) < 0.002] = 0.0
    ds[rng.random(ds.shape) < 0.002] = 0.0
    T = np.tile(np.eye(4, dtype=np.float32), (N, F, 1, 1))
    T[:, :, :3, 3] = rng.uniform(-0.03, 0.03, (N, F, 3))
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 0.65 * W; K[0, 2] = W / 2; K[1, 2] = H / 2
    Ks = np.tile(K, (N, 1, 1))
    blocks = rng.integers(0, 11, (N, -(-H // 32), -(-W // 32))) * 20
    mask = np.repeat(np.repeat(blocks, 32, axis=1), 32, axis=2)[:, :H, :W].astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dev(d0), dev(ds.astype(np.float32)), dev(T), dev(Ks), dev(np.linalg.inv(Ks).astype(np.float32)), dev(mask)


def torch_consistency(d0, ds, T, K, inv_K, mask, classes, min_depth=0.1, max_depth=2.0, taus=((4, 0.04), (2, 0.02), (1, 0.01))):
    """The figures of pd_depth_consistency with torch ops, fp32: per image and class n, the three level counts, the five reason
    counts (no `absent`, no `filtered`: neither input is given), the four sums and the 256-bin histogram."""
    import torch
    import torch.nn.functional as Fn
    N, Fv, H, W = ds.shape
    yy, xx = torch.meshgrid(torch.arange(H, device=d0.device, dtype=torch.float32),
                            torch.arange(W, device=d0.device, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xx, yy, torch.ones_like(xx)], 0).reshape(1, 3, -1)
    rays = inv_K[:, :3, :3] @ pix                                                      # [N,3,HW]
    valid0 = ((d0 >= min_depth) & (d0 <= max_depth)).reshape(N, -1)
    ok_src = ((ds >= min_depth) & (ds <= max_depth)).float()
    outcome, terms, levels = [], [], []
    for f in range(Fv):
        P = (K @ T[:, f])[:, :3]
        h = P[:, :, :3] @ (rays * d0.reshape(N, 1, -1)) + P[:, :, 3:]
        hz = h[:, 2] + 1e-7
        u, v = h[:, 0] / hz, h[:, 1] / hz
        inside = (hz > 1e-3) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        grid = torch.stack([2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1], -1).reshape(N, H, W, 2)
        d1 = Fn.grid_sample(ds[:, f:f + 1], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(N, -1)
        taps = Fn.grid_sample(ok_src[:, f:f + 1], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(N, -1)
        Pi = (K @ torch.linalg.inv(T[:, f]))[:, :3]
        r1 = inv_K[:, :3, :3] @ torch.stack([u, v, torch.ones_like(u)], 1)
        h2 = Pi[:, :, :3] @ (r1 * d1[:, None]) + Pi[:, :, 3:]
        hz2 = h2[:, 2] + 1e-7
        e2 = (h2[:, 0] / hz2 - pix[:, 0]) ** 2 + (h2[:, 1] / hz2 - pix[:, 1]) ** 2
        e_rel = (hz2 - d0.reshape(N, -1)).abs() / d0.reshape(N, -1)
        hole = taps < 0.9999
        out = torch.full_like(u, 4, dtype=torch.int64)                                 # 0 invalid, 1 outside, 2 hole, 4 compared
        out = torch.where(~(hz2 > 1e-3), 1, out)
        out = torch.where(hole, 2, out)
        out = torch.where(~inside, 1, out)
        out = torch.where(~valid0, 0, out)
        outcome.append(out)
        terms.append(torch.stack([e2.sqrt(), e_rel, e2, e_rel * e_rel], -1))
        levels.append(torch.stack([(e2 < a * a) & (e_rel < b) for a, b in taus], -1))
    outcome, terms, levels = torch.stack(outcome, 1), torch.stack(terms, 1), torch.stack(levels, 1)      # [N,F,HW,..]
    cmp_ = outcome == 4
    bins = (terms[..., 1] * 1024).floor().clamp(0, 255).nan_to_num(255).long()
    m = mask.reshape(N, 1, -1)
    rec = []
    img = torch.arange(N, device=d0.device).view(N, 1, 1)
    for _, rng in classes:
        cl = torch.ones_like(m, dtype=torch.bool) if rng is None else (m >= rng[0]) & (m <= rng[1])
        sel = cmp_ & cl
        n = sel.sum((1, 2))
        lv = (levels & sel[..., None]).sum((1, 2))
        reasons = torch.stack([((outcome == c) & cl).sum((1, 2)) for c in (0, 1, 2)], -1)
        sums = torch.where(sel[..., None], terms, torch.zeros_like(terms)).sum((1, 2))
        hist = torch.bincount((img * 256 + bins)[sel], minlength=N * 256).view(N, 256)
        rec.append((n, lv, reasons, sums, hist))
    return rec


def sets_for(N, H, W, sets=None):
    return sets if sets is not None else max(2, min(24, -(-int(2.5 * 256e6) // (N * H * W * bytes_per_pixel(F)))))


def time_consistency(N, H, W, iters=24, sets=None):
    import ctypes
    import torch
    from polardepth import consistency_eval as ce
    from polardepth._lib import lib, check, ptr, stream_ptr
    if not torch.cuda.is_available():
        raise RuntimeError("bench_consistency needs the GPU; there is no CPU fallback")
    sets = sets_for(N, H, W, sets)
    data = [make_set(N, H, W, s) for s in range(sets)]
    names, table = ce.class_table(ce.DEFAULT_CLASSES)
    K = len(names)
    tau_px, tau_rel = (ctypes.c_double * 3)(4, 2, 1), (ctypes.c_double * 3)(0.04, 0.02, 0.01)
    rec = torch.empty((N, K, ce.RECORD_BYTES), dtype=torch.uint8, device="cuda")
    level = torch.empty((N, F, H, W), dtype=torch.uint8, device="cuda")
    fused = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.pd_depth_consistency_workspace(N, H, W, K)), dtype=torch.uint8, device="cuda")

    def kernel(i):
        d0, ds, T, Km, iK, mask = data[i % sets]
        check(lib.pd_depth_consistency(ptr(d0), ptr(ds), ptr(T), ptr(Km), ptr(iK), None, None, ptr(mask), table, K, 0.1, 2.0,
                                       tau_px, tau_rel, 4, ptr(level), None, ptr(fused), ptr(rec), ptr(ws), ws.numel(), N, F, H,
                                       W, stream_ptr()), "pd_depth_consistency")

    def torch_ops(i):
        d0, ds, T, Km, iK, mask = data[i % sets]
        torch_consistency(d0, ds, T, Km, iK, mask, ce.DEFAULT_CLASSES)

    timed = {}
    for what, call in (("torch_ops", torch_ops), ("depth_consistency", kernel)):
        for i in range(sets):
            call(i)
        torch.cuda.synchronize()
        timed[what] = _median_ms(call, iters)
    # the two agree on what they count (fp32 against fp64: a pair near a threshold may change sides)
    kernel(0)
    st = ce.ConsistencyStats(rec, names)
    ref = torch_consistency(*data[0], ce.DEFAULT_CLASSES)
    n_kernel, n_torch = int(st.n[:, 0].sum()), int(ref[0][0].sum())
    pooled = st.pooled().cpu().numpy()
    ms, ms_min, ms_max = timed["depth_consistency"]
    moved = N * H * W * bytes_per_pixel(F)
    copy_ms, copy_gbps = _copy_rate(moved, sets, iters)
    gbps = moved / (ms * 1e-3) / 1e9
    tm = timed["torch_ops"]
    return [{"op": "depth_consistency", "N": N, "F": F, "H": H, "W": W, "K": K, "sets": sets, "bytes": moved,
             "ms": round(ms, 4), "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4), "GBps": round(gbps, 1),
             "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbps, 1), "fraction_of_copy": round(gbps / copy_gbps, 3),
             "torch_ops_ms": round(tm[0], 4), "torch_ops_ms_min": round(tm[1], 4), "ratio_to_torch_ops": round(ms / tm[0], 4),
             "compared_all": n_kernel, "compared_all_torch_ops": n_torch, "tight_share_all": round(float(pooled[0, 3]), 5),
             "median_rel_percent_all": round(float(pooled[0, 5]), 5)}]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--sets", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency.log"), help="the log; '' = print only")
    args = ap.parse_args()
    log = open(args.out, "w") if args.out else None
    for N, H, W in SIZES:
        for row in time_consistency(N, H, W, args.iters, args.sets):
            line = json.dumps(row)
            print(line, flush=True)
            if log:
                log.write(line + "\n")
                log.flush()
    if log:
        log.close()
