"""LANCZOS resize of one item's four polarizer planes, 832x1088 -> 512x612 (HAMMER's frames at the training size): what a
loader worker pays with PIL against the device passes of polardepth/resize.py.

``--pil``     ms per item on one core: four ``Image.resize((612, 512), Image.LANCZOS)`` calls in mode I;16 (``--dtype u16``),
              F (``f32``) or L (``u8``); no GPU needed.
``--device``  ms per batch and per item of ``resize_lanczos`` (horizontal + vertical pass) with HIP events, warm: one event
              pair per call, median of ``--iters`` calls, every call on another of ``--sets`` rotating input buffers (sized
              past the 256 MB Infinity Cache by default, as tools/bench_polar.py does), so the reads come from HBM as they do
              in a training step.  The two launches of a call are inside one event pair, so the figure holds the launch gap
              between them.
Without either flag both run.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

SRC, DST = (832, 1088), (512, 612)
NP_DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def make_item(dtype, seed=0):
    """four planes of a smooth field with noise: 8-bit, 12-bit counts or floats in the 12-bit range"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:SRC[0], 0:SRC[1]].astype(np.float64)
    hi = 255.0 if dtype == "u8" else 4095.0
    field = hi * (0.5 + 0.3 * np.sin(xx / 41.0 + seed) * np.cos(yy / 37.0))
    planes = np.stack([field * (1 + 0.2 * np.cos(a + xx / 90.0)) for a in (0.0, 0.79, 1.57, 2.36)])
    planes = np.clip(planes + rng.normal(0, hi / 170.0, planes.shape), 0, hi)
    return planes.astype(np.float32) if dtype == "f32" else np.rint(planes).astype(NP_DTYPES[dtype])


def time_pil(dtype, items=5):
    from PIL import Image
    planes = make_item(dtype)
    imgs = [Image.fromarray(p) for p in planes]
    resize = lambda: [im.resize((DST[1], DST[0]), Image.LANCZOS) for im in imgs]
    resize()
    ts = []
    for _ in range(items):
        t0 = time.perf_counter()
        resize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"path": "PIL", "mode": imgs[0].mode, "src": list(SRC), "dst": list(DST), "planes": 4,
            "ms_per_item": round(ts[len(ts) // 2], 3), "ms_min": round(ts[0], 3)}


def time_device(dtype, B=16, iters=24, sets=None):
    import torch
    from polardepth import resize as pdresize
    elem = np.dtype(NP_DTYPES[dtype]).itemsize
    if sets is None:                       # enough rotating sets to exceed 2.5x the Infinity Cache
        per_set = B * 4 * SRC[0] * SRC[1] * elem
        sets = max(1, min(8, -(-int(2.5 * 256e6) // per_set)))
    xs = [torch.from_numpy(np.stack([make_item(dtype, seed=s)] * B)).cuda() for s in range(sets)]
    for x in xs:                           # table upload, allocator warm-up
        pdresize.resize_lanczos(x, DST)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (e0, e1) in enumerate(evs):
        e0.record()
        pdresize.resize_lanczos(xs[i % sets], DST)
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    ms = ts[iters // 2]
    moved = B * 4 * elem * (SRC[0] * SRC[1] + 2 * SRC[0] * DST[1] + DST[0] * DST[1])      # read, write + read between, write
    return {"path": "device", "dtype": dtype, "B": B, "src": list(SRC), "dst": list(DST), "planes": 4, "sets": sets,
            "ms": round(ms, 4), "ms_min": round(ts[0], 4), "ms_per_item": round(ms / B, 4),
            "GBps": round(moved / (ms * 1e-3) / 1e9, 1)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pil", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--dtype", choices=sorted(NP_DTYPES), action="append", help="default: u16 (may be given more than once)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--sets", type=int, default=None)
    args = ap.parse_args()
    both = not (args.pil or args.device)
    for dt in args.dtype or ["u16"]:
        if args.pil or both:
            print(json.dumps(time_pil(dt)), flush=True)
        if args.device or both:
            print(json.dumps(time_device(dt, args.batch, args.iters, args.sets)), flush=True)
