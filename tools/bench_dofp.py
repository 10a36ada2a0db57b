"""Demosaic of interleaved polarizer frames (polardepth/dofp.py, csrc/dofp.hip) at the sensor's size: one 2048x2448 frame of
an IMX250MZR per item, B = 16, uint8 / uint16 / float32, super-pixel and bilinear.

``--device``  ms per call of ``demosaic`` with HIP events, warm: one event pair per call, median of ``--iters`` calls, every
              call on another of ``--sets`` rotating buffer sets (sized past the 256 MB Infinity Cache by default, as
              tools/bench_polar.py and tools/bench_resize.py do; the output of a set is allocated once and reused, so the
              figure holds no allocation).  GB/s from the bytes the algorithm needs per mosaic pixel -- the frame read once,
              the planes written once: bilinear 1 + 16 / 2 + 16 / 4 + 16, super-pixel 2 / 4 / 8 -- over that time.
              ``--copy-gbps X``: the 1:1 copy rate tools/membench5.hip reaches on the same machine; adds the fraction of it.
``--numpy``   ms for ONE frame on one core with plain NumPy (padding + shifted slices in float64, or strided slices): what a
              loader worker would pay; no GPU needed.
Without either flag both run.  One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

FRAME = (2048, 2448)
LAYOUT = (2, 1, 3, 0)
NP_DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
MODES = ("superpixel", "bilinear")


def bytes_per_pixel(dtype, mode):
    elem = np.dtype(NP_DTYPES[dtype]).itemsize
    return elem + 16 if mode == "bilinear" else 2 * elem


def make_frames(dtype, B, seed=0):
    rng = np.random.default_rng(seed)
    hi = 256 if dtype == "u8" else 4096
    a = rng.integers(0, hi, (B,) + FRAME)
    return a.astype(np.float32) if dtype == "f32" else a.astype(NP_DTYPES[dtype])


def numpy_demosaic(m, mode):
    sites = [(LAYOUT.index(p) >> 1, LAYOUT.index(p) & 1) for p in range(4)]
    if mode == "superpixel":
        return np.stack([m[r::2, c::2] for r, c in sites])
    H2, W2 = m.shape
    pad = np.pad(m.astype(np.float64), 1, mode="reflect")
    at = lambda dy, dx: pad[1 + dy:1 + dy + H2, 1 + dx:1 + dx + W2]
    cand = [at(0, 0), (at(0, -1) + at(0, 1)) * 0.5, (at(-1, 0) + at(1, 0)) * 0.5,
            ((at(-1, -1) + at(-1, 1)) + (at(1, -1) + at(1, 1))) * 0.25]
    out = np.empty((4, H2, W2), np.float32)
    for p, (r, c) in enumerate(sites):
        for dy in (0, 1):
            for dx in (0, 1):
                out[p, (r + dy) % 2::2, (c + dx) % 2::2] = cand[2 * dy + dx][(r + dy) % 2::2, (c + dx) % 2::2]
    return out


def time_numpy(dtype, mode, items=5):
    m = make_frames(dtype, 1)[0]
    numpy_demosaic(m, mode)
    ts = []
    for _ in range(items):
        t0 = time.perf_counter()
        numpy_demosaic(m, mode)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"path": "numpy", "dtype": dtype, "mode": mode, "frame": list(FRAME), "ms_per_item": round(ts[len(ts) // 2], 3),
            "ms_min": round(ts[0], 3)}


def time_device(dtype, mode, B=16, iters=24, sets=None, copy_gbps=None):
    import torch
    from polardepth import dofp
    from polardepth._lib import lib, check, ptr, stream_ptr
    if not torch.cuda.is_available():
        raise RuntimeError("bench_dofp --device needs the GPU; there is no CPU fallback")
    moved = B * FRAME[0] * FRAME[1] * bytes_per_pixel(dtype, mode)
    if sets is None:                       # enough rotating sets to exceed 2.5x the Infinity Cache, at least two
        sets = max(2, min(8, -(-int(2.5 * 256e6) // moved)))
    frames = make_frames(dtype, B)
    ins = [torch.from_numpy(np.roll(frames, s, axis=0)).cuda() for s in range(sets)]
    outs = [dofp.demosaic(x, LAYOUT, mode) for x in ins]        # warm-up of every buffer, and the outputs to reuse
    layout = (ctypes.c_int * 4)(*LAYOUT)
    code, dt = dofp.MODES[mode], {"u8": 0, "u16": 1, "f32": 2}[dtype]

    def call(i):
        check(lib.pd_dofp_demosaic(ptr(ins[i % sets]), dt, ptr(outs[i % sets]), code, layout, B, FRAME[0], FRAME[1], stream_ptr()),
              "pd_dofp_demosaic")

    for i in range(sets):
        call(i)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (e0, e1) in enumerate(evs):
        e0.record()
        call(i)
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    ms = ts[iters // 2]
    res = {"path": "device", "dtype": dtype, "mode": mode, "B": B, "frame": list(FRAME), "sets": sets,
           "bytes_per_pixel": bytes_per_pixel(dtype, mode), "ms": round(ms, 4), "ms_min": round(ts[0], 4),
           "ms_max": round(ts[-1], 4), "ms_per_item": round(ms / B, 4), "GBps": round(moved / (ms * 1e-3) / 1e9, 1)}
    if copy_gbps:
        res["copy_GBps"] = copy_gbps
        res["fraction_of_copy"] = round(res["GBps"] / copy_gbps, 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--dtype", choices=sorted(NP_DTYPES), action="append", help="default: all three")
    ap.add_argument("--mode", choices=MODES, action="append", help="default: both")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--sets", type=int, default=None)
    ap.add_argument("--copy-gbps", type=float, default=None)
    args = ap.parse_args()
    both = not (args.numpy or args.device)
    for dt in args.dtype or ["u8", "u16", "f32"]:
        for mode in args.mode or MODES:
            if args.numpy or both:
                print(json.dumps(time_numpy(dt, mode)), flush=True)
            if args.device or both:
                print(json.dumps(time_device(dt, mode, args.batch, args.iters, args.sets, args.copy_gbps)), flush=True)
