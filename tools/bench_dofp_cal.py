"""Super-pixel calibration of DoFP frames (polardepth/calibration.py, csrc/dofp_cal.hip) at the sensor's size: 2048x2448
frames of an IMX250MZR, B = 16, uint8 / uint16 (12-bit) / float32, per-cell matrices and per-pixel gains.

``--device``  ms per call of ``pd_dofp_calibrate`` with HIP events, warm: one event pair per call, median of ``--iters`` calls,
              every call on another of ``--sets`` rotating buffer sets (sized past the 256 MB Infinity Cache; outputs are
              allocated once and reused).  GB/s from the algorithm's own byte count -- H2 W2 (16 + 4 + B (sizeof(T) + 4)) for
              the matrices, (4 + 4 + B (sizeof(T) + 4)) for the gains: calibration data read once, every frame read once and
              written once -- next to the rate of a device copy that moves the SAME number of bytes (half read, half written;
              rotating buffers, the same timing) and the ratio of the two.  The same three numbers for ``pd_dofp_demosaic``
              (bilinear) on the same frames in the same run: the neighbouring kernel of the data path, as a yardstick.
``--fit``     ms for ``calibration.fit`` on N = 36 uint16 flat-field frames (moments + solve + the host's 3x3 inverse and its
              one device read; host clock around a synchronised call) and for its two kernels alone with HIP events.
``--numpy``   ms for ONE frame on one core with plain NumPy (the definition as tests/dofp_cal_ref.py states it); no GPU needed.
Without a flag everything runs.  One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAME = (2048, 2448)
NP_DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
CODES = {"u8": 0, "u16": 1, "f32": 2}


def apply_bytes(dtype, kind, B, frame=FRAME):
    per_pixel = (16 + 4 if kind == "cell" else 4 + 4) + B * (np.dtype(NP_DTYPES[dtype]).itemsize + 4)
    return frame[0] * frame[1] * per_pixel


def make_frames(dtype, B, seed=0, frame=FRAME):
    rng = np.random.default_rng(seed)
    if dtype == "f32":
        return (rng.random((B,) + frame, dtype=np.float32) * 4095.0)
    return rng.integers(0, 256 if dtype == "u8" else 4096, (B,) + frame).astype(NP_DTYPES[dtype])


def make_calibration(kind, seed=1, frame=FRAME):
    rng = np.random.default_rng(seed)
    dark = rng.uniform(0.0, 8.0, frame).astype(np.float32)
    if kind == "pixel":
        return dark, rng.uniform(0.85, 1.15, frame).astype(np.float32)
    proj = np.where(np.eye(4, dtype=bool), 0.75, -0.25).astype(np.float32)
    return dark, (proj + rng.normal(0, 0.05, (frame[0] // 2, frame[1] // 2, 4, 4)).astype(np.float32))


def time_numpy(dtype, kind, items=3):
    import dofp_cal_ref
    m = make_frames(dtype, 1)
    dark, gain = make_calibration(kind)
    ts = []
    for _ in range(items):
        t0 = time.perf_counter()
        dofp_cal_ref.calibrate(m, dark, gain)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"path": "numpy", "op": "apply", "dtype": dtype, "kind": kind, "frame": list(FRAME),
            "ms_per_item": round(ts[len(ts) // 2], 1), "ms_min": round(ts[0], 1)}


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


def _sets_for(moved, sets):
    return sets if sets is not None else max(2, min(8, -(-int(2.5 * 256e6) // moved)))


def time_apply(dtype, kind, B=16, iters=24, sets=None):
    import torch
    from polardepth._lib import lib, check, ptr, stream_ptr
    if not torch.cuda.is_available():
        raise RuntimeError("bench_dofp_cal --device needs the GPU; there is no CPU fallback")
    moved = apply_bytes(dtype, kind, B)
    sets = _sets_for(moved, sets)
    frames = make_frames(dtype, B)
    dark, gain = (torch.from_numpy(a).cuda() for a in make_calibration(kind))
    ins = [torch.from_numpy(np.roll(frames, s, axis=0)).cuda() for s in range(sets)]
    outs = [torch.empty((B,) + FRAME, dtype=torch.float32, device="cuda") for _ in range(sets)]
    code = 0 if kind == "cell" else 1

    def call(i):
        check(lib.pd_dofp_calibrate(ptr(ins[i % sets]), CODES[dtype], ptr(dark), ptr(gain), code, ptr(outs[i % sets]), B,
                                    FRAME[0], FRAME[1], stream_ptr()), "pd_dofp_calibrate")

    for i in range(sets):
        call(i)
    torch.cuda.synchronize()
    ms, ms_min, ms_max = _median_ms(call, iters)
    copy_ms, copy_gbps = _copy_rate(moved, sets, iters)
    gbps = moved / (ms * 1e-3) / 1e9
    return {"path": "device", "op": "apply", "dtype": dtype, "kind": kind, "B": B, "frame": list(FRAME), "sets": sets,
            "bytes": moved, "ms": round(ms, 4), "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4),
            "ms_per_item": round(ms / B, 4), "GBps": round(gbps, 1), "copy_ms": round(copy_ms, 4),
            "copy_GBps": round(copy_gbps, 1), "fraction_of_copy": round(gbps / copy_gbps, 3)}


def time_demosaic(dtype, B=16, iters=24, sets=None):
    """pd_dofp_demosaic (bilinear) on the same frames: sizeof(T) + 16 bytes per mosaic pixel"""
    import torch
    from polardepth._lib import lib, check, ptr, stream_ptr
    moved = B * FRAME[0] * FRAME[1] * (np.dtype(NP_DTYPES[dtype]).itemsize + 16)
    sets = _sets_for(moved, sets)
    frames = make_frames(dtype, B)
    ins = [torch.from_numpy(np.roll(frames, s, axis=0)).cuda() for s in range(sets)]
    outs = [torch.empty((B, 4) + FRAME, dtype=torch.float32, device="cuda") for _ in range(sets)]
    layout = (ctypes.c_int * 4)(2, 1, 3, 0)

    def call(i):
        check(lib.pd_dofp_demosaic(ptr(ins[i % sets]), CODES[dtype], ptr(outs[i % sets]), 1, layout, B, FRAME[0], FRAME[1],
                                   stream_ptr()), "pd_dofp_demosaic")

    for i in range(sets):
        call(i)
    torch.cuda.synchronize()
    ms, ms_min, ms_max = _median_ms(call, iters)
    copy_ms, copy_gbps = _copy_rate(moved, sets, iters)
    gbps = moved / (ms * 1e-3) / 1e9
    return {"path": "device", "op": "demosaic_bilinear", "dtype": dtype, "B": B, "frame": list(FRAME), "sets": sets,
            "bytes": moved, "ms": round(ms, 4), "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4), "GBps": round(gbps, 1),
            "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbps, 1), "fraction_of_copy": round(gbps / copy_gbps, 3)}


def time_fit(N=36, iters=5):
    import torch
    from polardepth import calibration as cal
    if not torch.cuda.is_available():
        raise RuntimeError("bench_dofp_cal --fit needs the GPU; there is no CPU fallback")
    rng = np.random.default_rng(2)
    deg = [180.0 * k / N for k in range(N)]
    a = np.deg2rad(np.asarray(deg))
    # the flat-field series of an IMX250MZR with per-pixel gains, in 64 x 64 tiles: the arithmetic does not depend on the values
    yy, xx = np.mgrid[0:64, 0:64]
    theta = np.deg2rad(np.asarray([90.0, 45.0, 135.0, 0.0]))[2 * (yy & 1) + (xx & 1)]
    base = 1500.0 * rng.uniform(0.85, 1.15, (1, 64, 64)) * (1.0 + np.cos(2 * a[:, None, None] - 2 * theta[None]))
    tiled = np.tile(np.rint(base).astype(np.uint16), (1, FRAME[0] // 64, FRAME[1] // 64 + 1))[:, :, :FRAME[1]]
    frames = torch.from_numpy(np.ascontiguousarray(tiled)).cuda()
    dark = torch.zeros(FRAME, dtype=torch.float32, device="cuda")
    w = cal.fit_weights(deg)
    cal.fit(frames, deg, dark=dark)                       # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        c = cal.fit(frames, deg, dark=dark)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    # the two kernels alone: the library calls, with every argument already on the device and every output allocated
    from polardepth._lib import lib, check, ptr, stream_ptr
    M = cal.frame_moments(frames, w, dark)
    w_dev = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    rinv = np.ascontiguousarray(np.linalg.inv((w[:, :, None] * w[:, None, :]).sum(axis=0)) / 1500.0).reshape(9)
    a_nom = np.ascontiguousarray(cal.nominal_matrix()).reshape(12)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    gain = torch.empty((FRAME[0] // 2, FRAME[1] // 2, 4, 4), dtype=torch.float32, device="cuda")
    quality = torch.empty((FRAME[0] // 2, FRAME[1] // 2), dtype=torch.float32, device="cuda")

    def moments(i):
        check(lib.pd_frame_moments(ptr(frames), CODES["u16"], ptr(dark), ptr(w_dev), ptr(M), N, 3, FRAME[0], FRAME[1], 0,
                                   stream_ptr()), "pd_frame_moments")

    def solve(i):
        check(lib.pd_dofp_cal_solve(ptr(M), dp(rinv), dp(a_nom), 1e-3, ptr(gain), ptr(quality), FRAME[0], FRAME[1],
                                    stream_ptr()), "pd_dofp_cal_solve")

    moments(0), solve(0)
    torch.cuda.synchronize()
    mom_ms, _, _ = _median_ms(moments, 4 * iters)
    sol_ms, _, _ = _median_ms(solve, 4 * iters)
    px = FRAME[0] * FRAME[1]
    mom_bytes, sol_bytes = px * (N * 2 + 4 + 2 * 3 * 8), px * (3 * 8 + 16 + 1)
    return {"path": "device", "op": "fit", "N": N, "dtype": "u16", "frame": list(FRAME), "fit_ms": round(ts[len(ts) // 2], 2),
            "fit_ms_min": round(ts[0], 2), "moments_ms": round(mom_ms, 4), "moments_GBps": round(mom_bytes / mom_ms / 1e6, 1),
            "solve_ms": round(sol_ms, 4), "solve_GBps": round(sol_bytes / sol_ms / 1e6, 1), "bad_cells": c.bad_cells}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--dtype", choices=sorted(NP_DTYPES), action="append", help="default: all three")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--sets", type=int, default=None)
    args = ap.parse_args()
    every = not (args.numpy or args.device or args.fit)
    for dt in args.dtype or ["u8", "u16", "f32"]:
        for kind in ("cell", "pixel"):
            if args.numpy or every:
                print(json.dumps(time_numpy(dt, kind)), flush=True)
            if args.device or every:
                print(json.dumps(time_apply(dt, kind, args.batch, args.iters, args.sets)), flush=True)
        if args.device or every:
            print(json.dumps(time_demosaic(dt, args.batch, args.iters, args.sets)), flush=True)
    if args.fit or every:
        print(json.dumps(time_fit()), flush=True)
