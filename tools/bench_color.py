"""The colour path of one batch on the device next to the PIL path of one item on one core of the same box.

Device: HIP-event time of ``polardepth.color.color_pyramid`` for B = 16 decoded 832x1088 frames -> 512x640, 4 scales, every
sample augmented (seeded ColorJitter draws), warm, median of ``--iters`` calls; and of its jitter kernel alone
(pd_color_jitter_u8: reduce + apply at scale 0, fp32 out).  GB/s are the algorithmic bytes over that time: the bytes each
pass has to read and write, computed from the shapes below -- not measured traffic.
Host: the colour loop of ``HAMMER_Dataset._load_item`` (four LANCZOS resizes, ColorJitter of every scale, / 255) on the same
frame size, one thread, median of ``--host_iters`` items, plain and augmented.

    python tools/bench_color.py --out profiles/color_pipeline.log
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))
from manydepth import datasets  # noqa: E402
from polardepth import color as pdcolor  # noqa: E402


def pyramid_bytes(B, Hf, Wf, H, W, scales, augmented=True):
    """Bytes the passes of color_pyramid read + write.  Per scale: horizontal resize (in -> Hs x Wd), vertical resize
    (-> Hd x Wd), the plain conversion (3 B in, 12 B out per pixel) and, augmented, the jitter (3 B read by the reduction,
    3 B read + 12 B written by the apply pass)."""
    total, hs, ws = 0, Hf, Wf
    for s in range(scales):
        hd, wd = H >> s, W >> s
        total += 3 * B * (hs * ws + hs * wd)          # horizontal pass
        total += 3 * B * (hs * wd + hd * wd)          # vertical pass
        total += B * hd * wd * (3 + 12)               # color
        if augmented:
            total += B * hd * wd * (3 + 3 + 12)       # color_aug
        hs, ws = hd, wd
    return total


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[len(ts) // 2], ts[0], ts[-1]


def device_rows(args):
    if not torch.cuda.is_available():
        raise RuntimeError("bench_color.py needs the MI355X: there is no CPU fallback for the device figures")
    B, (Hf, Wf), (H, W), S = args.batch, args.frame, args.size, args.scales
    g = torch.Generator().manual_seed(0)
    raw = torch.randint(0, 256, (B, 3, Hf, Wf), dtype=torch.uint8, generator=g).cuda()
    random.seed(0)
    rows = torch.from_numpy(np.stack([pdcolor.pack_jitter(datasets.color_jitter_params()) for _ in range(B)])).cuda()
    out = []
    ms, lo, hi = median_ms(lambda: pdcolor.color_pyramid(raw, rows, (H, W), S), args.iters)
    nbytes = pyramid_bytes(B, Hf, Wf, H, W, S)
    out.append({"what": "color_pyramid (device)", "B": B, "frame": [Hf, Wf], "size": [H, W], "scales": S, "augmented": B,
                "iters": args.iters, "ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                "ms_per_item": round(ms / B, 4), "items_per_s": round(B / (ms * 1e-3), 1),
                "algorithmic_MB": round(nbytes / 1e6, 1), "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1)})
    from polardepth.resize import resize_lanczos_u8
    s0 = resize_lanczos_u8(raw, (H, W))
    for what, p, bpp in (("pd_color_jitter_u8 reduce + apply, scale 0", rows, 3 + 3 + 12),
                         ("pd_color_jitter_u8 plain conversion, scale 0", None, 3 + 12)):
        ms, lo, hi = median_ms(lambda: pdcolor.color_jitter_u8(s0, p), args.iters)
        nbytes = B * H * W * bpp
        out.append({"what": what, "B": B, "size": [H, W], "iters": args.iters, "ms": round(ms, 4), "ms_min": round(lo, 4),
                    "ms_max": round(hi, 4), "bytes_px": bpp, "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1)})
    return out


def host_rows(args):
    """The PIL colour loop of the loader, one item at a time on one thread."""
    from PIL import Image
    torch.set_num_threads(1)
    (Hf, Wf), (H, W), S = args.frame, args.size, args.scales
    rng = np.random.default_rng(0)
    frame = Image.fromarray(rng.integers(0, 256, (Hf, Wf, 3), dtype=np.uint8))
    to_t = lambda im: torch.from_numpy(np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0)
    random.seed(0)

    def item(jitter):
        prev, res = frame, {}
        for s in range(S):
            prev = prev.resize((W >> s, H >> s), Image.LANCZOS)
            res[("color", 0, s)] = to_t(prev)
            res[("color_aug", 0, s)] = to_t(datasets.apply_color_jitter(prev, jitter)) if jitter else res[("color", 0, s)]
        return res

    out = []
    for what, aug in (("PIL colour loop, plain item (host, 1 thread)", False), ("PIL colour loop, augmented item (host, 1 thread)", True)):
        item(datasets.color_jitter_params() if aug else None)
        ts = []
        for _ in range(args.host_iters):
            j = datasets.color_jitter_params() if aug else None
            t0 = time.perf_counter()
            item(j)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        out.append({"what": what, "frame": [Hf, Wf], "size": [H, W], "scales": S, "iters": args.host_iters,
                    "ms_per_item": round(ts[len(ts) // 2], 2), "ms_min": round(ts[0], 2), "ms_max": round(ts[-1], 2)})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frame", type=int, nargs=2, default=[832, 1088], metavar=("HF", "WF"))
    ap.add_argument("--size", type=int, nargs=2, default=[512, 640], metavar=("H", "W"))
    ap.add_argument("--scales", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host_iters", type=int, default=7)
    ap.add_argument("--host_only", action="store_true", help="skip the device figures (they need the GPU)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    rows = ([] if args.host_only else device_rows(args)) + host_rows(args)
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
