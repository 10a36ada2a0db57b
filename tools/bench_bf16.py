"""The opt-in bf16 training mode (opt.bf16 / ops.CONV_BF16) against the default step, in one process, on one GPU: eager
images/s and ms/step of both modes at BASELINE configs[2] (3 encoders, B = 16, 512x640 network input from 512x612 synthetic
frames) and at configs[4] (the attention variant), and the HIP-event time and TFLOP/s of every single-bf16 kernel label
against the 2.5 PF dense bf16 MFMA peak.  Prints one JSON line.  Reuses bench.build_trainer / bench.train_step.
    python tools/bench_bf16.py [--steps K] [--warmup W]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd")]

import torch  # noqa: E402

import bench  # noqa: E402

BF16_PEAK_TF = 2500.0


def _trainer(batch, attention):
    if attention:
        os.environ["PD_JOINT_ATTENTION"] = "1"
    try:
        tr = bench.build_trainer(batch, bench.H, bench.W, tempfile.mkdtemp(prefix="pd_bench_bf16_"))
    finally:
        os.environ.pop("PD_JOINT_ATTENTION", None)
    tr.set_train()
    return tr


def _timed(tr, batch, steps, warmup):
    for _ in range(warmup):
        bench.train_step(tr, batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = bench.train_step(tr, batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"images_per_s": round(batch[("color_aug", 0, 0)].shape[0] / dt, 3), "ms_per_step": round(dt * 1e3, 3),
            "final_loss": round(float(loss.detach()), 6)}


def _kernels(tr, batch, steps=2):
    """Per-label HIP-event time of the convolution launches (weight gradients and encoders serialised on one stream)."""
    from polardepth import ops
    from polardepth import functional as PF
    overlap, PF.USE_WGRAD_STREAM = PF.USE_WGRAD_STREAM, False
    enc, tr.encoder_streams = tr.encoder_streams, False
    ops.PROFILE = []
    try:
        for _ in range(steps):
            bench.train_step(tr, batch)
        torch.cuda.synchronize()
        prof = ops.PROFILE
    finally:
        ops.PROFILE = None
        PF.USE_WGRAD_STREAM = overlap
        tr.encoder_streams = enc
    by = {}
    for name, flops, e0, e1, _shape in prof:
        k = by.setdefault(name, [0.0, 0.0, 0])
        k[0] += flops; k[1] += e0.elapsed_time(e1) * 1e-3; k[2] += 1
    return {n: {"ms_per_step": round(v[1] / steps * 1e3, 3), "launches_per_step": v[2] // steps,
                "tflops": round(v[0] / v[1] / 1e12, 2)} for n, v in sorted(by.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=bench.BATCH)
    args = ap.parse_args()
    from polardepth import synthetic
    from polardepth import functional as PF
    PF.DropoutState.manual_seed(1234)
    batch = synthetic.make_batch(args.batch, bench.H, bench.W, frame_w=bench.FRAME_W, device="cuda:0", seed=0)
    batch[("pol", 0, 0)] = batch[("pol", 0, 0)][..., :bench.FRAME_W].contiguous()
    batch.pop("depth_gt"); batch.pop(("mask", 0, 0))
    out = {"batch": args.batch, "input": f"{bench.H}x{bench.W} (frames {bench.H}x{bench.FRAME_W})", "steps": args.steps}
    for cfg, attention in (("configs[2]", False), ("configs[4]", True)):
        tr = _trainer(args.batch, attention)
        res = {"default": _timed(tr, batch, args.steps, args.warmup)}
        tr.bf16 = True                      # what opt.bf16 = True selects at construction
        res["bf16"] = _timed(tr, batch, args.steps, args.warmup)
        res["speedup"] = round(res["default"]["ms_per_step"] / res["bf16"]["ms_per_step"], 3)
        if not attention:
            tr.bf16 = False
            res["kernels_default"] = _kernels(tr, batch)
            tr.bf16 = True
            ks = _kernels(tr, batch)
            res["kernels_bf16"] = ks
            res["bf16_kernels"] = {n: dict(v, frac_of_bf16_peak=round(v["tflops"] / BF16_PEAK_TF, 4))
                                   for n, v in ks.items() if "bf16" in n}
        out[cfg] = res
        del tr
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
