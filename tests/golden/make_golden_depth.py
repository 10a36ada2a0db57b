#!/usr/bin/env python3
"""Generate tests/golden/g11_depth_errors.npz by RUNNING THE REFERENCE's manydepth.layers.compute_depth_errors_numpy.

Like make_golden_general.py this runs only where the reference checkout is available ($PD_REFERENCE); the output is data only
(inputs and the reference's seven figures), no reference source text is stored.  Re-run with:

    PD_REFERENCE=<reference checkout> python tests/golden/make_golden_depth.py

Two 24x32 images (float32 depth in metres, some ground truth outside (0.1, 2.0), some predictions outside the clamps):
  "material"  the pixels of the validity gate whose instance-mask value is 60 (the selection of trainer.py:1380-1413)
  "frame"     every pixel of the validity gate
each scored as it is ("<case>__errors": the prediction clamped to [0.1, 2.0], trainer.py:1418-1419) and median-scaled
("<case>__errors_scaled": the selected prediction -- clamped to [0.1, 2.0] first, as the network's output always is
(disp_to_depth) -- multiplied by np.median(gt) / np.median(pred) in float32, then clamped, trainer.py:1416-1419;
"<case>__ratio" is that factor).

Key layout of the .npz: "cases", "min_depth", "max_depth", "mask_value", "<case>__gt" / "__pred" [24,32] float32, "<case>__mask"
[24,32] int32, "<case>__errors" / "__errors_scaled" [7] float64 = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, "<case>__ratio"
float32, "<case>__count" the number of selected pixels.
"""
import os
import sys

import numpy as np

REF = os.environ.get("PD_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
H, W = 24, 32
MIN_DEPTH, MAX_DEPTH = 0.1, 2.0
MASK_VALUE = 60


def image(rng, spread):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = (0.9 + 0.5 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 0.05, (H, W))).astype(np.float32)
    gt[rng.random((H, W)) < 0.05] = 0.0                       # holes of the depth map
    gt[rng.random((H, W)) < 0.03] = 2.4                       # beyond the range
    pred = (gt * rng.normal(1.0, spread, (H, W)) * 1.3 + rng.normal(0, 0.02, (H, W))).astype(np.float32)
    pred[rng.random((H, W)) < 0.04] = 0.02                    # below the lower clamp
    pred[rng.random((H, W)) < 0.04] = 3.0                     # above the upper clamp
    mask = (rng.integers(0, 11, (H, W)) * 20).astype(np.int32)
    return gt, pred, mask


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set PD_REFERENCE to the reference checkout")
    sys.path.insert(0, os.path.join(REF, "manydepth"))
    sys.path.insert(0, REF)
    from layers import compute_depth_errors_numpy
    rng = np.random.default_rng(11)
    data = {"cases": np.array(["material", "frame"]), "min_depth": np.float64(MIN_DEPTH), "max_depth": np.float64(MAX_DEPTH),
            "mask_value": np.int64(MASK_VALUE)}
    for case, spread in (("material", 0.08), ("frame", 0.03)):
        gt, pred, mask = image(rng, spread)
        sel = np.logical_and(gt > MIN_DEPTH, gt < MAX_DEPTH)
        if case == "material":
            sel = np.logical_and(sel, np.logical_and(mask >= MASK_VALUE, mask <= MASK_VALUE))
        g = gt[sel]
        for key, scaled in (("errors", False), ("errors_scaled", True)):
            p = pred[sel].copy()
            if scaled:
                p = np.clip(p, np.float32(MIN_DEPTH), np.float32(MAX_DEPTH))
                ratio = np.median(g) / np.median(p)
                assert ratio.dtype == np.float32
                data[f"{case}__ratio"] = ratio
                p *= ratio
            p[p < MIN_DEPTH] = MIN_DEPTH
            p[p > MAX_DEPTH] = MAX_DEPTH
            assert p.dtype == np.float32 and g.dtype == np.float32
            data[f"{case}__{key}"] = np.array(compute_depth_errors_numpy(g, p), np.float64)
        data[f"{case}__gt"], data[f"{case}__pred"], data[f"{case}__mask"] = gt, pred, mask
        data[f"{case}__count"] = np.int64(g.size)
    path = os.path.join(OUT, "g11_depth_errors.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(data):
        if "errors" in k or "ratio" in k or "count" in k:
            print(k, data[k])


if __name__ == "__main__":
    main()
