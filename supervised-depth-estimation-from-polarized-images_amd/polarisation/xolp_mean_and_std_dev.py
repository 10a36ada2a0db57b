"""polarisation.xolp_mean_and_std_dev façade: mean and standard deviation of DoLP and AoLP over a chosen set of frames, the
statistics that standardise the XOLP encoder's input -- on the device (polardepth.polar.XolpStats, pd_xolp_stats).

Reference: polarisation/xolp_mean_and_std_dev.py:10-32, which stacks 46 frames of 832 x 1088 from two folders of .npy files
(``dolp/NAME.npy``, ``aolp/NAME.npy``) in fp64 and calls ndarray.mean() / .std().  Differences, by design: the folders are
arguments instead of a path in the source, any number of frames of any size is taken (frame by frame, nothing is stacked),
and each value is rounded to fp32 first -- the precision of the tensor the network consumes.  For any other input the
project reads (calibrated angles, 16-bit frames, DoFP sensors) tools/xolp_stats.py runs the same pass behind the loader.
"""
import os
import sys

import numpy as np
import torch

from polardepth import polar as _polar


def stats_of_folders(dolp_dir, aolp_dir, device="cuda"):
    """Every NAME.npy of ``dolp_dir`` with its namesake in ``aolp_dir`` ([H,W] each) -> the dict of XolpStats.result()."""
    names = sorted(f for f in os.listdir(dolp_dir) if f.endswith(".npy"))
    if not names:
        raise FileNotFoundError(f"no .npy frame in {dolp_dir}")
    acc = _polar.XolpStats(device)
    for name in names:
        dolp = np.load(os.path.join(dolp_dir, name))
        aolp = np.load(os.path.join(aolp_dir, name))
        if dolp.ndim != 2 or dolp.shape != aolp.shape:
            raise ValueError(f"{name}: DoLP {dolp.shape} and AoLP {aolp.shape} must be two [H,W] frames of one shape")
        H, W = dolp.shape
        frame = np.zeros((1, 2, H, W + (-W) % 4), dtype=np.float32)      # rows padded to whole quads, `width` says how far the data go
        frame[0, 0, :, :W], frame[0, 1, :, :W] = dolp, aolp
        acc.add(torch.from_numpy(frame).to(acc.device), width=W)
    return acc.result()


def report(res, out=None):
    """The reference's six lines (xolp_mean_and_std_dev.py:25-30)."""
    out = sys.stdout if out is None else out
    for label, key in (("DOLP MEAN: ", "dolp_mean"), ("DOLP STD: ", "dolp_std"), ("AOLP MEAN: ", "aolp_mean"),
                       ("AOLP STD: ", "aolp_std"), ("XOLP MEAN: ", "xolp_mean"), ("XOLP STD: ", "xolp_std")):
        print(label, res[key], file=out)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 1:
        dolp_dir, aolp_dir = os.path.join(argv[0], "dolp"), os.path.join(argv[0], "aolp")
    elif len(argv) == 2:
        dolp_dir, aolp_dir = argv
    else:
        raise SystemExit("usage: xolp_mean_and_std_dev.py PATH   (with PATH/dolp and PATH/aolp)   |   DOLP_DIR AOLP_DIR")
    report(stats_of_folders(dolp_dir, aolp_dir))


if __name__ == "__main__":
    main()
