"""Multi-frame matching from known poses: the pieces of the reference's ResnetEncoderMatching around the plane sweep
(manydepth/networks/resnet_encoder.py:406-541), on polardepth.ops.cost_volume (csrc/matching.hip).  Everything here is
forward only and runs without host synchronisation."""
import numpy as np
import torch

from . import ops


def depth_bins(min_depth_bin, max_depth_bin, num_depth_bins, binning="linear"):
    """compute_depth_bins (:406-420): the hypothesised depths as a float32 CPU tensor, bit-equal to the reference's --
    float64 numpy.linspace, in depth ("linear") or in inverse depth kept in ascending depth order ("inverse"), then rounded."""
    if binning == "inverse":
        bins = 1 / np.linspace(1 / max_depth_bin, 1 / min_depth_bin, num_depth_bins)[::-1]
    elif binning == "linear":
        bins = np.linspace(min_depth_bin, max_depth_bin, num_depth_bins)
    else:
        raise NotImplementedError(f"depth_binning {binning!r}: linear or inverse")
    return torch.from_numpy(np.ascontiguousarray(bins)).float()


def match_features(current_feats, lookup_feats, relative_poses, K, invK, bins, valid=None):
    """match_features (:430-511): (cost_volume [B,D,h,w] float32 with the missing entries filled with the pixel's maximum,
    missing [B,D,h,w] float32 0/1).  current_feats [B,C,h,w], lookup_feats [B,F,C,h,w], relative_poses [B,F,4,4] (an all-zero
    pose marks a missing frame), K / invK [B,4,4] of the feature resolution, bins [D] on the device."""
    cost, _, _, _, missing = ops.cost_volume(current_feats, lookup_feats, relative_poses, K, invK, bins, valid=valid,
                                             want_missing=True)
    return cost, missing.float()


def compute_confidence_mask(cost_volume, num_bins_threshold=None):
    """compute_confidence_mask (:534-541): 1 where a pixel has more than zero cost in num_bins_threshold (default: all) bins.
    ops.cost_volume returns the default mask from the sweep itself; this is the reference's function for any other use."""
    if num_bins_threshold is None:
        num_bins_threshold = cost_volume.shape[1]
    return ((cost_volume > 0).sum(1) == num_bins_threshold).float()


def indices_to_disparity(indices, bins):
    """indices_to_disparity (:526-532): 1 / bins[indices], on the device of ``indices``."""
    return 1 / bins.to(indices.device)[indices.long()]
