"""Multi-frame matching: the pieces of the reference's ResnetEncoderMatching around the plane sweep
(manydepth/networks/resnet_encoder.py:406-541), on polardepth.ops.cost_volume (csrc/matching.hip), and the poses for it from
the pose network (``matching_poses``: the second half of predict_poses, trainer.py:708-746, on polardepth.ops.pose_chain,
csrc/pose.hip).  Everything here is forward only and runs without host synchronisation."""
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


def chain_pairs(matching_ids):
    """{fi: (first frame, second frame)} for every matching id but 0, in the order of ``matching_ids``: the pair the pose
    network sees for fi, stacked in temporal order -- (fi, fi + 1) for a negative id, (fi - 1, fi) for a positive one
    (trainer.py:714-716, 727-729).  The ids must be what the reference's ``matching_ids`` are: 0 first, the negative ones
    -1 .. -Ln and the positive ones 1 .. Lp without gaps, each sign nearest first (a link continues the stored pose of the
    frame before it); anything else is a ValueError."""
    ids = [int(i) for i in matching_ids]
    neg, pos = [i for i in ids if i < 0], [i for i in ids if i > 0]
    if not ids or ids[0] != 0 or 0 in ids[1:] or len(ids) < 2 or neg != list(range(-1, -1 - len(neg), -1)) or \
            pos != list(range(1, 1 + len(pos))) or max(len(neg), len(pos)) > ops.POSE_CHAIN_MAX_LINKS:
        raise ValueError(f"matching_ids {ids}: 0 first, then -1 .. -Ln and 1 .. Lp without gaps, nearest first, at most "
                         f"{ops.POSE_CHAIN_MAX_LINKS} per direction")
    return {fi: ((fi, fi + 1) if fi < 0 else (fi - 1, fi)) for fi in ids[1:]}


def matching_poses(pose_encoder, pose_decoder, frames, matching_ids, present):
    """The matching-pose half of predict_poses (trainer.py:708-746): ({fi: relative_pose [N,4,4]}, {fi: relative_pose_inv
    [N,4,4]}) for every matching id but 0.  ``frames`` maps a frame id to its picture [N,3,H,W]; ``present`` maps a frame id
    to [N], the loader's ``frame_valid`` (0 = the frame does not exist: the loaders serve a zero picture with it, which is
    what the reference's per-item ``feat.sum() == 0`` looks for, one host synchronisation each).  Under no_grad: one
    pose-network pass per id, in the order of ``matching_ids``, on the pair ``chain_pairs`` states; slot 0 of each pass; then
    ONE ``ops.pose_chain`` call per direction.  relative_pose[fi] is the pose 0 -> fi, all zeros from an absent frame on;
    relative_pose_inv[fi] is the LINK's inverse, as in the reference.  The pass for fi = -1 sees the same pair as the first
    half's pass for the neighbour -1 and is run again nevertheless: in training mode the reference's second pass updates the
    BatchNorm running statistics a second time."""
    pairs = chain_pairs(matching_ids)
    with torch.no_grad():
        params = {}
        for fi, (a, b) in pairs.items():
            feats = pose_encoder(torch.cat([frames[a].float(), frames[b].float()], 1))
            axisangle, translation = pose_decoder([feats])
            params[fi] = (axisangle[:, 0].reshape(-1, 3), translation[:, 0].reshape(-1, 3))
        rel, rel_inv = {}, {}
        for s in (-1, 1):
            chain = sorted((fi for fi in pairs if fi * s > 0), key=abs)
            if not chain:
                continue
            r, ri = ops.pose_chain(torch.stack([params[fi][0] for fi in chain]), torch.stack([params[fi][1] for fi in chain]),
                                   torch.stack([present[fi].float() for fi in chain]), None, s)
            for k, fi in enumerate(chain):
                rel[fi], rel_inv[fi] = r[k], ri[k]
    order = list(pairs)
    return {fi: rel[fi] for fi in order}, {fi: rel_inv[fi] for fi in order}


def indices_to_disparity(indices, bins):
    """indices_to_disparity (:526-532): 1 / bins[indices], on the device of ``indices``."""
    return 1 / bins.to(indices.device)[indices.long()]
