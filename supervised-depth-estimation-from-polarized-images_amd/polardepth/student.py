"""Host-side pieces of the cost-volume student's training step (the reference's --train_student branch) around the kernels
of csrc/student.hip: the adaptive depth-bin tracker (trainer.py:120-121, 650-664) and the matching augmentation
(trainer.py:587-605).  Nothing here synchronises with the device."""
import random

import torch

from . import ops


class DepthBinTracker:
    """The running estimate of the scene's depth range that the plane sweep's bins follow: two doubles ON THE DEVICE
    (min, max), initialised from ``opt.min_depth`` / ``opt.max_depth``.  ``update`` moves them by the exponential average of
    update_adaptive_depth_bins and rewrites the encoder's ``depth_bins`` in place (``ops.depth_bins_update``: one launch,
    no ``.item()``); the reference does four reductions and two host round trips per step here."""

    def __init__(self, min_depth, max_depth, device):
        self.floor = float(min_depth)
        self.state = torch.tensor([float(min_depth), float(max_depth)], dtype=torch.float64, device=device)

    def update(self, minmax, encoder):
        """``minmax`` [N,2] fp32 from ``ops.student_masks``; writes into ``encoder.depth_bins``, the tensor the next
        ``ops.cost_volume`` reads."""
        ops.depth_bins_update(minmax, self.state, self.floor, encoder.depth_bins, encoder.depth_binning)

    def values(self):
        """(min_depth_bin, max_depth_bin) as Python floats: a device-to-host copy, for checkpoints only."""
        mn, mx = self.state.tolist()
        return mn, mx

    def load(self, min_depth_bin, max_depth_bin, encoder):
        """A checkpoint's pair back into the tracker, and the bins it implies into ``encoder.depth_bins``."""
        self.state.copy_(torch.tensor([float(min_depth_bin), float(max_depth_bin)], dtype=torch.float64))
        encoder.compute_depth_bins(float(min_depth_bin), float(max_depth_bin))


def matching_augmentation(lookup_frames, relative_poses, color0, is_train, enabled, rng=random):
    """The static-frame and zero-pose augmentation of trainer.py:587-605.  One ``rng.random()`` per batch item on the host,
    in batch order (none when ``is_train`` or ``enabled`` is false); the draws travel to the device as ONE small code tensor
    and are applied there:
      draw < 0.25   the item's lookup frames are replaced by ``color0``, the un-jittered ("color", 0, 0), as the reference does
      draw < 0.5    the item's poses are zeroed: the plane sweep's "pose sums to 0" rule then skips its frames
    lookup_frames [B,F,3,H,W], relative_poses [B,F,4,4], color0 [B,3,H,W].  Returns (aug [B] fp32, 1 = augmented item,
    lookup_frames, relative_poses); the inputs are not modified."""
    B = lookup_frames.shape[0]
    codes = [0] * B
    if is_train and enabled:
        for b in range(B):
            draw = rng.random()
            codes[b] = 1 if draw < 0.25 else (2 if draw < 0.5 else 0)
    dev = lookup_frames.device
    if not any(codes):
        return torch.zeros(B, dtype=torch.float32, device=dev), lookup_frames, relative_poses
    code = torch.tensor(codes, dtype=torch.float32).to(dev, non_blocking=True)
    static = (code == 1).view(B, 1, 1, 1, 1)
    lookup_frames = torch.where(static, color0[:, None].to(lookup_frames.dtype).expand_as(lookup_frames), lookup_frames)
    relative_poses = relative_poses * (code != 2).to(relative_poses.dtype).view(B, 1, 1, 1)
    return (code != 0).float(), lookup_frames, relative_poses
