"""PoseDecoder (reference manydepth/networks/pose_decoder.py) on HIP kernels.

The state dict carries the reference's names (``net.0`` squeeze, ``net.1`` / ``net.2`` the two 3x3 layers, ``net.3`` the
1x1 output layer).  The squeeze and the 3x3 layers are convolutions with the ReLU in their epilogue; everything from the
input of ``net.3`` on -- the 1x1 convolution, the spatial mean, the 0.01, and where wanted both 4x4 matrices -- is one
launch (polardepth.functional.pose_head, csrc/pose.hip).
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from polardepth import functional as PF
from polardepth import ops


def _cl(conv):
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    return conv


class PoseDecoder(nn.Module):
    def __init__(self, num_ch_enc, num_input_features, num_frames_to_predict_for=None, stride=1):
        super().__init__()
        self.num_ch_enc = num_ch_enc
        self.num_input_features = num_input_features
        if num_frames_to_predict_for is None:
            num_frames_to_predict_for = num_input_features - 1
        self.num_frames_to_predict_for = num_frames_to_predict_for
        self.convs = OrderedDict()
        self.convs[("squeeze")] = _cl(nn.Conv2d(int(self.num_ch_enc[-1]), 256, 1))
        self.convs[("pose", 0)] = _cl(nn.Conv2d(num_input_features * 256, 256, 3, stride, 1))
        self.convs[("pose", 1)] = _cl(nn.Conv2d(256, 256, 3, stride, 1))
        self.convs[("pose", 2)] = _cl(nn.Conv2d(256, 6 * num_frames_to_predict_for, 1))
        self.net = nn.ModuleList(list(self.convs.values()))

    def _trunk(self, input_features):
        """pose_decoder.py:34-43 up to the input of ("pose", 2)."""
        cat = [PF.conv_bias_act(f[-1], self.convs["squeeze"], ops.ACT_RELU) for f in input_features]
        out = cat[0] if len(cat) == 1 else torch.cat(cat, 1)
        for i in range(2):
            out = PF.conv_bias_act(out, self.convs[("pose", i)], ops.ACT_RELU)
        return out

    def forward(self, input_features):
        """(axisangle, translation), each [B, num_frames_to_predict_for, 1, 3]."""
        return self.forward_with_matrices(input_features, False)[:2]

    def forward_with_matrices(self, input_features, invert=False):
        """(axisangle, translation, cam_T_cam, cam_T_cam_inv): the two [B,4,4] matrices are
        transformation_from_parameters(axisangle[:, 0], translation[:, 0], invert) and the same with ``invert`` flipped
        (trainer.py:694-707), from the same launch."""
        return PF.pose_head(self._trunk(input_features), self.convs[("pose", 2)], invert)
