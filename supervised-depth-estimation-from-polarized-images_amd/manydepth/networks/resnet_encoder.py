"""ShallowResnetEncoder (reference manydepth/networks/resnet_encoder.py:783-822) and ResnetEncoderMatching (:292-714) on
HIP kernels.

The module tree reproduces torchvision's ``resnet18`` names (conv1, bn1, layer1..4.{0,1}.{conv1,bn1,
conv2,bn2,downsample.{0,1}}, fc) so that ``rgb_encoder.pth`` checkpoints round-trip, including the
layer3 / layer4 / fc parameters the reference constructs but never runs (:819-820).
``pretrained=True`` would download ImageNet weights in the reference (options.py:261-265); there is
no network here: weights are loaded from $PD_RESNET18_WEIGHTS if set, else scratch with a warning.
"""
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from polardepth import functional as PF
from polardepth import matching, ops


def _cl(conv):
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    return conv


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = _cl(nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False))
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _cl(nn.Conv2d(planes, planes, 3, 1, 1, bias=False))
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(_cl(nn.Conv2d(inplanes, planes, 1, stride, bias=False)),
                                            nn.BatchNorm2d(planes))
        self.stride = stride

    def forward(self, x):
        tr = self.training
        # identity blocks: conv1 and the skip read the same x -- the skip gradient rides in conv1's data-gradient epilogue
        mail = PF.SkipGrad() if (self.downsample is None and torch.is_grad_enabled() and x.requires_grad) else None
        y = PF.conv_bn_chain(x, self.conv1, self.bn1, PF.ChainCfg(stride=self.stride, pad=1, relu_pre=True, skip_in=mail),
                             training=tr)
        idt = x
        if self.downsample is not None:
            idt = PF.conv_bn_chain(x, self.downsample[0], self.downsample[1],
                                   PF.ChainCfg(stride=self.stride, pad=0, relu_pre=False), training=tr)
        # bn2 -> + identity -> relu
        return PF.conv_bn_chain(y, self.conv2, self.bn2,
                                PF.ChainCfg(stride=1, pad=1, relu_pre=False, relu_post=True, skip_out=mail),
                                res=idt, training=tr)


class ResNet18(nn.Module):
    def __init__(self, in_ch=3):
        super().__init__()
        self.conv1 = _cl(nn.Conv2d(in_ch, 64, 7, 2, 3, bias=False))
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        chans = [64, 64, 128, 256, 512]
        for i in range(1, 5):
            setattr(self, f"layer{i}", nn.Sequential(BasicBlock(chans[i - 1], chans[i], 1 if i == 1 else 2),
                                                     BasicBlock(chans[i], chans[i], 1)))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, 1000)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')


class ShallowResnetEncoder(nn.Module):
    def __init__(self, num_layers, pretrained, num_input_images=1, **kwargs):
        super().__init__()
        if num_layers != 18:
            raise ValueError("{} is not a supported number of resnet layers (the hot path uses 18)".format(num_layers))
        if num_input_images != 1:
            raise NotImplementedError("multi-image input belongs to the self-supervised path (out of scope)")
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        self.encoder = ResNet18()
        if pretrained:
            path = os.environ.get("PD_RESNET18_WEIGHTS")
            if path and os.path.exists(path):
                self.encoder.load_state_dict(torch.load(path, map_location="cpu"))
            else:
                warnings.warn("weights_init=pretrained: no local resnet18 weights ($PD_RESNET18_WEIGHTS) and no "
                              "network access -- training the RGB encoder from scratch")

    def forward(self, input_image):
        e = self.encoder
        tr = self.training
        self.features = []
        # (x - 0.45) / 0.225 is folded into the stem's gather (resnet_encoder.py:812)
        cfg = PF.ChainCfg(stride=2, pad=3, relu_pre=True, affine=(0.45, 0.225))
        f0 = PF.conv_bn_chain(input_image.float(), e.conv1, e.bn1, cfg, training=tr)
        self.features.append(f0)
        # f0 feeds the max-pool and, as a skip connection, the decoder: the decoder deposits its gradient in this mailbox and
        # the max-pool's backward kernel adds it (functional.SkipGrad), instead of autograd's pass over three 335 MB tensors
        mail = PF.SkipGrad() if (PF.USE_SKIP_FUSION and torch.is_grad_enabled() and f0.requires_grad) else None
        if mail is not None:
            f0._pd_skip_mail = mail
        x = PF.maxpool3s2(f0, mail)
        for blk in e.layer1:
            x = blk(x)
        self.features.append(x)
        for blk in e.layer2:
            x = blk(x)
        self.features.append(x)
        return self.features


class ResnetEncoder(nn.Module):
    """The full five-level ResNet-18 encoder (reference resnet_encoder.py:736-781) for 1 or 2 stacked input images: the
    pose network's encoder reads two frames, 6 channels (:26-69).  torchvision's names under ``encoder.``; the 3 n-channel
    7x7 stem runs on the space-to-depth route with (x - 0.45) / 0.225 folded into its gather.  ``pretrained`` reads
    $PD_RESNET18_WEIGHTS and, for two images, stores cat([conv1.weight] * 2, 1) / 2 (:62-68)."""

    def __init__(self, num_layers, pretrained, num_input_images=1, **kwargs):
        super().__init__()
        if num_layers != 18:
            raise ValueError("{} is not a supported number of resnet layers (the hot path uses 18)".format(num_layers))
        if num_input_images not in (1, 2):
            raise ValueError(f"num_input_images must be 1 or 2, got {num_input_images}")
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        self.encoder = ResNet18(3 * num_input_images)
        if pretrained:
            path = os.environ.get("PD_RESNET18_WEIGHTS")
            if path and os.path.exists(path):
                loaded = dict(torch.load(path, map_location="cpu"))
                loaded["conv1.weight"] = torch.cat([loaded["conv1.weight"]] * num_input_images, 1) / num_input_images
                self.encoder.load_state_dict(loaded)
                _cl(self.encoder.conv1)
            else:
                warnings.warn("weights_init=pretrained: no local resnet18 weights ($PD_RESNET18_WEIGHTS) and no "
                              "network access -- training the pose encoder from scratch")

    def forward(self, input_image):
        e = self.encoder
        tr = self.training
        self.features = []
        cfg = PF.ChainCfg(stride=2, pad=3, relu_pre=True, affine=(0.45, 0.225))
        x = PF.conv_bn_chain(input_image.float(), e.conv1, e.bn1, cfg, training=tr)
        self.features.append(x)
        x = PF.maxpool3s2(x)
        for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
            for blk in layer:
                x = blk(x)
            self.features.append(x)
        return self.features


def _layer(inplanes, planes, stride):
    return nn.Sequential(BasicBlock(inplanes, planes, stride), BasicBlock(planes, planes, 1))


class _FeaturesIntoBuffer(torch.autograd.Function):
    """Channels [0, C) of the NHWC buffer that reduce_conv reads receive the current frame's features; the cost volume is
    already in the channels behind them (ops.cost_volume(out=)), so torch.cat([features, cost_volume], 1) is never formed.
    Backward: the feature channels of the buffer's gradient; the cost-volume channels were built without a gradient."""

    @staticmethod
    def forward(ctx, feats, buf):
        ctx.C = feats.shape[1]
        buf[:, :ctx.C].copy_(feats)
        ctx.mark_dirty(buf)
        return buf

    @staticmethod
    def backward(ctx, g):
        return ops.as_nhwc(g[:, :ctx.C]), None


class ResnetEncoderMatching(nn.Module):
    """The reference's ResNet-18 encoder with a cost volume after the second block (resnet_encoder.py:292-714), for KNOWN
    poses: the plane sweep, the confidence mask and the lowest-cost map are one launch of pd_cost_volume (csrc/matching.hip).

    The module tree carries the reference's names -- layer0 = (conv1, bn1, relu), layer1 = (maxpool, torchvision layer1),
    layer2..4, prematching_conv (constructed, never run, as in the reference), reduce_conv -- so its checkpoints load; the
    reference's backprojector / projector hold index grids only, and their entries of a checkpoint are dropped on loading.
    ``pretrained=True`` would download ImageNet weights in the reference; here they come from $PD_RESNET18_WEIGHTS or not at
    all.  ``depth_bins`` lives on the module's device and is read by the kernel: adaptive bins overwrite it in place."""

    def __init__(self, num_layers, pretrained, input_height, input_width, min_depth_bin=0.1, max_depth_bin=20.0,
                 num_depth_bins=96, adaptive_bins=False, depth_binning='linear', batch_size=8):
        super().__init__()
        if num_layers != 18:
            raise ValueError("{} is not a supported number of resnet layers (the hot path uses 18)".format(num_layers))
        if not 1 <= num_depth_bins <= ops.COST_VOLUME_MAX_BINS:
            raise ValueError(f"num_depth_bins must be in 1..{ops.COST_VOLUME_MAX_BINS}, got {num_depth_bins}")
        self.adaptive_bins = adaptive_bins
        self.depth_binning = depth_binning
        self.set_missing_to_max = True
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        self.num_depth_bins = num_depth_bins
        self.matching_height, self.matching_width = input_height // 4, input_width // 4   # the cost volume is at 1/4 resolution
        self.layer0 = nn.Sequential(_cl(nn.Conv2d(3, 64, 7, 2, 3, bias=False)), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
        self.layer1 = nn.Sequential(nn.MaxPool2d(3, 2, 1), _layer(64, 64, 1))
        self.layer2 = _layer(64, 128, 2)
        self.layer3 = _layer(128, 256, 2)
        self.layer4 = _layer(256, 512, 2)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        self.register_buffer("depth_bins", matching.depth_bins(min_depth_bin, max_depth_bin, num_depth_bins, depth_binning),
                             persistent=False)
        self.prematching_conv = nn.Sequential(nn.Conv2d(64, 16, 1, 1, 0), nn.ReLU(inplace=True))
        self.reduce_conv = nn.Sequential(_cl(nn.Conv2d(64 + num_depth_bins, 64, 3, 1, 1)), nn.ReLU(inplace=True))
        self._register_load_state_dict_pre_hook(self._drop_index_grids)
        if pretrained:
            path = os.environ.get("PD_RESNET18_WEIGHTS")
            if path and os.path.exists(path):
                self.load_torchvision_state_dict(torch.load(path, map_location="cpu"))
            else:
                warnings.warn("weights_init=pretrained: no local resnet18 weights ($PD_RESNET18_WEIGHTS) and no "
                              "network access -- training the matching encoder from scratch")

    @staticmethod
    def _drop_index_grids(state_dict, prefix, *_):
        for k in [k for k in state_dict if k.startswith((prefix + "backprojector.", prefix + "projector."))]:
            del state_dict[k]

    def load_torchvision_state_dict(self, sd):
        """A torchvision resnet18 state_dict (conv1, bn1, layer1..4, fc) into this module's tree."""
        own = {}
        for k, v in sd.items():
            head = k.split(".")[0]
            if head in ("conv1", "bn1"):
                own["layer0." + ("0" if head == "conv1" else "1") + k[len(head):]] = v
            elif head == "layer1":
                own["layer1.1" + k[len(head):]] = v
            elif head in ("layer2", "layer3", "layer4"):
                own[k] = v
        missing, unexpected = self.load_state_dict(own, strict=False)
        left = [k for k in missing if not k.startswith(("prematching_conv.", "reduce_conv."))]
        if left or unexpected:
            raise RuntimeError(f"resnet18 weights do not fit: missing {left}, unexpected {list(unexpected)}")

    def compute_depth_bins(self, min_depth_bin, max_depth_bin):
        """compute_depth_bins (:406-428): new bins into the tensor the kernel reads, in place (a captured graph sees them)."""
        self.depth_bins.copy_(matching.depth_bins(float(min_depth_bin), float(max_depth_bin), self.num_depth_bins,
                                                  self.depth_binning), non_blocking=True)

    def match_features(self, current_feats, lookup_feats, relative_poses, K, invK):
        return matching.match_features(current_feats, lookup_feats, relative_poses, K, invK, self.depth_bins)

    def compute_confidence_mask(self, cost_volume, num_bins_threshold=None):
        return matching.compute_confidence_mask(cost_volume, num_bins_threshold)

    def indices_to_disparity(self, indices):
        return matching.indices_to_disparity(indices, self.depth_bins)

    def feature_extraction(self, image, return_all_feats=False):
        """The first two blocks of the ResNet (:513-524); (x - 0.45) / 0.225 is folded into the stem's gather."""
        tr = self.training
        cfg = PF.ChainCfg(stride=2, pad=3, relu_pre=True, affine=(0.45, 0.225))
        feats_0 = PF.conv_bn_chain(image.float(), self.layer0[0], self.layer0[1], cfg, training=tr)
        x = PF.maxpool3s2(feats_0)
        for blk in self.layer1[1]:
            x = blk(x)
        return [feats_0, x] if return_all_feats else x

    def forward(self, current_image, lookup_images, poses, K, invK, min_depth_bin=None, max_depth_bin=None):
        self.features = self.feature_extraction(current_image, return_all_feats=True)
        current_feats = self.features[-1]
        B, C, h, w = current_feats.shape
        D = self.num_depth_bins
        buf = ops.empty_nhwc(B, C + D, h, w, current_feats.device)
        with torch.no_grad():
            # a caller that keeps ``depth_bins`` current on the device itself (polardepth.student.DepthBinTracker) passes
            # no range: the host-side recomputation is for callers that hold the range as Python numbers
            if self.adaptive_bins and min_depth_bin is not None:
                self.compute_depth_bins(min_depth_bin, max_depth_bin)
            batch_size, num_frames, chns, height, width = lookup_images.shape
            lookup_feats = self.feature_extraction(lookup_images.reshape(batch_size * num_frames, chns, height, width))
            lookup_feats = ops.as_nhwc(lookup_feats).view(batch_size, num_frames, C, h, w)
            # the cost volume, already multiplied by the confidence mask (:630), straight into the channels behind the features
            _, confidence_mask, _, lowest_cost = ops.cost_volume(current_feats, lookup_feats, poses, K, invK, self.depth_bins,
                                                                 out=buf[:, C:], apply_confidence=True)
        x = _FeaturesIntoBuffer.apply(current_feats, buf)
        x = PF.conv_bias_act(x, self.reduce_conv[0], ops.ACT_RELU)
        for layer in (self.layer2, self.layer3, self.layer4):
            for blk in layer:
                x = blk(x)
            self.features.append(x)
        return self.features, lowest_cost, confidence_mask
