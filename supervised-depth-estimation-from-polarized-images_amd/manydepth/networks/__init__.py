"""Network classes re-exported like reference manydepth/networks/__init__.py:2-6.

ShallowResnetEncoder, the pre-encoders and the decoders are the supervised hot path.  ResnetEncoderMatching is the
multi-frame encoder for KNOWN poses (the cost volume of csrc/matching.hip).  ResnetEncoder (the full five-level ResNet-18,
one or two stacked input images) and PoseDecoder are the pose network of the monodepth2 / ManyDepth setting: two frames in,
axisangle and translation out, the decoder's tail and both 4x4 matrices in one launch (csrc/pose.hip).  PoseCNN, the
reference's alternative pose network, is not built: a placeholder that raises on construction.
"""
from .resnet_encoder import ShallowResnetEncoder, ResnetEncoder, ResnetEncoderMatching
from .pre_encoders import ShallowEncoder, ShallowNormalsEncoder, JointEncoder
from .depth_decoder import DepthDecoder
from .normals_decoder import NormalsDecoder      # `arch1++_separate_normals_dec` variant (README.md:54)
from .pose_decoder import PoseDecoder


def build_models(pretrained, dropout_rate, xolp_norm, scales, augment_normals, augment_xolp, attention, uncertainty,
                 normals_decoder, pose_network):
    """The ordered model table of the Trainer (trainer.py:192-236) and of Evaluation, which differ in the arguments only.  The
    order of construction is part of the contract: every module draws its initialisation from torch's generator, so a
    module added anywhere but at the end changes what the ones behind it draw."""
    models = {"rgb_encoder": ShallowResnetEncoder(18, pretrained)}
    if augment_normals:
        models["normals_encoder"] = ShallowNormalsEncoder(in_channels=9, dropout_rate=dropout_rate)
    if augment_xolp:
        models["xolp_encoder"] = ShallowEncoder(mode='XOLP', in_channels=2, dropout_rate=dropout_rate, xolp_norm=xolp_norm)
    models["joint_encoder"] = JointEncoder(dropout_rate=dropout_rate, include_normals=augment_normals,
                                           include_xolp=augment_xolp, attention=attention)
    # with ``uncertainty`` the reference's heads, under its checkpoint names (depth_decoder.py:46-73)
    models["mono_depth"] = DepthDecoder(models["rgb_encoder"].num_ch_enc, scales, uncertainty=bool(uncertainty))
    if normals_decoder:                           # `arch1++_separate_normals_dec`
        if not augment_normals:
            raise ValueError("the separate normals decoder sits behind the normals encoder: it needs augment_normals")
        models["normals_decoder"] = NormalsDecoder(64)
    if pose_network:                              # trainer.py:222-236 for pose_model_type "separate_resnet"
        models["pose_encoder"] = ResnetEncoder(18, pretrained, num_input_images=2)
        models["pose"] = PoseDecoder(models["pose_encoder"].num_ch_enc, num_input_features=1, num_frames_to_predict_for=2)
    return models


def _out_of_scope(name):
    class _Placeholder:
        def __init__(self, *a, **k):
            raise NotImplementedError(f"networks.{name} is not built: the pose network here is ResnetEncoder + PoseDecoder")
    _Placeholder.__name__ = name
    return _Placeholder


PoseCNN = _out_of_scope("PoseCNN")
