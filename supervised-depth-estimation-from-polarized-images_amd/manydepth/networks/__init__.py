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


def _out_of_scope(name):
    class _Placeholder:
        def __init__(self, *a, **k):
            raise NotImplementedError(f"networks.{name} is not built: the pose network here is ResnetEncoder + PoseDecoder")
    _Placeholder.__name__ = name
    return _Placeholder


PoseCNN = _out_of_scope("PoseCNN")
