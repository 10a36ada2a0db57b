"""manydepth.trainer.Trainer -- the reference's supervised training loop (manydepth/trainer.py:73)
on the MI355X-native engine.

Kept from the reference: constructor contract (options Namespace), attributes (models,
model_optimizer, model_lr_scheduler, opt, device, epoch, step), method names and return values of
train / run_epoch / process_batch / compute_losses / compute_supervised_normals_losses / val / test /
set_train / set_eval / save_opts / save_model / load_model / load_mono_model / log / log_time, the
per-model ``<name>.pth`` + ``adam.pth`` checkpoint layout and the loss dictionary keys.

Implemented scope: the supervised single-frame branch (``--depth_supervision_only``,
``--depth_supervision``) -- trainer.py:192-216, 469-477, 497-513, 531-545, 567, 1126-1150, 1241-1265,
1298-1309 -- and the supervised mode with photometric multi-view consistency from known poses (``--depth_supervision True
--pose_input True`` without ``--depth_supervision_only``; trainer.py:479-530, 983-1098, 1150-1236): the same five networks and
supervised terms, plus the neighbouring frames of ``--frame_ids`` warped into the current view through the predicted depth and
the ground-truth relative poses of ``_pose/%06d.txt``, compared by monodepth2's reprojection loss (minimum over the frames,
automasking; ``--no_ssim``, ``--disable_automasking``, ``--avg_reprojection`` are honoured).  It adds ``reproj_loss/{s}`` to
``loss/{s}`` and their mean over the scales to ``loss``; under data parallelism the term is normalised per rank; it is not
captured yet (``PD_STEP_GRAPH=1`` is refused with it).  With ``opt.pose_network = True`` (``PD_POSE_NETWORK=1``; needs
``--depth_supervision True`` without ``--depth_supervision_only`` and without ``--pose_input``) the poses of that term are
PREDICTED: ``pose_encoder`` (ResnetEncoder, two stacked frames) and ``pose`` (PoseDecoder) see the jittered frame pair of
every neighbour in temporal order (trainer.py:222-236, 669-707), their output goes through transformation_from_parameters into
the same warp, and the term trains depth and pose together; ``--res_pose`` is not built, and ``PD_STEP_GRAPH=1`` /
``opt.bf16`` / ``torch.distributed`` are refused with it; its loaders
take a neighbour's picture without asking for pose files (``HAMMER_Dataset(need_poses=False)``).  ``opt.matching_poses = True``
(``PD_MATCHING_POSES=1``; only with the pose network, else ValueError) adds the matching-pose half of predict_poses
(trainer.py:708-746): ``matching_ids`` from ``--num_matching_frames`` / ``--use_future_frame`` as trainer.py:131-137 forms them,
loaders that serve ``frame_ids`` plus the matching ids not among them (appended at the end), and after every ``predict_poses``
``inputs[("relative_pose", fi)]`` -- the pose 0 -> fi composed link by link from the jittered frames, all zeros from a missing
frame on -- and ``inputs[("relative_pose_inv", fi)]`` -- the link's own inverse, as the reference stores it -- without a tape
(``polardepth.matching.matching_poses``: one pose-network pass per id, one pd_pose_chain launch per direction).  Nothing in a
training step consumes them yet; ``frame_ids`` keeps its meaning for the photometric term and the pose supervision, and
without the option nothing changes in a bit.  ``--supervise_pose`` (only
with the pose network; trainer.py:1267-1285) adds the predicted ``cam_T_cam`` against the ground-truth relative pose,
rotations compared as rotation vectors (``roma.rotmat_to_rotvec``, restated in csrc/pose_loss.hip: one launch forward, one
backward, for all frames): ``r_loss`` / ``t_loss`` are the plain sums over the frames, and what joins ``loss`` (after the
division by the number of scales) weights frame f of F with F - f, because the reference adds its RUNNING sums inside the loop
over the frames -- with ``frame_ids 0 -1 1`` the first neighbour counts twice, the second once.  The loaders are then built
with ``need_poses=True``, and -- a deliberate difference from the reference, which has no mask here and supervises a missing
neighbour towards whatever its loader substituted -- items whose ``frame_valid`` is 0 are left out, the mean being taken over
the present ones, as in the photometric term.  ``opt.polar_loss = (w_n, w_a)`` (``PD_POLAR_LOSS``; any of the modes above)
adds the polarimetric normals loss: per scale the normals of the predicted depth map against the candidates K1 derives from
DoLP / AoLP, on the decisions of ``Evaluation.test_polar_normals`` (``polar_normal_loss/{s}``, ``polar_azimuth_loss/{s}``;
``_polar_loss_option``; ``opt.polar_ray_frame`` / ``PD_POLAR_RAY_FRAME=1``: in the frame of each pixel's viewing ray); without it
nothing changes in a bit, and ``PD_STEP_GRAPH=1`` is refused with it.  ``opt.uncertainty_loss = w`` (``PD_UNCERTAINTY_LOSS``; any
of the modes above) builds the decoder with its uncertainty heads and trains the ``unc_conv`` ones as the scale of a Laplace error
model of the depth (``uncertainty_loss/{s}``; ``_uncertainty_option``; ``opt.uncertainty_range``, ``opt.uncertainty_detach``);
``PD_STEP_GRAPH=1``, ``opt.bf16`` and ``torch.distributed`` are refused with it.  The cost-volume student's building
blocks exist -- the plane sweep (``polardepth.ops.cost_volume``) and ``networks.ResnetEncoderMatching`` -- but its training
branch (``--train_student``: matching augmentation, consistency loss, adaptive-bin tracker, second decoder) does not: it,
``--v1_multiscale``, DPT and stereo branches raise NotImplementedError.

What runs where: every tensor operation of a training step is a hand-written HIP kernel from
libpolardepth.so (polar preprocessing K1, implicit-GEMM convolutions K2, fused BN/ReLU/pool chains
K3, decoder glue K4, multi-scale loss K5, Adam); torch supplies memory, streams, the autograd tape
and torch.distributed (RCCL).  There is no CPU fallback: ``--no_cuda`` is rejected.
"""
import json
import logging
import os
import time
import warnings
from datetime import datetime

import numpy as np
import torch
from torch.utils.data import DataLoader

from .options import MODELS_TO_LOAD_DEFAULT
from .utils import readlines, sec_to_hm_str
from .layers import SSIM, compute_depth_errors, compute_depth_errors_numpy
from manydepth import datasets, networks
from polardepth import functional as PF
from polardepth import polar as pdpolar
from polardepth import dofp as pddofp
from polardepth import cdofp as pdcdofp
from polardepth import calibration as pdcal
from polardepth import color as pdcolor
from polardepth import ops
from polardepth import depth_eval
from polardepth import matching as pdmatching
from polardepth.engine import ParamStore, FusedAdam, GradReducer
from polardepth._lib import lib, check, ptr, stream_ptr

try:
    from torch.utils.tensorboard import SummaryWriter
except Exception:                                   # tensorboard is optional: keep the interface
    class SummaryWriter:
        def __init__(self, *a, **k): pass
        def add_scalar(self, *a, **k): pass
        def add_image(self, *a, **k): pass
        def close(self): pass

_MATERIAL_GREY = {"box": 20, "bottle": 40, "can": 60, "cup": 80, "remote": 100, "teapot": 120, "cutlery": 140,
                  "glass": 160, "table": 180, "wall": 200}     # instance-mask grey values, trainer.py:1388-1407


def _unused_resnet_param(model_name, param_name):
    """ShallowResnetEncoder builds a full resnet18 but never runs layer3/layer4/fc (resnet_encoder.py:819-820)."""
    if model_name == "pose_encoder":              # the full encoder runs every layer but the classifier
        return param_name.split(".")[1] == "fc"
    return model_name == "rgb_encoder" and param_name.split(".")[1] in ("layer3", "layer4", "fc")


def _attention_variant(opt):
    """BASELINE config 5 ("arch1++_attention"): the reference's master parser has no flag for it, so the option
    table stays identical to manydepth/options.py and the variant is switched by an attribute set on the options
    object (``opt.joint_attention = True``) or by ``PD_JOINT_ATTENTION=1``."""
    return bool(getattr(opt, "joint_attention", False)) or os.environ.get("PD_JOINT_ATTENTION") == "1"


def _normals_decoder_variant(opt):
    """`arch1++_separate_normals_dec` (reference README.md:54): like the attention variant the reference's master parser has
    no flag for it; selected on the options object (``opt.normals_decoder = True``) or by ``PD_NORMALS_DECODER=1``."""
    return bool(getattr(opt, "normals_decoder", False)) or os.environ.get("PD_NORMALS_DECODER") == "1"


def _bf16_variant(opt):
    """Opt-in bf16 training mode: every convolution the single-bf16 kernels take rounds its operands once to bf16 and forms each
    product with one bf16 MFMA (fp32 storage, epilogue, gradients and Adam: ops.CONV_BF16); with the attention variant the
    attention block runs on the bf16 kernels as well.  Not a reference CLI flag: selected on the options object only
    (``opt.bf16 = True``; the shell entry point manydepth/train.py maps PD_BF16=1 onto it)."""
    return bool(getattr(opt, "bf16", False))


def _polar_loss_option(opt):
    """The polarimetric normals loss (polardepth.ops.polar_loss): ``opt.polar_loss = (w_n, w_a)``, the weights of its normal and
    azimuth terms, or "w_n,w_a"; None / absent = the term is off and nothing changes in a bit.  ``opt.polar_loss_where`` =
    "all" (default) or "holes": only the pixels whose ground-truth depth is outside [min_depth, max_depth], where the
    supervised terms see nothing.  ``opt.pol_aolp_sign`` = +1 (default) or -1, the handedness of the sensor's AoLP, as
    ``Evaluation(aolp_sign=)``.  Not reference CLI flags: manydepth/train.py maps PD_POLAR_LOSS / PD_POLAR_LOSS_WHERE /
    PD_POL_AOLP_SIGN onto them.  Returns (weights or None, where, sign); the weights are written back as a list of two floats,
    so that they travel in opt.json.  ``opt.polar_ray_frame`` (PD_POLAR_RAY_FRAME=1; default off) forms the term in the frame
    of each pixel's viewing ray instead of the orthographic convention; it is validated here, written back as a bool, and
    refused without ``opt.polar_loss``: there is no term it could apply to."""
    w = getattr(opt, "polar_loss", None)
    ray = getattr(opt, "polar_ray_frame", None)
    if ray is not None and not (isinstance(ray, (bool, int, np.integer)) and int(ray) in (0, 1)):
        raise ValueError(f"opt.polar_ray_frame must be True or False, got {ray!r}")
    if w is None:
        if ray:
            raise ValueError("opt.polar_ray_frame is set without opt.polar_loss: the ray frame is an option of the "
                             "polarimetric term, set opt.polar_loss = (w_n, w_a) too")
        return None, "all", 1
    if isinstance(w, str):
        w = w.split(",")
    try:
        w = [float(x) for x in w]
    except (TypeError, ValueError):
        raise ValueError(f"opt.polar_loss must be (w_n, w_a), got {getattr(opt, 'polar_loss')!r}")
    if len(w) != 2 or not all(np.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError(f"opt.polar_loss must be two finite weights >= 0 (w_n, w_a), got {getattr(opt, 'polar_loss')!r}")
    where = getattr(opt, "polar_loss_where", None) or "all"
    if where not in ("all", "holes"):
        raise ValueError(f'opt.polar_loss_where must be "all" or "holes", got {where!r}')
    sign = getattr(opt, "pol_aolp_sign", None)
    sign = 1 if sign is None else int(sign)
    if sign not in (1, -1):
        raise ValueError(f"opt.pol_aolp_sign must be +1 or -1, got {getattr(opt, 'pol_aolp_sign')!r}")
    opt.polar_loss = w
    if ray is not None:
        opt.polar_ray_frame = bool(ray)
    return w, where, sign


def _uncertainty_option(opt):
    """The depth-uncertainty term (polardepth.functional.uncertainty_loss): ``opt.uncertainty_loss = w``, its weight; None /
    absent = the term is off, the decoder is built without its uncertainty heads and nothing changes in a bit.
    ``opt.uncertainty_range = (b_lo, b_hi)`` or "lo,hi": the Laplace scale in metres at u = 0 and u = 1 (default
    ``ops.UNCERTAINTY_RANGE``; a convention, not a measurement).  ``opt.uncertainty_detach``: the term trains the heads only --
    no gradient reaches the depth maps or the decoder's features.  Not reference CLI flags: manydepth/train.py maps
    PD_UNCERTAINTY_LOSS / PD_UNCERTAINTY_RANGE / PD_UNCERTAINTY_DETACH onto them.  Returns (w or None, range, detach); with
    the term on, the three are written back in a form that travels in opt.json."""
    w = getattr(opt, "uncertainty_loss", None)
    rng = getattr(opt, "uncertainty_range", None)
    detach = getattr(opt, "uncertainty_detach", None)
    if detach is not None and not (isinstance(detach, (bool, int, np.integer)) and int(detach) in (0, 1)):
        raise ValueError(f"opt.uncertainty_detach must be True or False, got {detach!r}")
    if w is None:
        if rng is not None or detach:
            raise ValueError("opt.uncertainty_range / opt.uncertainty_detach are set without opt.uncertainty_loss: they are "
                             "options of the uncertainty term, set opt.uncertainty_loss = w too")
        return None, None, False
    try:
        w = float(w)
    except (TypeError, ValueError):
        raise ValueError(f"opt.uncertainty_loss must be a finite weight >= 0, got {getattr(opt, 'uncertainty_loss')!r}")
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError(f"opt.uncertainty_loss must be a finite weight >= 0, got {getattr(opt, 'uncertainty_loss')!r}")
    if isinstance(rng, str):
        rng = rng.split(",")
    if rng is not None:
        try:
            rng = [float(x) for x in rng]
        except (TypeError, ValueError):
            rng = ()
        if len(rng) != 2:
            raise ValueError(f"opt.uncertainty_range must be (b_lo, b_hi), got {getattr(opt, 'uncertainty_range')!r}")
    rng = ops.uncertainty_range(rng)              # 0 < b_lo < b_hi < inf, or ValueError
    opt.uncertainty_loss, opt.uncertainty_range, opt.uncertainty_detach = w, list(rng), bool(detach)
    return w, rng, bool(detach)


class _Bf16Step:
    """The flag words of this Trainer's training forward passes in bf16 mode, restored on exit: the precision is recorded by
    every autograd node when its forward runs, so the backward (and a captured replay) follows it without a global switch."""

    def __enter__(self):
        self.attn = PF.USE_BF16_ATTENTION
        self.flags = ops.conv_flags(conv=ops._with_bf16(ops.CONV_FLAGS, True), wgrad=ops._with_bf16(ops.WGRAD_FLAGS, True))
        self.flags.__enter__()
        PF.USE_BF16_ATTENTION = True
        return self

    def __exit__(self, *exc):
        PF.USE_BF16_ATTENTION = self.attn
        return self.flags.__exit__(*exc)


class Trainer:
    def __init__(self, options):
        self.opt = options
        if self.opt.no_cuda:
            raise RuntimeError("--no_cuda: this build has no CPU path (the CPU restatement lives in oracle/ and "
                               "is test infrastructure only)")
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible: the HIP hot path cannot run and there is no CPU fallback")
        for flag in ("train_stereo_only", "train_dpt", "train_student", "use_stereo", "res_pose", "supervise_pose"):
            # --supervise_pose supervises the PREDICTED poses: with the pose network it is built (below), without it there
            # is nothing to supervise
            if getattr(self.opt, flag, False) and not (flag == "supervise_pose" and getattr(self.opt, "pose_network", False)):
                raise NotImplementedError(f"--{flag}: outside the supervised hot path of this build")
        # the one further configuration: the supervised terms plus the photometric reprojection term from the neighbouring
        # frames, warped with the ground-truth relative poses (no pose network, no cost volume)
        # ... or with the relative poses PREDICTED by a pose network that is trained along (monodepth2's setting;
        # trainer.py:222-236, 669-707).  Not a reference CLI flag (--pose_input False alone keeps its meaning): selected on
        # the options object (``opt.pose_network = True``; manydepth/train.py maps PD_POSE_NETWORK=1 onto it)
        self.pose_network = bool(getattr(self.opt, "pose_network", False))
        if self.pose_network:
            if not self.opt.depth_supervision or self.opt.depth_supervision_only or self.opt.pose_input:
                raise ValueError("opt.pose_network: needs --depth_supervision True, without --depth_supervision_only and "
                                 "without --pose_input (the poses are predicted, not read)")
            if os.environ.get("PD_STEP_GRAPH") == "1" or bool(getattr(self.opt, "step_graph", False)):
                raise NotImplementedError("PD_STEP_GRAPH=1 with opt.pose_network: this mode is not captured yet")
            if _bf16_variant(self.opt):
                raise NotImplementedError("opt.bf16 with opt.pose_network: the pose network has not been verified in bf16")
            # the pose modules run once per neighbouring frame, so their gradient buffers are written twice per step; the
            # gradient reducer marks a parameter ready -- and all-reduces its bucket -- after the FIRST write
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                raise NotImplementedError("torch.distributed with opt.pose_network: the gradient reducer expects one "
                                          "backward pass per module and step; run this mode on one GPU")
        # the matching-pose half of predict_poses (trainer.py:708-746): the pose network's poses 0 -> fi of the cost volume's
        # lookup frames, composed link by link (polardepth.matching.matching_poses, csrc/pose.hip: one launch per
        # direction).  Not a reference CLI flag: ``opt.matching_poses = True`` (manydepth/train.py maps PD_MATCHING_POSES=1)
        self.matching_poses = bool(getattr(self.opt, "matching_poses", False))
        if self.matching_poses and not self.pose_network:
            raise ValueError("opt.matching_poses: the matching poses are the pose network's; it needs opt.pose_network")
        # --supervise_pose (trainer.py:1267-1285): the predicted cam_T_cam against the ground-truth relative pose of
        # ``_pose/%06d.txt``, one launch for all frames (polardepth.ops.pose_supervision, csrc/pose_loss.hip)
        self.supervise_pose = bool(self.pose_network and getattr(self.opt, "supervise_pose", False))
        self.photometric = bool(self.opt.depth_supervision and (self.opt.pose_input or self.pose_network)
                                and not self.opt.depth_supervision_only and not getattr(self.opt, "v1_multiscale", False))
        if not (self.opt.depth_supervision_only and self.opt.depth_supervision) and not self.photometric:
            raise NotImplementedError("only --depth_supervision_only True --depth_supervision True is implemented "
                                      "(the path of train_supervised_GT.sh)")
        if self.photometric and (os.environ.get("PD_STEP_GRAPH") == "1" or bool(getattr(self.opt, "step_graph", False))):
            raise NotImplementedError("PD_STEP_GRAPH=1 with --pose_input: the photometric term is not captured yet; "
                                      "run this mode without the step graph")
        # the polarimetric normals loss: the depth map's normals against the candidates K1 derives from DoLP / AoLP, on the
        # decisions of Evaluation.test_polar_normals (polardepth.functional.polarimetric_loss, csrc/polar_loss.hip).  It needs
        # no ground truth and no pose, so it works in the supervised-only mode and in both photometric modes
        self.polar_loss, self.polar_loss_where, self.pol_aolp_sign = _polar_loss_option(self.opt)
        self.polar_ray_frame = bool(getattr(self.opt, "polar_ray_frame", False))     # validated just above
        if self.polar_loss is not None and (os.environ.get("PD_STEP_GRAPH") == "1" or bool(getattr(self.opt, "step_graph", False))):
            raise NotImplementedError("PD_STEP_GRAPH=1 with opt.polar_loss: the polarimetric term is not captured yet; "
                                      "run it without the step graph")
        # the depth-uncertainty term: the decoder's uncertainty heads as the scale of a Laplace error model of the depth
        # (polardepth.functional.uncertainty_loss, csrc/unc_loss.hip); it needs the ground-truth depth every mode here has
        self._uncertainty_range_given = getattr(self.opt, "uncertainty_range", None) is not None
        self.uncertainty_loss, self.uncertainty_range, self.uncertainty_detach = _uncertainty_option(self.opt)
        if self.uncertainty_loss is not None:
            if os.environ.get("PD_STEP_GRAPH") == "1" or bool(getattr(self.opt, "step_graph", False)):
                raise NotImplementedError("PD_STEP_GRAPH=1 with opt.uncertainty_loss: the uncertainty term is not captured "
                                          "yet; run it without the step graph")
            if _bf16_variant(self.opt):
                raise NotImplementedError("opt.bf16 with opt.uncertainty_loss: the uncertainty heads have not been verified in "
                                          "bf16")
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                raise NotImplementedError("torch.distributed with opt.uncertainty_loss: the gradient reducer's bucket order "
                                          "has not been verified with the uncertainty heads; run this mode on one GPU")
        self.frame_ids = [int(i) for i in self.opt.frame_ids] if self.photometric else [0]
        if self.photometric and (self.frame_ids[0] != 0 or len(self.frame_ids) < 2 or 0 in self.frame_ids[1:]
                                 or len(self.frame_ids) - 1 > ops.REPROJ_MAX_FRAMES):
            raise ValueError(f"--frame_ids {self.frame_ids}: 0 first, then 1 .. {ops.REPROJ_MAX_FRAMES} neighbouring frames")
        # trainer.py:128-137: the frames the loaders serve are frame_ids plus the matching ids not among them, appended at
        # the end (a synthetic item draws its neighbours in this order: the existing ones keep their draws).  frame_ids keeps
        # its meaning for the photometric term and for pose supervision
        self.frames_to_load = list(self.frame_ids)
        if self.matching_poses:
            self.matching_ids = [0] + ([1] if self.opt.use_future_frame else []) + \
                list(range(-1, -1 - int(self.opt.num_matching_frames), -1))
            pdmatching.chain_pairs(self.matching_ids)          # ValueError for what the chain cannot take (no frame, too many)
            self.frames_to_load += [i for i in self.matching_ids if i not in self.frames_to_load]
        local_rank = int(os.environ.get("LOCAL_RANK", 0))
        self.device = torch.device("cuda", local_rank)
        torch.cuda.set_device(self.device)
        self.distributed = torch.distributed.is_available() and torch.distributed.is_initialized()
        self.rank = torch.distributed.get_rank() if self.distributed else 0

        # calibrated polarizer angles (degrees, in the order of the planes of ("pol", 0, 0)): not a reference CLI flag --
        # selected on the options object (``opt.pol_angles``; manydepth/train.py maps PD_POL_ANGLES="a,b,c,d" onto it).
        # None = the nominal 0/45/90/135 set; given, K1 runs its general kernel (polardepth.polar.polar_forward(angles=))
        self.pol_angles = pdpolar.angles_from_degrees(getattr(self.opt, "pol_angles", None))
        # interleaved sensor frames (("pol_dofp", 0, 0), HAMMER_Dataset(pol_dofp=True)): which plane each site of the 2x2
        # super-pixel feeds and how the planes are reconstructed (``opt.pol_layout`` / ``opt.pol_demosaic``; train.py maps
        # PD_POL_LAYOUT / PD_POL_DEMOSAIC onto them).  None = IMX250MZR / bilinear; pol_angles refer to the layout's planes
        self.pol_dofp = pddofp.options(getattr(self.opt, "pol_layout", None), getattr(self.opt, "pol_demosaic", None))
        # colour sensor frames (("pol_cdofp", 0, 0), HAMMER_Dataset(pol_cdofp=True)): ``opt.pol_layout`` again, the Bayer order,
        # white-balance gains and the factor to the 0..255 of the colour picture (``opt.pol_bayer`` / ``opt.pol_gains`` /
        # ``opt.pol_color_scale``; train.py maps PD_POL_BAYER / PD_POL_GAINS / PD_POL_COLOR_SCALE onto them).  None = RGGB, no
        # gains, scale 1 for 8-bit frames (wider ones need one)
        self.pol_cdofp = pdcdofp.options(getattr(self.opt, "pol_layout", None), getattr(self.opt, "pol_bayer", None),
                                         getattr(self.opt, "pol_gains", None), getattr(self.opt, "pol_color_scale", None))
        # the sensor's super-pixel calibration (``opt.pol_calibration``: the path of a saved ``polardepth.calibration.Calibration``
        # or the object; train.py maps PD_POL_CALIBRATION onto it): loaded once to this device and applied to ("pol_dofp", 0, 0)
        # / ("pol_cdofp", 0, 0) frames before their demosaic, inside the captured step too.  None = frames are taken as they
        # come.  Its matrices are in site order, but its nominal cell must be the one ``opt.pol_layout`` names
        self.pol_calibration = pdcal.parse(getattr(self.opt, "pol_calibration", None), self.device)
        if self.pol_calibration is not None and tuple(self.pol_calibration.layout) != tuple(self.pol_dofp[0]):
            raise ValueError(f"opt.pol_calibration was fitted for the layout {tuple(self.pol_calibration.layout)}, "
                             f"opt.pol_layout is {tuple(self.pol_dofp[0])}")

        # the (mean, std) pair that standardises the XOLP encoder's input (``opt.xolp_norm``: a pair or "mean,std"; train.py
        # maps PD_XOLP_NORM onto it; tools/xolp_stats.py measures it).  None = the reference's HAMMER constants, or the pair
        # of a loaded checkpoint (load_model).  A launch constant of the stem: the captured step needs nothing
        self.xolp_norm = pdpolar.parse_xolp_norm(getattr(self.opt, "xolp_norm", None))

        timestamp = datetime.now()
        self.data_path, self.data_path_val, self.log_dir = self.opt.data_path, self.opt.data_path_val, self.opt.log_dir
        self.log_path = os.path.join(self.opt.log_dir, self.opt.model_name + '_' + timestamp.strftime("%m-%d_%H-%M-%S"))
        self.log_args(timestamp)

        assert self.opt.height % 32 == 0, "'height' must be a multiple of 32"
        assert self.opt.width % 32 == 0, "'width' must be a multiple of 32"

        self.parameters_to_train = []
        self.num_scales = len(self.opt.scales)
        self.train_teacher_and_pose = not self.opt.freeze_teacher_and_pose

        # MODEL SETUP (trainer.py:192-236)
        self.models = networks.build_models(
            self.opt.weights_init == "pretrained", self.opt.dropout_rate, self.xolp_norm, self.opt.scales,
            self.opt.augment_normals, self.opt.augment_xolp, attention=_attention_variant(self.opt),
            uncertainty=self.uncertainty_loss is not None, normals_decoder=_normals_decoder_variant(self.opt),
            pose_network=self.pose_network)
        if self.uncertainty_loss is not None:
            self.models["mono_depth"].uncertainty_detach = self.uncertainty_detach
        for m in self.models.values():
            m.to(self.device)
        if self.distributed:                    # identical replicas: broadcast rank 0's initialisation
            for m in self.models.values():
                for t in list(m.parameters()) + list(m.buffers()):
                    torch.distributed.broadcast(t.data, 0)

        order = [n for n in ("rgb_encoder", "xolp_encoder", "normals_encoder", "joint_encoder", "mono_depth",
                             "normals_decoder", "pose_encoder", "pose") if n in self.models]
        unused = _unused_resnet_param
        if self.uncertainty_loss is not None:
            # the unc_conv_color heads run but nothing consumes them: no gradient, no Adam update; they stay in the checkpoint.
            # Found through the decoder's own keys, not by their place in its ModuleList
            dec = self.models["mono_depth"]
            idle = {id(p) for key, m in dec.convs.items() if key[0] == "unc_conv_color" for p in m.parameters()}
            idle_names = {n for n, p in dec.named_parameters() if id(p) in idle}
            unused = lambda mn, pn: _unused_resnet_param(mn, pn) or (mn == "mono_depth" and pn in idle_names)
        self.store = ParamStore(self.models, order=order, unused=unused, device=self.device)
        for n in order:
            self.parameters_to_train += list(self.models[n].parameters())
        self.reducer = GradReducer(self.store) if self.distributed else None
        self.model_optimizer = FusedAdam(self.store, self.opt.learning_rate, reducer=self.reducer)
        if self.distributed:
            self.model_optimizer.grad_scale = 1.0 / torch.distributed.get_world_size()
        self.model_lr_scheduler = torch.optim.lr_scheduler.StepLR(self.model_optimizer, self.opt.scheduler_step_size, 0.1)

        if self.opt.load_weights_folder is not None:
            self.load_model()
        if self.opt.mono_weights_folder is not None:
            self.load_mono_model()

        # DATA (trainer.py:254-303)
        if self.opt.dataset != "HAMMER":
            raise NotImplementedError("only --dataset HAMMER is on the hot path")
        self.dataset = datasets.HAMMER_Dataset

        def _split(split, which, data_path):
            path = os.path.join("splits", split, f"{which}_files.txt")
            if os.path.exists(path):
                return readlines(path)
            if str(data_path) == datasets.SYNTHETIC:      # seeded synthetic items need no scene list
                return []
            raise FileNotFoundError(f"{path} not found (run from the repository root, trainer.py:261-263; "
                                    f"--data_path {datasets.SYNTHETIC} serves synthetic items)")
        train_files = [self.opt.overfit_scene] if self.opt.overfit else _split(self.opt.split, "train", self.data_path)
        val_files = [self.opt.overfit_scene] if self.opt.overfit else _split(self.opt.split, "val", self.data_path)
        test_files = _split(self.opt.eval_split, "test", self.data_path_val)
        mk = lambda path, files, tr: self.dataset(path, files, self.opt.height, self.opt.width, self.frames_to_load, 4, is_train=tr,
                                                  img_ext='.png', offset=self.opt.offset, modality=self.opt.modality,
                                                  supervised_depth=True, supervised_depth_only=not self.photometric,
                                                  depth_modality=self.opt.depth_modality, lookup_aug=self.pose_network,
                                                  need_poses=not self.pose_network or self.supervise_pose)
        train_dataset, val_dataset, test_dataset = mk(self.data_path, train_files, True), \
            mk(self.data_path, val_files, False), mk(self.data_path_val, test_files, False)
        if self.pol_calibration is not None:
            self._check_calibration((("training", train_dataset), ("validation", val_dataset), ("test", test_dataset)))
        sampler = torch.utils.data.distributed.DistributedSampler(train_dataset) if self.distributed else None
        self.train_loader = DataLoader(train_dataset, self.opt.batch_size, sampler is None, sampler=sampler,
                                       num_workers=self.opt.num_workers, pin_memory=True, drop_last=True)
        self.val_loader = DataLoader(val_dataset, self.opt.batch_size, False, num_workers=self.opt.num_workers,
                                     pin_memory=True, drop_last=True)
        self.val_iter = iter(self.val_loader)
        self.test_loader = DataLoader(test_dataset, self.opt.batch_size, False, num_workers=self.opt.num_workers,
                                      pin_memory=True, drop_last=True)
        self.num_total_steps = len(train_dataset) // self.opt.batch_size * self.opt.num_epochs

        self.writers = {}
        modes = ["train", "val", "val_mono", "test", "test_mono"] + ["test_mono_" + m for m in
                                                                     ("glass", "cutlery", "can", "bottle", "cup", "teapot",
                                                                      "remote", "box", "table", "wall")]
        for mode in modes:
            self.writers[mode] = SummaryWriter(os.path.join(self.log_path, mode)) if self.rank == 0 else SummaryWriter()
        if not self.opt.no_ssim:
            self.ssim = SSIM()
        self.depth_metric_names = ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]
        self.depth_metric_names_mono = [n.replace("/", "_mono/", 1) for n in self.depth_metric_names]
        # PD_GLOBAL_LOSS_NORM=1 (or opt.global_loss_norm): mask-normalise over the global batch like the reference's
        # single process; default = per replica (standard DDP semantics, no exchange on the loss path)
        global_norm = self.distributed and (bool(getattr(self.opt, "global_loss_norm", False))
                                            or os.environ.get("PD_GLOBAL_LOSS_NORM") == "1")
        # independent encoders on separate HIP streams (PD_ENCODER_STREAMS=0: everything on the current stream)
        self.encoder_streams = os.environ.get("PD_ENCODER_STREAMS", "1") != "0" and self.device.type == "cuda"
        self.step_graph = os.environ.get("PD_STEP_GRAPH") == "1" or bool(getattr(self.opt, "step_graph", False))
        self.bf16 = _bf16_variant(self.opt)        # training steps only: evaluation and the folded inference path stay fp32
        self._graphed = None
        self._enc_streams = []
        self.loss_cfg = PF.LossCfg(self.opt.scales, self.opt.min_depth, self.opt.max_depth, self.opt.normals_loss_weight,
                                   self.opt.disparity_smoothness, self.opt.height, self.opt.width, global_norm=global_norm)
        self.epoch, self.step = 0, 0
        self.start_time = time.time()
        if self.rank == 0:
            print("There are {:d} training items and {:d} validation items and {:d} test items\n".format(
                len(train_dataset), len(val_dataset), len(test_dataset)))
            self.save_opts()

    # ------------------------------------------------------------------ bookkeeping
    def log_args(self, timestamp):
        if int(os.environ.get("RANK", 0)) != 0:
            return
        os.makedirs(self.log_path, exist_ok=True)
        logging.basicConfig(filename=os.path.join(self.log_path, 'args.log'), level=logging.INFO, format='%(message)s')
        logging.info('Run started at: %s', str(timestamp))
        for arg, value in sorted(vars(self.opt).items()):
            logging.info("%s: %r", arg, value)

    def _check_calibration(self, datasets):
        """A calibration serves one sensor: the first sensor frame of the training, validation and test loaders must have its
        size (``polardepth.calibration.check_dataset``).  Loaders that serve no sensor frames make the option idle: one
        warning."""
        served = [pdcal.check_dataset(self.pol_calibration, ds, f"the {name} loader") for name, ds in datasets]
        if not any(served):
            warnings.warn('opt.pol_calibration is set, but the loaders serve no ("pol_dofp", 0, 0) / ("pol_cdofp", 0, 0) frames '
                          "(PD_POL_DOFP / PD_POL_CDOFP): it applies only to batches that carry one")

    def set_train(self):
        for m in self.models.values():
            m.train()

    def set_eval(self):
        for m in self.models.values():
            m.eval()

    # ------------------------------------------------------------------ training loop (trainer.py:379-467)
    def train(self):
        # a loaded trainer_state.pth continues where the checkpoint stopped (the reference restarts at epoch 0)
        first_epoch = getattr(self, "resume_epoch", 0)
        self.epoch, self.step = first_epoch, getattr(self, "resume_step", 0)
        self.test()
        self.start_time = time.time()
        for self.epoch in range(first_epoch, self.opt.num_epochs):
            self.run_epoch()
            if (self.epoch + 1) % self.opt.save_frequency == 0:
                self.save_model(epoch_complete=True)     # rank 0 writes, every rank waits (no torn files under torchrun)
                self.test()

    def run_epoch(self):
        self.set_train()
        if self.distributed and hasattr(self.train_loader.sampler, "set_epoch"):
            self.train_loader.sampler.set_epoch(self.epoch)
        # a checkpoint written in the middle of an epoch resumes in that epoch, behind the batches already consumed
        skip = getattr(self, "resume_batch", 0) if self.epoch == getattr(self, "resume_epoch", -1) else 0
        self.resume_batch = 0
        for batch_idx, inputs in enumerate(self.train_loader):
            if batch_idx < skip:
                continue
            before_op_time = time.time()
            if self.step_graph:
                # PD_STEP_GRAPH=1: the whole step (zero_grad .. Adam) replayed from a hipGraph captured on the first batch
                # (polardepth/graph.py; same bits as the eager step, ~2 ms of host time instead of 13-35)
                dev_inputs = {k: v.to(self.device, non_blocking=True) for k, v in inputs.items()}
                if self._graphed is None:
                    from polardepth.graph import GraphedTrainStep
                    self._graphed = GraphedTrainStep(self, dev_inputs, warmup=1, restore_state=True)
                self._graphed.step(dev_inputs)
                outputs, losses = self._graphed.outputs, self._graphed.losses
                inputs = {**dev_inputs, **{k: v for k, v in self._graphed.static.items() if k not in dev_inputs}}
            else:
                self.model_optimizer.zero_grad()
                outputs, losses, mono_outputs = self.process_batch(inputs, is_train=True)
                losses["loss"].backward()
                self.model_optimizer.step()
            early_phase = batch_idx % self.opt.log_frequency == 0 and self.step < 2000
            late_phase = self.step % 2000 == 0
            if early_phase or late_phase:
                duration = time.time() - before_op_time
                self.log_time(batch_idx, duration, losses["loss"].cpu().data)    # the only host sync of the loop
                if "depth_gt" in inputs:
                    self.compute_depth_losses(inputs, outputs, losses)
                self.log("train", inputs, outputs, losses)
                self.val()
                self.save_model(epoch_complete=False, batch_idx=batch_idx)
            self.step += 1
        self.model_lr_scheduler.step()

    # ------------------------------------------------------------------ forward (trainer.py:469-648)
    def _polar_inputs(self, inputs):
        """On-device XOLP / normals from the raw planes when the loader hands them over (K1)."""
        want = []
        if self.opt.augment_xolp or self.opt.augment_normals:
            want = ["xolp"] + (["normals"] if self.opt.augment_normals else [])
        if self.polar_loss is not None:           # the polarimetric term scores against the candidates, whatever the encoders take
            want = ["xolp", "normals"]
        # raw frames from the loader (HAMMER_Dataset(raw_pol=True), uint8 / uint16 / float32) are resized on the device first
        normals = pdpolar.polar_inputs(inputs, (self.opt.height, self.opt.width), tuple(want), self.pol_angles,
                                       dofp=self.pol_dofp, cdofp=self.pol_cdofp, calibration=self.pol_calibration)
        if self.polar_loss is not None:
            if normals is None:                   # a loader that hands over XOLP itself, no planes
                if ("xolp", 0, 0) not in inputs:
                    raise ValueError('opt.polar_loss needs the polarisation: a batch with ("pol", 0, 0) planes, a sensor frame '
                                     'or ("xolp", 0, 0)')
                normals = pdpolar.normals_from_xolp(inputs[("xolp", 0, 0)].float().contiguous())
            inputs[("pol_normals", 0, 0)] = normals
        return normals

    def _forward_models(self, inputs):
        normals = self._polar_inputs(inputs)
        xolp_feats = normals_feats = None
        side = []
        if self.encoder_streams and (self.opt.augment_xolp or self.opt.augment_normals):
            # The three encoders are independent until the joint encoder: the shallow XOLP / normals encoders run on
            # two side streams next to the ResNet on the main one, so the HBM-bound kernels of one encoder (BatchNorm /
            # ReLU / pool chains) overlap the matrix-bound convolutions of another.  autograd replays every backward
            # node on its forward stream and inserts the cross-stream waits itself.
            main = torch.cuda.current_stream()
            x_in = inputs["xolp", 0, 0].float()
            if self.opt.augment_xolp:
                sx = self._encoder_stream(0)
                sx.wait_stream(main)
                with torch.cuda.stream(sx):
                    xolp_feats = self.models["xolp_encoder"](x_in)
                x_in.record_stream(sx)
                side.append((sx, xolp_feats))
            if self.opt.augment_normals:
                sn = self._encoder_stream(1)
                sn.wait_stream(main)
                with torch.cuda.stream(sn):
                    normals_feats = self.models["normals_encoder"](x_in, normals=normals)
                x_in.record_stream(sn)
                if normals is not None:
                    normals.record_stream(sn)
                side.append((sn, normals_feats))
        feats = self.models["rgb_encoder"](inputs["color_aug", 0, 0].float())
        if side:
            main = torch.cuda.current_stream()
            for st, out in side:
                main.wait_stream(st)
                for t in (out if isinstance(out, (list, tuple)) else [out]):
                    if torch.is_tensor(t):
                        t.record_stream(main)
        else:
            if self.opt.augment_xolp:
                xolp_feats = self.models["xolp_encoder"](inputs["xolp", 0, 0].float())
            if self.opt.augment_normals:
                normals_feats = self.models["normals_encoder"](inputs["xolp", 0, 0].float(), normals=normals)
        enc_feats = self.models["joint_encoder"](feats[-1], xolp_feats, normals_feats)
        feats = list(feats) + enc_feats
        outputs = dict(self.models['mono_depth'](feats))
        if "normals_decoder" in self.models:      # `arch1++_separate_normals_dec`: normals straight from the normals encoder
            outputs[("normals_pred", 0)] = self.models["normals_decoder"](normals_feats)
        return outputs

    def _encoder_stream(self, i):
        while len(self._enc_streams) <= i:
            self._enc_streams.append(PF.side_stream(self.device, self._enc_streams + [torch.cuda.current_stream(self.device)]))
            PF.register_producer_stream(self._enc_streams[-1])      # the gradient reducer / Adam wait for it too
        return self._enc_streams[i]

    def process_batch(self, inputs, is_train=False):
        for key, ipt in inputs.items():
            inputs[key] = ipt.to(self.device, non_blocking=True)
        # raw frames + jitter rows from the loader (HAMMER_Dataset(raw_color=True)): the colour pyramids on the device,
        # 4 scales like the loaders above; inside the captured step under PD_STEP_GRAPH=1, like the raw_pol resize
        pdcolor.expand_batch(inputs, (self.opt.height, self.opt.width), 4, cdofp=self.pol_cdofp,
                             calibration=self.pol_calibration)
        if self.train_teacher_and_pose and is_train and self.bf16:
            with _Bf16Step():
                mono_outputs = self._forward_models(inputs)
        elif self.train_teacher_and_pose:
            mono_outputs = self._forward_models(inputs)
        else:
            with torch.no_grad():
                mono_outputs = self._forward_models(inputs)
        if self.pose_network:                     # --freeze_teacher_and_pose: the pose pass runs without a tape too
            with torch.set_grad_enabled(self.train_teacher_and_pose and torch.is_grad_enabled()):
                mono_outputs.update(self.predict_poses(inputs))
        for scale in self.opt.scales:
            mono_outputs[("disp", 0, scale)] = mono_outputs[("disp", scale)]
        losses = self.compute_losses(inputs, mono_outputs, is_multi=False)
        return mono_outputs, losses, mono_outputs

    def predict_poses(self, inputs):
        """The first half of trainer.py:669-707 (``opt.pose_network``): one pass of the pose network per neighbouring frame,
        the two jittered frames stacked in temporal order -- NOT one batched pass over the frames: the BatchNorm statistics
        are per pass in the reference.  The decoder's tail and both matrices are one launch (csrc/pose.hip)."""
        outputs = {}
        cur = inputs[("color_aug", 0, 0)].float()
        for f_i in self.frame_ids[1:]:
            other = inputs[("color_aug", f_i, 0)].float()
            pair = [other, cur] if f_i < 0 else [cur, other]
            feats = self.models["pose_encoder"](torch.cat(pair, 1))
            axisangle, translation, T, T_inv = self.models["pose"].forward_with_matrices([feats], invert=f_i < 0)
            outputs[("axisangle", 0, f_i)], outputs[("translation", 0, f_i)] = axisangle, translation
            outputs[("cam_T_cam", 0, f_i)], outputs[("cam_T_cam_inv", 0, f_i)] = T, T_inv
        if self.matching_poses:
            # the second half (trainer.py:708-746), without a tape: inputs[("relative_pose", fi)] = the pose 0 -> fi of every
            # matching frame, all zeros from a missing frame on, and ("relative_pose_inv", fi) = the LINK's inverse, as the
            # reference stores it.  The jittered frames, as there; the loader's frame_valid stands for its feat.sum() == 0.
            # Nothing in a training step consumes them yet (the cost-volume student's branch is not built)
            ids = self.matching_ids
            rel, rel_inv = pdmatching.matching_poses(self.models["pose_encoder"], self.models["pose"],
                                                     {i: inputs[("color_aug", i, 0)] for i in ids}, ids,
                                                     {i: inputs[("frame_valid", i)] for i in ids[1:]})
            for i in ids[1:]:
                inputs[("relative_pose", i)], inputs[("relative_pose_inv", i)] = rel[i], rel_inv[i]
        return outputs

    def compute_losses(self, inputs, outputs, is_multi=False):
        """Supervised branch of trainer.py:1126-1296; also fills ("depth",0,s) / ("mono_depth",0,s)
        (trainer.py:538-545) because K5 produces the full-resolution depth maps on the way."""
        scales = list(self.opt.scales)
        disps = [outputs[("disp", s)] for s in scales]
        colors = [inputs[("color", 0, s)] for s in scales]
        vals, depths = PF.multiscale_loss(self.loss_cfg, inputs["depth"], inputs[("K", 0)], disps, colors)
        losses = {"loss": vals[0]}
        for i, s in enumerate(scales):
            losses[f"loss/{s}"] = vals[1 + 3 * i]
            losses[f"supervised_depth_loss/{s}"] = vals[2 + 3 * i]
            losses[f"supervised_normals_loss/{s}"] = vals[3 + 3 * i]
            outputs[("depth", 0, s)] = depths[i]
            outputs[("mono_depth", 0, s)] = depths[i]
        if self.photometric:
            # trainer.py:983-1067, 1150-1236 with --pose_input: the neighbours warped into frame 0 through each scale's depth
            # map and the ground-truth relative poses, minimum over the frames with automasking (polardepth/functional.py)
            ids = self.frame_ids[1:]
            automask = not self.opt.disable_automasking
            noise = None
            if automask:                          # the tie-breaker of trainer.py:1193-1194, one draw per scale, on the device
                noise = [torch.randn(depths[0].shape, device=depths[0].device).mul_(1e-5) for _ in scales]
            reproj = PF.photometric_loss(self.loss_cfg, disps, depths, inputs[("color", 0, 0)],
                                         [inputs[("color", i, 0)] for i in ids], inputs[("K", 0)], inputs[("inv_K", 0)],
                                         [outputs[("cam_T_cam", 0, i)] if self.pose_network else inputs[("poses", i)]
                                          for i in ids],
                                         torch.stack([inputs[("frame_valid", i)] for i in ids], 1).float(), noise=noise,
                                         no_ssim=self.opt.no_ssim, automask=automask, avg=self.opt.avg_reprojection)
            for i, s in enumerate(scales):        # trainer.py:1234-1236, 1262-1265
                losses[f"reproj_loss/{s}"] = reproj[i]
                losses[f"loss/{s}"] = losses[f"loss/{s}"] + reproj[i]
            losses["loss"] = losses["loss"] + sum(reproj[1:], reproj[0]) / len(reproj)
        if self.polar_loss is not None:
            # per scale, the depth map's normals against the polarisation normals of K1 (functional.polarimetric_loss): the
            # weighted sum of the two terms joins loss/{s}, its mean over the scales joins loss, as the reprojection term does
            valid = None
            if self.polar_loss_where == "holes":
                valid = ~((inputs["depth"] >= self.opt.min_depth) & (inputs["depth"] <= self.opt.max_depth))
            terms = PF.polarimetric_loss(self.loss_cfg, disps, depths, inputs[("K", 0)], inputs[("pol_normals", 0, 0)],
                                         inputs[("xolp", 0, 0)], valid, aolp_sign=self.pol_aolp_sign,
                                         ray_frame=self.polar_ray_frame)
            w_n, w_a = self.polar_loss
            polar = []
            for i, s in enumerate(scales):
                losses[f"polar_normal_loss/{s}"], losses[f"polar_azimuth_loss/{s}"] = terms[i]
                polar.append(w_n * terms[i][0] + w_a * terms[i][1])
                losses[f"loss/{s}"] = losses[f"loss/{s}"] + polar[i]
            losses["loss"] = losses["loss"] + sum(polar[1:], polar[0]) / len(polar)
        if self.uncertainty_loss is not None:
            # per scale, the ground truth under the Laplace model whose scale the scale's uncertainty head states
            # (functional.uncertainty_loss): w L_s joins loss/{s}, its mean over the scales joins loss, as the polarimetric term
            terms = PF.uncertainty_loss(self.loss_cfg, disps, depths, [outputs[("uncertainty", s)] for s in scales],
                                        inputs["depth"], self.uncertainty_range, detach_depth=self.uncertainty_detach)
            unc = []
            for i, s in enumerate(scales):
                losses[f"uncertainty_loss/{s}"] = terms[i]
                unc.append(self.uncertainty_loss * terms[i])
                losses[f"loss/{s}"] = losses[f"loss/{s}"] + unc[i]
            losses["loss"] = losses["loss"] + sum(unc[1:], unc[0]) / len(unc)
        if ("normals_pred", 0) in outputs:
            # `arch1++_separate_normals_dec`: the predicted normals against the normals of the ground truth, weighted like
            # the normals term of the depth loss (README.md:54,67: normals_loss_weight)
            nl = PF.normals_pred_loss(outputs[("normals_pred", 0)], inputs["depth"], inputs[("K", 0)], self.opt.min_depth,
                                      self.opt.max_depth)
            losses["normals_decoder_loss"] = nl
            losses["loss"] = losses["loss"] + self.opt.normals_loss_weight * nl
        if self.supervise_pose and not is_multi:
            # trainer.py:1267-1285, added after the division by the number of scales.  ``total`` carries the reference's
            # cumulative frame weights [F .. 1] (it adds the running sums inside its loop over the frames); r_loss / t_loss
            # are the plain sums it logs.  Unlike the reference, a neighbour the loader flags as missing is left out and
            # the mean is taken over the present items (ops.pose_supervision).  Under --freeze_teacher_and_pose the
            # matrices carry no tape, and neither do these terms.
            ids = self.frame_ids[1:]
            r_loss, t_loss, total = ops.pose_supervision(
                [outputs[("cam_T_cam", 0, i)] for i in ids], [inputs[("poses", i)] for i in ids],
                valid=torch.stack([inputs[("frame_valid", i)] for i in ids], 1).float())
            losses["r_loss"], losses["t_loss"] = r_loss, t_loss
            losses["loss"] = losses["loss"] + total
        return losses

    def compute_supervised_normals_losses(self, depth_gt, depth_pred, intrinsics, mask=None):
        """trainer.py:1298-1309 (value only): sum((2 - cos(n_gt, n_pred)) * mask) / sum(mask) with the CALLER's mask
        [N,1,H,W] (the reference passes the depth-range mask, trainer.py:1242-1243,1250; None selects it here)."""
        N, _, H, W = depth_gt.shape
        dev = depth_gt.device
        K = torch.eye(4, device=dev)[None].repeat(N, 1, 1)
        K[:, :3, :3] = intrinsics[:, :3, :3]
        gt, pred = depth_gt.contiguous().float(), depth_pred.detach().contiguous().float()
        if mask is None:
            mask = (gt >= self.opt.min_depth) & (gt <= self.opt.max_depth)
        mask = mask.to(device=dev, dtype=torch.float32).expand(N, 1, H, W).contiguous()
        part = torch.empty((lib.pd_loss_rows(N * H * W), 2), dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.pd_normals_loss_masked(ptr(pred), ptr(gt), ptr(K.contiguous()), ptr(mask), ptr(part), ptr(out), N, H, W,
                                         stream_ptr()), "pd_normals_loss_masked")
        return out[0]

    # ------------------------------------------------------------------ validation / test
    def _next_val(self):
        try:
            return next(self.val_iter)
        except StopIteration:
            self.val_iter = iter(self.val_loader)
            return next(self.val_iter)

    def val(self):
        self.set_eval()
        inputs = self._next_val()
        with torch.no_grad():
            outputs, losses, _ = self.process_batch(inputs)
            losses = {}
            if "depth_gt" in inputs:
                self.compute_depth_losses(inputs, outputs, losses, mono=True)
            self.log("val_mono", inputs, outputs, losses, log_images=False, log_essential_images=True)
        self.set_train()

    def test(self):
        """trainer.py:782-980: full test split, "all" + per-material metrics.  The per-image masked metrics
        (compute_depth_losses_from_list, trainer.py:1357-1434) are reduced on the device by pd_depth_metrics;
        only 11 x 7 numbers per batch leave the GPU."""
        if self.rank == 0:
            print("Running full test set at Epoch: ", self.epoch)
        self.set_eval()
        table = depth_eval.MaterialTable(_MATERIAL_GREY, self.opt.min_depth, self.opt.max_depth, self.device)
        with torch.no_grad():
            for inputs in self.test_loader:
                for key, ipt in inputs.items():
                    inputs[key] = ipt.to(self.device)
                outputs = self._forward_models(inputs)
                depth = ops.disp_to_depth(outputs[("disp", 0)], inputs["depth_gt"].shape[2:], self.opt.min_depth,
                                          self.opt.max_depth)
                table.add(inputs["depth_gt"], depth, inputs[("mask", 0, 0)])
        if self.rank == 0:
            for o, mean_errors in table.means().items():
                print("\n  " + o + "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
                print(("&{: 8.5f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
                losses = {metric: np.array(mean_errors[i]) for i, metric in enumerate(self.depth_metric_names)}
                self.log("test_mono" if o == "all" else "test_mono_" + o, None, None, losses, log_images=False)
        self.set_train()

    def compute_depth_losses(self, inputs, outputs, losses, mono=False):
        """trainer.py:1311-1355."""
        depth_pred = outputs[("depth", 0, 0)].detach().clamp(self.opt.min_depth, self.opt.max_depth)
        depth_gt = inputs["depth_gt"]
        mask = (depth_gt > self.opt.min_depth) * (depth_gt < self.opt.max_depth)
        errs = compute_depth_errors(depth_gt[mask], depth_pred[mask])
        for i, metric in enumerate(self.depth_metric_names):
            losses[metric] = np.array(errs[i].cpu())

    def compute_depth_losses_from_list(self, gts, preds, losses, masks, object="all"):
        """trainer.py:1357-1434: per-image metrics, optionally restricted to one material class."""
        errors = []
        lo, hi = self.opt.min_depth, self.opt.max_depth
        for k in range(len(preds)):
            pred_b = preds[k].clamp(lo, hi)[:, 0].numpy()
            gt_b = gts[k][:, 0].numpy()
            m_b = masks[k][:, 0].numpy()
            for b in range(pred_b.shape[0]):
                mask = np.logical_and(gt_b[b] > lo, gt_b[b] < hi)
                if object != "all":
                    mask = np.logical_and(mask, m_b[b] == _MATERIAL_GREY[object])
                if not mask.any():
                    continue
                errors.append(compute_depth_errors_numpy(gt_b[b][mask], np.clip(pred_b[b][mask], lo, hi)))
        if not errors:
            return
        mean_errors = np.array(errors).mean(0)
        print("\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
        print(("&{: 8.5f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
        for i, metric in enumerate(self.depth_metric_names):
            losses[metric] = np.array(mean_errors[i])

    # ------------------------------------------------------------------ logging
    def log_time(self, batch_idx, duration, loss):
        samples_per_sec = self.opt.batch_size / duration
        time_sofar = time.time() - self.start_time
        left = (self.num_total_steps / self.step - 1.0) * time_sofar if self.step > 0 else 0
        if self.rank == 0:
            print("epoch {:>3} | batch {:>6} | examples/s: {:5.1f} | loss: {:.5f} | time elapsed: {} | time left: {}".format(
                self.epoch, batch_idx, samples_per_sec, float(loss), sec_to_hm_str(time_sofar), sec_to_hm_str(left)))

    def log(self, mode, inputs, outputs, losses, log_images=True, log_essential_images=False, mono_depth=False):
        writer = self.writers[mode]
        for l, v in losses.items():
            try:
                value = float(v)
            except (TypeError, ValueError):      # non-scalar entries (images, per-pixel maps) are not logged by this build
                continue
            writer.add_scalar("{}".format(l), value, self.step)

    # ------------------------------------------------------------------ checkpoints (trainer.py:1586-1691)
    def save_opts(self):
        models_dir = os.path.join(self.log_path, "models")
        os.makedirs(models_dir, exist_ok=True)
        with open(os.path.join(models_dir, 'opt.json'), 'w') as f:
            to_save = self.opt.__dict__.copy()
            if not isinstance(to_save.get("pol_calibration"), (str, type(None))):      # the calibration travels as its path only
                to_save["pol_calibration"] = None
            json.dump(to_save, f, indent=2)

    def save_model(self, epoch_complete=True, batch_idx=-1):
        """trainer.py:1597-1617 layout (<model>.pth + adam.pth) plus trainer_state.pth.  Only rank 0 writes; every file
        goes through a temporary name + os.replace, and all ranks meet at a barrier afterwards.

        "A loaded trainer_state.pth continues where the checkpoint stopped" (train) covers what these files hold.  Restored by
        load_model: every model's parameters and buffers (BatchNorm running statistics, num_batches_tracked); Adam's two
        moment buffers, step count (the bias correction of the next step; the device word of a captured step too) and
        hyper-parameters, the learning rate among them; the StepLR state; epoch, step and the batch to resume behind; the
        dropout stream (Philox seed and step counter); the XOLP standardisation and the uncertainty range.  A resumed run
        fed the batches and torch seeds of the uninterrupted one repeats it bit for bit, in every training mode
        (tests/test_resume_gpu.py).

        NOT in the checkpoint, so a resumed run differs from the uninterrupted one in them:
          * the order of the shuffled ``train_loader`` (``shuffle=True`` without a seeded generator): ``resume_batch`` skips
            that many batches of a DIFFERENT permutation of the epoch;
          * the loaders' augmentation draws (colour jitter, flips);
          * torch's global generator, from which the photometric modes draw their automask noise."""
        save_folder = os.path.join(self.log_path, "models", "weights_{}".format(self.epoch))
        if self.rank == 0:
            os.makedirs(save_folder, exist_ok=True)

            def _save(obj, name):
                tmp = os.path.join(save_folder, name + ".tmp")
                torch.save(obj, tmp)
                os.replace(tmp, os.path.join(save_folder, name))
            for model_name, model in self.models.items():
                _save({k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}, "{}.pth".format(model_name))
            _save(self.model_optimizer.state_dict(), "adam.pth")
            # resume state (not in the reference, which restarts epoch/step/LR schedule on load).
            # run_epoch saves on its logging steps BEFORE self.step += 1 and before lr_scheduler.step(): such a
            # checkpoint is marked incomplete and resumes inside the same epoch.
            state = {"epoch": self.epoch, "step": self.step, "epoch_complete": bool(epoch_complete),
                     "batch_idx": int(batch_idx), "lr_scheduler": self.model_lr_scheduler.state_dict(),
                     "dropout_seed": PF.DropoutState.seed,
                     "dropout_step": PF.DropoutState.get_step(getattr(self, "device", None)),
                     "xolp_norm": None if getattr(self, "xolp_norm", None) is None else list(self.xolp_norm)}
            if getattr(self, "uncertainty_loss", None) is not None:      # the scale the uncertainty heads were trained to state
                state["uncertainty_range"] = list(self.uncertainty_range)
            _save(state, "trainer_state.pth")
        if self.distributed:
            torch.distributed.barrier()

    def _load_into(self, name, path, strict=False):
        model_dict = self.models[name].state_dict()
        pretrained = torch.load(path, map_location="cpu")
        pretrained = {k: v for k, v in pretrained.items() if k in model_dict}
        model_dict.update(pretrained)
        self.models[name].load_state_dict(model_dict, strict=strict)     # copies in place: flat-buffer views stay valid

    def load_mono_model(self):
        for n in ['rgb_encoder', 'mono_depth', 'normals_encoder', 'xolp_encoder', 'joint_encoder', 'normals_decoder']:
            path = os.path.join(self.opt.mono_weights_folder, "{}.pth".format(n))
            if n in self.models and os.path.isfile(path):
                self._load_into(n, path, strict=True)

    def _models_to_load(self):
        """The models load_model reads.  --models_to_load left at the parser's preset (options.MODELS_TO_LOAD_DEFAULT: the
        reference's names, which never cover this build's depth networks) means nothing was named: every model of this run,
        in every mode -- with the pose network too, whose ``pose_encoder`` / ``pose`` are among the preset's names.  A list
        that differs from the preset is explicit and keeps the reference's meaning (trainer.py:1659): exactly those names;
        the ones this run does not build are skipped, and a list none of whose names it builds falls back to every model."""
        named = list(getattr(self.opt, "models_to_load", None) or [])
        if named == list(MODELS_TO_LOAD_DEFAULT):
            return list(self.models)
        return [n for n in named if n in self.models] or list(self.models)

    def load_model(self):
        """Reads what save_model wrote: of the models ``_models_to_load`` names those that have a file in the folder, then
        adam.pth and trainer_state.pth (``opt.resume_state = False`` leaves the resume point, the LR schedule and the dropout
        stream alone).  Works on a Trainer that has already trained: nothing derived from the weights outlives a forward
        pass (the transposed data-gradient operands are rebuilt behind every forward convolution)."""
        folder = os.path.expanduser(self.opt.load_weights_folder)
        assert os.path.isdir(folder), "Cannot find folder {}".format(folder)
        for n in Trainer._models_to_load(self):
            path = os.path.join(folder, "{}.pth".format(n))
            if os.path.isfile(path):
                self._load_into(n, path)
        opt_path = os.path.join(folder, "adam.pth")
        if os.path.isfile(opt_path):
            try:
                self.model_optimizer.load_state_dict(torch.load(opt_path, map_location=self.device))
            except (ValueError, KeyError, RuntimeError) as e:
                print("Can't load Adam - using random ({})".format(e))
        state_path = os.path.join(folder, "trainer_state.pth")
        st = torch.load(state_path, map_location="cpu") if os.path.isfile(state_path) else None
        if st is not None:
            # the weights were trained behind the checkpoint's standardisation: adopt it, or refuse a different one
            theirs = pdpolar.parse_xolp_norm(st.get("xolp_norm"))
            mine = getattr(self, "xolp_norm", None)
            if theirs is not None and mine is not None and tuple(theirs) != tuple(mine):
                raise ValueError(f"xolp_norm = {tuple(mine)!r} is set, but the checkpoint in {folder} was trained with "
                                 f"{tuple(theirs)!r}: unset the option to adopt the checkpoint's pair")
            if theirs is not None and mine is None:
                self.xolp_norm = theirs
                self.opt.xolp_norm = list(theirs)
                if "xolp_encoder" in self.models:
                    self.models["xolp_encoder"].Conv1.in_affine = theirs
        if st is not None and getattr(self, "uncertainty_loss", None) is not None and st.get("uncertainty_range") is not None:
            # the heads state their scale in the checkpoint's range: adopt it, or refuse a different one
            theirs = ops.uncertainty_range(st["uncertainty_range"])
            if getattr(self, "_uncertainty_range_given", False) and tuple(theirs) != tuple(self.uncertainty_range):
                raise ValueError(f"uncertainty_range = {tuple(self.uncertainty_range)!r} is set, but the heads of the "
                                 f"checkpoint in {folder} were trained with {tuple(theirs)!r}: unset the option to adopt "
                                 "the checkpoint's range")
            self.uncertainty_range = theirs
            self.opt.uncertainty_range = list(theirs)
        if st is not None and getattr(self.opt, "resume_state", True):
            if st.get("epoch_complete", True):       # written by train() after run_epoch (scheduler already stepped)
                self.resume_epoch, self.resume_step, self.resume_batch = int(st["epoch"]) + 1, int(st["step"]), 0
            else:                                    # written inside run_epoch: same epoch, next batch, next step
                self.resume_epoch, self.resume_step = int(st["epoch"]), int(st["step"]) + 1
                self.resume_batch = int(st.get("batch_idx", -1)) + 1
            self.model_lr_scheduler.load_state_dict(st["lr_scheduler"])
            PF.DropoutState.seed = int(st["dropout_seed"])
            PF.DropoutState.set_step(getattr(self, "device", None), int(st.get("dropout_step", 0)))
