"""Entry point: ``python -m manydepth.train <flags>`` (reference manydepth/train.py:7-18).

Single GPU: run as is.  Data parallel: ``python -m torch.distributed.run --nproc-per-node N -m
manydepth.train <flags>`` -- one process per GPU, RCCL gradient all-reduce over xGMI.
"""
import os

import torch

from .trainer import Trainer
from .options import MonodepthOptions


def options_from_environment(opts, env=os.environ):
    """The options that are no reference CLI flags, from the variables of the same meaning; returns ``opts``."""
    # PD_BF16=1: the opt-in bf16 training mode of the convolutions (and of the attention variant); the reference CLI has no
    # flag for it, and the library and the Trainer read no environment variable for it -- only this entry point does
    if env.get("PD_BF16") == "1":
        opts.bf16 = True
    # PD_POL_ANGLES="a,b,c,d": the calibrated polarizer angles in degrees, in the order of the planes of ("pol", 0, 0)
    # (opt.pol_angles; default: the nominal 0/45/90/135 set) -- read here only, like PD_BF16
    if env.get("PD_POL_ANGLES"):
        opts.pol_angles = [float(x) for x in env["PD_POL_ANGLES"].split(",")]
    # PD_POL_LAYOUT="2,1,3,0" / PD_POL_DEMOSAIC=bilinear|superpixel: interleaved sensor frames (PD_POL_DOFP=1 makes the loader
    # serve them) -- the plane each site of the 2x2 super-pixel feeds, in reading order, and how the planes are reconstructed
    # (opt.pol_layout / opt.pol_demosaic; defaults: the IMX250MZR's 2,1,3,0 and bilinear)
    if env.get("PD_POL_LAYOUT"):
        opts.pol_layout = [int(x) for x in env["PD_POL_LAYOUT"].split(",")]
    if env.get("PD_POL_DEMOSAIC"):
        opts.pol_demosaic = env["PD_POL_DEMOSAIC"]
    # PD_POL_BAYER=RGGB|BGGR|GRBG|GBRG / PD_POL_GAINS="r,g,b" / PD_POL_COLOR_SCALE: colour sensor frames (PD_POL_CDOFP=1 makes
    # the loader serve them) -- the Bayer order over the polarizer array, white-balance gains and the factor from frame values
    # to the 0..255 of the colour picture, 255/4095 for 12-bit frames (opt.pol_bayer / opt.pol_gains / opt.pol_color_scale;
    # defaults: RGGB, none, 1 for 8-bit frames); PD_POL_LAYOUT is shared
    if env.get("PD_POL_BAYER"):
        opts.pol_bayer = env["PD_POL_BAYER"]
    if env.get("PD_POL_GAINS"):
        opts.pol_gains = [float(x) for x in env["PD_POL_GAINS"].split(",")]
    if env.get("PD_POL_COLOR_SCALE"):
        opts.pol_color_scale = float(env["PD_POL_COLOR_SCALE"])
    # PD_POL_CALIBRATION=cal.npz: the sensor's super-pixel calibration (tools/dofp_calibrate.py writes it), applied to
    # ("pol_dofp", 0, 0) / ("pol_cdofp", 0, 0) frames on the device before their demosaic (opt.pol_calibration; default: none)
    if env.get("PD_POL_CALIBRATION"):
        opts.pol_calibration = env["PD_POL_CALIBRATION"]
    # PD_XOLP_NORM="mean,std": the pair that standardises the XOLP encoder's input, measured on the user's own data by
    # tools/xolp_stats.py (opt.xolp_norm; default: the reference's HAMMER constants, or a loaded checkpoint's pair)
    if env.get("PD_XOLP_NORM"):
        opts.xolp_norm = env["PD_XOLP_NORM"]
    # PD_POSE_NETWORK=1: the photometric term with poses PREDICTED by a pose network (opt.pose_network; needs
    # --depth_supervision True without --depth_supervision_only and without --pose_input); the reference's option table has no
    # flag that could select it here, since --pose_input False alone keeps its present meaning
    if env.get("PD_POSE_NETWORK") == "1":
        opts.pose_network = True
    # PD_MATCHING_POSES=1: with the pose network, also the matching-pose half of predict_poses -- the poses 0 -> fi of the
    # lookup frames of --num_matching_frames / --use_future_frame into inputs[("relative_pose", fi)] (opt.matching_poses)
    if env.get("PD_MATCHING_POSES") == "1":
        opts.matching_poses = True
    # PD_POLAR_LOSS="w_n,w_a": the polarimetric normals loss with these weights on its normal and azimuth terms
    # (opt.polar_loss; works in every training mode of this build, PD_STEP_GRAPH=1 is refused with it).
    # PD_POLAR_LOSS_WHERE=all|holes: every pixel, or only those without ground-truth depth (opt.polar_loss_where; default all).
    # PD_POL_AOLP_SIGN=-1: a sensor of the other AoLP handedness, as for the evaluation's report (opt.pol_aolp_sign)
    # PD_POLAR_RAY_FRAME=1: the term in the frame of each pixel's viewing ray (opt.polar_ray_frame; needs PD_POLAR_LOSS)
    if env.get("PD_POLAR_LOSS"):
        opts.polar_loss = [float(x) for x in env["PD_POLAR_LOSS"].split(",")]
    if env.get("PD_POLAR_LOSS_WHERE"):
        opts.polar_loss_where = env["PD_POLAR_LOSS_WHERE"]
    if env.get("PD_POL_AOLP_SIGN"):
        opts.pol_aolp_sign = int(env["PD_POL_AOLP_SIGN"])
    if env.get("PD_POLAR_RAY_FRAME"):
        opts.polar_ray_frame = env["PD_POLAR_RAY_FRAME"] == "1"
    # PD_UNCERTAINTY_LOSS=w: build the decoder's uncertainty heads and train them as the scale of a Laplace error model of the
    # depth, with weight w (opt.uncertainty_loss; PD_STEP_GRAPH=1, PD_BF16=1 and torch.distributed are refused with it).
    # PD_UNCERTAINTY_RANGE="lo,hi": the scale at u = 0 and u = 1 in metres (opt.uncertainty_range; default 0.0005,0.5: a
    # convention).  PD_UNCERTAINTY_DETACH=1: the term trains the heads only, on top of the network as it is
    # (opt.uncertainty_detach)
    if env.get("PD_UNCERTAINTY_LOSS"):
        opts.uncertainty_loss = float(env["PD_UNCERTAINTY_LOSS"])
    if env.get("PD_UNCERTAINTY_RANGE"):
        opts.uncertainty_range = [float(x) for x in env["PD_UNCERTAINTY_RANGE"].split(",")]
    if env.get("PD_UNCERTAINTY_DETACH"):
        opts.uncertainty_detach = env["PD_UNCERTAINTY_DETACH"] == "1"
    return opts


def main():
    opts = options_from_environment(MonodepthOptions().parse())
    if int(os.environ.get("WORLD_SIZE", 1)) > 1 and not torch.distributed.is_initialized():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        torch.distributed.init_process_group("nccl")      # "nccl" is RCCL on ROCm
    Trainer(opts).train()


if __name__ == "__main__":
    main()
