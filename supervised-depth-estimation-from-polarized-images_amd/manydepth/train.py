"""Entry point: ``python -m manydepth.train <flags>`` (reference manydepth/train.py:7-18).

Single GPU: run as is.  Data parallel: ``python -m torch.distributed.run --nproc-per-node N -m
manydepth.train <flags>`` -- one process per GPU, RCCL gradient all-reduce over xGMI.
"""
import os

import torch

from .trainer import Trainer
from .options import MonodepthOptions


def main():
    opts = MonodepthOptions().parse()
    # PD_BF16=1: the opt-in bf16 training mode of the convolutions (and of the attention variant); the reference CLI has no
    # flag for it, and the library and the Trainer read no environment variable for it -- only this entry point does
    if os.environ.get("PD_BF16") == "1":
        opts.bf16 = True
    # PD_POL_ANGLES="a,b,c,d": the calibrated polarizer angles in degrees, in the order of the planes of ("pol", 0, 0)
    # (opt.pol_angles; default: the nominal 0/45/90/135 set) -- read here only, like PD_BF16
    if os.environ.get("PD_POL_ANGLES"):
        opts.pol_angles = [float(x) for x in os.environ["PD_POL_ANGLES"].split(",")]
    # PD_POL_LAYOUT="2,1,3,0" / PD_POL_DEMOSAIC=bilinear|superpixel: interleaved sensor frames (PD_POL_DOFP=1 makes the loader
    # serve them) -- the plane each site of the 2x2 super-pixel feeds, in reading order, and how the planes are reconstructed
    # (opt.pol_layout / opt.pol_demosaic; defaults: the IMX250MZR's 2,1,3,0 and bilinear)
    if os.environ.get("PD_POL_LAYOUT"):
        opts.pol_layout = [int(x) for x in os.environ["PD_POL_LAYOUT"].split(",")]
    if os.environ.get("PD_POL_DEMOSAIC"):
        opts.pol_demosaic = os.environ["PD_POL_DEMOSAIC"]
    # PD_POL_BAYER=RGGB|BGGR|GRBG|GBRG / PD_POL_GAINS="r,g,b" / PD_POL_COLOR_SCALE: colour sensor frames (PD_POL_CDOFP=1 makes
    # the loader serve them) -- the Bayer order over the polarizer array, white-balance gains and the factor from frame values
    # to the 0..255 of the colour picture, 255/4095 for 12-bit frames (opt.pol_bayer / opt.pol_gains / opt.pol_color_scale;
    # defaults: RGGB, none, 1 for 8-bit frames); PD_POL_LAYOUT is shared
    if os.environ.get("PD_POL_BAYER"):
        opts.pol_bayer = os.environ["PD_POL_BAYER"]
    if os.environ.get("PD_POL_GAINS"):
        opts.pol_gains = [float(x) for x in os.environ["PD_POL_GAINS"].split(",")]
    if os.environ.get("PD_POL_COLOR_SCALE"):
        opts.pol_color_scale = float(os.environ["PD_POL_COLOR_SCALE"])
    if int(os.environ.get("WORLD_SIZE", 1)) > 1 and not torch.distributed.is_initialized():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        torch.distributed.init_process_group("nccl")      # "nccl" is RCCL on ROCm
    Trainer(opts).train()


if __name__ == "__main__":
    main()
