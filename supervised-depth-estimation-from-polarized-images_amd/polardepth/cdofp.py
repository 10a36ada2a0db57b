"""Demosaic of COLOUR division-of-focal-plane frames on the GPU (csrc/cdofp.hip, pd_cdofp_demosaic).

The colour model of the polarization sensor (Sony IMX250MYR class) has a Bayer colour filter over the polarizer array: every
4x4 super-pixel is a 2x2 Bayer cell of 2x2 polarizer cells, and ONE raw frame holds the RGB picture and the four polarizer
planes.  ``demosaic`` reconstructs both on the full grid (each of the 16 sub-lattices interpolated bilinearly, fp64 in a
fixed order): the float32 planes of ``("pol", 0, 0)`` and the uint8 picture of ``("color_raw", 0, 0)``; ``expand`` does it for
a batch that carries ``("pol_cdofp", 0, 0)``.  The definition is in include/polardepth.h; tests/cdofp_ref.py states it in
NumPy."""
import ctypes
import math

import torch

from ._lib import lib, check, ptr, stream_ptr
from .dofp import parse_layout

# layout[2 (y & 1) + (x & 1)] = the plane of ("pol", 0, 0) the site feeds; bayer[2 ((y >> 1) & 1) + ((x >> 1) & 1)] = its colour
IMX250MYR_POL = (2, 1, 3, 0)      # the polarizer array of the IMX250MZR: 90 / 45 / 135 / 0 degrees in reading order
RGGB, BGGR, GRBG, GBRG = (0, 1, 1, 2), (2, 1, 1, 0), (1, 0, 2, 1), (1, 2, 0, 1)      # 0 = R, 1 = G, 2 = B
BAYER_ORDERS = {"RGGB": RGGB, "BGGR": BGGR, "GRBG": GRBG, "GBRG": GBRG}
WANT = ("planes", "color", "rgb_planes")
_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}             # PD_POLAR_U8 / _U16 / _F32
KEY = ("pol_cdofp", 0, 0)


def parse_bayer(spec):
    """A Bayer order as a tuple of four colour codes (0 = R, 1 = G, 2 = B, cells in reading order): a name ("RGGB", "BGGR",
    "GRBG", "GBRG"), a string "0,1,1,2" or a sequence; ValueError unless it is one of the four orders."""
    if isinstance(spec, str) and spec.strip().upper() in BAYER_ORDERS:
        return BAYER_ORDERS[spec.strip().upper()]
    try:
        order = tuple(int(x) for x in (spec.split(",") if isinstance(spec, str) else spec))
    except (TypeError, ValueError):
        raise ValueError(f"Bayer order must be one of {sorted(BAYER_ORDERS)} or four colour codes, got {spec!r}") from None
    if order not in BAYER_ORDERS.values():
        raise ValueError(f"Bayer order must be one of {sorted(BAYER_ORDERS)} (one R, one B, two G on a diagonal), got {spec!r}")
    return order


def parse_gains(spec):
    """White-balance gains as three finite floats (r, g, b): a sequence, or a string "r,g,b"; None stays None."""
    if spec is None:
        return None
    try:
        gains = tuple(float(x) for x in (spec.split(",") if isinstance(spec, str) else spec))
    except (TypeError, ValueError):
        raise ValueError(f"colour gains must be three numbers r,g,b, got {spec!r}") from None
    if len(gains) != 3 or not all(math.isfinite(g) for g in gains):
        raise ValueError(f"colour gains must be three finite numbers r,g,b, got {spec!r}")
    return gains


def parse_color_scale(spec):
    """The factor from frame values to the 0..255 of the colour picture (255 / 4095 for 12-bit frames): a finite number > 0 or
    a string holding one; None stays None."""
    if spec is None:
        return None
    try:
        scale = float(spec)
    except (TypeError, ValueError):
        raise ValueError(f"color_scale must be a number, got {spec!r}") from None
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"color_scale must be finite and greater than 0, got {spec!r}")
    return scale


def options(layout=None, bayer=None, gains=None, color_scale=None):
    """The ``opts`` argument of ``expand`` from four optional settings (None: IMX250MYR_POL, RGGB, no gains, scale 1 for uint8
    frames), validated: (layout, bayer, gains, color_scale)."""
    return (IMX250MYR_POL if layout is None else parse_layout(layout), RGGB if bayer is None else parse_bayer(bayer),
            parse_gains(gains), parse_color_scale(color_scale))


def demosaic(mosaic, layout=IMX250MYR_POL, bayer=RGGB, gains=None, color_scale=None, want=("planes", "color")):
    """mosaic: uint8 / uint16 / float32 CUDA tensor [B,1,H4,W4] or [B,H4,W4], H4 and W4 multiples of 4.  Returns a dict with
    what ``want`` names: "planes" float32 [B,4,H4,W4] (the polarizer planes in the order ``layout`` names them, Pillow's L of
    the three colours), "color" uint8 [B,3,H4,W4] (the mean of the four planes per colour, times ``color_scale``, rounded) and
    "rgb_planes" float32 [B,4,3,H4,W4].  ``gains``: (r, g, b) multipliers, None = (1,1,1).  ``color_scale=None`` means 1 for
    a uint8 frame; a uint16 / float32 frame with "color" wanted needs one (255 / 4095 for 12-bit data)."""
    if not isinstance(mosaic, torch.Tensor):
        raise RuntimeError("demosaic needs a CUDA(HIP) tensor; there is no CPU fallback")
    want = tuple(want)
    if not want or any(w not in WANT for w in want):
        raise ValueError(f"demosaic: want must name some of {WANT}, got {want!r}")
    layout, bayer, gains, color_scale = options(layout, bayer, gains, color_scale)
    if mosaic.dtype not in _DTYPES:
        raise ValueError(f"demosaic: the mosaic must be uint8, uint16 or float32, got {mosaic.dtype}")
    if not (mosaic.dim() == 3 or (mosaic.dim() == 4 and mosaic.shape[1] == 1)):
        raise ValueError(f"demosaic: the mosaic must be [B,1,H4,W4] or [B,H4,W4], got {tuple(mosaic.shape)}")
    B, H4, W4 = mosaic.shape[0], mosaic.shape[-2], mosaic.shape[-1]
    if H4 < 4 or W4 < 4 or H4 % 4 or W4 % 4:
        raise ValueError(f"demosaic: the mosaic's sides must be multiples of 4 and >= 4, got {H4}x{W4}")
    if color_scale is None:
        if "color" in want and mosaic.dtype != torch.uint8:
            raise ValueError(f'demosaic: a {mosaic.dtype} frame needs color_scale for "color" (255 / 4095 for 12-bit data)')
        color_scale = 1.0
    if not mosaic.is_cuda:      # after the argument checks, which need no device
        raise RuntimeError("demosaic needs a CUDA(HIP) tensor; there is no CPU fallback")
    mosaic = mosaic.contiguous()
    out = {}
    for key, shape, dt in (("planes", (B, 4, H4, W4), torch.float32), ("color", (B, 3, H4, W4), torch.uint8),
                           ("rgb_planes", (B, 4, 3, H4, W4), torch.float32)):
        if key in want:
            out[key] = torch.empty(shape, dtype=dt, device=mosaic.device)
    with torch.cuda.device(mosaic.device):
        check(lib.pd_cdofp_demosaic(ptr(mosaic), _DTYPES[mosaic.dtype], (ctypes.c_int * 4)(*layout), (ctypes.c_int * 4)(*bayer),
                                    None if gains is None else (ctypes.c_double * 3)(*gains), color_scale,
                                    ptr(out.get("planes")), ptr(out.get("color")), ptr(out.get("rgb_planes")), B, H4, W4,
                                    stream_ptr()), "pd_cdofp_demosaic")
    return out


def expand(inputs, opts=None, calibration=None):
    """A batch that carries the colour sensor frame ("pol_cdofp", 0, 0) (``HAMMER_Dataset(pol_cdofp=True)``) and neither
    ("pol", 0, 0) nor ("color_raw", 0, 0) gets both from ONE demosaic call; anything else is left as it is, so a second call
    does nothing.  ``opts``: what ``options`` returns, None = its defaults.  ``calibration``
    (``polardepth.calibration.Calibration``): the frame is calibrated first (every 2x2 polarizer cell lies under one Bayer
    colour, so the same per-cell matrices serve); the calibration keeps the raw frame's level, so ``color_scale`` keeps
    referring to the raw scale, and None still means 1 for a uint8 frame."""
    if KEY in inputs and ("pol", 0, 0) not in inputs and ("color_raw", 0, 0) not in inputs:
        layout, bayer, gains, color_scale = options() if opts is None else opts
        frame = inputs[KEY]
        if calibration is not None:
            from . import calibration as pdcal
            if color_scale is None and frame.dtype == torch.uint8:
                color_scale = 1.0
            frame = pdcal.apply(frame, calibration)
        out = demosaic(frame, layout, bayer, gains, color_scale, want=("planes", "color"))
        inputs[("pol", 0, 0)] = out["planes"]
        inputs[("color_raw", 0, 0)] = out["color"]
    return inputs
