"""Demosaic of division-of-focal-plane (DoFP) polarizer frames on the GPU (csrc/dofp.hip, pd_dofp_demosaic).

A polarization sensor emits ONE interleaved frame: every 2x2 super-pixel carries the four polarizer filters.  ``demosaic``
turns it into the four planes of ``("pol", 0, 0)`` -- by sampling (``"superpixel"``: half-size planes of the frame's own
dtype) or by bilinear interpolation to the full grid (``"bilinear"``: float32 planes; the four samples of a super-pixel sit
at four different positions, so sampling alone reads an unpolarised intensity gradient as polarisation).  The definition is
in include/polardepth.h; tests/dofp_ref.py states it in NumPy."""
import ctypes

import torch

from ._lib import lib, check, ptr, stream_ptr

# layout[2 r + c] = the plane of ("pol", 0, 0) that the site at row parity r, column parity c feeds
IMX250MZR = (2, 1, 3, 0)      # Sony IMX250MZR: 90 / 45 / 135 / 0 degrees in reading order, planes in 0/45/90/135 order
MODES = {"superpixel": 0, "bilinear": 1}                                  # PD_DOFP_SUPERPIXEL / PD_DOFP_BILINEAR
_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}             # PD_POLAR_U8 / _U16 / _F32


def parse_layout(spec):
    """A layout as a tuple of four ints: a sequence, or a string "a,b,c,d"; ValueError unless it is a permutation of 0..3."""
    try:
        layout = tuple(int(x) for x in (spec.split(",") if isinstance(spec, str) else spec))
    except (TypeError, ValueError):
        raise ValueError(f"DoFP layout must be four integers, got {spec!r}") from None
    if sorted(layout) != [0, 1, 2, 3]:
        raise ValueError(f"DoFP layout must be a permutation of 0..3, got {spec!r}")
    return layout


def options(layout=None, mode=None):
    """The ``dofp=(layout, mode)`` argument of ``polardepth.polar.polar_inputs`` from two optional settings (None: IMX250MZR,
    "bilinear"), validated."""
    mode = "bilinear" if mode is None else mode
    if mode not in MODES:
        raise ValueError(f"DoFP demosaic mode must be one of {sorted(MODES)}, got {mode!r}")
    return (IMX250MZR if layout is None else parse_layout(layout), mode)


def demosaic(mosaic, layout=IMX250MZR, mode="bilinear"):
    """mosaic: uint8 / uint16 / float32 CUDA tensor [B,1,H2,W2] or [B,H2,W2], H2 and W2 even.  Returns the planes in the
    order ``layout`` names them: [B,4,H2/2,W2/2] of the same dtype (``mode="superpixel"``) or [B,4,H2,W2] float32
    (``"bilinear"``: fp64 arithmetic rounded once, mirrored edges)."""
    if not (isinstance(mosaic, torch.Tensor) and mosaic.is_cuda):
        raise RuntimeError("demosaic needs a CUDA(HIP) tensor; there is no CPU fallback")
    if mode not in MODES:
        raise ValueError(f"demosaic: mode must be one of {sorted(MODES)}, got {mode!r}")
    layout = parse_layout(layout)
    if mosaic.dtype not in _DTYPES:
        raise ValueError(f"demosaic: the mosaic must be uint8, uint16 or float32, got {mosaic.dtype}")
    if not (mosaic.dim() == 3 or (mosaic.dim() == 4 and mosaic.shape[1] == 1)):
        raise ValueError(f"demosaic: the mosaic must be [B,1,H2,W2] or [B,H2,W2], got {tuple(mosaic.shape)}")
    B, H2, W2 = mosaic.shape[0], mosaic.shape[-2], mosaic.shape[-1]
    if H2 < 2 or W2 < 2 or H2 % 2 or W2 % 2:
        raise ValueError(f"demosaic: the mosaic must have even sides >= 2, got {H2}x{W2}")
    mosaic = mosaic.contiguous()
    if mode == "superpixel":
        planes = torch.empty((B, 4, H2 // 2, W2 // 2), dtype=mosaic.dtype, device=mosaic.device)
    else:
        planes = torch.empty((B, 4, H2, W2), dtype=torch.float32, device=mosaic.device)
    with torch.cuda.device(mosaic.device):
        check(lib.pd_dofp_demosaic(ptr(mosaic), _DTYPES[mosaic.dtype], ptr(planes), MODES[mode], (ctypes.c_int * 4)(*layout),
                                   B, H2, W2, stream_ptr()), "pd_dofp_demosaic")
    return planes
