"""polarisation.xolp façade: ``Iun_and_xolp`` served by the fused HIP kernels of K1.

Reference: polarisation/xolp.py:8-34.  Differences, by design (SURVEY.md §7 hard part 1):
the canonical closed form x = P I, P = (A^T A)^-1 A^T, replaces the LAPACK least-squares solve (identical up to
lstsq noise; the AoLP branch x2 == 0, x1 < 0 is +pi/2), intensities must be exactly representable as uint8, uint16
or float32 (what sensors and image files deliver), and Iun / DoLP / AoLP are the fp32-rounded values the network
consumes (returned as float64 arrays like the reference).

Integer intensities in 0..255 with the 0/45/90/135 degree set take the look-up-table kernel (pd_polar_fwd);
everything else -- any four angles of rank 3, 16-bit or real-valued intensities -- takes the general kernel
(pd_polar_general_fwd).
"""
import numpy as np
import torch

from polardepth import polar as _polar

_ANGLES = np.array([0, 45, 90, 135]) * np.pi / 180


def _planes(images, dtype):
    """[H,W,4] -> device tensor [1,4,1,H*W (+pad)] of ``dtype`` (the kernels work on multiples of 4 pixels)."""
    H, W, _ = images.shape
    pad = (-H * W) % 4
    flat = np.zeros((1, 4, 1, H * W + pad), dtype=dtype)
    flat[0, :, 0, :H * W] = np.moveaxis(images, -1, 0).reshape(4, -1)
    return torch.from_numpy(flat).cuda()


def Iun_and_xolp(images, angles=None):
    """images [H,W,4], angles: the four polarizer angles in radians, in the order of the last axis (None = 0/45/90/135
    degrees) -> (Iun, rho, phi), each [H,W] float64."""
    images = np.asarray(images)
    if images.ndim != 3 or images.shape[2] != 4:
        raise ValueError(f"images must be [H,W,4], got {images.shape}")
    standard = True
    if angles is not None:
        angles = np.asarray(angles, dtype=np.float64).reshape(-1)
        _polar.fit_matrix(angles)         # ValueError unless four finite angles of rank 3
        standard = bool(np.allclose(angles, _ANGLES))
    H, W, _ = images.shape
    unflat = lambda t: t.double().cpu().numpy().reshape(-1)[:H * W].reshape(H, W)
    with np.errstate(invalid="ignore"):
        u8 = images.astype(np.uint8)
        u16 = images.astype(np.uint16)
    if standard and np.array_equal(u8, images):
        out = _polar.polar_forward(_planes(u8, np.uint8), want=("xolp",))["xolp"][0]
        Iun = u8.astype(np.float64).sum(2) / 4.0      # (Imax + Imin) / 2 == x0
        return Iun, unflat(out[0]), unflat(out[1])
    if np.array_equal(u16, images):
        pol = _planes(u16, np.uint16)
    else:
        f64 = images.astype(np.float64)
        f32 = f64.astype(np.float32)
        bad = ~((f32.astype(np.float64) == f64) | (np.isnan(f32) & np.isnan(f64)))
        if bad.any():
            idx = tuple(int(i) for i in np.argwhere(bad)[0])
            raise ValueError(f"Iun_and_xolp (HIP) expects intensities that are exact in uint8, uint16 or float32; "
                             f"images{list(idx)} = {float(f64[idx])!r} is not (nearest float32: {float(f32[idx])!r})")
        pol = _planes(f32, np.float32)
    out = _polar.polar_forward(pol, want=("iun", "xolp"), angles=_ANGLES if angles is None else angles)
    return unflat(out["iun"][0, 0]), unflat(out["xolp"][0, 0]), unflat(out["xolp"][0, 1])
