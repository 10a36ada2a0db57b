"""Pillow's LANCZOS resize (``Image.resize(size, Image.ANTIALIAS)``, indoor_dataset.py:335-349) on the GPU: uint8 planes
(mode ``L``), and the two other element types K1 takes, uint16 (``I;16``) and float32 (``F``).

The coefficient tables follow Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` (src/libImaging/Resample.c)
literally, in double precision with libm's sin (``math.sin``), so the device result is bit-identical to PIL."""
import functools
import math

import numpy as np
import torch

from ._lib import lib, check, ptr, stream_ptr

PRECISION_BITS = 32 - 8 - 2
_LANCZOS_SUPPORT = 3.0


def _lanczos(x):
    def sinc(v):
        if v == 0.0:
            return 1.0
        v *= math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def _precompute_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs: (k float64 [out_size, ksize] = w[x] / ww, bounds int32 [out_size, 2])."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = _LANCZOS_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.float64)
    bounds = np.zeros((out_size, 2), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            kk[xx, x] = w[x] / ww if ww != 0.0 else w[x]
        bounds[xx] = (xmin, xmax)
    return kk, bounds


@functools.lru_cache(maxsize=64)
def lanczos_coeffs(in_size, out_size):
    """(coeffs int32 [out_size, ksize], bounds int32 [out_size, 2]) of one resampling pass (normalize_coeffs_8bpc)."""
    k, bounds = _precompute_coeffs(in_size, out_size)
    kk = np.zeros(k.shape, np.int32)
    for xx in range(out_size):
        for x in range(bounds[xx, 1]):
            v = float(k[xx, x])
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return kk, bounds


@functools.lru_cache(maxsize=64)
def lanczos_coeffs_f64(in_size, out_size):
    """(coeffs float64 [out_size, ksize], bounds int32 [out_size, 2]) of one pass over 16-bit or float planes: the
    coefficients as precompute_coeffs leaves them (``w[x] / ww`` in double), the bounds of ``lanczos_coeffs``."""
    return _precompute_coeffs(in_size, out_size)


_DEV_TABLES = {}


def _tables(in_size, out_size, device):
    key = (in_size, out_size, device.index)
    t = _DEV_TABLES.get(key)
    if t is None:
        kk, b = lanczos_coeffs(in_size, out_size)
        t = (torch.from_numpy(kk).to(device), torch.from_numpy(b).to(device), kk.shape[1])
        _DEV_TABLES[key] = t
    return t


def _tables_f64(in_size, out_size, device):
    """The double tables, uploaded on the first call for a size and device like the integer ones: for a captured step that
    is its warm-up run, outside the captured region."""
    key = (in_size, out_size, device.index, "f64")
    t = _DEV_TABLES.get(key)
    if t is None:
        kk, b = lanczos_coeffs_f64(in_size, out_size)
        t = (torch.from_numpy(kk).to(device), torch.from_numpy(b).to(device), kk.shape[1])
        _DEV_TABLES[key] = t
    return t


def resize_lanczos_u8(x, size):
    """x: uint8 CUDA tensor [..., Hs, Ws]; size = (Hd, Wd).  Horizontal pass, then vertical pass (Pillow's order)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8):
        raise RuntimeError("resize_lanczos_u8 needs a CUDA(HIP) uint8 tensor; there is no CPU fallback (PIL is the CPU path)")
    Hd, Wd = int(size[0]), int(size[1])
    lead, (Hs, Ws) = x.shape[:-2], x.shape[-2:]
    P = int(np.prod(lead)) if lead else 1
    cur = x.contiguous().view(P, Hs, Ws)
    with torch.cuda.device(x.device):
        if Wd != Ws:
            kk, b, ks = _tables(Ws, Wd, x.device)
            out = torch.empty((P, Hs, Wd), dtype=torch.uint8, device=x.device)
            check(lib.pd_resize_u8_pass(ptr(cur), ptr(out), ptr(kk), ptr(b), ks, P, Hs, Ws, Wd, 0, stream_ptr()),
                  "pd_resize_u8_pass")
            cur = out
        if Hd != Hs:
            kk, b, ks = _tables(Hs, Hd, x.device)
            out = torch.empty((P, Hd, cur.shape[2]), dtype=torch.uint8, device=x.device)
            check(lib.pd_resize_u8_pass(ptr(cur), ptr(out), ptr(kk), ptr(b), ks, P, Hs, cur.shape[2], Hd, 1, stream_ptr()),
                  "pd_resize_u8_pass")
            cur = out
    return cur.view(*lead, Hd, Wd)


_WIDE_DTYPES = {torch.uint16: 1, torch.float32: 2}      # PD_POLAR_U16 / PD_POLAR_F32


def resize_lanczos(x, size):
    """x: uint8, uint16 or float32 CUDA tensor [..., Hs, Ws]; size = (Hd, Wd).  What ``Image.resize((Wd, Hd), Image.LANCZOS)``
    gives for every plane in mode ``L`` / ``I;16`` / ``F``, bit for bit.  uint8 is ``resize_lanczos_u8``.  uint16 rounds and
    stores like Pillow: undershoot becomes 0, overshoot past 65535 clips the high byte to 255 and wraps the low byte
    (include/polardepth.h, pd_resize_wide_pass).  float32: NaN and infinity spread over their filter windows as IEEE has it."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise RuntimeError("resize_lanczos needs a CUDA(HIP) tensor; there is no CPU fallback (PIL is the CPU path)")
    if x.dtype == torch.uint8:
        return resize_lanczos_u8(x, size)
    if x.dtype not in _WIDE_DTYPES:
        raise ValueError(f"resize_lanczos serves uint8, uint16 and float32 planes, got {x.dtype}")
    if x.dim() < 2:
        raise ValueError(f"resize_lanczos: expected [..., Hs, Ws], got {tuple(x.shape)}")
    dt = _WIDE_DTYPES[x.dtype]
    Hd, Wd = int(size[0]), int(size[1])
    lead, (Hs, Ws) = x.shape[:-2], x.shape[-2:]
    P = int(np.prod(lead)) if lead else 1
    cur = x.contiguous().view(P, Hs, Ws)
    with torch.cuda.device(x.device):
        if Wd != Ws:
            kk, b, ks = _tables_f64(Ws, Wd, x.device)
            out = torch.empty((P, Hs, Wd), dtype=x.dtype, device=x.device)
            check(lib.pd_resize_wide_pass(ptr(cur), ptr(out), dt, ptr(kk), ptr(b), ks, P, Hs, Ws, Wd, 0, stream_ptr()),
                  "pd_resize_wide_pass")
            cur = out
        if Hd != Hs:
            kk, b, ks = _tables_f64(Hs, Hd, x.device)
            out = torch.empty((P, Hd, cur.shape[2]), dtype=x.dtype, device=x.device)
            check(lib.pd_resize_wide_pass(ptr(cur), ptr(out), dt, ptr(kk), ptr(b), ks, P, Hs, cur.shape[2], Hd, 1, stream_ptr()),
                  "pd_resize_wide_pass")
            cur = out
    return cur.view(*lead, Hd, Wd)
