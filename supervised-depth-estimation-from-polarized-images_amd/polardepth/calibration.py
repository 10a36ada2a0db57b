"""Super-pixel calibration of division-of-focal-plane (DoFP) polarizer frames on the GPU (csrc/dofp_cal.hip).

A real polarization sensor is not four ideal analyzers per super-pixel: gains, extinction ratios and filter angles vary from
pixel to pixel and there is a dark offset.  The classical remedy (Powell & Gruev, Opt. Express 2013) is a dark frame plus one
4x4 matrix per 2x2 polarizer cell that maps the four measured samples to what an ideal cell would have measured.  ``fit``
estimates the matrices once, offline, from flat-field frames behind a rotating linear polarizer (pd_frame_moments,
pd_dofp_cal_solve); ``apply`` corrects incoming frames on the data path, before the demosaic (pd_dofp_calibrate: no
allocation beyond its output, no synchronisation, capturable).  The definition is in include/polardepth.h;
tests/dofp_cal_ref.py states it in NumPy and the device agrees with it bit for bit."""
import ctypes

import numpy as np
import torch

from ._lib import lib, check, ptr, stream_ptr
from .dofp import IMX250MZR, parse_layout

_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}             # PD_POLAR_U8 / _U16 / _F32
KINDS = {"cell": 0, "pixel": 1}                                           # PD_DOFP_CAL_CELL / PD_DOFP_CAL_PIXEL
NOMINAL_DEG = (0.0, 45.0, 90.0, 135.0)
VERSION = 1


def _frames(frames, what, cuda=True):
    """[N,H2,W2] or [N,1,H2,W2] of a supported dtype with even sides -> contiguous [N,H2,W2]"""
    if not isinstance(frames, torch.Tensor) or (cuda and not frames.is_cuda):
        raise RuntimeError(f"{what} needs a CUDA(HIP) tensor; there is no CPU fallback")
    if frames.dtype not in _DTYPES:
        raise ValueError(f"{what}: the frames must be uint8, uint16 or float32, got {frames.dtype}")
    if not (frames.dim() == 3 or (frames.dim() == 4 and frames.shape[1] == 1)):
        raise ValueError(f"{what}: the frames must be [N,1,H2,W2] or [N,H2,W2], got {tuple(frames.shape)}")
    H2, W2 = frames.shape[-2], frames.shape[-1]
    if H2 < 2 or W2 < 2 or H2 % 2 or W2 % 2:
        raise ValueError(f"{what}: the frames must have even sides >= 2, got {H2}x{W2}")
    return frames.reshape(frames.shape[0], H2, W2).contiguous()


def _dark(dark, frames, what):
    if dark is None:
        return None
    dark = torch.as_tensor(dark)
    if tuple(dark.shape) != tuple(frames.shape[-2:]):
        raise ValueError(f"{what}: the dark frame is {tuple(dark.shape)}, the frames are {tuple(frames.shape[-2:])}")
    return dark.to(frames.device, torch.float32).contiguous()


def frame_moments(frames, weights, dark=None, out=None):
    """out[q] (+)= sum_n weights[n][q] * (frames[n] - dark) in fp64, n ascending (pd_frame_moments).  frames: CUDA [N,H2,W2] or
    [N,1,H2,W2]; weights: [N,Q] (Q in 1..4), anything ``torch.as_tensor`` takes; ``out``: a float64 [Q,H2,W2] tensor to
    accumulate onto (in place), None = start from zero.  Returns the float64 [Q,H2,W2] tensor."""
    frames = _frames(frames, "frame_moments")
    N, H2, W2 = frames.shape
    w = torch.as_tensor(weights, dtype=torch.float64)
    if w.dim() != 2 or w.shape[0] != N or not 1 <= w.shape[1] <= 4:
        raise ValueError(f"frame_moments: weights must be [N={N}, Q in 1..4], got {tuple(w.shape)}")
    if N < 1:
        raise ValueError("frame_moments: needs at least one frame, got 0")
    Q = w.shape[1]
    w = w.to(frames.device).contiguous()
    dark = _dark(dark, frames, "frame_moments")
    if out is None:
        acc, accumulate = torch.empty((Q, H2, W2), dtype=torch.float64, device=frames.device), 0
    else:
        if not (out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (Q, H2, W2) and out.is_contiguous()):
            raise ValueError(f"frame_moments: out must be a contiguous CUDA float64 {(Q, H2, W2)} tensor, got {out.dtype} "
                             f"{tuple(out.shape)}")
        acc, accumulate = out, 1
    with torch.cuda.device(frames.device):
        check(lib.pd_frame_moments(ptr(frames), _DTYPES[frames.dtype], ptr(dark), ptr(w), ptr(acc), N, Q, H2, W2, accumulate,
                                   stream_ptr()), "pd_frame_moments")
    return acc


def _chunks(frames):
    """One tensor or an iterable of chunks -> an iterator over chunks, consumed one at a time."""
    return iter([frames] if isinstance(frames, torch.Tensor) else frames)


def mean_frame(frames, count=None):
    """The mean of a stack of frames as float32 [H2,W2] (fp64 sum of frame / N in frame order, rounded once): the dark frame
    from a stack taken with the cap on.  ``frames``: CUDA [N,H2,W2] / [N,1,H2,W2], or an iterable of such chunks.  The weight
    1 / N is part of every term, so N must be known before the first chunk: a tensor, a list or a tuple says it itself; for any
    other iterable (a generator that loads chunks from disk) pass ``count`` = N, and the chunks are taken one at a time, each
    released before the next is asked for, so N frames need not fit in memory."""
    if count is None:
        if isinstance(frames, torch.Tensor):
            count = int(frames.shape[0])
        elif isinstance(frames, (list, tuple)):
            count = sum(int(c.shape[0]) for c in frames)
        else:
            raise ValueError("mean_frame: the number of frames of an iterable of chunks is not known in advance; pass count=N")
    count = int(count)
    if count < 1:
        raise ValueError(f"mean_frame: needs at least one frame, got {count}")
    acc, seen, it = None, 0, _chunks(frames)
    while True:
        c = next(it, None)
        if c is None:
            break
        seen += int(c.shape[0])
        if seen > count:
            raise ValueError(f"mean_frame: more than the announced {count} frames")
        acc = frame_moments(c, np.full((int(c.shape[0]), 1), 1.0 / count), out=acc)
        del c                                                  # the caller's generator may free the chunk now
    if seen != count:
        raise ValueError(f"mean_frame: {seen} frames, but count = {count}")
    return acc[0].float()


def fit_weights(polarizer_deg, dolp=1.0, intensity=None):
    """w[n] = intensity[n] * (1, dolp cos 2a_n, dolp sin 2a_n) as float64 [N,3]."""
    a = np.deg2rad(np.asarray(polarizer_deg, np.float64))
    iota = np.ones_like(a) if intensity is None else np.asarray(intensity, np.float64)
    if a.ndim != 1 or iota.shape != a.shape:
        raise ValueError(f"fit: polarizer_deg and intensity must be sequences of one length, got {polarizer_deg!r}, {intensity!r}")
    return np.stack([iota, iota * (dolp * np.cos(2.0 * a)), iota * (dolp * np.sin(2.0 * a))], axis=1)


def nominal_matrix(layout=IMX250MZR, pol_angles=None):
    """float64 [4 sites][3]: row s = 1/2 (1, cos 2 theta_s, sin 2 theta_s), theta_s the nominal angle of the plane that site s
    feeds (``pol_angles``: degrees in plane order, None = 0/45/90/135)."""
    layout = parse_layout(layout)
    deg = NOMINAL_DEG if pol_angles is None else tuple(float(x) for x in pol_angles)
    if len(deg) != 4:
        raise ValueError(f"pol_angles must be four angles in degrees, got {pol_angles!r}")
    th = np.deg2rad(np.asarray([deg[layout[s]] for s in range(4)], np.float64))
    return 0.5 * np.stack([np.ones_like(th), np.cos(2.0 * th), np.sin(2.0 * th)], axis=1)


def solve(moments, rinv, a_nom, qmin=1e-3, want_quality=True):
    """The per-cell matrices from the three moments (pd_dofp_cal_solve): float32 [H2/2,W2/2,4,4] and the quality float32
    [H2/2,W2/2] (None unless wanted)."""
    if not (isinstance(moments, torch.Tensor) and moments.is_cuda):
        raise RuntimeError("solve needs a CUDA(HIP) tensor; there is no CPU fallback")
    if moments.dtype != torch.float64 or moments.dim() != 3 or moments.shape[0] != 3:
        raise ValueError(f"solve: moments must be float64 [3,H2,W2], got {moments.dtype} {tuple(moments.shape)}")
    moments = moments.contiguous()
    H2, W2 = moments.shape[1:]
    rinv = np.ascontiguousarray(rinv, np.float64).reshape(9)
    a_nom = np.ascontiguousarray(a_nom, np.float64).reshape(12)
    gain = torch.empty((H2 // 2, W2 // 2, 4, 4), dtype=torch.float32, device=moments.device)
    quality = torch.empty((H2 // 2, W2 // 2), dtype=torch.float32, device=moments.device) if want_quality else None
    with torch.cuda.device(moments.device):
        check(lib.pd_dofp_cal_solve(ptr(moments), rinv.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    a_nom.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(qmin), ptr(gain), ptr(quality),
                                    H2, W2, stream_ptr()), "pd_dofp_cal_solve")
    return gain, quality


class Calibration:
    """dark: float32 [H2,W2] or None; gain: float32 [H2/2,W2/2,4,4] (one matrix per cell, in site order) or [H2,W2] (the
    classical per-pixel flat-field gain); quality: float32 [H2/2,W2/2] or None (Hadamard's ratio of the cell's fit, 0 = the
    cell could not be fitted and keeps the identity); layout / pol_angles: what the nominal cell was taken to be."""

    def __init__(self, gain, dark=None, quality=None, layout=IMX250MZR, pol_angles=None):
        self.gain = torch.as_tensor(gain, dtype=torch.float32).contiguous()
        if self.gain.dim() == 4 and tuple(self.gain.shape[2:]) == (4, 4):
            self.shape = (2 * self.gain.shape[0], 2 * self.gain.shape[1])
        elif self.gain.dim() == 2 and self.gain.shape[0] % 2 == 0 and self.gain.shape[1] % 2 == 0 and self.gain.numel():
            self.shape = tuple(self.gain.shape)
        else:
            raise ValueError(f"Calibration: gain must be [H2/2,W2/2,4,4] or [H2,W2] with even sides, got {tuple(self.gain.shape)}")
        self.dark = None if dark is None else torch.as_tensor(dark, dtype=torch.float32).to(self.gain.device).contiguous()
        if self.dark is not None and tuple(self.dark.shape) != self.shape:
            raise ValueError(f"Calibration: the dark frame is {tuple(self.dark.shape)}, the gain serves frames of {self.shape}")
        self.quality = None if quality is None else torch.as_tensor(quality, dtype=torch.float32).to(self.gain.device).contiguous()
        self.layout = parse_layout(layout)
        self.pol_angles = None if pol_angles is None else tuple(float(x) for x in pol_angles)
        self.bad_cells = 0 if self.quality is None else int((self.quality == 0).sum())

    @property
    def kind(self):
        return "cell" if self.gain.dim() == 4 else "pixel"

    @property
    def device(self):
        return self.gain.device

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        cal = Calibration.__new__(Calibration)
        cal.gain, cal.dark, cal.quality = mv(self.gain), mv(self.dark), mv(self.quality)
        cal.shape, cal.layout, cal.pol_angles, cal.bad_cells = self.shape, self.layout, self.pol_angles, self.bad_cells
        return cal

    def save(self, path):
        arrays = {"version": np.int32(VERSION), "gain": self.gain.cpu().numpy(), "layout": np.asarray(self.layout, np.int32)}
        for name in ("dark", "quality"):
            if getattr(self, name) is not None:
                arrays[name] = getattr(self, name).cpu().numpy()
        if self.pol_angles is not None:
            arrays["pol_angles"] = np.asarray(self.pol_angles, np.float64)
        with open(path, "wb") as f:      # np.savez(path) would append ".npz" to a name without it
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "version" not in z.files or int(z["version"]) != VERSION:
                raise ValueError(f"{path}: not a calibration file of version {VERSION} "
                                 f"(version = {int(z['version']) if 'version' in z.files else None})")
            get = lambda name: z[name] if name in z.files else None
            return cls(z["gain"], get("dark"), get("quality"), tuple(int(x) for x in z["layout"]), get("pol_angles"))

    @classmethod
    def from_flat_field(cls, flat_mean, dark=None, layout=IMX250MZR):
        """The PIXEL kind from a mean flat-field frame under unpolarised light, on the host, offline: gain = (mean of the
        pixel's site class) / (pixel) of flat_mean - dark, so every site class keeps its mean level."""
        e = torch.as_tensor(flat_mean).cpu().numpy().astype(np.float64)
        d = None if dark is None else torch.as_tensor(dark).cpu().numpy().astype(np.float32)
        if e.ndim != 2 or e.shape[0] % 2 or e.shape[1] % 2 or not e.size:
            raise ValueError(f"from_flat_field: the flat field must be [H2,W2] with even sides, got {e.shape}")
        if d is not None:
            e = e - d.astype(np.float64)
        g = np.empty(e.shape, np.float64)
        with np.errstate(all="ignore"):
            for r in (0, 1):
                for c in (0, 1):
                    g[r::2, c::2] = np.mean(e[r::2, c::2]) / e[r::2, c::2]
        return cls(g.astype(np.float32), d, None, layout)


def parse(spec, device=None):
    """None, a ``Calibration`` or the path of a saved one -> None or a ``Calibration`` (on ``device`` when given)."""
    if spec is None:
        return None
    cal = spec if isinstance(spec, Calibration) else Calibration.load(spec)
    return cal if device is None else cal.to(device)


def check_dataset(cal, dataset, what="the loader"):
    """A calibration serves one sensor.  True when ``dataset`` (a ``HAMMER_Dataset``) serves ("pol_dofp", 0, 0) /
    ("pol_cdofp", 0, 0) frames from files and its first one has the calibration's size (read from the file's header: nothing is
    decoded), False when it serves no sensor frames; a frame of another size is a ValueError that names both."""
    import os
    sensor = "pol_dofp" if getattr(dataset, "pol_dofp", False) else ("pol_cdofp" if getattr(dataset, "pol_cdofp", False) else None)
    if sensor is None or not getattr(dataset, "frames", None):
        return False
    from PIL import Image
    folder, idx = dataset.frames[0]
    path = os.path.join(folder, sensor, "{:06d}.png".format(idx))
    with Image.open(path) as im:
        w, h = im.size
    if (h, w) != tuple(cal.shape):
        raise ValueError(f"the calibration serves frames of {cal.shape[0]}x{cal.shape[1]}, {what}'s {path} is {h}x{w}")
    return True


def fit(frames, polarizer_deg, dark=None, layout=IMX250MZR, pol_angles=None, dolp=1.0, intensity=None, qmin=1e-3):
    """Fit the per-cell matrices from N flat-field frames behind a linear polarizer at ``polarizer_deg[n]`` degrees.

    frames: CUDA [N,H2,W2] or [N,1,H2,W2] (uint8 / uint16 / float32), or an iterable of such chunks in the order of
    ``polarizer_deg``, taken one at a time and released before the next is asked for (N need not fit in memory: the moments
    accumulate).  dark: the mean dark frame (``mean_frame``) or None.
    layout / pol_angles: the nominal cell, as everywhere (which plane each site feeds; the planes' angles in degrees, None =
    0/45/90/135).  dolp: the polarizer's degree of polarization.  intensity: the relative radiometric level of every frame in
    units in which an ideal site reads 1/2 (1 + dolp cos(2 theta - 2 a)); None: the level is unknown and is taken from the
    frames so that calibrated frames keep the mean level of raw - dark.  Cells whose fit has Hadamard ratio below ``qmin``
    keep the identity (``Calibration.bad_cells``).  Offline: the call synchronises and copies."""
    layout = parse_layout(layout)
    w = fit_weights(polarizer_deg, dolp, intensity)
    if len(w) < 3:
        raise ValueError(f"fit: needs at least three polarizer angles, got {len(w)}")
    M, n0, it = None, 0, _chunks(frames)
    while True:                                                # one chunk at a time: N frames need not fit in memory
        c = next(it, None)
        if c is None:
            break
        n1 = n0 + int(c.shape[0])
        if n1 > len(w):
            raise ValueError(f"fit: {n1} frames but {len(w)} polarizer angles")
        M = frame_moments(c, w[n0:n1], dark, out=M)
        n0 = n1
        del c                                                  # the caller's generator may free the chunk now
    if n0 != len(w):
        raise ValueError(f"fit: {n0} frames but {len(w)} polarizer angles")
    R1 = (w[:, :, None] * w[:, None, :]).sum(axis=0)
    kappa = 1.0 if intensity is not None else 2.0 * np.mean(M[0].cpu().numpy()) / len(w)
    if not (np.isfinite(kappa) and kappa > 0):
        raise ValueError(f"fit: the mean level of the flat-field frames is {kappa}; it must be finite and positive")
    rinv = np.linalg.inv(R1) / kappa
    gain, quality = solve(M, rinv, nominal_matrix(layout, pol_angles), qmin)
    d = None if dark is None else _dark(dark, M, "fit")
    return Calibration(gain, d, quality, layout, pol_angles)


def apply(mosaic, cal):
    """mosaic: uint8 / uint16 / float32 CUDA tensor [B,1,H2,W2] or [B,H2,W2] -> float32 of the same shape: dark subtracted and
    every cell multiplied by its matrix (or every pixel by its gain), fp64 rounded once (pd_dofp_calibrate)."""
    if not isinstance(cal, Calibration):
        raise TypeError(f"apply: cal must be a Calibration, got {type(cal).__name__}")
    if not (isinstance(mosaic, torch.Tensor) and mosaic.is_cuda):
        raise RuntimeError("apply needs a CUDA(HIP) tensor; there is no CPU fallback")
    shape = mosaic.shape
    m = _frames(mosaic, "apply")
    if tuple(m.shape[1:]) != tuple(cal.shape):
        raise ValueError(f"apply: the frame is {m.shape[1]}x{m.shape[2]}, the calibration serves {cal.shape[0]}x{cal.shape[1]}")
    if cal.gain.device != m.device:
        raise ValueError(f"apply: the calibration is on {cal.gain.device}, the frame on {m.device}; use Calibration.to once")
    out = torch.empty(m.shape, dtype=torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        check(lib.pd_dofp_calibrate(ptr(m), _DTYPES[m.dtype], ptr(cal.dark), ptr(cal.gain), KINDS[cal.kind], ptr(out),
                                    m.shape[0], m.shape[1], m.shape[2], stream_ptr()), "pd_dofp_calibrate")
    return out.reshape(shape)
