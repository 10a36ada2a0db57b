"""Host wrapper of K1, the fused Stokes/DoLP/AoLP/normals kernel (csrc/polar.hip).

Mirrors polarisation/xolp.py:8-34 (Iun_and_xolp), indoor_dataset.py:430-442 (get_xolp),
normals_vec.py:11-60 and pre_encoders.py:78-79,99-113 of the reference.
"""
import ctypes
import functools

import numpy as np
import torch

from ._lib import lib, check, ptr, stream_ptr

MODE_LS, MODE_STOKES = 0, 1
N_THETA = 1000


def theta_tables_numpy(n=1.5):
    """The three theta(rho) tables exactly as the reference builds them (NumPy, fp64).

    normals_vec.py:13-19 (diffuse) and :27-47 (specular split at argmax); each table is
    returned x-ascending the way scipy.interp1d(assume_sorted=False) stores it.
    """
    th = np.linspace(0, np.pi / 2, N_THETA)
    s = np.sin(th)
    rho_d = ((n - 1 / n) ** 2 * s ** 2) / (
        2 + 2 * n ** 2 - (n + 1 / n) ** 2 * s ** 2 + 4 * np.cos(th) * np.sqrt(n ** 2 - s ** 2))
    rho_s = (2 * s ** 2 * np.cos(th) * np.sqrt(n ** 2 - s ** 2)) / (
        n ** 2 - s ** 2 - n ** 2 * s ** 2 + 2 * s ** 4)
    imax = int(np.argmax(rho_s))

    def asc(x, y):
        ind = np.argsort(x, kind="mergesort")
        return np.ascontiguousarray(x[ind]), np.ascontiguousarray(y[ind])

    return asc(rho_d, th), asc(rho_s[:imax], th[:imax]), asc(rho_s[imax:], th[imax:])


def pack_tables(tables):
    """[(x,y)]*3 fp64 -> packed host blob (uint8 tensor) via pd_polar_tables_pack."""
    (xd, yd), (x1, y1), (x2, y2) = tables
    nbytes = lib.pd_polar_tables_bytes(len(xd), len(x1), len(x2))
    if nbytes == 0:
        raise ValueError("theta tables need at least two nodes each")
    blob = torch.empty(nbytes, dtype=torch.uint8)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    check(lib.pd_polar_tables_pack(dp(xd), dp(yd), len(xd), dp(x1), dp(y1), len(x1), dp(x2), dp(y2), len(x2),
                                   ctypes.c_void_p(blob.data_ptr()), nbytes), "pd_polar_tables_pack")
    return blob


def build_tables_libm(n=1.5):
    """Packed blob computed entirely inside the library (libm); for C-only consumers."""
    nbytes = lib.pd_polar_tables_bytes(N_THETA, N_THETA, N_THETA)
    blob = torch.empty(nbytes, dtype=torch.uint8)
    used = ctypes.c_size_t(0)
    check(lib.pd_polar_tables_build(float(n), ctypes.c_void_p(blob.data_ptr()), nbytes, ctypes.byref(used)),
          "pd_polar_tables_build")
    return blob[:used.value].clone()


@functools.lru_cache(maxsize=8)
def _device_tables(n, device_index):
    blob = pack_tables(theta_tables_numpy(n))
    return blob.to(torch.device("cuda", device_index))


STD_ANGLES = np.array([0.0, 45.0, 90.0, 135.0]) * np.pi / 180
DTYPE_U8, DTYPE_U16, DTYPE_F32 = 0, 1, 2      # PD_POLAR_U8 / _U16 / _F32
_GENERAL_DTYPES = {torch.uint8: DTYPE_U8, torch.uint16: DTYPE_U16, torch.float32: DTYPE_F32}


def fit_matrix(angles):
    """The 3x4 least-squares coefficients P = (A^T A)^-1 A^T of I(theta) = x0 + x1 cos 2theta + x2 sin 2theta for four
    polarizer angles in radians (pd_polar_fit_matrix: host only, fp64).  float64 [3,4]; ValueError for anything but four
    finite angles of rank 3."""
    a = np.ascontiguousarray(np.asarray(angles, dtype=np.float64).reshape(-1))
    if a.size != 4:
        raise ValueError(f"fit_matrix needs four polarizer angles, got {a.size}")
    coef = np.empty(12, dtype=np.float64)
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if lib.pd_polar_fit_matrix(dp(a), dp(coef)) != 0:
        msg = lib.pd_last_error()
        raise ValueError(msg.decode() if msg else "pd_polar_fit_matrix failed")
    return coef.reshape(3, 4)


def angles_from_degrees(spec):
    """Four polarizer angles in degrees -- a sequence, or a string "a,b,c,d" -- as a float64 radians array for
    ``polar_forward(angles=)``; None stays None.  ValueError unless they are four finite angles of rank 3."""
    if spec is None:
        return None
    if isinstance(spec, str):
        spec = [float(x) for x in spec.split(",")]
    angles = np.asarray(spec, dtype=np.float64).reshape(-1) * np.pi / 180
    fit_matrix(angles)
    return angles


def _polar_general(pol, angles, n, want, tables, out_width, out, precise):
    """The general kernel (pd_polar_general_fwd): any four angles, uint8 / uint16 / float32 planes."""
    coef = np.ascontiguousarray(fit_matrix(STD_ANGLES if angles is None else angles).reshape(-1))
    pol = pol.contiguous()
    B, _, H, W = pol.shape
    if tables is None and "normals" in want:
        tables = _device_tables(float(n), pol.device.index)
    out = dict(out) if out is not None else {}      # pre-allocated outputs may be passed in
    Wout = W if out_width is None else int(out_width)
    for key, ch in (("iun", 1), ("xolp", 2), ("xolp_std", 2), ("normals", 9)):
        if key in want and key not in out:
            out[key] = torch.empty((B, ch, H, Wout), dtype=torch.float32, device=pol.device)
    with torch.cuda.device(pol.device):
        check(lib.pd_polar_general_fwd(ptr(pol), _GENERAL_DTYPES[pol.dtype], coef.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       ptr(out.get("iun")), ptr(out.get("xolp")), ptr(out.get("xolp_std")),
                                       ptr(out.get("normals")), ptr(tables), 0 if tables is None else tables.numel(),
                                       B, H, W, Wout, int(bool(precise)), stream_ptr()), "pd_polar_general_fwd")
    return out


def polar_forward(pol, n=1.5, mode=MODE_LS, mask=None, want=("xolp",), tables=None, out_width=None, out=None,
                  precise=False, ieee_rho=False, nt_loads=None, angles=None):
    """Run K1 on ``pol`` [B,4,H,W] uint8 (planes 0/45/90/135 deg) on the GPU.

    want: any of "xolp", "xolp_std", "normals", "ints".  Returns a dict of fp32 NCHW tensors
    ([B,2,H,W], [B,2,H,W], [B,9,H,W]) and the int32 [B,5,H,W] by-products.  out_width > W makes every
    output [.., H, out_width] with the extra right columns zero (612 -> 640 padding for the network).
    precise=True selects PD_POLAR_PRECISE_NORMALS (fp64 theta trig; the default fp32 path is within ~3e-7 of it);
    ieee_rho=True selects PD_POLAR_IEEE_RHO (the literal fp64 sqrt/div sequence for every pixel: same bits, slower).
    nt_loads=True / False forces the nontemporal hint on / off the plane loads (PD_POLAR_NT_LOADS / PD_POLAR_PLAIN_LOADS:
    measurement; None = the library's size rule).

    angles (four polarizer angles in radians, in the order of the planes) or a uint16 / float32 ``pol`` select the general
    kernel (pd_polar_general_fwd: fp64 least-squares fit per pixel instead of the look-up tables; ``angles=None`` then means
    0/45/90/135 deg).  It also serves want "iun" ([B,1,H,W], the unpolarised intensity); it has no Stokes mode, mask,
    "ints", ieee_rho or nt_loads (ValueError).  uint8 planes without ``angles`` take K1 exactly as before.

    "xolp_std" is standardised with the reference's HAMMER constants in both kernels, whatever ``xolp_norm`` a
    ShallowEncoder was given: the kernels' correctly rounded division shortcut was verified exhaustively for those two
    constants only, and the training path does not use this output (the stem's gather standardises, with the run-time pair).
    """
    if not (isinstance(pol, torch.Tensor) and pol.is_cuda):
        raise RuntimeError("polar_forward needs a CUDA(HIP) uint8 tensor; there is no CPU fallback")
    if angles is not None or pol.dtype in (torch.uint16, torch.float32):
        if pol.dtype not in _GENERAL_DTYPES or pol.dim() != 4 or pol.shape[1] != 4:
            raise ValueError(f"pol must be uint8, uint16 or float32 [B,4,H,W], got {pol.dtype} {tuple(pol.shape)}")
        bad = [name for name, on in (("mode=MODE_STOKES", mode != MODE_LS), ("mask", mask is not None),
                                     ('want "ints"', "ints" in want), ("ieee_rho", bool(ieee_rho)),
                                     ("nt_loads", nt_loads is not None)) if on]
        if bad:
            raise ValueError("polar_forward: the general kernel (angles= / uint16 / float32 planes) has no " + ", ".join(bad))
        return _polar_general(pol, angles, n, want, tables, out_width, out, precise)
    if "iun" in want:
        raise ValueError('polar_forward: want "iun" is served by the general kernel only (pass angles=)')
    if pol.dtype != torch.uint8 or pol.dim() != 4 or pol.shape[1] != 4:
        raise ValueError(f"pol must be uint8 [B,4,H,W], got {pol.dtype} {tuple(pol.shape)}")
    pol = pol.contiguous()
    B, _, H, W = pol.shape
    if tables is None:
        tables = _device_tables(float(n), pol.device.index)
    out = dict(out) if out is not None else {}      # pre-allocated outputs may be passed in
    Wout = W if out_width is None else int(out_width)
    mk = lambda c, dt=torch.float32: torch.empty((B, c, H, Wout), dtype=dt, device=pol.device)
    for key, ch, dt in (("xolp", 2, torch.float32), ("xolp_std", 2, torch.float32), ("normals", 9, torch.float32),
                        ("ints", 5, torch.int32)):
        if key in want and key not in out:
            out[key] = mk(ch, dt)
    if mask is not None:
        mask = mask.to(torch.uint8).contiguous()
    with torch.cuda.device(pol.device):
        check(lib.pd_polar_fwd(ptr(pol), ptr(mask), ptr(out.get("xolp")), ptr(out.get("xolp_std")),
                               ptr(out.get("normals")), ptr(out.get("ints")), ptr(tables), tables.numel(),
                               B, H, W, Wout, mode, int(bool(precise)) | (2 if ieee_rho else 0) |
                               (0 if nt_loads is None else (4 if nt_loads else 8)), stream_ptr()), "pd_polar_fwd")
    return out


def split_mosaic(mosaic):
    """Raw sensor frame [..., 2h, 2w] with the four polarizer images as QUADRANTS -> planes [..., 4, h, w] in K1's
    order 0/45/90/135 degrees.  Quadrant layout of the reference's offline splitter (polarisation/
    pol_split_and_save.py:16-25 with the angle labels of indoor_dataset.py:435-438): top-left = pol00 (0 deg),
    top-right = pol01 (45), bottom-left = pol10 (90), bottom-right = pol11 (135).  Works on host or device tensors
    (one strided copy); with it the loader can hand over the un-split frame."""
    H2, W2 = mosaic.shape[-2], mosaic.shape[-1]
    if H2 % 2 or W2 % 2:
        raise ValueError(f"split_mosaic: the quadrant frame must have even sides, got {H2}x{W2}")
    h, w = H2 // 2, W2 // 2
    # torch's unsigned 16 / 32 / 64-bit types have few kernels: the copy runs on the signed type of the same width
    signed = {torch.uint16: torch.int16, torch.uint32: torch.int32, torch.uint64: torch.int64}.get(mosaic.dtype)
    m = mosaic if signed is None else mosaic.view(signed)
    tl, tr = m[..., :h, :w], m[..., :h, w:]
    bl, br = m[..., h:, :w], m[..., h:, w:]
    planes = torch.stack((tl, tr, bl, br), dim=-3).contiguous()
    return planes if signed is None else planes.view(mosaic.dtype)


def polar_inputs(inputs, size, want, angles=None, dofp=None, cdofp=None, calibration=None):
    """The loader's hand-over to K1, shared by Trainer._polar_inputs and Evaluation.predict.  ``inputs`` is a batch on the
    device; size = (height, width) of the network input; want as for ``polar_forward`` (empty: only the split below).

    An un-split sensor frame ("pol_mosaic", 0, 0) becomes ("pol", 0, 0) (``split_mosaic``).  Raw planes from
    ``HAMMER_Dataset(raw_pol=True)`` -- any height but ``height``, or wider than ``width`` -- take the Pillow-exact LANCZOS
    resize on the device (``polardepth.resize.resize_lanczos``: uint8, uint16 or float32); planes already at network size
    take none.  uint16 / float32 planes with FEWER rows than ``height`` are a ValueError (raw frames are never shorter than the
    network input; ``resize_lanczos`` itself enlarges any of the three types).  Planes narrower than ``width`` (512x612 frames -> 512x640) are padded by K1 on the fly.  Writes
    ("xolp", 0, 0) into ``inputs`` and returns the normals [B,9,H,W] when wanted, else None.

    An interleaved division-of-focal-plane frame ("pol_dofp", 0, 0) ([B,1,H2,W2] or [B,H2,W2], uint8 / uint16 / float32:
    ``HAMMER_Dataset(pol_dofp=True)``) without ("pol", 0, 0) is demosaicked into ("pol", 0, 0) first
    (``polardepth.dofp.demosaic``); ``dofp = (layout, mode)`` selects how, None = (IMX250MZR, "bilinear").  The planes come
    out in the order the layout gives them -- the order ``angles`` refers to -- and then take the path above.

    A COLOUR sensor frame ("pol_cdofp", 0, 0) (``HAMMER_Dataset(pol_cdofp=True)``) in a batch with neither ("pol", 0, 0) nor
    ("color_raw", 0, 0) gives both in one launch (``polardepth.cdofp.expand``; ``cdofp`` = its options, None = the defaults);
    ``polardepth.color.expand_batch`` makes the same call, and whichever runs first serves the other.

    ``calibration`` (a ``polardepth.calibration.Calibration`` on the batch's device): both kinds of sensor frame are
    calibrated -- dark subtracted, every 2x2 polarizer cell multiplied by its matrix -- BEFORE their demosaic, which then
    takes the float32 frame.  None: nothing changes.  Batches without a sensor frame ignore it."""
    if ("pol_cdofp", 0, 0) in inputs:
        from . import cdofp as pdcdofp
        pdcdofp.expand(inputs, cdofp, calibration=calibration)
    if ("pol_dofp", 0, 0) in inputs and ("pol", 0, 0) not in inputs:
        from . import dofp as pddofp
        layout, mode = (pddofp.IMX250MZR, "bilinear") if dofp is None else dofp
        frame = inputs[("pol_dofp", 0, 0)]
        if calibration is not None:
            from . import calibration as pdcal
            frame = pdcal.apply(frame, calibration)
        inputs[("pol", 0, 0)] = pddofp.demosaic(frame, layout, mode)
    if ("pol_mosaic", 0, 0) in inputs and ("pol", 0, 0) not in inputs:
        inputs[("pol", 0, 0)] = split_mosaic(inputs[("pol_mosaic", 0, 0)])
    if not want or ("pol", 0, 0) not in inputs:
        return None
    height, width = int(size[0]), int(size[1])
    pol = inputs[("pol", 0, 0)]
    if pol.shape[2] != height or pol.shape[3] > width:
        from . import resize as pdresize
        if pol.dtype not in _GENERAL_DTYPES:
            raise ValueError(f'("pol", 0, 0) must be uint8, uint16 or float32, got {pol.dtype} {tuple(pol.shape)}')
        if pol.dtype != torch.uint8 and pol.shape[2] < height:
            # a loader's raw frame is never shorter than the network input: 16-bit / float planes with fewer rows are a
            # mismatch between loader and options, not something to enlarge silently (uint8 planes keep what they had)
            raise ValueError(f'("pol", 0, 0) is {pol.dtype} {tuple(pol.shape[2:])}, fewer rows than the network\'s {height}: this '
                             f"hand-over enlarges uint8 planes only -- raw 16-bit / float frames are resized down on the device, "
                             f"smaller ones must arrive at {height} rows and at most {width} columns")
        pol = pdresize.resize_lanczos(pol, (height, width))
    # (uint16 / float32 planes, or calibrated angles: the general kernel; otherwise the call is unchanged)
    kw = {} if angles is None else {"angles": angles}
    out = polar_forward(pol, want=tuple(want), out_width=width if pol.shape[3] < width else None, **kw)
    inputs[("xolp", 0, 0)] = out["xolp"]
    return out.get("normals")


def normals_from_xolp(xolp, n=1.5, precise=False):
    """ShallowNormalsEncoder.get_normals on the GPU: fp32 [B,2,H,W] (DoLP, AoLP) -> fp32 [B,9,H,W]."""
    if not (isinstance(xolp, torch.Tensor) and xolp.is_cuda):
        raise RuntimeError("normals_from_xolp needs a CUDA(HIP) tensor; there is no CPU fallback")
    if xolp.dim() != 4 or xolp.shape[1] != 2:
        raise ValueError(f"xolp must be [B,2,H,W], got {tuple(xolp.shape)}")
    xolp = xolp.float().contiguous()
    B, _, H, W = xolp.shape
    tables = _device_tables(float(n), xolp.device.index)
    out = torch.empty((B, 9, H, W), dtype=torch.float32, device=xolp.device)
    with torch.cuda.device(xolp.device):
        check(lib.pd_polar_normals_from_xolp(ptr(xolp), ptr(out), ptr(tables), tables.numel(), B, H, W,
                                             int(bool(precise)), stream_ptr()), "pd_polar_normals_from_xolp")
    return out


def theta_from_rho(rho, n=1.5, want=("d", "s1", "s2"), want_bins=False):
    """rho_diffuse / rho_spec of the reference on the GPU (normals_vec.py:11-50): fp32 rho of any shape -> dict of fp64
    tensors theta_d / theta_s1 / theta_s2 of that shape (scipy interp1d 'extrapolate' semantics, evaluated in fp64 in
    scipy's operation order) and, optionally, "bins": int32 [3, *shape] searchsorted indices."""
    if not (isinstance(rho, torch.Tensor) and rho.is_cuda):
        raise RuntimeError("theta_from_rho needs a CUDA(HIP) tensor; there is no CPU fallback")
    r = rho.float().contiguous()
    tables = _device_tables(float(n), r.device.index)
    out = {k: torch.empty(r.shape, dtype=torch.float64, device=r.device) for k in want}
    bins = torch.empty((3,) + tuple(r.shape), dtype=torch.int32, device=r.device) if want_bins else None
    with torch.cuda.device(r.device):
        check(lib.pd_polar_theta(ptr(r), ptr(out.get("d")), ptr(out.get("s1")), ptr(out.get("s2")), ptr(bins), ptr(tables),
                                 tables.numel(), r.numel(), stream_ptr()), "pd_polar_theta")
    if want_bins:
        out["bins"] = bins
    return out


def calc_normals(phi, theta):
    """normals_vec.py:53-60 on the GPU (pd_polar_calc_normals): phi, theta of one shape [B, ...] -> [B,3,...]; fp64 when
    either operand is fp64 (a factor of an fp32 operand is evaluated in fp32 and promoted, as torch does there)."""
    if not (phi.is_cuda and theta.is_cuda):
        raise RuntimeError("calc_normals needs CUDA(HIP) tensors; there is no CPU fallback")
    if phi.shape != theta.shape:
        raise ValueError(f"calc_normals: phi {tuple(phi.shape)} and theta {tuple(theta.shape)} must have one shape")
    conv = lambda t: t.contiguous() if t.dtype in (torch.float32, torch.float64) else t.float().contiguous()
    phi, theta = conv(phi), conv(theta)
    B = phi.shape[0] if phi.dim() > 0 else 1
    P = phi.numel() // max(B, 1)
    f64 = phi.dtype == torch.float64 or theta.dtype == torch.float64
    out = torch.empty((B, 3) + tuple(phi.shape[1:]), dtype=torch.float64 if f64 else torch.float32, device=phi.device)
    with torch.cuda.device(phi.device):
        check(lib.pd_polar_calc_normals(ptr(phi), ptr(theta), ptr(out), B, P, int(phi.dtype == torch.float64),
                                        int(theta.dtype == torch.float64), stream_ptr()), "pd_polar_calc_normals")
    return out


# ------------------------------------------------------------------------------------------------ XOLP statistics
STATS_BYTES = 4184                                # PD_XOLP_STATS_BYTES
HIST_DOLP_BINS, HIST_AOLP_BINS = 257, 256
_MASK_DTYPES = (torch.bool, torch.uint8, torch.int32)


def parse_xolp_norm(spec):
    """The (mean, std) pair of ShallowEncoder.normalizeInput('XOLP') from a pair or the string "mean,std" (the form of
    $PD_XOLP_NORM); None and "" stay None.  ValueError unless mean is finite and std finite and > 0."""
    if spec is None or (isinstance(spec, str) and not spec.strip()):
        return None
    try:
        vals = [float(x) for x in spec.split(",")] if isinstance(spec, str) else [float(x) for x in spec]
    except (TypeError, ValueError):
        vals = []
    if len(vals) != 2:
        raise ValueError(f'xolp_norm must be a (mean, std) pair or the string "mean,std", got {spec!r}')
    mean, std = vals
    if not (np.isfinite(mean) and np.isfinite(std) and std > 0):
        raise ValueError(f"xolp_norm needs a finite mean and a finite std > 0, got {spec!r}")
    return mean, std


def format_xolp_norm(pair):
    """(mean, std) -> the "mean,std" string ``parse_xolp_norm`` reads back to the same two doubles."""
    return f"{float(pair[0])!r},{float(pair[1])!r}"


class XolpStats:
    """DoLP / AoLP statistics of XOLP tensors, accumulated on the device (pd_xolp_stats): moments, extrema, histograms and
    the counts of DoLP beyond the zenith tables.  Holds the device record and a grow-on-demand workspace; ``add`` enqueues
    one call and never synchronises, ``result`` makes the only host read.  n: the refractive index whose diffuse table
    gives the first threshold."""

    def __init__(self, device, n=1.5):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("XolpStats needs a CUDA(HIP) device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.thresholds = (float(np.float32(theta_tables_numpy(n)[0][0].max())), 1.0)
        self._thr = (ctypes.c_float * 2)(*self.thresholds)
        self._record = torch.empty(STATS_BYTES, dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(int(lib.pd_xolp_stats_workspace(1, 1, 1)), dtype=torch.uint8, device=self.device)
        self.reset()

    def _call(self, xolp, mask, B, H, W, ld, accumulate):
        need = int(lib.pd_xolp_stats_workspace(B, H, W))
        if self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(lib.pd_xolp_stats(ptr(xolp), ptr(mask), ptr(self._record), ptr(self._ws), self._ws.numel(), B, H, W, ld,
                                    self._thr, accumulate, stream_ptr()), "pd_xolp_stats")

    def reset(self):
        """Clear the record (an empty batch with accumulate = 0)."""
        self._call(None, None, 0, 1, 1, 4, 0)

    def add(self, xolp, width=None, mask=None):
        """Add fp32 ``xolp`` [B,2,H,Wp] (ch0 DoLP, ch1 AoLP; Wp % 4 == 0).  width: the data columns of a padded tensor
        (612 of 640), None = all.  mask: bool, uint8 or int32, [B,H,Wp] or [B,1,H,Wp]; non-zero = the pixel counts."""
        if not (isinstance(xolp, torch.Tensor) and xolp.is_cuda):
            raise RuntimeError("XolpStats.add needs a CUDA(HIP) tensor; there is no CPU fallback")
        if xolp.dim() != 4 or xolp.shape[1] != 2 or xolp.dtype != torch.float32:
            raise ValueError(f"xolp must be float32 [B,2,H,W], got {xolp.dtype} {tuple(xolp.shape)}")
        if xolp.device != self.device:
            raise ValueError(f"xolp is on {xolp.device}, the record on {self.device}")
        B, _, H, ld = xolp.shape
        W = ld if width is None else int(width)
        if mask is not None:
            if not (isinstance(mask, torch.Tensor) and mask.is_cuda):
                raise RuntimeError("XolpStats.add needs the mask on the device")
            if mask.dim() == 4 and mask.shape[1] == 1:
                mask = mask[:, 0]
            if mask.dtype not in _MASK_DTYPES or tuple(mask.shape) != (B, H, ld):
                raise ValueError(f"mask must be bool, uint8 or int32 [B,H,W] or [B,1,H,W] matching xolp {tuple(xolp.shape)}, "
                                 f"got {mask.dtype} {tuple(mask.shape)}")
            mask = (mask if mask.dtype == torch.bool else mask != 0).to(torch.uint8).contiguous()
        if B == 0 or H == 0 or ld == 0:
            return self
        self._call(xolp.contiguous(), mask, B, H, W, ld, 1)
        return self

    def result(self):
        """The one host read.  dict: n, nonfinite, dolp_mean / dolp_std / aolp_mean / aolp_std (population std, like
        ndarray.std(), formed in fp64 from the four sums and n; NaN while n == 0), xolp_mean / xolp_std (the reference's
        pair, xolp_mean_and_std_dev.py:29-30: the mean of the two channels' values), the extrema, both histograms,
        frac_over_diffuse / frac_over_one and the two thresholds."""
        raw = self._record.cpu().numpy()
        cnt = raw[0:32].view(np.int64)
        sums = raw[32:64].view(np.float64)
        ext = raw[64:80].view(np.float32)
        n = int(cnt[0])

        def moments(s1, s2):
            if n == 0:
                return float("nan"), float("nan")
            mean = float(s1) / n
            return mean, float(np.sqrt(max(float(s2) / n - mean * mean, 0.0)))

        dolp_mean, dolp_std = moments(sums[0], sums[1])
        aolp_mean, aolp_std = moments(sums[2], sums[3])
        frac = lambda c: int(c) / n if n else float("nan")
        return {
            "n": n, "nonfinite": int(cnt[1]), "over_diffuse": int(cnt[2]), "over_one": int(cnt[3]),
            "sums": sums.copy(),
            "dolp_mean": dolp_mean, "dolp_std": dolp_std, "aolp_mean": aolp_mean, "aolp_std": aolp_std,
            "xolp_mean": 0.5 * (dolp_mean + aolp_mean), "xolp_std": 0.5 * (dolp_std + aolp_std),
            "dolp_min": float(ext[0]), "dolp_max": float(ext[1]), "aolp_min": float(ext[2]), "aolp_max": float(ext[3]),
            "hist_dolp": raw[80:80 + 8 * HIST_DOLP_BINS].view(np.uint64).copy(),
            "hist_aolp": raw[80 + 8 * HIST_DOLP_BINS:STATS_BYTES].view(np.uint64).copy(),
            "frac_over_diffuse": frac(cnt[2]), "frac_over_one": frac(cnt[3]),
            "thresholds": self.thresholds,
        }


def xolp_stats(xolp, width=None, mask=None, n=1.5):
    """One-shot form of ``XolpStats``: the statistics of one fp32 [B,2,H,Wp] tensor as ``XolpStats.result`` returns them."""
    if not (isinstance(xolp, torch.Tensor) and xolp.is_cuda):
        raise RuntimeError("xolp_stats needs a CUDA(HIP) tensor; there is no CPU fallback")
    return XolpStats(xolp.device, n).add(xolp, width, mask).result()
