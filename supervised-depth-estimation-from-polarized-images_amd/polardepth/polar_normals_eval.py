"""Polarimetric normals evaluation per material on the device (pd_polar_normals_stats, csrc/polar_normals_stats.hip).

K1 turns every pixel's DoLP / AoLP into three physical normal candidates (N_diff, N_spec1, N_spec2).  ``polar_normals_stats``
asks the converse question: does the surface we predict agree with the polarisation we measured?  For every pixel class of the
instance mask, in one evaluator launch, it scores predicted normals -- a decoder's [N,3,H,W] output, or the normals of a depth
map -- in two ways: the angle to the best of the six candidates (each of the three and its pi flip; ``.normal``), and the
azimuth residual modulo pi against the diffuse and the specular branch (``.azimuth``).  It needs one frame, no ground truth
and no pose.  The by-product is the classical use of a coarse depth prior: the prediction resolves the pi ambiguity and the
diffuse / specular ambiguity, and the winning candidate per pixel is a disambiguated normal map (``maps=True``).

The candidates are quantities about the viewing ray of their pixel; by default the prediction is scored the orthographic way
of calc_normals, whose error grows towards the frame's edge.  ``ray_frame=True`` rotates the prediction into the frame of each
pixel's ray first (the minimal rotation of the ray onto the optical axis; include/polardepth.h).  The training loss on the same
decisions is ``ops.polar_loss``.

The per-image, per-class records stay on the device; ``Pool.metrics`` / ``pooled`` turn them into the report with torch ops.
The definition is the header's; tests/polar_normals_ref.py states it in NumPy."""
import math

import numpy as np
import torch

from ._lib import lib, check, ptr, stream_ptr
from ._records import Pool, frames, need_cuda
from .normals_eval import DEFAULT_CLASSES, class_table, cos_edges, metrics_from_fields, pixel_major

NORMAL_BINS = 720                   # PD_PNSTAT_NORMAL_BINS: 0.25-degree bins over [0, 180]
AZIMUTH_BINS = 360                  # PD_PNSTAT_AZIMUTH_BINS: 0.25-degree bins over [0, 90]
MAX_CLASSES = 16                    # PD_PNSTAT_MAX_CLASSES
NORMAL_RECORD_BYTES = 2960          # PD_PNSTAT_NORMAL_RECORD_BYTES
AZIMUTH_RECORD_BYTES = 1520         # PD_PNSTAT_AZIMUTH_RECORD_BYTES
NORMAL_COUNTERS = ("bad", "dolp_out", "spec", "flipped")
AZIMUTH_COUNTERS = ("bad", "dolp_out", "frontal", "spec")
SUM_NAMES = ("deg", "deg2", "rho_deg", "rho")
METRIC_NAMES = ("mean", "median", "rmse", "11.25", "22.5", "30", "n", "rho_mean")
CHOICE_NAMES = ("none", "diff+", "diff-", "spec1+", "spec1-", "spec2+", "spec2-")

_F32_MAX = float(np.finfo(np.float32).max)


def _metrics(n, sums, hist):
    """[..., 8] float64 (METRIC_NAMES): the seven figures of normals_eval.metrics_from_fields, then the DoLP-weighted mean
    sum(rho deg) / sum(rho).  A record with n == 0 gives NaN (and n = 0)."""
    base = metrics_from_fields(n, sums[..., 0], sums[..., 1], hist)
    return torch.cat([base, (sums[..., 2] / sums[..., 3])[..., None]], -1)


class RecordSet(Pool):
    """One of the two [N][K] record sets of a ``polar_normals_stats`` call, on the device, plus a device-side pool: ``a += b``
    adds b's images to a's pool (int64 counts, fp64 sums, histograms widened to int64).  Nothing reaches the host until the
    caller asks.  The counters are attributes by name (``.bad``, ``.dolp_out``, ...) and ``.counters`` [N, K, 4]."""
    METRIC_NAMES = METRIC_NAMES

    def __init__(self, records, names, counter_names, bins):
        self.records = records                # uint8 [N, K, record bytes]
        self.names = list(names)
        self.counter_names = tuple(counter_names)
        self.bins = bins

    @property
    def n(self):
        return self.records.view(torch.int64)[..., 0]

    @property
    def counters(self):
        return self.records.view(torch.int64)[..., 1:5]

    @property
    def sums(self):
        return self.records.view(torch.float64)[..., 5:9]

    @property
    def hist(self):
        return self.records.view(torch.int32)[..., 20:20 + self.bins]      # a bin holds at most 2^30 pixels: int32 reads it

    def __getattr__(self, name):
        names = self.__dict__.get("counter_names", ())
        if name in names:
            return self.counters[..., names.index(name)]
        raise AttributeError(name)

    def metrics(self):
        """[N, K, 8] float64 on the device (METRIC_NAMES), per image and class."""
        return _metrics(self.n, self.sums, self.hist)

    def _pool_fields(self):
        return self.n, self.counters, self.sums, self.hist.long()

    def pooled(self):
        """[K, 8] float64 on the device: the same figures over all pixels of all images pooled so far (this call's, and every
        call's added with ``+=``)."""
        n, _, s, h = self._totals()
        return _metrics(n, s, h)

    def pooled_counters(self):
        """[K, 4] int64 on the device: the counters (``counter_names``) over the pool."""
        return self._totals()[1]


class PolarNormalsStats:
    """What one ``polar_normals_stats`` call returns: ``.normal`` and ``.azimuth`` (``RecordSet``), the class ``names``, and
    with ``maps=True`` the per-pixel maps ``az_deg``, ``n_deg`` (fp32 [N,H,W], NaN where the pixel does not count), ``choice``
    (uint8 [N,H,W], an index into CHOICE_NAMES) and ``pol_normal`` (fp32 [N,H,W,4]: the winning candidate on the prediction's
    side, zeros where not counted).  ``a += b`` pools both record sets on the device."""

    def __init__(self, normal, azimuth, names, az_deg=None, n_deg=None, choice=None, pol_normal=None):
        self.normal, self.azimuth, self.names = normal, azimuth, list(names)
        self.az_deg, self.n_deg, self.choice, self.pol_normal = az_deg, n_deg, choice, pol_normal

    def __iadd__(self, other):
        self.normal += other.normal
        self.azimuth += other.azimuth
        return self


def polar_normals_stats(pred, pol_normals, xolp, K=None, mask=None, valid=None, classes=DEFAULT_CLASSES, rho_min=0.05,
                        rho_max=1.0, tilt_min_deg=5.0, aolp_sign=1, maps=False, ray_frame=False):
    """Records of ``pred`` against the polarisation normals -> ``PolarNormalsStats``.

    pred          [N,3,H,W] normals (any length; a channels-last tensor is read in place), or [N,1,H,W] a depth map, whose
                  normals come from pd_gt_normals without a depth range (then ``K``, the [N,4,4] intrinsics, is needed)
    pol_normals   [N,9,H,W] fp32: N_diff, N_spec1, N_spec2, what ``polar_forward`` / ``polar_inputs`` return as "normals".  A
                  view whose rows are padded (row stride >= W, as the 612 -> 640 frames) is read in place together with an
                  ``xolp`` of the same row stride
    xolp          [N,2,H,W] fp32; only channel 0 (DoLP) is read
    mask          [N,1,H,W] or [N,H,W] integer instance mask, or None (then every class must be None = every pixel)
    valid         [N,1,H,W] or [N,H,W] bool / uint8 or None: a 0 takes the pixel out altogether
    classes       (name, None | (lo, hi)) pairs, at most 16
    rho_min, rho_max   the DoLP range in which a pixel is scored.  rho_min = 0.05 is a CONVENTION, not a measurement: below a
                  few percent of polarisation the AoLP is dominated by sensor noise.  Pixels outside count as ``dolp_out``
    tilt_min_deg  the smallest tilt of the prediction against the optical axis at which its azimuth is defined; flatter pixels
                  count as ``frontal`` in the azimuth set.  5 degrees is a CONVENTION too, not a measurement
    aolp_sign     +1 or -1: multiplies the y component of every candidate -- the handedness of the sensor's AoLP
    maps          also return the per-pixel maps (class docstring)
    ray_frame     score in the frame of each pixel's viewing ray; ``K`` is then needed for [N,3,H,W] normals too.  ``choice``,
                  ``n_deg`` and ``az_deg`` are those of the ray frame, ``pol_normal`` is returned in camera coordinates"""
    need_cuda("polar_normals_stats", pred, pol_normals, xolp, K, mask, valid)
    if pred.dim() != 4 or pred.shape[1] not in (1, 3):
        raise ValueError(f"pred must be [N,3,H,W] normals or [N,1,H,W] depth, got {tuple(pred.shape)}")
    N, C, H, W = pred.shape
    if tuple(pol_normals.shape) != (N, 9, H, W) or tuple(xolp.shape) != (N, 2, H, W):
        raise ValueError(f"pol_normals must be {(N, 9, H, W)} and xolp {(N, 2, H, W)}, got {tuple(pol_normals.shape)} and "
                         f"{tuple(xolp.shape)}")
    if C == 1 and K is None:
        raise ValueError("a depth map needs the intrinsics K to become normals")
    if ray_frame and K is None:
        raise ValueError("ray_frame=True needs the intrinsics K [N,4,4]: the viewing ray of a pixel comes from them")
    if ray_frame and tuple(K.shape) != (N, 4, 4):
        raise ValueError(f"K must be [{N},4,4], got {tuple(K.shape)}")
    if aolp_sign not in (1, -1):
        raise ValueError(f"aolp_sign must be +1 or -1, got {aolp_sign!r}")
    if not 0.0 <= float(tilt_min_deg) < 90.0:
        raise ValueError(f"tilt_min_deg must be in [0, 90), got {tilt_min_deg!r}")
    names, table = class_table(classes)
    nk = len(names)
    dev = pred.device
    if mask is not None:
        mask = frames(mask, "mask", N, H, W).to(torch.int32).contiguous()
    if valid is not None:
        valid = frames(valid, "valid", N, H, W).ne(0).to(torch.uint8).contiguous()
    rec_n = torch.empty((N, nk, NORMAL_RECORD_BYTES), dtype=torch.uint8, device=dev)
    rec_a = torch.empty((N, nk, AZIMUTH_RECORD_BYTES), dtype=torch.uint8, device=dev)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev) if maps else None
    az_deg, n_deg = new((N, H, W), torch.float32), new((N, H, W), torch.float32)
    choice, pol_normal = new((N, H, W), torch.uint8), new((N, H, W, 4), torch.float32)
    out = PolarNormalsStats(RecordSet(rec_n, names, NORMAL_COUNTERS, NORMAL_BINS),
                            RecordSet(rec_a, names, AZIMUTH_COUNTERS, AZIMUTH_BINS), names, az_deg, n_deg, choice, pol_normal)
    if N == 0 or H == 0 or W == 0:
        rec_n.zero_()
        rec_a.zero_()
        return out
    pol_normals, xolp, ldp = _planar(pol_normals, xolp, H, W)
    tilt2 = math.sin(math.radians(float(tilt_min_deg))) ** 2
    with torch.cuda.device(dev):
        st = stream_ptr()
        Km = K.float().contiguous() if (C == 1 or ray_frame) else None
        if C == 1:
            depth = pred.float().contiguous()
            pred, ld = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev), 4
            check(lib.pd_gt_normals(ptr(depth), ptr(Km), ptr(pred), N, H, W, -_F32_MAX, _F32_MAX, st), "pd_gt_normals")
        else:
            pred, ld = pixel_major(pred)
        ws = torch.empty(int(lib.pd_polar_normals_stats_workspace(N, H, W, nk)), dtype=torch.uint8, device=dev)
        check(lib.pd_polar_normals_stats_ray(ptr(pred), ld, ptr(Km) if ray_frame else None, int(bool(ray_frame)), ptr(pol_normals),
                                             ptr(xolp), ldp, ptr(mask), table, nk, ptr(valid), ptr(cos_edges(dev)), float(rho_min),
                                             float(rho_max), tilt2, int(aolp_sign), ptr(rec_n), ptr(rec_a), ptr(az_deg),
                                             ptr(n_deg), ptr(choice), ptr(pol_normal), ptr(ws), ws.numel(), N, H, W, st),
              "pd_polar_normals_stats_ray")
    return out


def _row_pitch(t, C, H, W):
    """The row pitch of a planar [N,C,H,W] fp32 tensor that the kernel can read in place, or None."""
    s = t.stride()
    ldp = s[2] if H > 1 else W
    ok = (t.dtype == torch.float32 and s[3] == 1 and ldp >= W and (C == 1 or s[1] == H * ldp) and
          (t.shape[0] == 1 or s[0] == C * H * ldp) and t.data_ptr() % 16 == 0)
    return ldp if ok else None


def _planar(pol_normals, xolp, H, W):
    """-> (pol_normals, xolp, ldp): in place when both have the same readable row pitch, else contiguous copies."""
    lp, lx = _row_pitch(pol_normals, 9, H, W), _row_pitch(xolp, 2, H, W)
    if lp is not None and lp == lx:
        return pol_normals, xolp, lp
    return pol_normals.float().contiguous(), xolp.float().contiguous(), W
