"""Surface-normal accuracy per material on the device (pd_normals_stats, csrc/normals_stats.hip).

``normals_stats`` scores predicted normals -- a decoder's [N,3,H,W] output, or the normals of a predicted depth map -- against
the normals of the ground-truth depth (pd_gt_normals) for every pixel class of the instance mask in one read of the batch.
The per-image, per-class records stay on the device; ``NormalsStats.metrics`` / ``pooled`` turn them into the standard report
(mean, median and RMS angular error, share of pixels within 11.25 / 22.5 / 30 degrees) with torch ops.  The reference stops at
depth (evaluation.py:120-288); the definition is the header's."""
import ctypes

import numpy as np
import torch

from ._lib import lib, check, ptr, stream_ptr
from ._records import Pool, device_table, frames, hist_median, need_cuda

BINS = 720                  # PD_NSTAT_BINS: 0.25-degree bins over [0, 180]
MAX_CLASSES = 16            # PD_NSTAT_MAX_CLASSES
RECORD_BYTES = 2912         # PD_NSTAT_RECORD_BYTES
BIN_DEG = 0.25
METRIC_NAMES = ("mean", "median", "rmse", "11.25", "22.5", "30", "n")
# the grey value of each material in HAMMER's instance masks (reference evaluation.py:242-261; manydepth.evaluation._MATERIAL_GREY)
# A copy: polardepth does not import manydepth.  Change it in BOTH places; tests/test_normals_stats_ref.py::test_default_classes
# compares the two.
MATERIAL_GREY = {"box": 20, "bottle": 40, "can": 60, "cup": 80, "remote": 100, "teapot": 120, "cutlery": 140,
                 "glass": 160, "table": 180, "wall": 200}
# (name, None = every pixel | (lo, hi) inclusive on the mask value), in the reference's order (evaluation.py:235-264)
DEFAULT_CLASSES = (("all", None), ("objects", (20, 160))) + tuple((m, (g, g)) for m, g in MATERIAL_GREY.items())

_F32_MAX = float(np.finfo(np.float32).max)


def cos_edges_numpy():
    """The bin edges as cosines: e[j-1] = cos(j * 0.25 degrees), j = 1 .. 719, float64, strictly decreasing.  The second half
    mirrors the first and the entry of 90 degrees is 0 exactly, so orthogonal normals (c == 0) land in bin 360 whatever libm
    makes of cos(pi / 2)."""
    e = np.empty(BINS - 1, np.float64)
    e[:359] = np.cos(np.arange(1, 360, dtype=np.float64) * (np.pi / 720.0))
    e[359] = 0.0
    e[360:] = -e[358::-1]
    assert np.all(np.diff(e) < 0)
    return e


def cos_edges(device):
    """The table on ``device``: built once with NumPy, cached."""
    return device_table(cos_edges_numpy, device)


def class_table(classes):
    """classes -> (names, ctypes int[K][2]); None is written as the empty range (1, 0) = every pixel."""
    classes = list(classes)
    if not 1 <= len(classes) <= MAX_CLASSES:
        raise ValueError(f"normals_stats takes 1 .. {MAX_CLASSES} classes, got {len(classes)}")
    flat = []
    for name, rng in classes:
        lo, hi = (1, 0) if rng is None else (int(rng[0]), int(rng[1]))
        flat += [lo, hi]
    return [str(name) for name, _ in classes], (ctypes.c_int * len(flat))(*flat)


def metrics_from_fields(n, sum_deg, sum_deg2, hist):
    """[..., 7] float64 = mean, median, rmse, share < 11.25 / 22.5 / 30 degrees, n -- from n [...], the two sums [...] and
    hist [..., 720], with torch ops on whatever device holds them.  The three thresholds are bin edges (bins 0..44, 0..89,
    0..119), so the shares are exact.  The median is interpolated linearly inside the bin that holds the n/2-th value.  A
    record with n == 0 gives NaN (and n = 0)."""
    nf = n.double()
    hist = hist.long()
    cs = hist.cumsum(-1)
    share = lambda k: cs[..., k - 1].double() / nf
    return torch.stack([sum_deg / nf, hist_median(n, hist, BIN_DEG), (sum_deg2 / nf).sqrt(), share(45), share(90), share(120),
                        nf], -1)


class NormalsStats(Pool):
    """The [N][K] records of one ``normals_stats`` call, on the device, plus a device-side pool: ``a += b`` adds b's images
    to a's pool (int64 counts, fp64 sums, histograms widened to int64).  Nothing reaches the host until the caller asks."""

    def __init__(self, records, names, err_deg=None):
        self.records = records                # uint8 [N, K, RECORD_BYTES]
        self.names = list(names)
        self.err_deg = err_deg                # fp32 [N, H, W] or None

    # ---- the fields of the records, as views
    @property
    def n(self):
        return self.records.view(torch.int64)[..., 0]

    @property
    def bad(self):
        return self.records.view(torch.int64)[..., 1]

    @property
    def sum_deg(self):
        return self.records.view(torch.float64)[..., 2]

    @property
    def sum_deg2(self):
        return self.records.view(torch.float64)[..., 3]

    @property
    def hist(self):
        return self.records.view(torch.int32)[..., 8:8 + BINS]      # a bin holds at most 2^30 pixels: int32 reads it

    def metrics(self):
        """[N, K, 7] float64 on the device: mean, median, rmse, the three shares, n -- per image and class."""
        return metrics_from_fields(self.n, self.sum_deg, self.sum_deg2, self.hist)

    def _pool_fields(self):
        return self.n, self.bad, self.sum_deg, self.sum_deg2, self.hist.long()

    def pooled(self):
        """[K, 7] float64 on the device: the same seven figures over all pixels of all images pooled so far (this call's,
        and every call's added with ``+=``) -- the pixel-pooled convention of the normals literature."""
        n, _, s, s2, h = self._totals()
        return metrics_from_fields(n, s, s2, h)

    def pooled_bad(self):
        """[K] int64 on the device: `bad` over the pool."""
        return self._totals()[1]


def pixel_major(pred):
    """[N,3,H,W] fp32 -> (tensor, ld): in place when the channel stride is 1 and the pixels are evenly spaced (a channels-last
    tensor: ld = 3; the first three channels of a wider one: ld = its channel count); else one channels-last copy."""
    N, C, H, W = pred.shape
    s = pred.stride()
    ld = s[3]
    if pred.dtype == torch.float32 and s[1] == 1 and ld >= 3 and (H == 1 or s[2] == W * ld) and (N == 1 or s[0] == H * W * ld):
        return pred, ld
    return pred.float().contiguous(memory_format=torch.channels_last), 3


def normals_stats(pred, gt_depth, K, mask=None, classes=DEFAULT_CLASSES, gate=True, min_depth=0.1, max_depth=2.0,
                  err_map=False):
    """Angular-error records of ``pred`` against the normals of ``gt_depth`` -> ``NormalsStats``.

    pred       [N,3,H,W] normals (any length; a channels-last tensor is read in place), or [N,1,H,W] a depth map, whose
               normals come from pd_gt_normals without a depth range (a non-finite depth gives a zero normal: counted `bad`)
    gt_depth   [N,1,H,W] or [N,H,W]; its normals come from pd_gt_normals at min_depth / max_depth
    K          [N,4,4] intrinsics, as for the losses
    mask       [N,1,H,W] or [N,H,W] integer instance mask, or None (then every class must be None = every pixel)
    classes    (name, None | (lo, hi)) pairs, at most 16
    gate       True: a pixel counts when all nine depths of its 3x3 window are inside [min_depth, max_depth]; False: its own
    err_map    also return the per-pixel angle in degrees (NaN where the pixel does not count) as ``.err_deg``"""
    need_cuda("normals_stats", pred, gt_depth, K, mask)
    if pred.dim() != 4 or pred.shape[1] not in (1, 3):
        raise ValueError(f"pred must be [N,3,H,W] normals or [N,1,H,W] depth, got {tuple(pred.shape)}")
    N, C, H, W = pred.shape
    names, table = class_table(classes)
    nk = len(names)
    dev = pred.device
    gt = frames(gt_depth, "gt_depth", N, H, W).float().contiguous()
    if mask is not None:
        mask = frames(mask, "mask", N, H, W).to(torch.int32).contiguous()
    records = torch.empty((N, nk, RECORD_BYTES), dtype=torch.uint8, device=dev)
    err = torch.empty((N, H, W), dtype=torch.float32, device=dev) if err_map else None
    if N == 0 or H == 0 or W == 0:
        return NormalsStats(records.zero_(), names, err)
    K = K.float().contiguous()
    with torch.cuda.device(dev):
        st = stream_ptr()
        gtn = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
        check(lib.pd_gt_normals(ptr(gt), ptr(K), ptr(gtn), N, H, W, float(min_depth), float(max_depth), st), "pd_gt_normals")
        if C == 1:
            depth = pred.float().contiguous()
            pred, ld = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev), 4
            check(lib.pd_gt_normals(ptr(depth), ptr(K), ptr(pred), N, H, W, -_F32_MAX, _F32_MAX, st), "pd_gt_normals")
        else:
            pred, ld = pixel_major(pred)
        ws = torch.empty(int(lib.pd_normals_stats_workspace(N, H, W, nk)), dtype=torch.uint8, device=dev)
        check(lib.pd_normals_stats(ptr(pred), ld, ptr(gtn), ptr(gt), ptr(mask), table, nk, ptr(cos_edges(dev)), 1 if gate else 0,
                                   ptr(err), ptr(records), ptr(ws), ws.numel(), N, H, W, float(min_depth), float(max_depth),
                                   st), "pd_normals_stats")
    return NormalsStats(records, names, err)
