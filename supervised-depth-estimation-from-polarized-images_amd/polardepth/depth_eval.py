"""Depth accuracy per material on the device (pd_depth_stats / pd_depth_medians, csrc/depth_stats.hip).

``depth_stats`` scores a predicted depth map against the ground truth for every pixel class of the instance mask in one read
of the batch: the seven figures of the reference's compute_depth_errors (layers.py:539-577) per image and class, the
distribution of the absolute error in 0.5 mm bins, and the count of unusable predictions.  ``median_scaling`` rescales the
prediction of every image and class by the ratio of the medians first, as the reference does for models without metric
supervision (trainer.py:1344 with torch.median, :1416 with np.median); the exact medians come from ``depth_medians``.  The
per-image, per-class records stay on the device; ``DepthStats.metrics`` / ``pooled`` turn them into the report with torch
ops.  The definition is the header's; tests/depth_stats_ref.py states it in NumPy."""
import numpy as np
import torch

from . import ops
from ._lib import lib, check, ptr, stream_ptr
from ._records import Pool, device_table, frames, hist_median, need_cuda
from .normals_eval import DEFAULT_CLASSES, class_table

BINS = 512                  # PD_DSTAT_BINS: 0.5 mm bins over |gt - pred|, the last one open-ended
MAX_CLASSES = 16            # PD_DSTAT_MAX_CLASSES
RECORD_BYTES = 2128         # PD_DSTAT_RECORD_BYTES
BIN_M = 0.0005
BIN_MM = 0.5
METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "mean_mm", "median_mm", "<5mm", "<10mm", "<20mm",
                "n")
MEDIAN_SCALING = (None, "numpy", "torch")


def edges_numpy():
    """The bin edges in metres: e[j-1] = j * 0.0005, j = 1 .. 511, float64, strictly increasing."""
    e = np.arange(1, BINS, dtype=np.float64) * BIN_M
    assert np.all(np.diff(e) > 0)
    return e


def edges(device):
    """The table on ``device``: built once with NumPy, cached."""
    return device_table(edges_numpy, device)


def metrics_from_fields(n, a, sums, hist):
    """[..., 13] float64 = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, the mean and the median of |d| in millimetres, the
    shares of |d| below 5 / 10 / 20 mm, n -- from n [...], a [..., 3], sums [..., 4] and hist [..., 512], with torch ops on
    whatever device holds them.  The three thresholds are bin edges (bins 0..9, 0..19, 0..39), so the shares are exact.  The
    record carries no sum of |d|: the mean takes every pixel at the centre of its bin (within 0.25 mm of the true mean while
    no error reaches the open last bin, which is counted at 255.75 mm); the median is interpolated linearly inside the bin
    that holds the n/2-th value.  A record with n == 0 gives NaN (and n = 0)."""
    nf = n.double()
    hist = hist.long()
    cs = hist.cumsum(-1)
    share = lambda k: cs[..., k - 1].double() / nf
    centres = (torch.arange(BINS, dtype=torch.float64, device=hist.device) + 0.5) * BIN_MM
    mean_mm = (hist.double() * centres).sum(-1) / nf
    return torch.stack([sums[..., 0] / nf, sums[..., 1] / nf, (sums[..., 2] / nf).sqrt(), (sums[..., 3] / nf).sqrt(),
                        a[..., 0].double() / nf, a[..., 1].double() / nf, a[..., 2].double() / nf, mean_mm,
                        hist_median(n, hist, BIN_MM), share(10), share(20), share(40), nf], -1)


class DepthStats(Pool):
    """The [N][K] records of one ``depth_stats`` call, on the device, plus a device-side pool: ``a += b`` adds b's images to
    a's pool (int64 counts, fp64 sums, histograms widened to int64).  Nothing reaches the host until the caller asks."""
    METRIC_NAMES = METRIC_NAMES

    def __init__(self, records, names, scale=None, err=None):
        self.records = records                # uint8 [N, K, RECORD_BYTES]
        self.names = list(names)
        self.scale = scale                    # fp32 [N, K] the factors of median scaling, or None
        self.err = err                        # fp32 [N, H, W] |gt - pred| in metres, or None

    # ---- the fields of the records, as views
    @property
    def n(self):
        return self.records.view(torch.int64)[..., 0]

    @property
    def a(self):
        return self.records.view(torch.int64)[..., 1:4]

    @property
    def bad(self):
        return self.records.view(torch.int64)[..., 4]

    @property
    def sums(self):
        return self.records.view(torch.float64)[..., 5:9]

    @property
    def hist(self):
        return self.records.view(torch.int32)[..., 20:20 + BINS]      # a bin holds at most 2^30 pixels: int32 reads it

    def metrics(self):
        """[N, K, 13] float64 on the device (METRIC_NAMES), per image and class."""
        return metrics_from_fields(self.n, self.a, self.sums, self.hist)

    def _pool_fields(self):
        return self.n, self.a, self.bad, self.sums, self.hist.long()

    def pooled(self):
        """[K, 13] float64 on the device: the same figures over all pixels of all images pooled so far (this call's, and
        every call's added with ``+=``)."""
        n, a, _, s, h = self._totals()
        return metrics_from_fields(n, a, s, h)

    def pooled_bad(self):
        """[K] int64 on the device: `bad` over the pool."""
        return self._totals()[2]


def _inputs(what, pred, gt, mask):
    need_cuda(what, pred, gt, mask)
    pred = frames(pred, "pred")
    N, H, W = pred.shape
    gt = frames(gt, "gt", N, H, W).float().contiguous()
    pred = pred.float().contiguous()
    if mask is not None:
        mask = frames(mask, "mask", N, H, W).to(torch.int32).contiguous()
    return pred, gt, mask, N, H, W


def _medians(pred, gt, mask, table, nk, N, H, W, min_depth, max_depth):
    dev = pred.device
    n = torch.empty((N, nk), dtype=torch.int64, device=dev)
    med = torch.empty((N, nk, 4), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.pd_depth_medians_workspace(N, nk)), dtype=torch.uint8, device=dev)
    check(lib.pd_depth_medians(ptr(gt), ptr(pred), ptr(mask), table, nk, ptr(n), ptr(med), ptr(ws), ws.numel(), N, H, W,
                               float(min_depth), float(max_depth), stream_ptr()), "pd_depth_medians")
    return n, med


def depth_medians(pred, gt, mask=None, classes=DEFAULT_CLASSES, min_depth=0.1, max_depth=2.0):
    """(n [N,K] int64, med [N,K,4] float32): per image and class, the number of pixels with min_depth < gt < max_depth and a
    finite prediction, and the order statistics of rank (n-1)//2 and n//2 of gt, then of the prediction clamped to
    [min_depth, max_depth], over those pixels -- exact, the values a sort would put there.  NaN where n == 0."""
    pred, gt, mask, N, H, W = _inputs("depth_medians", pred, gt, mask)
    names, table = class_table(classes)
    if N == 0 or H == 0 or W == 0:
        return (torch.zeros((N, len(names)), dtype=torch.int64, device=pred.device),
                torch.full((N, len(names), 4), float("nan"), dtype=torch.float32, device=pred.device))
    with torch.cuda.device(pred.device):
        return _medians(pred, gt, mask, table, len(names), N, H, W, min_depth, max_depth)


def scale_from_medians(med, how):
    """The factor of median scaling [N,K] fp32 from ``depth_medians``' med, in fp32 torch ops.  "numpy": np.median on float32
    averages the two middle values, trainer.py:1416; "torch": torch.median returns the lower one, trainer.py:1344."""
    if how == "numpy":
        return ((med[..., 0] + med[..., 1]) / 2) / ((med[..., 2] + med[..., 3]) / 2)
    if how == "torch":
        return med[..., 0] / med[..., 2]
    raise ValueError(f'median_scaling must be None, "numpy" or "torch", got {how!r}')


def depth_stats(pred, gt, mask=None, classes=DEFAULT_CLASSES, min_depth=0.1, max_depth=2.0, median_scaling=None,
                out_err=False):
    """Depth-error records of ``pred`` against ``gt`` -> ``DepthStats``.

    pred, gt         [N,1,H,W] or [N,H,W] depth in metres
    mask             [N,1,H,W] or [N,H,W] integer instance mask, or None (then every class must be None = every pixel)
    classes          (name, None | (lo, hi)) pairs, at most 16
    median_scaling   None, or "numpy" / "torch": multiply the clamped prediction of every image and class by the ratio of the
                     medians of gt and prediction over the class's pixels, then clamp again; the factors are ``.scale``.  A
                     class without a pixel has no factor (NaN) and stays empty
    out_err          also return |gt - pred| per pixel in metres (NaN where the pixel does not count) as ``.err``; not with
                     median_scaling, where the error depends on the class"""
    if median_scaling not in MEDIAN_SCALING:
        raise ValueError(f'median_scaling must be None, "numpy" or "torch", got {median_scaling!r}')
    if out_err and median_scaling is not None:
        raise ValueError("out_err needs median_scaling=None: a scaled error is per class")
    pred, gt, mask, N, H, W = _inputs("depth_stats", pred, gt, mask)
    names, table = class_table(classes)
    nk = len(names)
    dev = pred.device
    records = torch.empty((N, nk, RECORD_BYTES), dtype=torch.uint8, device=dev)
    err = torch.empty((N, H, W), dtype=torch.float32, device=dev) if out_err else None
    if N == 0 or H == 0 or W == 0:
        scale = None if median_scaling is None else torch.empty((N, nk), dtype=torch.float32, device=dev)
        return DepthStats(records.zero_(), names, scale, err)
    with torch.cuda.device(dev):
        scale = None
        if median_scaling is not None:
            _, med = _medians(pred, gt, mask, table, nk, N, H, W, min_depth, max_depth)
            scale = scale_from_medians(med, median_scaling).contiguous()
        ws = torch.empty(int(lib.pd_depth_stats_workspace(N, H, W, nk)), dtype=torch.uint8, device=dev)
        check(lib.pd_depth_stats(ptr(gt), ptr(pred), ptr(mask), table, nk, ptr(scale), ptr(edges(dev)), ptr(err), ptr(records),
                                 ptr(ws), ws.numel(), N, H, W, float(min_depth), float(max_depth), stream_ptr()),
              "pd_depth_stats")
    return DepthStats(records, names, scale, err)


class MaterialTable:
    """The reference's test table (evaluation.py:120-288, trainer.py:782-980) as one accumulator: per batch the seven figures of
    ``ops.depth_metrics`` for the whole frame and for every material of ``grey`` {name: the instance mask's grey value}, one
    launch each, added over the images that have a pixel of the class (fp64, on the device) and counted."""

    def __init__(self, grey, min_depth, max_depth, device):
        self.grey, self.min_depth, self.max_depth = grey, min_depth, max_depth
        self.objects = ["all"] + list(grey)
        self.sums = {o: torch.zeros(7, dtype=torch.float64, device=device) for o in self.objects}
        self.counts = {o: torch.zeros((), dtype=torch.float64, device=device) for o in self.objects}

    def add(self, gt, depth, mask):
        for o in self.objects:
            m = ops.depth_metrics(gt, depth, self.min_depth, self.max_depth, mask=None if o == "all" else mask,
                                  mask_value=self.grey.get(o, 0))
            valid = m[:, 7] > 0
            self.sums[o] += (m[:, :7].double() * valid[:, None]).sum(0)
            self.counts[o] += valid.sum()

    def means(self):
        """{class: float64 NumPy [7], the mean over its images} for the classes that some image has: the host reads here."""
        return {o: (self.sums[o] / self.counts[o]).cpu().numpy() for o in self.objects if self.counts[o].item() > 0}
