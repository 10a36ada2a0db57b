"""Calibration and sparsification of the depth uncertainty per material on the device (pd_unc_stats, csrc/unc_stats.hip).

The decoder's uncertainty head states, per pixel, the scale b of a Laplace error model of the predicted depth
(``ops.uncertainty_loss`` trains it).  ``uncertainty_stats`` asks, for every pixel class of the instance mask in one read of
the batch, whether that statement holds: the mean error next to the mean stated scale, the mean negative log-likelihood, the
share of pixels whose error lies inside the central 50 % and 90 % of their stated density (a calibrated model gives 0.5 and
0.9), and the integer tables from which ``sparsification`` draws the sparsification curves on the host.  The definition is
the header's; tests/unc_stats_ref.py states it in NumPy.

Sparsification (Ilg et al., ECCV 2018): remove the fraction f of the pixels the model trusts least and look at the mean
absolute error S(f) of the rest; the oracle O(f) removes the pixels with the largest error instead.  AUSE = mean_f (S - O) is
0 for a perfect ranking; AURG = mean_f (S(0) - S) is what the ranking gains over removing pixels at random, negative when
it is worse than random.  Both are computed from binned integers, with these limits: pixels that share a 1/512 step of u are
tied (their bin is removed proportionally); the oracle's last 0.5 mm error bin (>= 255.5 mm) is open-ended, which lifts the
oracle's curve a little at small f when errors that large exist; and at f -> 1 what is left lies in the first error bin, which
the binned oracle leaves at its mean (up to 0.25 mm above the exact-sort curve there; tests/test_unc_stats_ref.py)."""
import numpy as np
import torch

from . import ops
from ._lib import lib, check, ptr, stream_ptr
from ._records import Pool, format_table, frames, need_cuda
from .depth_eval import edges
from .normals_eval import DEFAULT_CLASSES, class_table

BINS = 512                  # PD_USTAT_BINS: the steps of u, and the 0.5 mm error bins of depth_eval
MAX_CLASSES = 16
RECORD_BYTES = 2112         # PD_USTAT_RECORD_BYTES
TABLE_ROWS = 3              # PD_USTAT_TABLE_ROWS: sum e_um by ub, count by eb, sum e_um by eb
MAX_DEPTH = 1000.0          # PD_USTAT_MAX_DEPTH
STEPS = 100                 # f = 0, 0.01, .. 0.99
METRIC_NAMES = ("mae_mm", "b_mm", "nll", "cover50", "cover90", "ause_mm", "aurg_mm", "ause_rel", "aurg_rel", "n")


def curve(count, total, steps=STEPS):
    """The mean of what is left after removing the fraction f = i / steps of the items, highest bin first: ``count`` [B] items
    and ``total`` [B] their summed value per bin (integers).  The bin in which the removed count r = f n ends is removed
    proportionally in count and in sum.  float64 [steps]; NaN for an empty set."""
    c = np.asarray(count, dtype=np.float64)[::-1]
    t = np.asarray(total, dtype=np.float64)[::-1]
    n = c.sum()
    if n == 0:
        return np.full(steps, np.nan)
    cc = np.concatenate([[0.0], np.cumsum(c)])
    tc = np.concatenate([[0.0], np.cumsum(t)])
    r = np.arange(steps, dtype=np.float64) * n / steps
    j = np.clip(np.searchsorted(cc, r, side="left") - 1, 0, c.size - 1)       # cc[j] < r <= cc[j + 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        part = np.where(c[j] > 0, (r - cc[j]) / c[j], 0.0) * t[j]
    return (tc[-1] - (tc[j] + part)) / (n - r)


def sparsification(hist, tables, steps=STEPS):
    """(S, O) float64 [steps] in millimetres from one record's ``hist`` [512] and ``tables`` [3, 512]: the sparsification
    curve keyed by the stated uncertainty (hist, row 0) and the oracle's keyed by the error itself (rows 1 and 2)."""
    return curve(hist, tables[0], steps) / 1e3, curve(tables[1], tables[2], steps) / 1e3


def figures(hist, tables):
    """(AUSE mm, AURG mm, AUSE / S(0), AURG / S(0)) of one record; NaN for an empty one."""
    s, o = sparsification(hist, tables)
    if np.isnan(s[0]):
        return (np.nan,) * 4
    ause, aurg = float(np.mean(s - o)), float(np.mean(s[0] - s))
    with np.errstate(invalid="ignore", divide="ignore"):
        return ause, aurg, float(np.float64(ause) / s[0]), float(np.float64(aurg) / s[0])


def metrics_from_fields(n, cover, sums, hist, tables):
    """[..., 10] float64 (METRIC_NAMES) from host arrays n [...], cover [..., 2], sums [..., 3], hist [..., 512] and tables
    [..., 3, 512] (integers of any kind, Python's included).  A record with n == 0 gives NaN (and n = 0)."""
    n = np.asarray(n)
    out = np.full(n.shape + (len(METRIC_NAMES),), np.nan)
    for idx in np.ndindex(*n.shape):
        c = float(n[idx])
        out[idx][9] = c
        if c == 0:
            continue
        s = np.asarray(sums[idx], dtype=np.float64)
        out[idx][:5] = (s[2] / c * 1e3, s[1] / c * 1e3, s[0] / c, float(cover[idx][0]) / c, float(cover[idx][1]) / c)
        out[idx][5:9] = figures(hist[idx], tables[idx])
    return out


class UncertaintyStats(Pool):
    """The [N][K] records and tables of one ``uncertainty_stats`` call, on the device, plus a pool: ``a += b`` adds b's images
    to a's pool.  The record fields pool on the device; the tables of every pooled call are summed over its images there
    (int64) and added across calls on the host as Python integers, which no total can overflow."""
    METRIC_NAMES = METRIC_NAMES

    def __init__(self, records, tables, names):
        self.records = records                # uint8 [N, K, RECORD_BYTES]
        self.tables = tables                  # int64 [N, K, 3, 512] (the kernel's uint64; every entry is below 2^63)
        self.names = list(names)
        self._table_parts = [tables]          # of every pooled call; summed when the pool is asked for

    @property
    def n(self):
        return self.records.view(torch.int64)[..., 0]

    @property
    def bad(self):
        return self.records.view(torch.int64)[..., 1]

    @property
    def cover(self):
        return self.records.view(torch.int64)[..., 2:4]

    @property
    def sums(self):
        return self.records.view(torch.float64)[..., 4:7]          # nll, b, e

    @property
    def hist(self):
        return self.records.view(torch.int32)[..., 16:16 + BINS]

    def metrics(self):
        """[N, K, 10] float64 NumPy (METRIC_NAMES), per image and class: the fields come to the host here."""
        f = lambda t: t.cpu().numpy()
        return metrics_from_fields(f(self.n), f(self.cover), f(self.sums), f(self.hist), f(self.tables))

    def _pool_fields(self):
        return self.n, self.bad, self.cover, self.sums, self.hist.long()

    def __iadd__(self, other):
        super().__iadd__(other)
        self._table_parts = self._table_parts + other._table_parts
        return self

    def pooled_tables(self):
        """[K, 3, 512] NumPy array of Python integers: the tables of all images pooled so far, added exactly."""
        total = None
        for part in self._table_parts:
            p = part.sum(0).cpu().numpy().astype(object)
            total = p if total is None else total + p
        return total

    def pooled(self):
        """[K, 10] float64 NumPy: the same figures over all pixels of all images pooled so far."""
        n, _, cover, sums, hist = (t.cpu().numpy() for t in self._totals())
        return metrics_from_fields(n, cover, sums, hist, self.pooled_tables())

    def pooled_bad(self):
        """[K] int64 on the device: `bad` over the pool."""
        return self._totals()[1]


def scale_of(u, b_range=None):
    """b in metres (fp32, u's shape) of an uncertainty map u in [0, 1]: exp(log b_lo + u log(b_hi / b_lo)), in fp64 torch ops."""
    import math
    lo, hi = ops.uncertainty_range(b_range)
    return torch.exp(math.log(lo) + u.double() * math.log(hi / lo)).float()


def uncertainty_stats(pred, gt, unc, mask=None, classes=DEFAULT_CLASSES, b_range=None, min_depth=0.1, max_depth=2.0):
    """Uncertainty records of ``pred`` and its stated uncertainty ``unc`` against ``gt`` -> ``UncertaintyStats``.

    pred, gt   [N,1,H,W] or [N,H,W] depth in metres
    unc        [N,1,H,W] or [N,H,W] the uncertainty head's output u in [0, 1] at full resolution (scale 0 of the decoder)
    mask       [N,1,H,W] or [N,H,W] integer instance mask, or None (then every class must be None = every pixel)
    classes    (name, None | (lo, hi)) pairs, at most 16
    b_range    (b_lo, b_hi) in metres, None = ``ops.UNCERTAINTY_RANGE``: the convention the heads were trained with
    max_depth  finite, at most 1000 m (the tables add errors in whole micrometres)"""
    need_cuda("uncertainty_stats", pred, gt, unc, mask)
    pred = frames(pred, "pred")
    N, H, W = pred.shape
    gt = frames(gt, "gt", N, H, W).float().contiguous()
    unc = frames(unc, "unc", N, H, W).float().contiguous()
    pred = pred.float().contiguous()
    if mask is not None:
        mask = frames(mask, "mask", N, H, W).to(torch.int32).contiguous()
    b_lo, b_hi = ops.uncertainty_range(b_range)
    names, table = class_table(classes)
    nk = len(names)
    dev = pred.device
    records = torch.empty((N, nk, RECORD_BYTES), dtype=torch.uint8, device=dev)
    tables = torch.empty((N, nk, TABLE_ROWS, BINS), dtype=torch.int64, device=dev)
    if N == 0 or H == 0 or W == 0:
        return UncertaintyStats(records.zero_(), tables.zero_(), names)
    with torch.cuda.device(dev):
        ws = torch.empty(int(lib.pd_unc_stats_workspace(N, H, W, nk)), dtype=torch.uint8, device=dev)
        check(lib.pd_unc_stats(ptr(gt), ptr(pred), ptr(unc), ptr(mask), table, nk, ptr(edges(dev)), b_lo, b_hi, ptr(records),
                               ptr(tables), ptr(ws), ws.numel(), N, H, W, float(min_depth), float(max_depth), stream_ptr()),
              "pd_unc_stats")
    return UncertaintyStats(records, tables, names)


def format_report(names, per_image, pooled, bad, title="uncertainty"):
    """The table ``Evaluation.test_uncertainty`` prints: per class the mean over images and the pooled figures."""
    return "\n".join(format_table(title, METRIC_NAMES, names, per_image, pooled, {"bad": bad}))
