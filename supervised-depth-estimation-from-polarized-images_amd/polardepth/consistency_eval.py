"""Multi-view depth consistency per material on the device (pd_depth_consistency, csrc/consistency.hip).

``consistency`` asks whether the depth maps of neighbouring frames describe the same surface once the camera motion between
them is taken into account: every pixel of the current view is projected into each source view at its depth, the source
depth is sampled there, and the sampled point is projected back (the forward-backward check of MVSNet's geometric filter).
The distance of the returned pixel from the one that was sent (``e_px``) and the relative difference of the returned depth
(``e_rel``) are scored for every pixel class of the instance mask in one read of the batch, at three nested levels.  The
figure needs no ground-truth depth -- only the poses -- so it is there on glass and metal, where the depth sensors have
holes, and on sequences without ground truth.

A true occlusion is not an inconsistency, but without ground truth the two cannot be told apart: an occluded pixel returns
somewhere else and counts as inconsistent, the shares and the means carry it, and the MEDIANS are the robust figures.  Where
ground truth exists, ``visibility`` runs the same call on the ground-truth depths and returns ``level >= 4`` as the
``visible`` mask of a second call, which limits the score to the pairs the true geometry says are mutually visible.

The per-image, per-class records stay on the device; ``ConsistencyStats.metrics`` / ``pooled`` turn them into the report with
torch ops.  The definition is the header's; tests/consistency_ref.py states it in NumPy."""
import ctypes

import torch

from ._lib import lib, check, ptr, stream_ptr
from ._records import Pool, frames, hist_median, need_cuda
from .normals_eval import DEFAULT_CLASSES, class_table

BINS = 256                  # PD_CONS_BINS: bins of e_rel, 1/1024 wide, the last one open-ended
MAX_CLASSES = 16            # PD_DSTAT_MAX_CLASSES
MAX_FRAMES = 8              # PD_REPROJ_MAX_FRAMES
RECORD_BYTES = 1136         # PD_CONS_RECORD_BYTES
BIN_PERCENT = 100.0 / 1024.0
DEFAULT_TAUS = ((4.0, 0.04), (2.0, 0.02), (1.0, 0.01))      # (tau_px, tau_rel), loose -> tight; the last is MVSNet's filter
COUNTER_NAMES = ("loose", "mid", "tight", "invalid", "absent", "filtered", "outside", "hole")
METRIC_NAMES = ("compared", "loose", "mid", "tight", "mean_rel%", "median_rel%", "mean_px", "rms_px", "invalid", "absent",
                "filtered", "outside", "hole", "n")
WANT = ("level", "n_cons", "fused")


def metrics_from_fields(n, counters, sums, hist):
    """[..., 14] float64 (METRIC_NAMES) from n [...], counters [..., 8], sums [..., 4] and hist [..., 256], with torch ops on
    whatever device holds them: the share of the (pixel, view) pairs that were compared; among the compared pairs, the shares
    consistent at the three levels, the mean and the median of e_rel in percent (the median interpolated inside its bin; with
    more than half of the pairs in the open last bin it reads 25 % or a little more), the mean and the RMS of e_px in pixels;
    the shares of the five reasons among all pairs; n.  A record without a pair gives NaN."""
    nf = n.double()
    total = nf + counters[..., 3:8].sum(-1).double()
    cols = [nf / total] + [counters[..., j].double() / nf for j in range(3)]
    cols += [100.0 * sums[..., 1] / nf, hist_median(n, hist.long(), BIN_PERCENT), sums[..., 0] / nf, (sums[..., 2] / nf).sqrt()]
    cols += [counters[..., j].double() / total for j in range(3, 8)] + [nf]
    return torch.stack(cols, -1)


class ConsistencyStats(Pool):
    """The [N][K] records of one ``consistency`` call, on the device, plus a device-side pool: ``a += b`` adds b's images to
    a's pool (int64 counts, fp64 sums, histograms widened to int64).  Nothing reaches the host until the caller asks."""
    METRIC_NAMES = METRIC_NAMES

    def __init__(self, records, names, level=None, n_cons=None, fused=None):
        self.records = records                # uint8 [N, K, RECORD_BYTES]
        self.names = list(names)
        self.level = level                    # uint8 [N, F, H, W] or None
        self.n_cons = n_cons                  # uint8 [N, H, W] or None
        self.fused = fused                    # fp32 [N, H, W] or None

    # ---- the fields of the records, as views
    @property
    def n(self):
        return self.records.view(torch.int64)[..., 0]

    @property
    def counters(self):
        return self.records.view(torch.int64)[..., 1:9]

    @property
    def sums(self):
        return self.records.view(torch.float64)[..., 9:13]

    @property
    def hist(self):
        return self.records.view(torch.int32)[..., 28:28 + BINS]      # a bin holds at most 2^30 * 8 pairs of one image

    def metrics(self):
        """[N, K, 14] float64 on the device (METRIC_NAMES), per image and class."""
        return metrics_from_fields(self.n, self.counters, self.sums, self.hist)

    def _pool_fields(self):
        return self.n, self.counters, self.sums, self.hist.long()

    def pooled(self):
        """[K, 14] float64 on the device: the same figures over all pairs of all images pooled so far (this call's, and
        every call's added with ``+=``)."""
        return metrics_from_fields(*self._totals())


def _taus(taus):
    taus = [(float(a), float(b)) for a, b in taus]
    if len(taus) != 3:
        raise ValueError(f"taus must be three (tau_px, tau_rel) pairs, loose to tight, got {taus!r}")
    return (ctypes.c_double * 3)(*[a for a, _ in taus]), (ctypes.c_double * 3)(*[b for _, b in taus])


def consistency(depth0, depths, T, K, inv_K, frame_valid=None, mask=None, classes=DEFAULT_CLASSES, visible=None,
                min_depth=0.1, max_depth=2.0, taus=DEFAULT_TAUS, fuse_level=4, want=("level", "fused")):
    """Consistency records of ``depth0`` against the source views' ``depths`` -> ``ConsistencyStats``.

    depth0        [N,1,H,W] or [N,H,W] depth of the current view in metres
    depths        [N,F,H,W] depth of each source view, 1 <= F <= 8
    T             [N,F,4,4] rigid motion from the current view to view f, as the loader's ("poses", i)
    K, inv_K      [N,4,4]
    frame_valid   [N,F] or None: a 0 takes the whole view of that item out (``absent``)
    mask          [N,1,H,W] or [N,H,W] integer instance mask, or None (then every class must be None = every pixel)
    classes       (name, None | (lo, hi)) pairs, at most 16
    visible       [N,F,H,W] bool / uint8 or None: a 0 takes the pair out (``filtered``); see ``visibility``
    taus          three (tau_px, tau_rel) pairs, loose to tight, non-increasing and positive
    fuse_level    2, 3 or 4: the level a view must reach to be counted in ``n_cons`` and averaged into ``fused``
    want          which per-pixel outputs to write: "level" uint8 [N,F,H,W] (0 not compared, 1 compared, 2 / 3 / 4 the
                  tightest level met), "n_cons" uint8 [N,H,W], "fused" fp32 [N,H,W]

    Without ground truth a true occlusion counts as inconsistent; the medians are the robust figures (module docstring)."""
    want = tuple(want)
    for w in want:
        if w not in WANT:
            raise ValueError(f"want takes {WANT}, got {w!r}")
    need_cuda("consistency", depth0, depths, T, K, inv_K, frame_valid, mask, visible)
    depth0 = frames(depth0, "depth0")
    N, H, W = depth0.shape
    if depths.dim() != 4 or depths.shape[0] != N or tuple(depths.shape[2:]) != (H, W):
        raise ValueError(f"depths must be [N,F,H,W] = ({N}, F, {H}, {W}), got {tuple(depths.shape)}")
    F = depths.shape[1]
    if not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"consistency takes 1 .. {MAX_FRAMES} source views, got {F}")
    if tuple(T.shape) != (N, F, 4, 4) or tuple(K.shape) != (N, 4, 4) or tuple(inv_K.shape) != (N, 4, 4):
        raise ValueError(f"T must be {(N, F, 4, 4)}, K and inv_K {(N, 4, 4)}; got {tuple(T.shape)}, {tuple(K.shape)}, "
                         f"{tuple(inv_K.shape)}")
    depth0 = depth0.float().contiguous()
    depths = depths.float().contiguous()
    T, K, inv_K = T.float().contiguous(), K.float().contiguous(), inv_K.float().contiguous()
    if frame_valid is not None:
        if tuple(frame_valid.shape) != (N, F):
            raise ValueError(f"frame_valid must be {(N, F)}, got {tuple(frame_valid.shape)}")
        frame_valid = frame_valid.float().contiguous()
    if mask is not None:
        mask = frames(mask, "mask", N, H, W).to(torch.int32).contiguous()
    if visible is not None:
        if tuple(visible.shape) != (N, F, H, W):
            raise ValueError(f"visible must be {(N, F, H, W)}, got {tuple(visible.shape)}")
        visible = visible.to(torch.uint8).contiguous()
    names, table = class_table(classes)
    nk = len(names)
    tau_px, tau_rel = _taus(taus)
    dev = depth0.device
    records = torch.empty((N, nk, RECORD_BYTES), dtype=torch.uint8, device=dev)
    level = torch.empty((N, F, H, W), dtype=torch.uint8, device=dev) if "level" in want else None
    n_cons = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if "n_cons" in want else None
    fused = torch.empty((N, H, W), dtype=torch.float32, device=dev) if "fused" in want else None
    if N == 0 or H == 0 or W == 0:
        return ConsistencyStats(records.zero_(), names, level, n_cons, fused)
    with torch.cuda.device(dev):
        ws = torch.empty(int(lib.pd_depth_consistency_workspace(N, H, W, nk)), dtype=torch.uint8, device=dev)
        check(lib.pd_depth_consistency(ptr(depth0), ptr(depths), ptr(T), ptr(K), ptr(inv_K), ptr(frame_valid), ptr(visible),
                                       ptr(mask), table, nk, float(min_depth), float(max_depth), tau_px, tau_rel,
                                       int(fuse_level), ptr(level), ptr(n_cons), ptr(fused), ptr(records), ptr(ws), ws.numel(),
                                       N, F, H, W, stream_ptr()), "pd_depth_consistency")
    return ConsistencyStats(records, names, level, n_cons, fused)


def visibility(depth0_gt, depths_gt, T, K, inv_K, frame_valid=None, min_depth=0.1, max_depth=2.0, taus=DEFAULT_TAUS):
    """bool [N,F,H,W]: the (pixel, view) pairs the GROUND-TRUTH geometry says are mutually visible -- the same call on the
    ground-truth depths, ``level >= 4``.  Pass it as ``visible`` to ``consistency`` on predicted depths: a pixel that the
    true scene occludes in view f, that leaves its frame or that falls on a hole of either ground-truth map is then
    ``filtered`` instead of being scored as an inconsistency of the prediction."""
    st = consistency(depth0_gt, depths_gt, T, K, inv_K, frame_valid=frame_valid, classes=(("all", None),),
                     min_depth=min_depth, max_depth=max_depth, taus=taus, want=("level",))
    return st.level >= 4
