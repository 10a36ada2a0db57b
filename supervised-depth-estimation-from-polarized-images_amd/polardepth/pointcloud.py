"""Point-cloud accuracy on the device (pd_backproject, pd_cloud_nn, pd_cloud_stats; csrc/pointcloud.hip).

The reference turns a prediction into a point cloud and opens it next to the ground truth's in a viewer
(pointcloud/eval_pointcloud.py:256-291).  ``cloud_stats`` measures what that demo is looked at for: both depth maps are
back-projected through the camera matrix, every point of one cloud finds its exact nearest neighbour in the other, and the
distances become per-image, per-class records -- accuracy (predicted -> true), completeness (true -> predicted), Chamfer
distance, precision / recall / F-score at 5 / 10 / 20 mm.  The records stay on the device; ``CloudStats.metrics`` / ``pooled``
turn them into the report with torch ops.  The definition is the header's; tests/pointcloud_ref.py states it in NumPy."""
import numpy as np
import torch

from ._lib import lib, check, ptr, stream_ptr
from ._records import Pool, device_table, frames as _frames, hist_median, need_cuda as _need_cuda
from .normals_eval import DEFAULT_CLASSES, class_table

TILE = 256                  # PD_PCD_TILE
BINS = 512                  # PD_PCD_BINS: 0.5 mm bins, the last one open-ended
MAX_CLASSES = 16            # PD_PCD_MAX_CLASSES
RECORD_BYTES = 2096         # PD_PCD_RECORD_BYTES
BRUTE = 1                   # PD_PCD_BRUTE
BIN_M = 0.0005
BIN_MM = 0.5
THRESHOLD_BINS = (10, 20, 40)      # 5 / 10 / 20 mm: the bins below them
METRIC_NAMES = ("acc", "comp", "chamfer", "acc_med", "comp_med", "f5", "f10", "f20", "n")


def edges2_numpy():
    """The bin edges as squared distances: e[j-1] = fp32((j * 0.0005 m)^2 computed in fp64), j = 1 .. 511, strictly
    increasing.  Entries 10 / 20 / 40 (e[9], e[19], e[39]) are 5 / 10 / 20 mm."""
    e = ((np.arange(1, BINS, dtype=np.float64) * BIN_M) ** 2).astype(np.float32)
    assert np.all(np.diff(e) > 0)
    return e


def edges2(device):
    """The table on ``device``: built once with NumPy, cached."""
    return device_table(edges2_numpy, device)


def tiles_of(H, W):
    return ((H + 15) // 16) * ((W + 15) // 16)


class Cloud:
    """A tiled cloud on the device: ``points`` fp32 [N, T * 256, 4] = (x, y, z, w) and ``boxes`` fp32 [N, T, 8] = lo xyz,
    hi xyz, the int32 count of w = 1 slots, 0 (the header's record).  ``H`` / ``W``: the depth map whose 16x16 pixel tiles
    these are, or None for a cloud tiled some other way (pd_cloud_nn does not care)."""

    def __init__(self, points, boxes, H=None, W=None):
        self.points, self.boxes, self.H, self.W = points, boxes, H, W

    @property
    def tiles(self):
        return self.boxes.shape[1]

    @property
    def counts(self):
        return self.boxes.view(torch.int32)[..., 6]

    def xyz(self, i):
        """[n, 3]: the w = 1 points of image i, in slot order."""
        p = self.points[i]
        return p[p[:, 3] == 1][:, :3]

    def slot_pixels(self):
        """int64 [T * 256] on the host: the pixel index v * W + u of each slot, -1 for slots outside the image."""
        H, W = self.H, self.W
        tx = (W + 15) // 16
        s = np.arange(self.tiles * TILE)
        t, r = s // TILE, s % TILE
        v, u = (t // tx) * 16 + r // 16, (t % tx) * 16 + r % 16
        return np.where((v < H) & (u < W), v * W + u, -1)


def backproject(depth, K, gate=None, min_depth=0.1, max_depth=2.0):
    """depth [N,1,H,W] or [N,H,W] -> ``Cloud`` (pd_backproject): z = depth, x = ((u - cx) / fx) z, y = ((v - cy) / fy) z for
    the pixels whose ``gate`` depth (None: the depth itself) is inside [min_depth, max_depth]; K [N,4,4]."""
    _need_cuda("backproject", depth, K, gate)
    depth = _frames(depth, "depth").float().contiguous()
    N, H, W = depth.shape
    if gate is not None:
        gate = _frames(gate, "gate", N, H, W).float().contiguous()
    if K.shape != (N, 4, 4):
        raise ValueError(f"K must be [{N},4,4], got {tuple(K.shape)}")
    K = K.float().contiguous()
    T = tiles_of(H, W)
    dev = depth.device
    points = torch.empty((N, T * TILE, 4), dtype=torch.float32, device=dev)
    boxes = torch.empty((N, T, 8), dtype=torch.float32, device=dev)
    if N and H and W:
        with torch.cuda.device(dev):
            check(lib.pd_backproject(ptr(depth), ptr(K), ptr(gate), ptr(points), ptr(boxes), N, H, W, float(min_depth),
                                     float(max_depth), stream_ptr()), "pd_backproject")
    return Cloud(points, boxes, H, W)


def nearest(query, target, prune=True, visited=False):
    """Squared distance of every slot of ``query`` to its nearest w = 1 point of ``target`` (pd_cloud_nn): fp32 [N, Tq * 256],
    NaN for slots that are no point, +inf where the target cloud of the image is empty.  ``prune=False`` scans every target
    tile (the same bits, slower).  ``visited=True``: also the int32 [N, Tq] count of target tiles scanned per query tile."""
    _need_cuda("nearest", query.points, query.boxes, target.points, target.boxes)
    N, Tq, Tt = query.points.shape[0], query.tiles, target.tiles
    if target.points.shape[0] != N:
        raise ValueError(f"query holds {N} images, target {target.points.shape[0]}")
    dev = query.points.device
    d2 = torch.empty((N, Tq * TILE), dtype=torch.float32, device=dev)
    seen = torch.empty((N, Tq), dtype=torch.int32, device=dev) if visited else None
    if N and Tq:
        if Tt == 0:
            raise ValueError("the target cloud has no tiles")
        with torch.cuda.device(dev):
            check(lib.pd_cloud_nn(ptr(query.points), ptr(query.boxes), Tq, ptr(target.points), ptr(target.boxes), Tt, ptr(d2),
                                  ptr(seen), 0 if prune else BRUTE, N, stream_ptr()), "pd_cloud_nn")
    return (d2, seen) if visited else d2


def shares_from_fields(n, unmatched, hist):
    """[..., 3] float64: the share of the direction's points within 5 / 10 / 20 mm -- exact integer ratios, the three
    thresholds being bin edges.  Unmatched points (an empty target cloud) are points that miss."""
    cs = hist.long().cumsum(-1)
    total = (n + unmatched).double()
    return torch.stack([cs[..., b - 1].double() / total for b in THRESHOLD_BINS], -1)


def metrics_from_fields(acc, comp):
    """[..., 9] float64 = acc, comp, chamfer = acc + comp (mean distances in millimetres), the two medians (millimetres),
    F-score at 5 / 10 / 20 mm, n (the predicted cloud's matched points).  ``acc`` / ``comp``: (n, unmatched, sum_d, hist) of
    the direction predicted -> true / true -> predicted, torch tensors on any device.  A direction with n == 0 gives NaN."""
    (na, ua, sa, ha), (nc, uc, sc, hc) = acc, comp
    ha, hc = ha.long(), hc.long()
    a, c = sa / na.double() * 1000.0, sc / nc.double() * 1000.0
    P, R = shares_from_fields(na, ua, ha), shares_from_fields(nc, uc, hc)
    F = torch.where(P + R > 0, 2 * P * R / (P + R), P + R)          # 0 where both are 0, NaN where either is
    return torch.stack([a, c, a + c, hist_median(na, ha, BIN_MM), hist_median(nc, hc, BIN_MM), F[..., 0], F[..., 1], F[..., 2],
                        na.double()], -1)


class _Direction:
    """The [N][K] records of one pd_cloud_stats call, as field views."""

    def __init__(self, records):
        self.records = records                # uint8 [N, K, RECORD_BYTES]

    n = property(lambda self: self.records.view(torch.int64)[..., 0])
    bad = property(lambda self: self.records.view(torch.int64)[..., 1])
    unmatched = property(lambda self: self.records.view(torch.int64)[..., 2])
    sum_d = property(lambda self: self.records.view(torch.float64)[..., 3])
    sum_d2 = property(lambda self: self.records.view(torch.float64)[..., 4])
    hist = property(lambda self: self.records.view(torch.int32)[..., 12:12 + BINS])      # a bin holds at most 2^30 slots

    def fields(self):
        return self.n, self.unmatched, self.sum_d, self.hist

    def pool_fields(self):
        return self.n, self.bad, self.unmatched, self.sum_d, self.sum_d2, self.hist.long()


class CloudStats(Pool):
    """Both directions' records of one ``cloud_stats`` call, on the device: ``acc`` (predicted -> true) and ``comp`` (true ->
    predicted), each with the field views n, bad, unmatched, sum_d, sum_d2, hist; plus a device-side pool: ``a += b`` adds
    b's images to a's.  Nothing reaches the host until the caller asks."""

    def __init__(self, acc_records, comp_records, names, dist_acc=None, dist_comp=None):
        self.acc, self.comp = _Direction(acc_records), _Direction(comp_records)
        self.names = list(names)
        self.dist_acc, self.dist_comp = dist_acc, dist_comp      # fp32 [N, H, W] metres, or None

    def metrics(self):
        """[N, K, 9] float64 on the device, per image and class: METRIC_NAMES."""
        return metrics_from_fields(self.acc.fields(), self.comp.fields())

    def shares(self):
        """(precision, recall), each [N, K, 3] float64: the share of predicted / true points within 5 / 10 / 20 mm."""
        return (shares_from_fields(self.acc.n, self.acc.unmatched, self.acc.hist),
                shares_from_fields(self.comp.n, self.comp.unmatched, self.comp.hist))

    def _pool_fields(self):
        return self.acc.pool_fields() + self.comp.pool_fields()      # six per direction

    def pooled(self):
        """[K, 9] float64 on the device: the same figures over all points of all images pooled so far."""
        na, _, ua, sa, _, ha, nc, _, uc, sc, _, hc = self._totals()
        return metrics_from_fields((na, ua, sa, ha), (nc, uc, sc, hc))

    def pooled_shares(self):
        na, _, ua, _, _, ha, nc, _, uc, _, _, hc = self._totals()
        return shares_from_fields(na, ua, ha), shares_from_fields(nc, uc, hc)

    def pooled_bad(self):
        """[K] int64 on the device: predicted points without a usable depth (`bad` of the accuracy direction) over the pool."""
        return self._totals()[1]

    def pooled_unmatched(self):
        """[K] int64 on the device: points of either cloud whose image has no point in the other cloud, over the pool."""
        return self._totals()[2] + self._totals()[8]


def direction_stats(d2, cloud, mask=None, classes=DEFAULT_CLASSES, dist_map=False):
    """One pd_cloud_stats call: the records of ``d2`` (from ``nearest(cloud, ...)``) for a cloud of ``backproject`` ->
    (uint8 [N, K, RECORD_BYTES], dist fp32 [N,H,W] or None)."""
    _need_cuda("cloud_stats", d2, cloud.points, mask)
    if cloud.H is None:
        raise ValueError("the records need the pixel tiling of backproject (Cloud.H / Cloud.W)")
    names, table = class_table(classes)
    N, H, W = cloud.points.shape[0], cloud.H, cloud.W
    dev = d2.device
    if mask is not None:
        mask = _frames(mask, "mask", N, H, W).to(torch.int32).contiguous()
    records = torch.empty((N, len(names), RECORD_BYTES), dtype=torch.uint8, device=dev)
    dist = torch.empty((N, H, W), dtype=torch.float32, device=dev) if dist_map else None
    if N == 0 or H == 0 or W == 0:
        return records.zero_(), dist
    with torch.cuda.device(dev):
        ws = torch.empty(int(lib.pd_cloud_stats_workspace(N, H, W, len(names))), dtype=torch.uint8, device=dev)
        check(lib.pd_cloud_stats(ptr(d2), ptr(cloud.points), ptr(mask), table, len(names), ptr(edges2(dev)), ptr(dist),
                                 ptr(records), ptr(ws), ws.numel(), N, H, W, stream_ptr()), "pd_cloud_stats")
    return records, dist


def cloud_stats(pred_depth, gt_depth, K, mask=None, classes=DEFAULT_CLASSES, min_depth=0.1, max_depth=2.0, dist_map=False,
                prune=True):
    """Point-cloud accuracy of ``pred_depth`` against ``gt_depth`` -> ``CloudStats``.

    pred_depth, gt_depth   [N,1,H,W] or [N,H,W]; both clouds hold the pixels whose GROUND-TRUTH depth is inside
                           [min_depth, max_depth] (a predicted depth there that is non-finite or <= 0 is counted `bad`)
    K          [N,4,4] intrinsics
    mask       [N,1,H,W] or [N,H,W] integer instance mask, or None (then every class must be None = every pixel)
    classes    (name, None | (lo, hi)) pairs, at most 16; a point belongs to the class of its pixel
    dist_map   also return the per-pixel distance in metres of both directions (``.dist_acc``, ``.dist_comp``)
    prune      False: the brute-force route of pd_cloud_nn (the same bits)"""
    names, _ = class_table(classes)
    _need_cuda("cloud_stats", pred_depth, gt_depth, K, mask)
    pred = backproject(pred_depth, K, gate=gt_depth, min_depth=min_depth, max_depth=max_depth)
    true = backproject(gt_depth, K, min_depth=min_depth, max_depth=max_depth)
    if (pred.points.shape, pred.H, pred.W) != (true.points.shape, true.H, true.W):
        raise ValueError(f"pred_depth {tuple(pred_depth.shape)} does not match gt_depth {tuple(gt_depth.shape)}")
    acc, dist_acc = direction_stats(nearest(pred, true, prune), pred, mask, classes, dist_map)
    comp, dist_comp = direction_stats(nearest(true, pred, prune), true, mask, classes, dist_map)
    return CloudStats(acc, comp, names, dist_acc, dist_comp)


def write_ply(path, xyz, rgb=None, flip=True, normals=None):
    """Host code: a binary little-endian PLY of the points ``xyz`` [n,3] or [n,4] (then only the rows with w == 1), with
    ``rgb`` [n,3] uint8 colours (rows as in xyz) if given.  ``flip`` negates y and z, as the reference's viewer transform
    does (eval_pointcloud.py:288).  ``normals`` [n,3] (rows as in xyz), if given, become the properties nx ny nz behind
    x y z, flipped with the points."""
    xyz = np.asarray(xyz.detach().cpu() if isinstance(xyz, torch.Tensor) else xyz, dtype=np.float32)
    if rgb is not None:
        rgb = np.asarray(rgb.detach().cpu() if isinstance(rgb, torch.Tensor) else rgb)
        if rgb.shape != (xyz.shape[0], 3):
            raise ValueError(f"rgb must be [{xyz.shape[0]},3], got {rgb.shape}")
        rgb = rgb.astype(np.uint8)
    if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
        raise ValueError(f"xyz must be [n,3] or [n,4], got {xyz.shape}")
    if normals is not None:
        normals = np.asarray(normals.detach().cpu() if isinstance(normals, torch.Tensor) else normals, dtype=np.float32)
        if normals.shape != (xyz.shape[0], 3):
            raise ValueError(f"normals must be [{xyz.shape[0]},3], got {normals.shape}")
    if xyz.shape[1] == 4:
        keep = xyz[:, 3] == 1
        xyz, rgb = xyz[keep, :3], (rgb[keep] if rgb is not None else None)
        normals = normals[keep] if normals is not None else None
    if flip:
        xyz = xyz * np.array([1, -1, -1], np.float32)
        normals = normals * np.array([1, -1, -1], np.float32) if normals is not None else None
    n = xyz.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if normals is not None else [])
    fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")] if rgb is not None else []
    rows = np.empty(n, dtype=fields)
    rows["x"], rows["y"], rows["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        rows["nx"], rows["ny"], rows["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if rgb is not None:
        rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    header += [f"property float {c}" for c in "xyz"]
    if normals is not None:
        header += [f"property float {c}" for c in ("nx", "ny", "nz")]
    if rgb is not None:
        header += [f"property uchar {c}" for c in ("red", "green", "blue")]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rows.tobytes())
    return n
