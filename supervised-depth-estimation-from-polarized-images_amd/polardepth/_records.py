"""What the wrappers of the per-class record evaluators (normals_eval, pointcloud, depth_eval, consistency_eval;
csrc/class_records.hpp) share: the cached
bin-edge table of a device, the input checks, the histogram median and the device-side pool; and what their drivers share
(manydepth.evaluation's ``test_*`` methods): the per-class report that pools the batches, averages over images and prints."""
import torch

_TABLES = {}                # (builder, device) -> the table


def device_table(build, device):
    """``build()``'s NumPy table on ``device``: built once, cached."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if (build, device) not in _TABLES:
        _TABLES[build, device] = torch.from_numpy(build()).to(device)
    return _TABLES[build, device]


def need_cuda(what, *tensors):
    for t in tensors:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{what} needs CUDA(HIP) tensors; there is no CPU fallback")


def frames(t, what, N=None, H=None, W=None):
    """[N,1,H,W] or [N,H,W] -> [N,H,W], of the given shape if one is given."""
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or (N is not None and tuple(t.shape) != (N, H, W)):
        raise ValueError(f"{what} must be [N,1,H,W] or [N,H,W]" + (f" = {(N, H, W)}" if N is not None else "") +
                         f", got {tuple(t.shape)}")
    return t


def hist_median(n, hist, bin_width):
    """The median of n [...] values with the int64 histogram hist [..., bins] of ``bin_width``: interpolated linearly inside
    the bin that holds the n/2-th value."""
    cs = hist.cumsum(-1)
    half = n.double() / 2
    b = (cs.double() < half[..., None]).sum(-1).clamp(max=hist.shape[-1] - 1)
    hb = hist.gather(-1, b[..., None])[..., 0]
    below = cs.gather(-1, b[..., None])[..., 0] - hb
    return (b.double() + (half - below.double()) / hb.double()) * bin_width


class Pool:
    """Device-side pool of [N][K] records: ``a += b`` adds b's images to a's pool.  A subclass has ``names`` and
    ``_pool_fields()``, its record fields [N, K, ...] in a fixed order (histograms widened to int64); ``_totals()`` is their
    sums over the images pooled so far."""
    _pool = None

    def _totals(self):
        if self._pool is None:
            self._pool = [f.sum(0) for f in self._pool_fields()]
        return self._pool

    def __iadd__(self, other):
        if other.names != self.names:
            raise ValueError(f"cannot pool the classes {other.names} into {self.names}")
        self._pool = [a + b for a, b in zip(self._totals(), other._totals())]
        return self


def format_table(title, metric_names, names, per_image, pooled, extras, width=9):
    """The lines of a per-class report: the heading, then for every class whose pooled count (``metric_names``' "n") is above
    zero the mean over images (unless ``per_image`` is None) and the pooled figures, the latter followed by the integers of
    ``extras`` {name: [K]}.  ``per_image`` / ``pooled``: host arrays [K, M]."""
    nm, n_col = len(metric_names), metric_names.index("n")
    row = f"&{{: {width}.4f}} " * nm
    lines = [f"{title} " + (f"{{:>{width}}} " * nm).format(*metric_names)]
    for k, name in enumerate(names):
        if pooled[k][n_col] > 0:
            if per_image is not None:
                lines.append(f"{name:>8} per-image " + row.format(*per_image[k].tolist()))
            lines.append(f"{name:>8} pooled    " + row.format(*pooled[k].tolist()) +
                         "".join(f" {c} {int(v[k])}" for c, v in extras.items()))
    return lines


class ClassReport:
    """The driver every per-class evaluator shares: ``add`` once per batch, ``finish`` once behind the loop.  It pools the
    batches' ``Pool`` objects with ``+=`` (the first one becomes the pool) and, where per-image ``metrics`` [N, K, M] come
    with their ``valid`` [N, K], adds the valid images' figures (one ``.sum(0)`` per batch, batches in the order they come,
    in the metrics' dtype) and counts them.  Nothing leaves the device before ``finish``."""

    def __init__(self, metric_names, width=9):
        self.metric_names, self.width = tuple(metric_names), width
        self.total = self.sums = self.counts = None

    def add(self, stats, metrics=None, valid=None):
        if metrics is not None:
            s, c = torch.where(valid[..., None], metrics, torch.zeros_like(metrics)).sum(0), valid.sum(0)
        if self.total is None:
            self.total = stats
            if metrics is not None:
                self.sums, self.counts = s, c
        else:
            self.total += stats
            if metrics is not None:
                self.sums += s
                self.counts += c

    def finish(self, title, extras=None, per_image=None, show_extras=True):
        """Prints the table and returns {class: {"per_image": [M], "pooled": [M], and one entry per extra}}; {} when nothing
        was added.  ``per_image``: the mean over the valid images, sums / counts (NaN for a class no image has), unless the
        caller reduced its own [K, M]; without either the report is pooled only.  ``extras``: the pool -> {name: [K, ...]},
        its pooled fields to report beside the figures, an int per class where [K]; default {"bad": ``pooled_bad()``}."""
        if self.total is None:
            return {}
        host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t
        if per_image is None and self.sums is not None:
            per_image = self.sums / self.counts[:, None].double()
        extras = {"bad": self.total.pooled_bad()} if extras is None else extras(self.total)
        self.per_image, self.pooled = host(per_image), host(self.total.pooled())
        self.extras = {c: host(v) for c, v in extras.items()}
        names = self.total.names
        print("\n".join(format_table(title, self.metric_names, names, self.per_image, self.pooled,
                                     self.extras if show_extras else {}, self.width)))
        results = {}
        for k, name in enumerate(names):
            r = {} if self.per_image is None else {"per_image": self.per_image[k]}
            r["pooled"] = self.pooled[k]
            r.update({c: int(v[k]) if v.ndim == 1 else v[k] for c, v in self.extras.items()})
            results[name] = r
        return results
