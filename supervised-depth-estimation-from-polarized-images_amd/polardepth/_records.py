"""What the wrappers of the per-class record evaluators (normals_eval, pointcloud, depth_eval, consistency_eval;
csrc/class_records.hpp) share: the cached
bin-edge table of a device, the input checks, the histogram median and the device-side pool."""
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
