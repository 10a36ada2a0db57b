"""pd_depth_stats / pd_depth_medians, host side (no GPU): the exported symbols, the defines, SIGNATURES, every refusal decided
before the device is touched, the workspace queries -- and the workspace sizes of the two evaluators that share the record
reducer, which the reducer's new `Sums` parameter must not have changed."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib
from polardepth import depth_eval as DE

HEADER = os.path.join(ROOT, "include", "polardepth.h")
ALL = (ctypes.c_int * 2)(1, 0)                       # one class: every pixel
RANGED = (ctypes.c_int * 4)(1, 0, 20, 160)
INF = float("inf")


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_DSTAT_BINS"]) == DE.BINS == 512
    assert int(defs["PD_DSTAT_MAX_CLASSES"]) == DE.MAX_CLASSES == 16
    assert int(defs["PD_DSTAT_COUNTERS"]) == 4 and int(defs["PD_DSTAT_SUMS"]) == 4
    assert int(defs["PD_DSTAT_RECORD_BYTES"]) == DE.RECORD_BYTES == 80 + 4 * 512
    so = ctypes.CDLL(_lib.lib.path)
    for name in ("pd_depth_stats", "pd_depth_stats_workspace", "pd_depth_medians", "pd_depth_medians_workspace"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    assert len(_lib.SIGNATURES["pd_depth_stats"][1]) == 17 and len(_lib.SIGNATURES["pd_depth_medians"][1]) == 15
    assert _lib.SIGNATURES["pd_depth_stats_workspace"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["pd_depth_medians_workspace"][0] is ctypes.c_size_t


def test_stats_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only

    def call(gt=p, pred=p, mask=None, classes=ALL, K=1, scale=None, edges=p, out_err=None, stats=p, ws=p, ws_bytes=1 << 40,
             N=1, H=8, W=8, lo=0.1, hi=2.0):
        return L.pd_depth_stats(gt, pred, mask, classes, K, scale, edges, out_err, stats, ws, ws_bytes, N, H, W, lo, hi, None)

    for kw in ({"gt": None}, {"pred": None}, {"classes": None}, {"edges": None}, {"stats": None}, {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for K in (0, -1, 17, 1 << 20):
        assert call(K=K) == -22 and b"classes" in err(), K
    assert call(classes=RANGED, K=2) == -22 and b"mask is null" in err() and b"[20, 160]" in err()
    assert call(classes=(ctypes.c_int * 2)(0, 0)) == -22 and b"mask is null" in err()      # lo == hi is a range too
    for lo in (0.0, -0.5, float("nan")):
        assert call(lo=lo) == -22 and b"min_depth" in err() and b"positive" in err(), lo
    for lo, hi in ((0.5, 0.5), (0.5, 0.25), (0.5, float("nan")), (INF, INF)):
        assert call(lo=lo, hi=hi) == -22 and b"above min_depth" in err(), (lo, hi)
    for kw in ({"stats": odd}, {"ws": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    need = L.pd_depth_stats_workspace(1, 8, 8, 1)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(ws_bytes=0) == -22 and b"workspace too small" in err()
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()      # offsets inside a frame are 32-bit
    assert call(scale=p, out_err=p) == -22 and b"unscaled call only" in err()
    # an empty batch is fine and touches nothing; max_depth = +inf is allowed
    assert call(N=0) == 0 and call(N=0, hi=INF) == 0 and call(N=0, scale=p) == 0 and call(N=0, out_err=p) == 0
    assert call(N=0, ws=None) == -22                                               # but its arguments are still checked


def test_medians_argument_validation_needs_no_gpu():
    L = _lib.lib
    err = L.pd_last_error
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(72)

    def call(gt=p, pred=p, mask=None, classes=ALL, K=1, count=p, med=p, ws=p, ws_bytes=1 << 40, N=1, H=8, W=8, lo=0.1, hi=2.0):
        return L.pd_depth_medians(gt, pred, mask, classes, K, count, med, ws, ws_bytes, N, H, W, lo, hi, None)

    for kw in ({"gt": None}, {"pred": None}, {"classes": None}, {"count": None}, {"med": None}, {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for K in (0, 17):
        assert call(K=K) == -22 and b"classes" in err(), K
    assert call(classes=RANGED, K=2) == -22 and b"mask is null" in err()
    assert call(lo=0.0) == -22 and b"positive" in err()
    assert call(lo=1.0, hi=1.0) == -22 and b"above min_depth" in err()
    for kw in ({"count": odd}, {"med": odd}, {"ws": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    need = L.pd_depth_medians_workspace(1, 1)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
    assert call(N=0) == 0 and call(N=0, hi=INF) == 0
    assert call(N=0, med=None) == -22


def test_workspaces_are_monotone_never_zero_and_multiples_of_16():
    ws = _lib.lib.pd_depth_stats_workspace
    assert ws(0, 0, 0, 0) > 0 and ws(0, 512, 640, 12) > 0 and ws(-1, -1, -1, -1) > 0
    shapes = [(1, 1, 4, 1), (2, 5, 7, 1), (3, 33, 70, 12), (4, 64, 96, 12), (12, 320, 480, 12), (16, 512, 640, 16),
              (4096, 4096, 4096, 16), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]
    sizes = [ws(*s) for s in shapes]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[4] < sizes[5]
    for N, H, W, K in shapes[:6]:
        base = ws(N, H, W, K)
        assert ws(N + 1, H, W, K) >= base and ws(N, H + 1, W, K) >= base and ws(N, H, W + 1, K) >= base
        assert ws(N, H, W, K + 1) >= base
    assert ws(3, 37, 53, 12) == 3 * 2 * 12 * 4 * 8             # [N][G][K][4] doubles, G = ceil(37 * 53 / 1024)
    wm = _lib.lib.pd_depth_medians_workspace
    assert wm(0, 0) > 0 and wm(-1, -1) > 0
    pairs = [(1, 1), (2, 1), (3, 12), (12, 12), (16, 16), (4096, 16), (2 ** 31 - 1, 2 ** 31 - 1)]
    msizes = [wm(*s) for s in pairs]
    assert all(s > 0 and s % 16 == 0 for s in msizes) and msizes == sorted(msizes) and len(set(msizes)) == len(msizes)
    assert wm(3, 12) == 3 * 12 * (4 * 4 * 256 * 4 + 32)         # four passes of four 256-bin histograms, and the state


# (N, H, W, K) -> bytes, as the parent commit returns them: [N][G][K][2] doubles with G = min(64, ceil(items / 1024)), items
# = H * ceil(W / 4) quads for the normals and 256 * ceil(H / 16) * ceil(W / 16) slots for the cloud
PARENT_WORKSPACES = [
    ((1, 8, 8, 1), 16, 16),
    ((3, 33, 70, 12), 576, 2304),
    ((4, 64, 96, 12), 1536, 4608),
    ((12, 320, 480, 12), 87552, 147456),
    ((16, 512, 640, 16), 262144, 262144),
    ((0, 0, 0, 0), 16, 16),
]


@pytest.mark.parametrize("shape,normals,cloud", PARENT_WORKSPACES)
def test_the_other_evaluators_keep_their_workspace_sizes(shape, normals, cloud):
    assert _lib.lib.pd_normals_stats_workspace(*shape) == normals
    assert _lib.lib.pd_cloud_stats_workspace(*shape) == cloud


def test_python_layer_refuses_cpu_tensors_and_bad_options():
    pred, gt = torch.ones(1, 1, 4, 4), torch.ones(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DE.depth_stats(pred, gt, classes=[("all", None)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DE.depth_medians(pred, gt, mask=torch.zeros(1, 1, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="median_scaling"):
        DE.depth_stats(pred, gt, median_scaling="median")
    with pytest.raises(ValueError, match="out_err"):
        DE.depth_stats(pred, gt, median_scaling="numpy", out_err=True)
    assert len(DE.METRIC_NAMES) == 13
