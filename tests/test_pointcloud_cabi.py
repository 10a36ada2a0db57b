"""pd_backproject / pd_cloud_nn / pd_cloud_stats, host side (no GPU): the exported symbols, the defines, SIGNATURES, every
refusal decided before the device is touched, the workspace query, and the Python layer's refusal of CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib
from polardepth import pointcloud as PC

HEADER = os.path.join(ROOT, "include", "polardepth.h")
ALL = (ctypes.c_int * 2)(1, 0)                       # one class: every pixel
RANGED = (ctypes.c_int * 4)(1, 0, 20, 160)
P = ctypes.c_void_p(64)                              # a non-null, 16-byte aligned dummy: never dereferenced on these paths
ODD = ctypes.c_void_p(72)                            # 8-byte aligned only


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)u?\)?", src))
    assert int(defs["PD_PCD_TILE"]) == PC.TILE == 256
    assert int(defs["PD_PCD_BINS"]) == PC.BINS == 512
    assert int(defs["PD_PCD_MAX_CLASSES"]) == PC.MAX_CLASSES == 16
    assert int(defs["PD_PCD_RECORD_BYTES"]) == PC.RECORD_BYTES == 48 + 4 * 512 == 2096
    assert int(defs["PD_PCD_BRUTE"]) == PC.BRUTE == 1
    so = ctypes.CDLL(_lib.lib.path)
    for name, nargs in (("pd_backproject", 11), ("pd_cloud_nn", 11), ("pd_cloud_stats", 14), ("pd_cloud_stats_workspace", 4)):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["pd_cloud_stats_workspace"][0] is ctypes.c_size_t
    assert "eval_pointcloud.py:256-291" in src and ":83-85" in src              # the header cites what it measures


def test_backproject_refusals_need_no_gpu():
    L, err = _lib.lib, _lib.lib.pd_last_error

    def call(depth=P, K=P, gate=None, points=P, boxes=P, N=1, H=8, W=8):
        return L.pd_backproject(depth, K, gate, points, boxes, N, H, W, 0.1, 2.0, None)

    for kw in ({"depth": None}, {"K": None}, {"points": None}, {"boxes": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"points": ODD}, {"boxes": ODD}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
    assert call(N=0) == 0 and call(N=0, gate=P) == 0
    assert call(N=0, points=None) == -22


def test_cloud_nn_refusals_need_no_gpu():
    L, err = _lib.lib, _lib.lib.pd_last_error

    def call(qp=P, qb=P, Tq=4, tp=P, tb=P, Tt=4, d2=P, visited=None, flags=0, N=1):
        return L.pd_cloud_nn(qp, qb, Tq, tp, tb, Tt, d2, visited, flags, N, None)

    for kw in ({"qp": None}, {"qb": None}, {"tp": None}, {"tb": None}, {"d2": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"qp": ODD}, {"qb": ODD}, {"tp": ODD}, {"tb": ODD}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    for kw in ({"N": -1}, {"Tq": 0}, {"Tq": -2}, {"Tt": 0}, {"Tt": -1}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for flags in (2, 4, 3, 1 << 31):
        assert call(flags=flags) == -22 and b"unknown flags" in err(), flags
    assert call(Tq=(1 << 22) + 1) == -22 and b"too large" in err()                # slot offsets inside a frame are 32-bit
    assert call(Tt=(1 << 22) + 1) == -22 and b"too large" in err()
    assert call(N=0) == 0 and call(N=0, flags=PC.BRUTE, visited=P) == 0
    assert call(N=0, d2=None) == -22


def test_cloud_stats_refusals_need_no_gpu():
    L, err = _lib.lib, _lib.lib.pd_last_error

    def call(d2=P, points=P, mask=None, classes=ALL, K=1, edges=P, dist=None, stats=P, ws=P, ws_bytes=1 << 40, N=1, H=8, W=8):
        return L.pd_cloud_stats(d2, points, mask, classes, K, edges, dist, stats, ws, ws_bytes, N, H, W, None)

    for kw in ({"d2": None}, {"points": None}, {"classes": None}, {"edges": None}, {"stats": None}, {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    need = L.pd_cloud_stats_workspace(1, 8, 8, 1)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(ws_bytes=0) == -22 and b"workspace too small" in err()
    for K in (0, -1, 17, 1 << 20):
        assert call(K=K) == -22 and b"classes" in err(), K
    assert call(classes=RANGED, K=2) == -22 and b"mask is null" in err() and b"[20, 160]" in err()
    assert call(classes=(ctypes.c_int * 2)(0, 0)) == -22 and b"mask is null" in err()      # lo == hi is a range too
    for kw in ({"points": ODD}, {"stats": ODD}, {"ws": ODD}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
    assert call(N=0) == 0
    assert call(N=0, ws=None) == -22                                               # but its arguments are still checked


def test_workspace_is_monotone_never_zero_and_a_multiple_of_16():
    ws = _lib.lib.pd_cloud_stats_workspace
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


def test_python_layer_refuses_cpu_tensors():
    depth, K = torch.ones(1, 1, 4, 4), torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.backproject(depth, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.cloud_stats(depth, depth, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.cloud_stats(depth, depth, K, mask=torch.zeros(1, 1, 4, 4, dtype=torch.int32))
    cloud = PC.Cloud(torch.zeros(1, 256, 4), torch.zeros(1, 1, 8), 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.nearest(cloud, cloud)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.direction_stats(torch.zeros(1, 256), cloud)


def test_class_table_limits():
    """The class table is looked at before any tensor: at most 16 classes, at least one."""
    depth, K = torch.ones(1, 1, 4, 4), torch.eye(4)[None]
    for classes in ([], [("c", None)] * 17):
        with pytest.raises(ValueError, match="1 .. 16"):
            PC.cloud_stats(depth, depth, K, classes=classes)
