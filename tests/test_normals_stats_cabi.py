"""pd_normals_stats, host side (no GPU): the exported symbols, the three defines, SIGNATURES, every refusal decided before the
device is touched, the workspace query, and the Python layer's refusal of CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib
from polardepth import normals_eval as NE

HEADER = os.path.join(ROOT, "include", "polardepth.h")
ALL = (ctypes.c_int * 2)(1, 0)                       # one class: every pixel
RANGED = (ctypes.c_int * 4)(1, 0, 20, 160)


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_NSTAT_BINS"]) == NE.BINS == 720
    assert int(defs["PD_NSTAT_MAX_CLASSES"]) == NE.MAX_CLASSES == 16
    assert int(defs["PD_NSTAT_RECORD_BYTES"]) == NE.RECORD_BYTES == 32 + 4 * 720
    so = ctypes.CDLL(_lib.lib.path)
    for name in ("pd_normals_stats", "pd_normals_stats_workspace"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    assert len(_lib.SIGNATURES["pd_normals_stats"][1]) == 19 and len(_lib.SIGNATURES["pd_normals_stats_workspace"][1]) == 4
    assert _lib.SIGNATURES["pd_normals_stats_workspace"][0] is ctypes.c_size_t


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only

    def call(pred=p, ld=3, gtn=p, gt=p, mask=None, classes=ALL, K=1, edges=p, gate=1, err_deg=None, stats=p, ws=p,
             ws_bytes=1 << 40, N=1, H=8, W=8):
        return L.pd_normals_stats(pred, ld, gtn, gt, mask, classes, K, edges, gate, err_deg, stats, ws, ws_bytes, N, H, W,
                                  0.1, 2.0, None)

    for kw in ({"pred": None}, {"gtn": None}, {"gt": None}, {"classes": None}, {"edges": None}, {"stats": None}, {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    need = L.pd_normals_stats_workspace(1, 8, 8, 1)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(ws_bytes=0) == -22 and b"workspace too small" in err()
    for K in (0, -1, 17, 1 << 20):
        assert call(K=K) == -22 and b"classes" in err(), K
    assert call(classes=RANGED, K=2) == -22 and b"mask is null" in err() and b"[20, 160]" in err()
    assert call(classes=(ctypes.c_int * 2)(0, 0)) == -22 and b"mask is null" in err()      # lo == hi is a range too
    for ld in (2, 1, 0, -3):
        assert call(ld=ld) == -22 and b"at least 3" in err(), ld
    for gate in (2, -1, 255):
        assert call(gate=gate) == -22 and b"gate" in err(), gate
    for kw in ({"gtn": odd}, {"stats": odd}, {"ws": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()      # offsets inside a frame are 32-bit
    # an empty batch is fine and touches nothing
    assert call(N=0) == 0
    assert call(N=0, ws=None) == -22                                               # but its arguments are still checked


def test_workspace_is_monotone_never_zero_and_a_multiple_of_16():
    ws = _lib.lib.pd_normals_stats_workspace
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
    pred, gt, K = torch.zeros(1, 3, 4, 4), torch.ones(1, 1, 4, 4), torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NE.normals_stats(pred, gt, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NE.normals_stats(pred, gt, K, mask=torch.zeros(1, 1, 4, 4, dtype=torch.int32))


def test_class_table_limits():
    with pytest.raises(ValueError, match="1 .. 16"):
        NE.class_table([])
    with pytest.raises(ValueError, match="1 .. 16"):
        NE.class_table([("c", None)] * 17)
    names, table = NE.class_table([("a", None), ("b", (3, 9))])
    assert names == ["a", "b"] and list(table) == [1, 0, 3, 9]
