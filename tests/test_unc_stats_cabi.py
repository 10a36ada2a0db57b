"""pd_unc_stats, host side (no GPU): the exported symbols, the defines, SIGNATURES, every refusal decided before the device is
touched, the workspace query, N == 0 -- and the Python layer's own refusals."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib
from polardepth import uncertainty_eval as UE

HEADER = os.path.join(ROOT, "include", "polardepth.h")
ALL = (ctypes.c_int * 2)(1, 0)                       # one class: every pixel
RANGED = (ctypes.c_int * 4)(1, 0, 20, 160)
INF = float("inf")


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_USTAT_BINS"]) == UE.BINS == int(defs["PD_DSTAT_BINS"]) == 512
    assert int(defs["PD_USTAT_COUNTERS"]) == 3 and int(defs["PD_USTAT_SUMS"]) == 3
    assert int(defs["PD_USTAT_TABLE_ROWS"]) == UE.TABLE_ROWS == 3
    assert int(defs["PD_USTAT_RECORD_BYTES"]) == UE.RECORD_BYTES == 64 + 4 * 512
    assert int(defs["PD_USTAT_MAX_DEPTH"]) == UE.MAX_DEPTH == 1000
    so = ctypes.CDLL(_lib.lib.path)
    for name in ("pd_unc_stats", "pd_unc_stats_workspace"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    assert len(_lib.SIGNATURES["pd_unc_stats"][1]) == 19 and _lib.SIGNATURES["pd_unc_stats_workspace"][0] is ctypes.c_size_t
    assert len(UE.METRIC_NAMES) == 10


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only

    def call(gt=p, pred=p, unc=p, mask=None, classes=ALL, K=1, edges=p, b_lo=0.0005, b_hi=0.5, stats=p, tables=p, ws=p,
             ws_bytes=1 << 40, N=1, H=8, W=8, lo=0.1, hi=2.0):
        return L.pd_unc_stats(gt, pred, unc, mask, classes, K, edges, b_lo, b_hi, stats, tables, ws, ws_bytes, N, H, W, lo, hi, None)

    for kw in ({"gt": None}, {"pred": None}, {"unc": None}, {"classes": None}, {"edges": None}, {"stats": None}, {"tables": None},
               {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for K in (0, -1, 17, 1 << 20):
        assert call(K=K) == -22 and b"classes" in err(), K
    assert call(classes=RANGED, K=2) == -22 and b"mask is null" in err() and b"[20, 160]" in err()
    for lo in (0.0, -0.5, float("nan")):
        assert call(lo=lo) == -22 and b"min_depth" in err() and b"positive" in err(), lo
    for lo, hi in ((0.5, 0.5), (0.5, 0.25), (0.5, float("nan"))):
        assert call(lo=lo, hi=hi) == -22 and b"above min_depth" in err(), (lo, hi)
    for hi in (INF, 1000.5, 1e30):                       # the integer tables rely on the bound
        assert call(hi=hi) == -22 and b"at most 1000 m" in err() and b"micrometres" in err(), hi
    assert call(hi=1000.0, N=0) == 0
    for b_lo, b_hi in ((0.0, 0.5), (-1.0, 0.5), (0.5, 0.5), (0.5, 0.1), (float("nan"), 0.5), (0.1, float("nan")), (0.1, INF)):
        assert call(b_lo=b_lo, b_hi=b_hi) == -22 and b"0 < b_lo < b_hi" in err(), (b_lo, b_hi)
    for kw in ({"stats": odd}, {"tables": odd}, {"ws": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    need = L.pd_unc_stats_workspace(1, 8, 8, 1)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(ws_bytes=0) == -22 and b"workspace too small" in err()
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
    assert call(N=0) == 0 and call(N=0, K=16, classes=(ctypes.c_int * 32)(*([1, 0] * 16))) == 0
    assert call(N=0, ws=None) == -22                                               # its arguments are still checked


def test_workspace_is_monotone_never_zero_and_a_multiple_of_16():
    ws = _lib.lib.pd_unc_stats_workspace
    assert ws(0, 0, 0, 0) > 0 and ws(-1, -1, -1, -1) > 0
    shapes = [(1, 1, 4, 1), (2, 5, 7, 1), (3, 33, 70, 12), (4, 64, 96, 12), (12, 320, 480, 12), (16, 512, 640, 16)]
    sizes = [ws(*s) for s in shapes]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert ws(2, 37, 70, 12) == 2 * 3 * 12 * 4 * 8             # [N][G][K][3 sums, padded to 4] doubles, G = ceil(2590 / 1024)


def test_python_layer_refuses_cpu_tensors_and_bad_options():
    x = torch.ones(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        UE.uncertainty_stats(x, x, x, classes=[("all", None)])
