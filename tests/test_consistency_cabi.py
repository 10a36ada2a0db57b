"""pd_depth_consistency, host side (no GPU): the exported symbols, the defines, SIGNATURES, every refusal decided before the
device is touched, and the workspace query."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib
from polardepth import consistency_eval as CE

HEADER = os.path.join(ROOT, "include", "polardepth.h")
ALL = (ctypes.c_int * 2)(1, 0)                       # one class: every pixel
RANGED = (ctypes.c_int * 4)(1, 0, 20, 160)
INF = float("inf")
NAN = float("nan")


def _d3(*v):
    return (ctypes.c_double * 3)(*v)


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_CONS_BINS"]) == CE.BINS == 256
    assert int(defs["PD_CONS_COUNTERS"]) == len(CE.COUNTER_NAMES) == 8 and int(defs["PD_CONS_SUMS"]) == 4
    assert int(defs["PD_CONS_RECORD_BYTES"]) == CE.RECORD_BYTES == 112 + 4 * 256
    assert int(defs["PD_REPROJ_MAX_FRAMES"]) == CE.MAX_FRAMES and int(defs["PD_DSTAT_MAX_CLASSES"]) == CE.MAX_CLASSES
    so = ctypes.CDLL(_lib.lib.path)
    for name in ("pd_depth_consistency", "pd_depth_consistency_workspace"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    assert len(_lib.SIGNATURES["pd_depth_consistency"][1]) == 26
    assert _lib.SIGNATURES["pd_depth_consistency_workspace"][0] is ctypes.c_size_t


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only
    TPX, TREL = _d3(4, 2, 1), _d3(0.04, 0.02, 0.01)

    def call(depth0=p, depths=p, T=p, K=p, inv_K=p, fv=None, visible=None, mask=None, classes=ALL, nk=1, lo=0.1, hi=2.0,
             tau_px=TPX, tau_rel=TREL, fuse=4, level=None, n_cons=None, fused=None, stats=p, ws=p, ws_bytes=1 << 40, N=1, F=2,
             H=8, W=8):
        return L.pd_depth_consistency(depth0, depths, T, K, inv_K, fv, visible, mask, classes, nk, lo, hi, tau_px, tau_rel, fuse,
                                      level, n_cons, fused, stats, ws, ws_bytes, N, F, H, W, None)

    for kw in ({"depth0": None}, {"depths": None}, {"T": None}, {"K": None}, {"inv_K": None}, {"classes": None},
               {"tau_px": None}, {"tau_rel": None}, {"stats": None}, {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for F in (0, -1, 9, 1 << 20):
        assert call(F=F) == -22 and b"source views" in err(), F
    for nk in (0, -1, 17, 1 << 20):
        assert call(nk=nk) == -22 and b"classes" in err(), nk
    assert call(classes=RANGED, nk=2) == -22 and b"mask is null" in err() and b"[20, 160]" in err()
    assert call(classes=(ctypes.c_int * 2)(0, 0)) == -22 and b"mask is null" in err()      # lo == hi is a range too
    for lo in (0.0, -0.5, NAN):
        assert call(lo=lo) == -22 and b"min_depth" in err() and b"positive" in err(), lo
    for lo, hi in ((0.5, 0.5), (0.5, 0.25), (0.5, NAN), (INF, INF)):
        assert call(lo=lo, hi=hi) == -22 and b"above min_depth" in err(), (lo, hi)
    for bad in (_d3(4, 2, 0), _d3(4, 2, -1), _d3(NAN, 2, 1), _d3(INF, 2, 1)):
        assert call(tau_px=bad) == -22 and b"positive and finite" in err(), list(bad)
        assert call(tau_rel=bad) == -22 and b"positive and finite" in err(), list(bad)
    for bad in (_d3(1, 2, 4), _d3(4, 1, 2), _d3(2, 4, 1)):
        assert call(tau_px=bad) == -22 and b"nested" in err(), list(bad)
        assert call(tau_rel=bad) == -22 and b"nested" in err(), list(bad)
    assert call(tau_px=_d3(2, 2, 2), tau_rel=_d3(0.5, 0.5, 0.5), N=0) == 0               # equal thresholds are nested
    for fuse in (1, 0, 5, -4):
        assert call(fuse=fuse) == -22 and b"fuse_level" in err(), fuse
    for kw in ({"stats": odd}, {"ws": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    need = L.pd_depth_consistency_workspace(1, 8, 8, 1)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(ws_bytes=0) == -22 and b"workspace too small" in err()
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()      # offsets inside a frame are 32-bit
    # an empty batch is fine and touches nothing; max_depth = +inf is allowed; every output may be asked for
    assert call(N=0) == 0 and call(N=0, hi=INF) == 0 and call(N=0, level=p, n_cons=p, fused=p, fv=p, visible=p) == 0
    assert call(N=0, F=1) == 0 and call(N=0, F=8) == 0 and call(N=0, fuse=2) == 0 and call(N=0, fuse=3) == 0
    assert call(N=0, ws=None) == -22                                               # but its arguments are still checked


def test_workspace_is_monotone_never_zero_and_a_multiple_of_16():
    ws = _lib.lib.pd_depth_consistency_workspace
    assert ws(0, 0, 0, 0) > 0 and ws(0, 512, 640, 12) > 0 and ws(-1, -1, -1, -1) > 0
    shapes = [(1, 1, 4, 1), (2, 5, 7, 1), (3, 33, 70, 12), (4, 64, 96, 12), (12, 320, 480, 12), (16, 512, 640, 16),
              (4096, 4096, 4096, 16), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]
    sizes = [ws(*s) for s in shapes]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[4] < sizes[5]
    assert ws(3, 37, 53, 12) == 3 * 2 * 12 * 4 * 8             # [N][G][K][4] doubles, G = ceil(37 * 53 / 1024)
    assert ws(1, 264, 256, 1) == 64 * 4 * 8                     # 66 workgroups' worth of pixels: the cap of 64


def test_python_layer_refuses_cpu_tensors_and_bad_options():
    d0, ds = torch.ones(1, 1, 4, 4), torch.ones(1, 2, 4, 4)
    T, K = torch.eye(4).expand(1, 2, 4, 4), torch.eye(4).expand(1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.consistency(d0, ds, T, K, K, classes=[("all", None)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CE.visibility(d0, ds, T, K, K)
    with pytest.raises(ValueError, match="want"):
        CE.consistency(d0, ds, T, K, K, want=("levels",))
    assert len(CE.METRIC_NAMES) == 14 and CE.DEFAULT_TAUS[2] == (1.0, 0.01)
