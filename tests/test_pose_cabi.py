"""The entry points of csrc/pose.hip and pd_view_synth_bwd_pose, host side (no GPU): exported symbols, SIGNATURES, the header,
and every refusal that is decided before the device is touched -- the pointers are dummies that are never dereferenced."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
N_ARGS = {"pd_view_synth_pose_rows": 2, "pd_view_synth_bwd_pose": 17, "pd_pose_matrix_fwd": 6, "pd_pose_matrix_bwd": 8,
          "pd_pose_head_fwd": 15, "pd_pose_head_bwd": 20}
P, ODD = ctypes.c_void_p(64), ctypes.c_void_p(68)        # aligned dummy / 4-byte aligned only


def test_symbols_and_signatures():
    src = open(HEADER).read()
    so = ctypes.CDLL(_lib.lib.path)
    for name, n in N_ARGS.items():
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src, name
        assert len(_lib.SIGNATURES[name][1]) == n, name


def test_pose_rows_is_a_pure_function_of_the_plane():
    rows = _lib.lib.pd_view_synth_pose_rows
    assert rows(0, 5) == 1 and rows(5, -1) == 1 and rows(3, 5) == 1 and rows(16, 16) == 1 and rows(16, 17) == 2
    assert rows(19, 37) == 3 and rows(260, 260) == 265 and rows(320, 480) == 512 and rows(512, 640) == 512
    assert rows(1 << 15, 1 << 15) == 512


def test_view_synth_bwd_pose_refusals_need_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def call(gw=P, src=P, coords=P, depth=P, K=P, iK=P, T=P, gdepth=P, ws=P, gP=P, gT=P, N=1, C=3, H=8, W=8, acc=0):
        return L.pd_view_synth_bwd_pose(gw, src, coords, depth, K, iK, T, gdepth, ws, gP, gT, N, C, H, W, acc, None)

    for kw in ({"depth": None}, {"src": None}, {"K": None}, {"iK": None}, {"T": None}, {"gw": None}, {"coords": None},
               {"ws": None}, {"gT": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"N": -1}, {"N": 65536}, {"C": 0}, {"H": 0}, {"W": -2}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
    for kw in ({"coords": ODD}, {"ws": ODD}, {"gP": ODD}):
        assert call(**kw) == -22 and b"8-byte aligned" in err(), kw
    assert call(N=0) == 0 and call(N=0, gdepth=None, gP=None) == 0       # an empty batch touches nothing; both are optional
    assert call(N=0, gT=None) == -22                                     # ... but its arguments are checked


def test_pose_matrix_refusals_need_no_gpu():
    L = _lib.lib
    err = L.pd_last_error
    for a in ((None, P, P), (P, None, P), (P, P, None)):
        assert L.pd_pose_matrix_fwd(*a, 1, 0, None) == -22 and b"must not be null" in err()
    for i in range(5):
        a = [P] * 5
        a[i] = None
        assert L.pd_pose_matrix_bwd(*a, 1, 0, None) == -22 and b"must not be null" in err()
    assert L.pd_pose_matrix_fwd(P, P, P, -1, 0, None) == -22 and b"item count" in err()
    assert L.pd_pose_matrix_bwd(P, P, P, P, P, -1, 0, None) == -22 and b"item count" in err()
    for inv in (2, -1):
        assert L.pd_pose_matrix_fwd(P, P, P, 1, inv, None) == -22 and b"invert" in err()
        assert L.pd_pose_matrix_bwd(P, P, P, P, P, 1, inv, None) == -22 and b"invert" in err()
    assert L.pd_pose_matrix_fwd(P, P, P, 0, 1, None) == 0 and L.pd_pose_matrix_bwd(P, P, P, P, P, 0, 0, None) == 0


def test_pose_head_refusals_need_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def fwd(x=P, w=P, b=P, aa=P, tr=P, T=P, Ti=P, mean=P, N=1, h=2, wd=3, Cin=256, Co=12, inv=0):
        return L.pd_pose_head_fwd(x, w, b, aa, tr, T, Ti, mean, N, h, wd, Cin, Co, inv, None)

    def bwd(gT=P, gTi=None, gaa=None, gtr=None, aa=P, tr=P, w=P, mean=P, gx=P, gw=P, gb=P, ws=P, N=1, h=2, wd=3, Cin=256,
            Co=12, inv=0, acc=0):
        return L.pd_pose_head_bwd(gT, gTi, gaa, gtr, aa, tr, w, mean, gx, gw, gb, ws, N, h, wd, Cin, Co, inv, acc, None)

    for call in (fwd, bwd):
        for kw in ({"N": -1}, {"N": 65536}, {"h": 0}, {"wd": -1}, {"h": 2048, "wd": 2048}):
            assert call(**kw) == -22 and b"bad shape" in err(), kw
        for cin in (0, 32, 100, 250, 1088, 2048):
            assert call(Cin=cin) == -22 and b"Cin must be a multiple of 64" in err(), cin
        for co in (0, 5, 7, 16, 390):
            assert call(Co=co) == -22 and b"Co must be a multiple of 6" in err(), co
        for inv in (2, -1):
            assert call(inv=inv) == -22 and b"invert" in err()
        assert call(mean=ODD) == -22 and b"8-byte aligned" in err()
        assert call(N=0) == 0
        for cin, co in ((64, 6), (1024, 384)):
            assert call(N=0, Cin=cin, Co=co) == 0
    for name in ("x", "w", "b", "aa", "tr", "T", "Ti", "mean"):
        assert fwd(**{name: None}) == -22 and b"must not be null" in err(), name
    for name in ("aa", "tr", "w", "mean", "gx", "gw", "gb", "ws"):
        assert bwd(**{name: None}) == -22 and b"must not be null" in err(), name
    assert bwd(ws=ODD) == -22 and b"8-byte aligned" in err()
    assert bwd(acc=2) == -22 and b"accumulate" in err()
    assert bwd(N=0, gT=None) == 0                                        # every cotangent is optional


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    a = torch.zeros(2, 1, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_matrix(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_head(torch.zeros(1, 256, 2, 3), torch.zeros(12, 256, 1, 1), torch.zeros(12))
