"""The entry points of csrc/reproj.hip, host side (no GPU): exported symbols, the define, SIGNATURES, and every refusal that is
decided before the device is touched -- the pointers are dummies that are never dereferenced on these paths."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
NAMES = ("pd_view_synth_fwd", "pd_view_synth_bwd", "pd_depth_to_updisp_bwd", "pd_reproj_combine_rows", "pd_reproj_combine_fwd",
         "pd_reproj_combine_bwd")
P, ODD = ctypes.c_void_p(64), ctypes.c_void_p(68)        # aligned dummy / 4-byte aligned only


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_symbols_define_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_REPROJ_MAX_FRAMES"]) == ops.REPROJ_MAX_FRAMES == 8
    so = ctypes.CDLL(_lib.lib.path)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    n_args = {"pd_view_synth_fwd": 12, "pd_view_synth_bwd": 14, "pd_depth_to_updisp_bwd": 7, "pd_reproj_combine_rows": 3,
              "pd_reproj_combine_fwd": 14, "pd_reproj_combine_bwd": 11}
    for name, n in n_args.items():
        assert len(_lib.SIGNATURES[name][1]) == n, name


def test_view_synthesis_argument_validation_needs_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def fwd(depth=P, src=P, K=P, iK=P, T=P, warped=P, coords=P, N=1, C=3, H=8, W=8):
        return L.pd_view_synth_fwd(depth, src, K, iK, T, warped, coords, N, C, H, W, None)

    def bwd(gw=P, src=P, coords=P, depth=P, K=P, iK=P, T=P, gdepth=P, N=1, C=3, H=8, W=8, acc=0):
        return L.pd_view_synth_bwd(gw, src, coords, depth, K, iK, T, gdepth, N, C, H, W, acc, None)

    for call in (fwd, bwd):
        for kw in ({"depth": None}, {"src": None}, {"K": None}, {"iK": None}, {"T": None}):
            assert call(**kw) == -22 and b"must not be null" in err(), kw
        for kw in ({"N": -1}, {"N": 65536}, {"C": 0}, {"H": 0}, {"W": -2}):
            assert call(**kw) == -22 and b"bad shape" in err(), kw
        assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
        assert call(coords=ODD) == -22 and b"8-byte aligned" in err()
        assert call(N=0) == 0                                                        # an empty batch touches nothing
        assert call(N=0, src=None) == -22                                            # ... but its arguments are checked
    for kw in ({"warped": None}, {"coords": None}):
        assert fwd(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"gw": None}, {"coords": None}, {"gdepth": None}):
        assert bwd(**kw) == -22 and b"must not be null" in err(), kw

    def d2u(g=P, d=P, out=P, n=16, lo=0.1, hi=2.0):
        return L.pd_depth_to_updisp_bwd(g, d, out, n, lo, hi, None)
    for kw in ({"g": None}, {"d": None}, {"out": None}):
        assert d2u(**kw) == -22 and b"must not be null" in err(), kw
    assert d2u(n=-1) == -22 and b"element count" in err()
    for lo, hi in ((0.0, 2.0), (-1.0, 2.0), (1.0, 1.0), (1.0, 0.5), (float("nan"), 2.0)):
        assert d2u(lo=lo, hi=hi) == -22 and b"depth range" in err(), (lo, hi)
    assert d2u(n=0) == 0


def test_combine_argument_validation_needs_no_gpu():
    L = _lib.lib
    err = L.pd_last_error
    two, nul = _ptrs(64, 128), _ptrs(64, None)

    def fwd(reproj=two, identity=None, F=2, noise=None, valid=None, sel=P, part=P, sums=P, loss=P, N=1, H=8, W=8, avg=0):
        return L.pd_reproj_combine_fwd(reproj, identity, F, noise, valid, sel, part, sums, loss, N, H, W, avg, None)

    def bwd(gloss=P, sel=P, sums=P, valid=None, greproj=two, F=2, N=1, H=8, W=8, avg=0):
        return L.pd_reproj_combine_bwd(gloss, sel, sums, valid, greproj, F, N, H, W, avg, None)

    for call in (fwd, bwd):
        for F in (0, -1, 9):
            assert call(F=F) == -22 and b"frames" in err(), F
        for kw in ({"N": -1}, {"H": 0}, {"W": -3}):
            assert call(**kw) == -22 and b"bad shape" in err(), kw
        assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
        for avg in (2, -1):
            assert call(avg=avg) == -22 and b"avg" in err()
        assert call(sums=ODD) == -22 and b"8-byte aligned" in err()
    for kw in ({"reproj": None}, {"sel": None}, {"part": None}, {"sums": None}, {"loss": None}):
        assert fwd(**kw) == -22 and b"must not be null" in err(), kw
    assert fwd(noise=P) == -22 and b"noise" in err()                                 # noise without identity maps
    assert fwd(part=ODD) == -22 and b"8-byte aligned" in err()
    assert fwd(reproj=nul) == -22 and b"map 1 is null" in err()
    assert fwd(identity=nul) == -22 and b"map 1 is null" in err()
    for kw in ({"gloss": None}, {"sel": None}, {"sums": None}, {"greproj": None}):
        assert bwd(**kw) == -22 and b"must not be null" in err(), kw
    assert bwd(greproj=nul) == -22 and b"map 1 is null" in err()
    assert bwd(N=0) == 0
    rows = L.pd_reproj_combine_rows
    assert rows(0, 0, 0) == 1 and rows(-1, 8, 8) == 1 and rows(1, 16, 16) == 1 and rows(1, 16, 17) == 2
    assert rows(16, 512, 640) == 2048 and rows(12, 320, 480) == 2048 and rows(2, 19, 37) == 6


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    d, s, m = torch.ones(1, 1, 4, 4), torch.ones(1, 3, 4, 4), torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_synthesis(d, s, m, m, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reproj_combine([d, d])
    with pytest.raises(ValueError, match="frames"):
        ops.reproj_combine([])
    with pytest.raises(ValueError, match="frames"):
        ops.reproj_combine([d] * 9)
    with pytest.raises(ValueError, match="identity"):
        ops.reproj_combine([d, d], identity=[d])
    with pytest.raises(ValueError, match="noise"):
        ops.reproj_combine([d, d], noise=d)
