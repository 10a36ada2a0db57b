"""pd_unc_loss_rows / _fwd / _bwd, host side (no GPU): the exported symbols, the defines, SIGNATURES, every refusal decided
before the device is touched, N == 0, and the any-ratio form of pd_up_gather_bwd the backward pass relies on."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_ULOSS_SUMS"]) == 4
    so = ctypes.CDLL(_lib.lib.path)
    for name in ("pd_unc_loss_rows", "pd_unc_loss_fwd", "pd_unc_loss_bwd"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    assert len(_lib.SIGNATURES["pd_unc_loss_fwd"][1]) == 20 and len(_lib.SIGNATURES["pd_unc_loss_bwd"][1]) == 19
    assert ops.UNCERTAINTY_RANGE == (0.0005, 0.5)


def test_rows_are_monotone_and_never_zero():
    rows = _lib.lib.pd_unc_loss_rows
    assert rows(0, 0, 0) == 1 and rows(-1, 5, 5) == 1 and rows(1, 1, 1) == 1 and rows(2, 37, 70) == 21
    sizes = [rows(*s) for s in ((1, 8, 8), (2, 24, 40), (12, 320, 480), (16, 512, 640), (4096, 4096, 4096))]
    assert sizes == sorted(sizes) and sizes[-1] == 2048


def _fwd(**kw):
    p = ctypes.c_void_p(64)
    a = dict(depth=p, gt=p, ldg=8, unc=p, hs=4, ws=4, valid=None, lo=0.1, hi=2.0, b_lo=0.0005, b_hi=0.5, sums=p, value=p, maps=None,
             ws_=p, ws_bytes=1 << 40, N=1, H=8, W=8)
    a.update(kw)
    return _lib.lib.pd_unc_loss_fwd(a["depth"], a["gt"], a["ldg"], a["unc"], a["hs"], a["ws"], a["valid"], a["lo"], a["hi"], a["b_lo"],
                                    a["b_hi"], a["sums"], a["value"], a["maps"], a["ws_"], a["ws_bytes"], a["N"], a["H"], a["W"], None)


def _bwd(**kw):
    p = ctypes.c_void_p(64)
    a = dict(depth=p, gt=p, ldg=8, unc=p, hs=4, ws=4, valid=None, lo=0.1, hi=2.0, b_lo=0.0005, b_hi=0.5, gvalue=p, sums=p, gdepth=p,
             gup=p, N=1, H=8, W=8)
    a.update(kw)
    return _lib.lib.pd_unc_loss_bwd(a["depth"], a["gt"], a["ldg"], a["unc"], a["hs"], a["ws"], a["valid"], a["lo"], a["hi"], a["b_lo"],
                                    a["b_hi"], a["gvalue"], a["sums"], a["gdepth"], a["gup"], a["N"], a["H"], a["W"], None)


@pytest.mark.parametrize("call,who", [(_fwd, b"pd_unc_loss_fwd"), (_bwd, b"pd_unc_loss_bwd")])
def test_shared_refusals_need_no_gpu(call, who):
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    err = _lib.lib.pd_last_error
    for kw in ({"depth": None}, {"gt": None}, {"unc": None}):
        assert call(**kw) == -22 and b"must not be null" in err() and who in err(), kw
    for kw in ({"N": -1}, {"H": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for kw in ({"hs": 0}, {"ws": -1}, {"hs": 9}, {"ws": 9}):
        assert call(**kw) == -22 and b"uncertainty map" in err(), kw
    assert call(ldg=7) == -22 and b"row pitch" in err()
    for lo, hi in ((0.0, 2.0), (-1.0, 2.0), (2.0, 2.0), (2.0, 1.0), (float("nan"), 2.0), (0.1, float("nan"))):
        assert call(lo=lo, hi=hi) == -22 and b"depth range" in err(), (lo, hi)
    for b_lo, b_hi in ((0.0, 0.5), (-1.0, 0.5), (0.5, 0.5), (0.5, 0.1), (float("nan"), 0.5), (0.1, float("nan")), (0.1, float("inf"))):
        assert call(b_lo=b_lo, b_hi=b_hi) == -22 and b"0 < b_lo < b_hi" in err(), (b_lo, b_hi)
    assert call(H=1 << 15, W=(1 << 15) + 1, ldg=1 << 16, hs=1, ws=1) == -22 and b"too large" in err()
    assert call(N=0) == 0                                                   # an empty batch is fine and touches nothing
    assert call(N=0, unc=None) == -22                                       # but its arguments are still checked


def test_forward_refusals():
    err = _lib.lib.pd_last_error
    odd8, odd4 = ctypes.c_void_p(72), ctypes.c_void_p(68)
    for kw in ({"sums": None}, {"value": None}, {"ws_": None}):
        assert _fwd(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"ws_": odd8}, {"sums": odd4}, {"maps": odd4}, {"depth": ctypes.c_void_p(66)}):
        assert _fwd(**kw) == -22 and b"aligned" in err(), kw
    need = _lib.lib.pd_unc_loss_rows(1, 8, 8) * 4 * 8
    assert _fwd(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert _fwd(ws_bytes=0) == -22 and b"workspace too small" in err()
    assert _fwd(N=0, maps=ctypes.c_void_p(64), valid=ctypes.c_void_p(1)) == 0


def test_backward_refusals_and_the_detached_mode():
    err = _lib.lib.pd_last_error
    for kw in ({"gvalue": None}, {"sums": None}, {"gup": None}):
        assert _bwd(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"sums": ctypes.c_void_p(68)}, {"gup": ctypes.c_void_p(66)}, {"gdepth": ctypes.c_void_p(65)}):
        assert _bwd(**kw) == -22 and b"aligned" in err(), kw
    assert _bwd(N=0, gdepth=None) == 0                                      # no depth gradient: the detached mode


def test_up_gather_takes_any_ratio_only_in_its_generic_form():
    L, err, p = _lib.lib, _lib.lib.pd_last_error, ctypes.c_void_p(64)
    assert L.pd_up_gather_bwd(p, p, 0, 5, 33, 9, 65, 0, 1, None) == 0
    assert L.pd_up_gather_bwd(p, p, 0, 5, 33, 9, 65, 0, 0, None) == -22 and b"integer multiple" in err()
    assert L.pd_up_gather_bwd(p, p, 0, 12, 20, 24, 40, 0, 0, None) == 0
    assert L.pd_up_gather_bwd(p, p, 0, 10, 33, 9, 65, 0, 1, None) == -22   # a head larger than the frame


def test_python_layer_refuses_cpu_tensors_and_bad_options():
    d, g, u = torch.ones(1, 1, 4, 4), torch.ones(1, 1, 4, 4), torch.full((1, 1, 2, 2), 0.5)
    with pytest.raises(RuntimeError, match="CUDA|cuda"):
        ops.uncertainty_loss(d, g, u)
    for bad in ((0.0, 0.5), (0.5, 0.5), (0.5, 0.1), (0.1, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="b_lo < b_hi"):
            ops.uncertainty_range(bad)
    assert ops.uncertainty_range(None) == ops.UNCERTAINTY_RANGE and ops.uncertainty_range(("0.001", 1)) == (0.001, 1.0)
