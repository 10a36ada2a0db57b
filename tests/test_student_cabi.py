"""The entry points of csrc/student.hip, host side (no GPU): exported symbols, the defines, SIGNATURES, the header's
definitions, and every refusal that is decided before the device is touched -- the pointers are dummies that are never
dereferenced on these paths."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
N_ARGS = {"pd_student_masks_rows": 3, "pd_student_masks": 16, "pd_depth_bins_update": 8, "pd_student_combine_rows": 3,
          "pd_student_combine_fwd": 15, "pd_student_combine_bwd": 14}
P, ODD = ctypes.c_void_p(64), ctypes.c_void_p(68)        # 16-byte aligned dummy / 4-byte aligned only
ODD2 = ctypes.c_void_p(66)                               # 2-byte aligned only


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_BINS_LINEAR"]) == ops.BINS_LINEAR == 0 and int(defs["PD_BINS_INVERSE"]) == ops.BINS_INVERSE == 1
    so = ctypes.CDLL(_lib.lib.path)
    for name, n in N_ARGS.items():
        assert name in _lib.SIGNATURES and hasattr(so, name), name
        assert len(_lib.SIGNATURES[name][1]) == n, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, src)
        assert decl and decl.group(1).count(",") + 1 == n, name


def test_header_states_the_definitions():
    src = " ".join(open(HEADER).read().split())
    for phrase in ("(y >> 2, x >> 2)", "that scale is exactly 0.25", "mm = ((md - t) / t < 1) && ((t - md) / md < 1)",
                   "rmask = (!motion_masking || cmask) && !(aug && aug[n] != 0)", "both NaN if the item holds a NaN",
                   "lo > floor_depth ? lo : floor_depth", "tracker[1] * 0.99 + mx64 * 0.01", "y[D-1] = stop",
                   "sum(m * r), sum(r), sum(|multi - mono| * (1 - r))", "sums[2] / (N * H * W)",
                   "sign(0) = 0 and sign(NaN) = 0", "torch.sign returns 0 for a NaN", "No gradient reaches mono_depth"):
        assert phrase in src, phrase


def test_masks_argument_validation_needs_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def masks(lowest=P, conf=P, mono=P, aug=None, mm=1, rmask=P, cmask=P, up=P, minmax=P, ws=P, N=1, h=2, w=3, H=None, W=None):
        return L.pd_student_masks(lowest, conf, mono, aug, mm, rmask, cmask, up, minmax, ws, N, h, w,
                                  4 * h if H is None else H, 4 * w if W is None else W, None)

    for kw in ({"lowest": None}, {"conf": None}, {"mono": None}, {"rmask": None}, {"minmax": None}, {"ws": None}):
        assert masks(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"N": -1}, {"N": 65536}, {"h": 0}, {"w": -1}):
        assert masks(**kw) == -22 and b"bad shape" in err(), kw
    assert masks(h=1 << 13, w=(1 << 13) + 1) == -22 and b"too large" in err()
    for kw in ({"H": 7}, {"H": 9}, {"W": 11}, {"W": 3}, {"H": 2, "W": 3}):
        assert masks(**kw) == -22 and b"H = 4h and W = 4w" in err(), kw
    for mm in (2, -1):
        assert masks(mm=mm) == -22 and b"motion_masking" in err()
    for kw in ({"mono": ODD}, {"cmask": ODD}, {"up": ODD}, {"rmask": ODD2}):
        assert masks(**kw) == -22 and b"aligned" in err(), kw
    assert masks(N=0) == 0                                   # an empty batch touches nothing
    assert masks(N=0, cmask=None, up=None, aug=P) == 0       # the optional maps
    assert masks(N=0, mono=None) == -22                      # ... but its arguments are checked
    rows = L.pd_student_masks_rows
    assert rows(0, 2, 3) == 1 and rows(1, 2, 3) == 1 and rows(3, 9, 13) == 2 and rows(2, 8, 16) == 2
    assert rows(12, 80, 120) == 150 and rows(16, 128, 160) == 256 and rows(5000, 8, 8) == 1


def test_bins_update_argument_validation_needs_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def upd(minmax=P, N=2, tracker=P, floor=0.1, D=96, binning=0, bins=P):
        return L.pd_depth_bins_update(minmax, N, tracker, floor, D, binning, bins, None)

    for kw in ({"minmax": None}, {"tracker": None}, {"bins": None}):
        assert upd(**kw) == -22 and b"must not be null" in err(), kw
    for n in (0, -1, 65536):
        assert upd(N=n) == -22 and b"items" in err(), n
    for d in (0, -1, 129):
        assert upd(D=d) == -22 and b"depth bins" in err(), d
    for b in (2, -1):
        assert upd(binning=b) == -22 and b"binning" in err(), b
    assert upd(tracker=ODD) == -22 and b"8-byte aligned" in err()


def test_combine_argument_validation_needs_no_gpu():
    L = _lib.lib
    err = L.pd_last_error
    two, nul, odd = _ptrs(64, 128), _ptrs(64, None), _ptrs(64, 68)

    def fwd(reproj=two, F=2, valid=None, rmask=P, multi=P, mono=P, sel=P, part=P, sums=P, loss=P, N=1, H=8, W=12, avg=0):
        return L.pd_student_combine_fwd(reproj, F, valid, rmask, multi, mono, sel, part, sums, loss, N, H, W, avg, None)

    def bwd(gloss=P, sel=P, sums=P, valid=None, multi=P, mono=P, greproj=two, gmulti=P, F=2, N=1, H=8, W=12, avg=0):
        return L.pd_student_combine_bwd(gloss, sel, sums, valid, multi, mono, greproj, gmulti, F, N, H, W, avg, None)

    for call in (fwd, bwd):
        for F in (0, -1, 9):
            assert call(F=F) == -22 and b"frames" in err(), F
        for kw in ({"N": -1}, {"H": 0}, {"W": -4}):
            assert call(**kw) == -22 and b"bad shape" in err(), kw
        for kw in ({"H": 6}, {"W": 13}, {"H": 9, "W": 12}):
            assert call(**kw) == -22 and b"multiples of 4" in err(), kw
        assert call(H=1 << 15, W=(1 << 15) + 4) == -22 and b"too large" in err()
        for avg in (2, -1):
            assert call(avg=avg) == -22 and b"avg" in err()
        assert call(sums=ODD) == -22 and b"8-byte aligned" in err()
        for kw in ({"multi": None}, {"mono": None}, {"sel": None}, {"sums": None}):
            assert call(**kw) == -22 and b"must not be null" in err(), kw
        for kw in ({"multi": ODD}, {"mono": ODD}, {"sel": ODD2}):
            assert call(**kw) == -22 and b"aligned" in err(), kw
        assert call(N=0) == 0
        assert call(N=0, mono=None) == -22
    for kw in ({"reproj": None}, {"rmask": None}, {"part": None}, {"loss": None}):
        assert fwd(**kw) == -22 and b"must not be null" in err(), kw
    assert fwd(part=ODD) == -22 and b"8-byte aligned" in err()
    assert fwd(rmask=ODD2) == -22 and b"aligned" in err()
    assert fwd(reproj=nul) == -22 and b"map 1 is null" in err()
    assert fwd(reproj=odd) == -22 and b"map 1 is null or not 16-byte aligned" in err()
    for kw in ({"gloss": None}, {"greproj": None}, {"gmulti": None}):
        assert bwd(**kw) == -22 and b"must not be null" in err(), kw
    assert bwd(gmulti=ODD) == -22 and b"aligned" in err()
    assert bwd(greproj=nul) == -22 and b"map 1 is null" in err()
    rows = L.pd_student_combine_rows
    assert rows(0, 0, 0) == 1 and rows(-1, 8, 8) == 1 and rows(1, 32, 32) == 1 and rows(1, 32, 36) == 2
    assert rows(16, 512, 640) == 2048 and rows(3, 36, 52) == 6


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    d, low = torch.ones(1, 1, 8, 8), torch.ones(1, 2, 2)
    rm = torch.ones(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.student_masks(low, low, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.student_combine([d, d], rm, d, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_bins_update(torch.ones(1, 2), torch.ones(2, dtype=torch.float64), 0.1, torch.ones(4))
    with pytest.raises(ValueError, match="frames"):
        ops.student_combine([], rm, d, d)
    with pytest.raises(ValueError, match="frames"):
        ops.student_combine([d] * 9, rm, d, d)
