"""pd_xolp_stats and the configurable XOLP norm, host side (no GPU): the exported symbols, every refusal decided before the
device is touched, the workspace query, ShallowEncoder(xolp_norm=), the PD_XOLP_NORM string, and the facade module."""
import ctypes
import math
import re
import os

import pytest
import torch

from conftest import ROOT

from polardepth import _lib
from polardepth import polar as pdpolar

HEADER = os.path.join(ROOT, "include", "polardepth.h")
THR = (ctypes.c_float * 2)(0.38, 1.0)


def test_symbols_and_header():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_XOLP_STATS_BYTES"]) == pdpolar.STATS_BYTES == 80 + 8 * (257 + 256)
    so = ctypes.CDLL(_lib.lib.path)
    for name in ("pd_xolp_stats", "pd_xolp_stats_workspace"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    assert len(_lib.SIGNATURES["pd_xolp_stats"][1]) == 12
    assert pdpolar.HIST_DOLP_BINS == 257 and pdpolar.HIST_AOLP_BINS == 256


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only

    def call(xolp=p, mask=None, stats=p, ws=p, ws_bytes=1 << 30, B=1, H=8, W=8, ld=8, thr=THR, acc=0):
        return L.pd_xolp_stats(xolp, mask, stats, ws, ws_bytes, B, H, W, ld, thr, acc, None)

    for kw in ({"xolp": None}, {"stats": None}, {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    assert call(B=0, stats=None) == -22 and b"must not be null" in err()      # the empty batch still writes the record
    need = L.pd_xolp_stats_workspace(1, 8, 8)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(ws_bytes=0) == -22 and b"workspace too small" in err()
    assert call(W=9, ld=8) == -22 and b"exceeds the row pitch" in err()
    for ld in (10, 9, 11):
        assert call(W=8, ld=ld) == -22 and b"multiple of 4" in err(), ld
    for kw in ({"xolp": odd}, {"mask": odd}, {"stats": odd}, {"ws": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    for bad in ((math.nan, 1.0), (0.38, math.inf), (-math.inf, 1.0)):
        assert call(thr=(ctypes.c_float * 2)(*bad)) == -22 and b"finite" in err(), bad
    assert call(thr=None) == -22 and b"finite" in err()
    for kw in ({"B": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}, {"ld": 0}, {"ld": -8}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    # 32-bit element offsets inside the kernel: a batch is split by frames on the host, one frame beyond 2^30 elements is refused
    assert call(H=1 << 15, W=1 << 15, ld=1 << 15) == -22 and b"too large" in err()
    assert call(H=1 << 16, W=4, ld=1 << 14) == -22 and b"too large" in err()


def test_workspace_is_monotone_and_never_zero():
    ws = _lib.lib.pd_xolp_stats_workspace
    assert ws(0, 0, 0) > 0 and ws(0, 512, 640) > 0 and ws(-1, -1, -1) > 0
    shapes = [(1, 1, 4), (2, 5, 10), (3, 64, 96), (2, 256, 612), (16, 512, 640), (64, 512, 640), (4096, 4096, 4096),
              (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]
    sizes = [ws(*s) for s in shapes]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[0] < sizes[3] < sizes[4]
    for B, H, W in shapes[:6]:
        assert ws(B + 1, H, W) >= ws(B, H, W) and ws(B, H + 1, W) >= ws(B, H, W) and ws(B, H, W + 1) >= ws(B, H, W)
    assert sizes[-1] == sizes[-2]        # the grid is capped: the workspace stops growing (and nothing overflows)


def test_python_layer_refusals():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdpolar.xolp_stats(torch.zeros(1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdpolar.XolpStats("cpu")


def test_encoder_takes_the_pair():
    from manydepth import networks
    from manydepth.networks import pre_encoders as pe
    torch.manual_seed(0)
    default = networks.ShallowEncoder('XOLP', 2, 0.0)
    assert default.Conv1.in_affine == (pe.XOLP_MEAN, pe.XOLP_STD) == (0.08693199701957657, 0.44430732785457433)
    own = networks.ShallowEncoder('XOLP', 2, 0.0, xolp_norm=(0.21, 0.17))
    assert own.Conv1.in_affine == (0.21, 0.17)
    assert networks.ShallowEncoder('XOLP', xolp_norm="0.21,0.17").Conv1.in_affine == (0.21, 0.17)
    assert list(own.state_dict()) == list(default.state_dict())                  # no new key: reference checkpoints keep loading
    assert not any("norm" in k or "affine" in k for k in own.state_dict())
    own.load_state_dict(default.state_dict())
    assert own.Conv1.in_affine == (0.21, 0.17)
    # the static method keeps its signature and the HAMMER constants
    x = torch.tensor([0.5])
    assert torch.equal(own.normalizeInput(x, 'XOLP'), (x - pe.XOLP_MEAN) / pe.XOLP_STD)
    assert networks.ShallowEncoder('RGB', 3, 0.0).Conv1.in_affine == (0.45, 0.225)
    assert networks.ShallowNormalsEncoder(9, 0.0).Conv1.in_affine is None
    for bad in ((0.1, 0.0), (0.1, -1.0), (math.nan, 1.0), (0.1, math.inf), (math.inf, 1.0), (0.1, math.nan), (0.1,), (1, 2, 3),
                "0.1", "a,b"):
        with pytest.raises(ValueError, match="xolp_norm"):
            networks.ShallowEncoder('XOLP', 2, 0.0, xolp_norm=bad)
    for mode, ch in (('RGB', 3), ('normals', 9)):
        with pytest.raises(ValueError, match="XOLP input only"):
            networks.ShallowEncoder(mode, ch, 0.0, xolp_norm=(0.21, 0.17))


def test_norm_string_parses():
    parse = pdpolar.parse_xolp_norm
    assert parse(None) is None and parse("") is None and parse("  ") is None
    assert parse("0.21,0.17") == (0.21, 0.17) and parse(" 0.21 , 1e-3 ") == (0.21, 0.001)
    assert parse((0.21, 0.17)) == (0.21, 0.17) and parse([-1, 2]) == (-1.0, 2.0)
    for bad in ("0.21", "0.21,0.17,3", "0.21;0.17", "mean,std", "0.21,0", "0.21,-0.17", "nan,1", "0.1,inf", 0.3, (0.1, None)):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            parse(bad)
    # the string the tool prints reads back to the same two doubles
    pair = (0.08693199701957657, 0.44430732785457433)
    assert parse(pdpolar.format_xolp_norm(pair)) == pair
    assert parse(pdpolar.format_xolp_norm((1 / 3, 2 / 7))) == (1 / 3, 2 / 7)


def test_train_entry_point_maps_the_environment():
    """manydepth/train.py hands PD_XOLP_NORM to opt.xolp_norm as it does PD_POL_ANGLES, and the Trainer's parser reads it."""
    import types
    from manydepth.train import options_from_environment
    opts = options_from_environment(types.SimpleNamespace(), {"PD_XOLP_NORM": "0.21,0.17", "PD_POL_ANGLES": "1,46,91,136"})
    assert opts.xolp_norm == "0.21,0.17" and pdpolar.parse_xolp_norm(opts.xolp_norm) == (0.21, 0.17)
    assert opts.pol_angles == [1.0, 46.0, 91.0, 136.0]
    for env in ({}, {"PD_XOLP_NORM": ""}):
        assert not hasattr(options_from_environment(types.SimpleNamespace(), env), "xolp_norm")


def test_facade_module_imports():
    from polarisation import xolp_mean_and_std_dev as m
    assert callable(m.stats_of_folders) and callable(m.main) and callable(m.report)
    import io
    buf = io.StringIO()
    m.report({"dolp_mean": 1.0, "dolp_std": 2.0, "aolp_mean": 3.0, "aolp_std": 4.0, "xolp_mean": 2.0, "xolp_std": 3.0}, buf)
    lines = buf.getvalue().splitlines()
    assert [l.split(":")[0] for l in lines] == ["DOLP MEAN", "DOLP STD", "AOLP MEAN", "AOLP STD", "XOLP MEAN", "XOLP STD"]
