"""pd_polar_loss_rows / _fwd / _bwd, host side (no GPU): the exported symbols, the defines, SIGNATURES, every refusal decided
before the device is touched, and the row count."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import polar_loss_ref as R
from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
INF = float("inf")
NAN = float("nan")


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_PLOSS_SUMS"]) == 4 and int(defs["PD_PLOSS_COUNTERS"]) == len(ops.POLAR_LOSS_COUNTERS) == len(R.COUNTERS) == 7
    assert ops.POLAR_LOSS_COUNTERS == R.COUNTERS
    assert int(defs["PD_PLOSS_RECORD_BYTES"]) == ops.POLAR_LOSS_RECORD_BYTES == 8 * (4 + 7 + 1)
    assert int(defs["PD_PLOSS_STATE_WINNER"]) == ops.POLAR_STATE_WINNER == R.WINNER == 7
    assert int(defs["PD_PLOSS_STATE_NEGATED"]) == ops.POLAR_STATE_NEGATED == R.NEGATED == 8
    assert int(defs["PD_PLOSS_STATE_BRANCH_SHIFT"]) == ops.POLAR_STATE_BRANCH_SHIFT == R.BRANCH_SHIFT == 4
    assert int(defs["PD_PLOSS_STATE_BRANCH"]) == 3 << R.BRANCH_SHIFT
    assert int(defs["PD_PLOSS_STATE_GATE_SHIFT"]) == ops.POLAR_STATE_GATE_SHIFT == R.GATE_SHIFT == 6
    assert int(defs["PD_PLOSS_BWD_TILES_PER_TRIP"]) == 4096
    so = ctypes.CDLL(_lib.lib.path)
    for name, nargs in (("pd_polar_loss_rows", 3), ("pd_polar_loss_fwd", 21), ("pd_polar_loss_bwd", 15)):
        assert name in _lib.SIGNATURES and hasattr(so, name)
        decl = re.search(r"int\s+%s\(([^;]*)\);" % name, src)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["pd_polar_loss_fwd"][1][8] is ctypes.c_double                 # tilt2_min
    assert _lib.SIGNATURES["pd_polar_loss_fwd"][1][16] is ctypes.c_size_t                # ws_bytes


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only
    odd4 = ctypes.c_void_p(68)   # 4-byte aligned only

    def fwd(depth=p, K=p, pol=p, xolp=p, ldp=8, valid=None, rho_min=0.05, rho_max=1.0, tilt2=0.0076, sign=1, weighted=1, state=p,
            sums=p, values=p, maps=None, ws=p, ws_bytes=1 << 40, N=1, H=8, W=8):
        return L.pd_polar_loss_fwd(depth, K, pol, xolp, ldp, valid, rho_min, rho_max, tilt2, sign, weighted, state, sums, values,
                                   maps, ws, ws_bytes, N, H, W, None)

    def bwd(depth=p, K=p, pol=p, xolp=p, ldp=8, state=p, g=p, sums=p, sign=1, weighted=1, gdepth=p, N=1, H=8, W=8):
        return L.pd_polar_loss_bwd(depth, K, pol, xolp, ldp, state, g, sums, sign, weighted, gdepth, N, H, W, None)

    for call in (fwd, bwd):
        for kw in ({"depth": None}, {"K": None}, {"pol": None}, {"xolp": None}, {"state": None}, {"sums": None}):
            assert call(**kw) == -22 and b"must not be null" in err(), (call.__name__, kw)
        for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
            assert call(**kw) == -22 and b"bad shape" in err(), kw
        for ldp in (7, 0, -8):
            assert call(ldp=ldp) == -22 and b"row pitch" in err(), ldp
        for sign in (0, 2, -2, 1 << 20):
            assert call(sign=sign) == -22 and b"aolp_sign" in err(), sign
        for w in (2, -1):
            assert call(weighted=w) == -22 and b"dolp_weighted" in err(), w
        assert call(pol=odd) == -22 and b"16-byte aligned" in err()
        assert call(sums=odd4) == -22 and b"8-byte aligned" in err()
        assert call(H=1 << 15, W=(1 << 15) + 1, ldp=1 << 16) == -22 and b"too large" in err()
        assert call(N=0) == 0 and call(N=0, sign=-1, weighted=0, ldp=1 << 20) == 0      # an empty batch touches nothing
        assert call(N=0, pol=None) == -22                                               # but its arguments are still checked
    for kw in ({"values": None}, {"ws": None}):
        assert fwd(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"g": None}, {"gdepth": None}):
        assert bwd(**kw) == -22 and b"must not be null" in err(), kw
    for lo, hi in ((NAN, 1.0), (0.05, NAN), (-INF, 1.0), (0.05, INF), (0.5, 0.25)):
        assert fwd(rho_min=lo, rho_max=hi) == -22 and b"finite and not inverted" in err(), (lo, hi)
    for t in (-0.1, 1.0, 1.5, NAN, INF):
        assert fwd(tilt2=t) == -22 and b"tilt2_min" in err(), t
    assert fwd(ws=odd) == -22 and b"16-byte aligned" in err()
    assert fwd(maps=odd4) == -22 and b"8-byte aligned" in err()
    need = L.pd_polar_loss_rows(1, 8, 8) * 11 * 8
    assert fwd(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert fwd(ws_bytes=0) == -22 and b"workspace too small" in err()
    assert fwd(N=0, ws_bytes=need) == 0 and fwd(N=0, maps=p, valid=p, tilt2=0.0, rho_min=0.3, rho_max=0.3) == 0
    assert bwd(N=1 << 20, H=1 << 15, W=1 << 15, ldp=1 << 15) == -22 and b"too many tiles" in err()


def test_rows_are_monotone_and_never_zero():
    rows = _lib.lib.pd_polar_loss_rows
    assert rows(0, 0, 0) == 1 and rows(-1, -1, -1) == 1 and rows(0, 512, 640) == 1 and rows(1, 1, 1) == 1
    shapes = [(1, 1, 4), (2, 5, 7), (3, 33, 70), (4, 64, 96), (12, 320, 480), (16, 512, 640), (4096, 4096, 4096)]
    got = [rows(*s) for s in shapes]
    assert got == sorted(got) and got[0] == 1 and got[2] == -(-3 * 33 * 70 // 256) and got[-1] == 2048 and all(r > 0 for r in got)


def test_python_layer_refuses_cpu_tensors_and_bad_options():
    depth, K, pol, xolp = torch.ones(1, 1, 4, 4), torch.eye(4)[None], torch.ones(1, 9, 4, 4), torch.ones(1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.polar_loss(depth, K, pol, xolp)


def test_trainer_option_and_environment_mapping():
    import types
    from manydepth.train import options_from_environment
    from manydepth.trainer import _polar_loss_option
    env = {"PD_POLAR_LOSS": "0.5,0.25", "PD_POLAR_LOSS_WHERE": "holes", "PD_POL_AOLP_SIGN": "-1"}
    opts = options_from_environment(types.SimpleNamespace(), env)
    assert opts.polar_loss == [0.5, 0.25] and opts.polar_loss_where == "holes" and opts.pol_aolp_sign == -1
    assert _polar_loss_option(opts) == ([0.5, 0.25], "holes", -1)
    for name in ("polar_loss", "polar_loss_where", "pol_aolp_sign"):
        assert not hasattr(options_from_environment(types.SimpleNamespace(), {}), name)
    assert _polar_loss_option(types.SimpleNamespace()) == (None, "all", 1)
    o = types.SimpleNamespace(polar_loss=(1, 0))
    assert _polar_loss_option(o) == ([1.0, 0.0], "all", 1) and o.polar_loss == [1.0, 0.0]       # what opt.json will carry
    for bad in ((-1.0, 0.0), (0.0, NAN), (INF, 1.0), (1.0,), (1.0, 2.0, 3.0), "x,y", 3.0):
        with pytest.raises(ValueError, match="polar_loss"):
            _polar_loss_option(types.SimpleNamespace(polar_loss=bad))
    with pytest.raises(ValueError, match="polar_loss_where"):
        _polar_loss_option(types.SimpleNamespace(polar_loss=(1, 1), polar_loss_where="everywhere"))
    with pytest.raises(ValueError, match="pol_aolp_sign"):
        _polar_loss_option(types.SimpleNamespace(polar_loss=(1, 1), pol_aolp_sign=2))
