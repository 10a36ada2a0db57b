"""pd_polar_refine_*, host side (no GPU): the exported symbols against include/polardepth.h and SIGNATURES, every refusal with
its message (decided before any launch), the empty batch, the workspace size, and the Python layer's own refusals."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import polardepth
from polardepth import _lib, ops, refine

HEADER = os.path.join(ROOT, "include", "polardepth.h")
NAN, INF = float("nan"), float("inf")
NAMES = ("pd_polar_refine_workspace", "pd_polar_refine_setup", "pd_polar_refine_table", "pd_polar_refine_step",
         "pd_polar_refine_steps", "pd_polar_refine_finish")
L = _lib.lib
err = L.pd_last_error
p, q2 = ctypes.c_void_p(64), ctypes.c_void_p(128)
odd16, odd8, odd4 = ctypes.c_void_p(72), ctypes.c_void_p(68), ctypes.c_void_p(66)
BIG = 1 << 40


def test_symbols_and_signatures():
    src = open(HEADER).read()
    so = ctypes.CDLL(L.path)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(so, name), name
        decl = re.search(r"(?:int|size_t)\s+%s\(([^;]*)\);" % name, src)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["pd_polar_refine_workspace"][0] is ctypes.c_size_t
    sig = _lib.SIGNATURES["pd_polar_refine_setup"][1]
    assert sig[4] is ctypes.c_long and sig[6] is sig[7] is sig[8] is ctypes.c_double and sig[13] is ctypes.c_size_t
    # the header states the definition, and says that the defaults are conventions
    for text in ("p = -nx / (fx * nr)", "rhs  = (((lam*zeta0 - wE*gE) + wW*gW) - wS*gS) + wN*gN", "a = lam / (lam + S)",
                 "beta_k = (2.0*rho_k) / delta", "conventions of the caller, not measurements"):
        assert text in src, text


def test_workspace_size():
    ws = L.pd_polar_refine_workspace
    assert ws(0, 8, 8) == ws(4, 0, 8) == ws(-1, 8, 8) == 16
    sizes = [ws(n, h, w) for n, h, w in ((1, 1, 1), (1, 4, 64), (1, 5, 64), (1, 5, 65), (2, 5, 65), (16, 512, 640))]
    assert all(s % 16 == 0 and s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[1] == 32 and sizes[2] == 32 and sizes[3] == 48 and sizes[5] == (16 * 10 * 128 * 8 + 16)


def setup(depth=p, K=p, pn=p, xolp=p, ldp=8, valid=None, lam=0.02, edge=0.05, cosi=0.17, zeta0=p, coef=p, pq=None, ws=p,
          ws_bytes=BIG, N=1, H=8, W=8):
    return L.pd_polar_refine_setup(depth, K, pn, xolp, ldp, valid, lam, edge, cosi, zeta0, coef, pq, ws, ws_bytes, N, H, W, None)


def table(ws=p, ws_bytes=BIG, lam=0.02, iters=10, S=p, tab=p, N=1, H=8, W=8):
    return L.pd_polar_refine_table(ws, ws_bytes, lam, iters, S, tab, N, H, W, None)


def step(coef=p, tab=p, iters=10, k=0, zin=p, zout=q2, d=p, N=1, H=8, W=8):
    return L.pd_polar_refine_step(coef, tab, iters, k, zin, zout, d, N, H, W, None)


def steps(coef=p, tab=p, iters=10, k0=0, T=8, zin=p, zout=q2, din=p, dout=q2, N=1, H=8, W=8):
    return L.pd_polar_refine_steps(coef, tab, iters, k0, T, zin, zout, din, dout, N, H, W, None)


def finish(depth=p, coef=p, zeta=p, out=p, touched=p, residual=p, ws=p, ws_bytes=BIG, N=1, H=8, W=8):
    return L.pd_polar_refine_finish(depth, coef, zeta, out, touched, residual, ws, ws_bytes, N, H, W, None)


def test_every_entry_refuses_bad_shapes_and_accepts_the_empty_batch():
    for call in (setup, table, step, steps, finish):
        name = ("pd_polar_refine_" + call.__name__).encode()
        for kw in ({"N": -1}, {"H": 0}, {"W": -4}):
            assert call(**kw) == -22 and b"bad shape" in err() and name in err(), (call.__name__, kw)
        assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
        assert call(N=1 << 30, H=1 << 10, W=1 << 10) == -22 and b"too many tiles" in err()
        assert call(N=0) == 0                                                   # nothing is launched: the pointers are fake


def test_setup_refusals():
    for kw in ({"depth": None}, {"K": None}, {"pn": None}, {"xolp": None}, {"zeta0": None}, {"coef": None}, {"ws": None}):
        assert setup(**kw) == -22 and b"must not be null" in err(), kw
        assert setup(N=0, **kw) == -22                                          # decided before the empty batch returns
    assert setup(ldp=7) == -22 and b"row pitch" in err()
    for lam in (0.0, -0.02, NAN, INF):
        assert setup(lam=lam) == -22 and b"lam" in err() and b"> 0" in err(), lam
    for edge in (-1e-3, NAN, INF):
        assert setup(edge=edge) == -22 and b"edge_max" in err(), edge
    for cosi in (0.0, -0.5, 1.5, NAN):
        assert setup(cosi=cosi) == -22 and b"cos_inc" in err(), cosi
    assert setup(pn=odd16) == -22 and b"16-byte aligned" in err()
    for kw in ({"zeta0": odd8}, {"coef": odd8}, {"pq": odd8}, {"depth": odd4}, {"xolp": odd4}, {"K": odd4}):
        assert setup(**kw) == -22 and b"aligned" in err(), kw
    assert setup(ws=odd16) == -22 and b"workspace must be 16-byte aligned" in err()
    need = L.pd_polar_refine_workspace(1, 8, 8)
    assert setup(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert setup(edge=0.0, cosi=1.0, N=0) == 0                                  # the closed ends of the ranges


def test_table_step_and_finish_refusals():
    for kw in ({"S": None}, {"tab": None}, {"ws": None}):
        assert table(**kw) == -22 and b"must not be null" in err(), kw
    for lam in (0.0, -1.0, NAN, INF):
        assert table(lam=lam) == -22 and b"lam" in err()
    for iters in (0, -3):
        assert table(iters=iters) == -22 and b"iters" in err() and b"at least 1" in err()
        assert step(iters=iters) == -22 and b"at least 1" in err()
    assert table(S=odd8) == -22 and b"8-byte aligned" in err()
    assert table(ws_bytes=16) == -22 and b"workspace too small" in err()

    for kw in ({"coef": None}, {"tab": None}, {"zin": None}, {"zout": None}, {"d": None}):
        assert step(**kw) == -22 and b"must not be null" in err(), kw
    for k in (-1, 10, 11):
        assert step(k=k) == -22 and b"must be in [0, iters = 10)" in err(), k
    assert step(k=9, N=0) == 0
    assert step(zout=p) == -22 and b"two buffers" in err()
    for kw in ({"coef": odd8}, {"tab": odd8}, {"zin": odd8}, {"zout": odd8}, {"d": odd8}):
        assert step(**kw) == -22 and b"8-byte aligned" in err(), kw

    for kw in ({"coef": None}, {"tab": None}, {"zin": None}, {"zout": None}, {"dout": None}):
        assert steps(**kw) == -22 and b"must not be null" in err(), kw
    for T in (0, -1, 9, 64):
        assert steps(T=T) == -22 and b"T = " in err() and b"must be in [1, 8]" in err(), T
        assert steps(T=T, N=0) == -22
    for k0, T in ((-1, 1), (3, 8), (10, 1), (9, 2)):
        assert steps(k0=k0, T=T) == -22 and b"must lie in [0, iters = 10)" in err(), (k0, T)
    assert steps(k0=2, T=8, N=0) == 0 and steps(k0=9, T=1, N=0) == 0
    assert steps(k0=2, din=None) == -22 and b"d_in must not be null unless k0 = 0" in err()
    assert steps(k0=0, din=None, N=0) == 0
    assert steps(zout=p) == -22 and b"two buffers" in err()
    assert steps(din=q2) == -22 and b"two buffers" in err()
    assert steps(iters=0) == -22 and b"at least 1" in err()
    for kw in ({"coef": odd8}, {"tab": odd8}, {"zin": odd8}, {"zout": odd8}, {"din": odd8}, {"dout": odd8}):
        assert steps(**kw) == -22 and b"8-byte aligned" in err(), kw

    for kw in ({"depth": None}, {"coef": None}, {"zeta": None}, {"out": None}, {"touched": None}, {"residual": None}, {"ws": None}):
        assert finish(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"coef": odd8}, {"zeta": odd8}, {"residual": odd8}, {"depth": odd4}, {"out": odd4}):
        assert finish(**kw) == -22 and b"aligned" in err(), kw
    assert finish(ws_bytes=0) == -22 and b"workspace too small" in err()


def test_python_layer_refusals():
    assert polardepth.polar_refine is refine.polar_refine and polardepth.PolarRefined is refine.PolarRefined
    assert refine.PolarRefined._fields == ("depth", "residual", "touched", "choice")
    depth, K, pol, xolp = torch.ones(1, 1, 4, 4), torch.eye(4)[None], torch.ones(1, 9, 4, 4), torch.ones(1, 2, 4, 4)
    for fn in (refine.polar_refine, ops.polar_refine):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(depth, K, pol, xolp)
    ok = dict(lam=0.02, iters=100, edge_max=0.05, incidence_max_deg=80.0, rounds=1)
    refine._check_solver_args(**ok)
    for bad in ({"lam": 0.0}, {"lam": -1.0}, {"lam": NAN}, {"lam": INF}, {"iters": 0}, {"iters": 2.5}, {"iters": True}, {"edge_max": NAN},
                {"edge_max": -0.1}, {"edge_max": INF}, {"incidence_max_deg": 90.0}, {"incidence_max_deg": NAN},
                {"incidence_max_deg": -1.0}, {"rounds": 0}, {"rounds": 1.5}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            refine._check_solver_args(**dict(ok, **bad))
    assert refine.MAX_FUSED_STEPS == 8 and 0 <= refine.FUSED_STEPS <= 8
    assert "#define PD_POLAR_REFINE_MAX_T 8" in open(HEADER).read()
    import inspect
    sig = inspect.signature(refine.polar_refine)
    assert [sig.parameters[k].default for k in ("lam", "iters", "edge_max", "incidence_max_deg", "rho_min", "rounds")] == \
        [0.02, 100, 0.05, 80.0, 0.05, 1]
    assert "CONVENTIONS, not measurements" in refine.polar_refine.__doc__
