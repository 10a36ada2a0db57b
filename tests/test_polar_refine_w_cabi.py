"""pd_polar_refine_setup_w, _table_w and _weights, host side (no GPU): the exported symbols against include/polardepth.h and
SIGNATURES, every refusal with its message (decided before any launch), the empty batch, and the Python layer's own refusals."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops, refine

HEADER = os.path.join(ROOT, "include", "polardepth.h")
NAN, INF = float("nan"), float("inf")
NAMES = ("pd_polar_refine_setup_w", "pd_polar_refine_table_w", "pd_polar_refine_weights")
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
        decl = re.search(r"int\s+%s\(([^;]*)\);" % name, src)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    old, new = _lib.SIGNATURES["pd_polar_refine_setup"][1], _lib.SIGNATURES["pd_polar_refine_setup_w"][1]
    assert new[:9] == old[:9] and new[9:12] == [ctypes.c_void_p, ctypes.c_double, ctypes.c_double] and new[12:] == old[9:]
    sig = _lib.SIGNATURES["pd_polar_refine_weights"][1]
    assert sig[2] is sig[5] is ctypes.c_double and _lib.SIGNATURES["pd_polar_refine_table_w"][1][1] is ctypes.c_size_t
    # the header states the definition, and says that the defaults are conventions
    for text in ("lam_i = lam * w_i", "weight_min where !(weight >= weight_min)", "diag = (((lam_i + wE) + wW) + wS) + wN",
                 "rhs = (((lam_i*zeta0 - wE*gE) + wW*gW) - wS*gS) + wN*gN", "a_i = lam_i / (lam_i + s_i)",
                 "t = (unc_ref * (double)z) / (double)b", "h = c / r", "variance 2 b^2",
                 "a >= lam*weight_min / (lam*weight_min + 4*rho_max)", "conventions of the caller, not measurements"):
        assert text in src, text


def setup_w(depth=p, K=p, pn=p, xolp=p, ldp=8, valid=None, lam=0.02, edge=0.05, cosi=0.17, weight=p, wmin=1 / 16, wmax=1.0, zeta0=p,
            coef=p, pq=None, ws=p, ws_bytes=BIG, N=1, H=8, W=8):
    return L.pd_polar_refine_setup_w(depth, K, pn, xolp, ldp, valid, lam, edge, cosi, weight, wmin, wmax, zeta0, coef, pq, ws, ws_bytes,
                                     N, H, W, None)


def table_w(ws=p, ws_bytes=BIG, iters=10, A=p, tab=p, N=1, H=8, W=8):
    return L.pd_polar_refine_table_w(ws, ws_bytes, iters, A, tab, N, H, W, None)


def weights(depth=p, b=None, unc_ref=0.002, zprev=None, zeta0=None, c=0.005, out=p, N=1, H=8, W=8):
    return L.pd_polar_refine_weights(depth, b, unc_ref, zprev, zeta0, c, out, N, H, W, None)


def test_every_entry_refuses_bad_shapes_and_accepts_the_empty_batch():
    for call in (setup_w, table_w, weights):
        name = ("pd_polar_refine_" + call.__name__).encode()
        for kw in ({"N": -1}, {"H": 0}, {"W": -4}):
            assert call(**kw) == -22 and b"bad shape" in err() and name in err(), (call.__name__, kw)
        assert call(H=1 << 15, W=(1 << 15) + 1) == -22 and b"too large" in err()
        assert call(N=1 << 30, H=1 << 10, W=1 << 10) == -22 and b"too many tiles" in err()
        assert call(N=0) == 0                                                   # nothing is launched: the pointers are fake


def test_setup_w_refusals():
    for kw in ({"depth": None}, {"K": None}, {"pn": None}, {"xolp": None}, {"weight": None}, {"zeta0": None}, {"coef": None},
               {"ws": None}):
        assert setup_w(**kw) == -22 and b"must not be null" in err(), kw
        assert setup_w(N=0, **kw) == -22                                        # decided before the empty batch returns
    assert setup_w(ldp=7) == -22 and b"row pitch" in err()
    for lam in (0.0, -0.02, NAN, INF):
        assert setup_w(lam=lam) == -22 and b"lam" in err() and b"> 0" in err(), lam
    for edge in (-1e-3, NAN, INF):
        assert setup_w(edge=edge) == -22 and b"edge_max" in err(), edge
    for cosi in (0.0, -0.5, 1.5, NAN):
        assert setup_w(cosi=cosi) == -22 and b"cos_inc" in err(), cosi
    for wmin, wmax in ((0.0, 1.0), (-0.5, 1.0), (NAN, 1.0), (0.5, 0.25), (0.5, NAN), (0.5, INF), (INF, INF)):
        assert setup_w(wmin=wmin, wmax=wmax) == -22 and b"0 < weight_min <= weight_max < inf" in err(), (wmin, wmax)
        assert setup_w(wmin=wmin, wmax=wmax, N=0) == -22
    assert setup_w(wmin=0.5, wmax=0.5, N=0) == 0 and setup_w(wmin=1e-300, wmax=1e300, N=0) == 0
    assert setup_w(pn=odd16) == -22 and b"16-byte aligned" in err()
    for kw in ({"zeta0": odd8}, {"coef": odd8}, {"pq": odd8}, {"depth": odd4}, {"xolp": odd4}, {"K": odd4}, {"weight": odd4}):
        assert setup_w(**kw) == -22 and b"aligned" in err(), kw
    assert setup_w(ws=odd16) == -22 and b"workspace must be 16-byte aligned" in err()
    need = L.pd_polar_refine_workspace(1, 8, 8)                                 # the unweighted route's size suffices
    assert setup_w(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert setup_w(ws_bytes=need, N=0) == 0


def test_table_w_and_weights_refusals():
    for kw in ({"A": None}, {"tab": None}, {"ws": None}):
        assert table_w(**kw) == -22 and b"must not be null" in err(), kw
    for iters in (0, -3):
        assert table_w(iters=iters) == -22 and b"iters" in err() and b"at least 1" in err()
    assert table_w(A=odd8) == -22 and b"8-byte aligned" in err() and table_w(tab=odd8) == -22
    assert table_w(ws=odd16) == -22 and b"16-byte aligned" in err()
    assert table_w(ws_bytes=16) == -22 and b"workspace too small" in err()

    for kw in ({"depth": None}, {"out": None}):
        assert weights(**kw) == -22 and b"must not be null" in err(), kw
        assert weights(N=0, **kw) == -22
    for unc_ref in (0.0, -0.002, NAN, INF):
        assert weights(b=p, unc_ref=unc_ref) == -22 and b"unc_ref" in err() and b"> 0" in err(), unc_ref
        assert weights(unc_ref=unc_ref, N=0) == 0                               # not read without b
    for c in (0.0, -0.005, NAN, INF):
        assert weights(zprev=p, zeta0=q2, c=c) == -22 and b"c = " in err() and b"> 0" in err(), c
        assert weights(c=c, N=0) == 0                                           # not read without zeta_prev
    assert weights(zprev=p) == -22 and b"both be given or both be null" in err()
    assert weights(zeta0=p) == -22 and b"both be given or both be null" in err()
    for kw in ({"depth": odd4}, {"b": odd4}, {"out": odd4}):
        assert weights(**kw) == -22 and b"aligned" in err(), kw
    for kw in ({"zprev": odd8, "zeta0": p}, {"zprev": p, "zeta0": odd8}):
        assert weights(**kw) == -22 and b"8-byte aligned" in err(), kw
    for kw in ({}, {"b": p}, {"zprev": p, "zeta0": q2}, {"b": p, "zprev": p, "zeta0": q2}):      # the four input modes
        assert weights(N=0, **kw) == 0, kw


def test_python_layer_refusals():
    ok = dict(unc_ref=0.002, robust=None, weight_min=1 / 16, weight_max=1.0, rounds=1)
    refine._check_weight_args(**ok)
    refine._check_weight_args(**dict(ok, robust=0.005, rounds=2))
    for bad in ({"unc_ref": 0.0}, {"unc_ref": NAN}, {"unc_ref": INF}, {"unc_ref": "x"}, {"weight_min": 0.0}, {"weight_min": 2.0},
                {"weight_min": NAN}, {"weight_max": INF}, {"weight_max": 0.01}, {"robust": 0.0}, {"robust": -1.0}, {"robust": NAN},
                {"robust": True, "rounds": 2}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            refine._check_weight_args(**dict(ok, **bad))
    with pytest.raises(ValueError, match="rounds >= 2"):
        refine._check_weight_args(**dict(ok, robust=0.005))
    sig = inspect.signature(refine.polar_refine)
    names = list(sig.parameters)
    assert names[names.index("normals") + 1:] == ["weight", "uncertainty", "unc_ref", "robust", "weight_min", "weight_max",
                                                  "return_weight"]
    assert [sig.parameters[k].default for k in names[names.index("normals") + 1:]] == [None, None, 0.002, None, 1 / 16, 1.0, False]
    ssig = inspect.signature(refine.solve)
    snames = list(ssig.parameters)
    assert snames[:11] == ["depth", "K", "pol_normal", "xolp", "ldp", "valid", "lam", "iters", "edge_max", "incidence_max_deg", "fused"]
    assert snames[11:14] == ["weight", "weight_min", "weight_max"]
    assert [ssig.parameters[k].default for k in snames[11:14]] == [None, 1 / 16, 1.0]
    doc = refine.polar_refine.__doc__
    assert "unc_ref = 0.002, weight_min = 1/16 and robust's 0.005 are CONVENTIONS, not measurements" in doc
    assert "a >= lam weight_min / (lam weight_min +" in doc and "needs more ``iters``" in doc
    assert refine.PolarRefined._fields == ("depth", "residual", "touched", "choice")
    depth, K, pol, xolp = torch.ones(1, 1, 4, 4), torch.eye(4)[None], torch.ones(1, 9, 4, 4), torch.ones(1, 2, 4, 4)
    for fn in (refine.polar_refine, ops.polar_refine):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(depth, K, pol, xolp, uncertainty=depth)


def test_evaluations_options_need_no_gpu(monkeypatch):
    from manydepth import evaluation as E
    for k in ("uncertainty", "unc_ref", "robust", "weight_min", "weight_max"):
        assert k in E._REFINE_OPTIONS
    opt = E._polar_refine_option
    assert opt({"uncertainty": True, "unc_ref": 0.004}) == {"uncertainty": True, "unc_ref": 0.004}
    assert opt({"robust": 0.005, "rounds": 2}) == {"robust": 0.005, "rounds": 2}
    with pytest.raises(ValueError, match="rounds >= 2"):
        opt({"robust": 0.005})
    for bad in ({"unc_ref": -1.0}, {"weight_min": 0.0}, {"weight_max": 0.01}, {"robust": NAN, "rounds": 2}, {"uncertainty": 0.004}):
        with pytest.raises(ValueError):
            opt(bad)
    # the environment fills what the options leave open, and means nothing while the refinement is off
    assert opt(None, "1", "0.005") is None
    assert opt("1", "1", None) == {"uncertainty": True}
    assert opt("1", "0.004", None) == {"uncertainty": True, "unc_ref": 0.004}
    assert opt("1", None, "0.005") == {"robust": 0.005, "rounds": 2}
    assert opt({"rounds": 3}, None, "0.005") == {"rounds": 3, "robust": 0.005}
    assert opt("0.05,30", "1", "0.01") == {"lam": 0.05, "iters": 30, "uncertainty": True, "robust": 0.01, "rounds": 2}
    assert opt({"uncertainty": False, "robust": 0.02, "rounds": 2}, "1", "0.005") == {"uncertainty": False, "robust": 0.02, "rounds": 2}
    assert opt("1", "0", "") == {} and opt(True) == {}
    src = inspect.getsource(E.Evaluation.__init__)
    assert 'os.environ.get("PD_POLAR_REFINE_UNCERTAINTY")' in src and 'os.environ.get("PD_POLAR_REFINE_ROBUST")' in src
    # decided before the constructor looks for the GPU
    for var in ("PD_POLAR_REFINE", "PD_POLAR_REFINE_UNCERTAINTY", "PD_POLAR_REFINE_ROBUST", "PD_UNCERTAINTY"):
        monkeypatch.delenv(var, raising=False)
    with pytest.raises(ValueError, match=r"needs Evaluation\(uncertainty=True\)"):
        E.Evaluation(data_path="synthetic", polar_refine={"uncertainty": True})
    monkeypatch.setenv("PD_POLAR_REFINE", "1")
    monkeypatch.setenv("PD_POLAR_REFINE_UNCERTAINTY", "0.004")
    with pytest.raises(ValueError, match=r"needs Evaluation\(uncertainty=True\)"):
        E.Evaluation(data_path="synthetic")
