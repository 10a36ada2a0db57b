"""pd_polar_normals_stats_ray, pd_polar_loss_fwd_ray / _bwd_ray, host side (no GPU): the exported symbols and SIGNATURES, the
new refusals with their messages, the old refusals reached through the new entries, the Python layers' own refusals, and the
Trainer option with its environment mapping."""
import ctypes
import os
import re
import types

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops
from polardepth import polar_normals_eval as PE

HEADER = os.path.join(ROOT, "include", "polardepth.h")
NAN = float("nan")


def test_symbols_and_signatures():
    src = open(HEADER).read()
    so = ctypes.CDLL(_lib.lib.path)
    for name, old, extra in (("pd_polar_normals_stats_ray", "pd_polar_normals_stats", 2), ("pd_polar_loss_fwd_ray", "pd_polar_loss_fwd", 1),
                             ("pd_polar_loss_bwd_ray", "pd_polar_loss_bwd", 1)):
        assert name in _lib.SIGNATURES and hasattr(so, name) and hasattr(so, old)
        decl = re.search(r"int\s+%s\(([^;]*)\);" % name, src)
        nargs = len(_lib.SIGNATURES[old][1]) + extra
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert "ray_frame" in decl.group(1)
    sig = _lib.SIGNATURES["pd_polar_normals_stats_ray"][1]
    assert sig[2] is ctypes.c_void_p and sig[3] is ctypes.c_int and sig[14] is ctypes.c_double and sig[23] is ctypes.c_size_t
    assert _lib.SIGNATURES["pd_polar_loss_fwd_ray"][1][11] is ctypes.c_int and _lib.SIGNATURES["pd_polar_loss_fwd_ray"][1][8] is ctypes.c_double
    assert _lib.SIGNATURES["pd_polar_loss_bwd_ray"][1][10] is ctypes.c_int
    # the header states the definition and no longer says "not built"
    assert "NOT BUILT: the residual uses the orthographic convention" not in src and "THE RAY FRAME" in src
    assert "s  = (d + pz) / (1.0 + uz)" in src and "t = 2.0*gz" in src


def test_the_evaluators_refusals_need_no_gpu():
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)
    odd = ctypes.c_void_p(72)
    classes = (ctypes.c_int * 2)(1, 0)
    ranged = (ctypes.c_int * 2)(20, 160)

    def call(pred=p, ld=4, K=p, ray=1, pol=p, xolp=p, ldp=8, mask=None, cls=classes, nk=1, valid=None, edges=p, rho_min=0.05,
             rho_max=1.0, tilt2=0.0076, sign=1, rec_n=p, rec_a=p, ws=p, ws_bytes=1 << 40, N=1, H=8, W=8):
        return L.pd_polar_normals_stats_ray(pred, ld, K, ray, pol, xolp, ldp, mask, cls, nk, valid, edges, rho_min, rho_max, tilt2,
                                            sign, rec_n, rec_a, None, None, None, None, ws, ws_bytes, N, H, W, None)

    # the new refusals
    for ray in (2, -1, 1 << 20):
        assert call(ray=ray) == -22 and b"ray_frame" in err() and b"must be 0 or 1" in err(), ray
        assert call(ray=ray, K=None) == -22 and b"must be 0 or 1" in err()
    assert call(ray=1, K=None) == -22 and b"needs the intrinsics K" in err() and b"pd_polar_normals_stats_ray" in err()
    assert call(ray=1, K=None, N=0) == -22                                      # decided before the empty batch returns
    assert call(ray=0, K=None, N=0) == 0 and call(ray=1, N=0) == 0 and call(ray=0, N=0) == 0
    # the old refusals, reached through the new entry with the frame on and off
    for ray in (0, 1):
        for kw in ({"pred": None}, {"pol": None}, {"xolp": None}, {"cls": None}, {"edges": None}, {"ws": None}):
            assert call(ray=ray, **kw) == -22 and b"must not be null" in err(), kw
        assert call(ray=ray, rec_n=None, rec_a=None) == -22 and b"nothing to fill" in err()
        for kw in ({"N": -1}, {"H": 0}, {"W": -4}):
            assert call(ray=ray, **kw) == -22 and b"bad shape" in err(), kw
        assert call(ray=ray, ld=2) == -22 and b"pixel stride" in err()
        assert call(ray=ray, ldp=7) == -22 and b"row pitch" in err()
        assert call(ray=ray, sign=0) == -22 and b"aolp_sign" in err()
        assert call(ray=ray, rho_min=NAN) == -22 and b"finite and not inverted" in err()
        assert call(ray=ray, tilt2=1.0) == -22 and b"tilt2_min" in err()
        assert call(ray=ray, pol=odd) == -22 and b"16-byte aligned" in err()
        assert call(ray=ray, nk=0) == -22 and call(ray=ray, nk=17) == -22
        assert call(ray=ray, cls=ranged) == -22 and b"mask is null" in err()
        assert call(ray=ray, H=1 << 15, W=(1 << 15) + 1, ldp=1 << 16) == -22 and b"too large" in err()
        assert call(ray=ray, ws_bytes=0) == -22 and b"workspace too small" in err()
    # the old entry names itself, the new one itself
    assert L.pd_polar_normals_stats(p, 2, p, p, 8, None, classes, 1, None, p, 0.05, 1.0, 0.0, 1, p, p, None, None, None, None, p,
                                    1 << 40, 1, 8, 8, None) == -22 and b"pd_polar_normals_stats:" in err()
    assert call(ld=2) == -22 and b"pd_polar_normals_stats_ray:" in err()
    assert L.pd_polar_normals_stats_workspace(3, 40, 52, 12) > 0                  # unchanged: one size for both entries


def test_the_loss_refusals_need_no_gpu():
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)
    odd = ctypes.c_void_p(72)
    odd4 = ctypes.c_void_p(68)

    def fwd(depth=p, K=p, pol=p, xolp=p, ldp=8, valid=None, rho_min=0.05, rho_max=1.0, tilt2=0.0076, sign=1, weighted=1, ray=1,
            state=p, sums=p, values=p, maps=None, ws=p, ws_bytes=1 << 40, N=1, H=8, W=8):
        return L.pd_polar_loss_fwd_ray(depth, K, pol, xolp, ldp, valid, rho_min, rho_max, tilt2, sign, weighted, ray, state, sums,
                                       values, maps, ws, ws_bytes, N, H, W, None)

    def bwd(depth=p, K=p, pol=p, xolp=p, ldp=8, state=p, g=p, sums=p, sign=1, weighted=1, ray=1, gdepth=p, N=1, H=8, W=8):
        return L.pd_polar_loss_bwd_ray(depth, K, pol, xolp, ldp, state, g, sums, sign, weighted, ray, gdepth, N, H, W, None)

    for call in (fwd, bwd):
        for ray in (2, -1, 7):
            assert call(ray=ray) == -22 and b"ray_frame" in err() and b"must be 0 or 1" in err(), (call.__name__, ray)
            assert call(ray=ray, N=0) == -22
        assert call.__name__.encode() in b"fwd bwd" and (b"pd_polar_loss_%s_ray" % call.__name__.encode()) in err()
        for ray in (0, 1):
            for kw in ({"depth": None}, {"K": None}, {"pol": None}, {"xolp": None}, {"state": None}, {"sums": None}):
                assert call(ray=ray, **kw) == -22 and b"must not be null" in err(), (call.__name__, kw)
            for kw in ({"N": -1}, {"H": 0}, {"W": -4}):
                assert call(ray=ray, **kw) == -22 and b"bad shape" in err(), kw
            assert call(ray=ray, ldp=7) == -22 and b"row pitch" in err()
            assert call(ray=ray, sign=2) == -22 and b"aolp_sign" in err()
            assert call(ray=ray, weighted=2) == -22 and b"dolp_weighted" in err()
            assert call(ray=ray, pol=odd) == -22 and b"16-byte aligned" in err()
            assert call(ray=ray, sums=odd4) == -22 and b"8-byte aligned" in err()
            assert call(ray=ray, H=1 << 15, W=(1 << 15) + 1, ldp=1 << 16) == -22 and b"too large" in err()
            assert call(ray=ray, N=0) == 0
    for ray in (0, 1):
        assert fwd(ray=ray, values=None) == -22 and b"must not be null" in err()
        assert fwd(ray=ray, rho_min=0.5, rho_max=0.25) == -22 and b"finite and not inverted" in err()
        assert fwd(ray=ray, tilt2=-0.1) == -22 and b"tilt2_min" in err()
        need = L.pd_polar_loss_rows(1, 8, 8) * 11 * 8
        assert fwd(ray=ray, ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
        assert bwd(ray=ray, gdepth=None) == -22 and b"must not be null" in err()
        assert bwd(ray=ray, N=1 << 20, H=1 << 15, W=1 << 15, ldp=1 << 15) == -22 and b"too many tiles" in err()


def test_python_layers_refuse_cpu_tensors():
    depth, K, pol, xolp = torch.ones(1, 1, 4, 4), torch.eye(4)[None], torch.ones(1, 9, 4, 4), torch.ones(1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.polar_loss(depth, K, pol, xolp, ray_frame=True)
    with pytest.raises(Exception, match="(?i)cuda|cpu"):
        PE.polar_normals_stats(torch.ones(1, 3, 4, 4), pol, xolp, K=K, ray_frame=True)


def test_trainer_option_and_environment_mapping():
    from manydepth.train import options_from_environment
    from manydepth.trainer import _polar_loss_option
    opts = options_from_environment(types.SimpleNamespace(), {"PD_POLAR_LOSS": "0.5,0.25", "PD_POLAR_RAY_FRAME": "1"})
    assert opts.polar_loss == [0.5, 0.25] and opts.polar_ray_frame is True
    assert _polar_loss_option(opts) == ([0.5, 0.25], "all", 1) and opts.polar_ray_frame is True        # what opt.json will carry
    opts = options_from_environment(types.SimpleNamespace(), {"PD_POLAR_LOSS": "1,1", "PD_POLAR_RAY_FRAME": "0"})
    assert opts.polar_ray_frame is False and _polar_loss_option(opts) == ([1.0, 1.0], "all", 1)
    # unset: the attribute does not appear, and _polar_loss_option does not invent it
    plain = options_from_environment(types.SimpleNamespace(), {"PD_POLAR_LOSS": "1,1"})
    assert not hasattr(plain, "polar_ray_frame")
    _polar_loss_option(plain)
    assert not hasattr(plain, "polar_ray_frame")
    assert not hasattr(options_from_environment(types.SimpleNamespace(), {}), "polar_ray_frame")
    o = types.SimpleNamespace(polar_loss=(1, 0), polar_ray_frame=1)
    _polar_loss_option(o)
    assert o.polar_ray_frame is True
    # without the term there is nothing the frame could apply to
    with pytest.raises(ValueError, match="polar_ray_frame is set without opt.polar_loss"):
        _polar_loss_option(types.SimpleNamespace(polar_ray_frame=True))
    with pytest.raises(ValueError, match="polar_ray_frame is set without opt.polar_loss"):
        _polar_loss_option(options_from_environment(types.SimpleNamespace(), {"PD_POLAR_RAY_FRAME": "1"}))
    assert _polar_loss_option(types.SimpleNamespace(polar_ray_frame=False)) == (None, "all", 1)
    assert _polar_loss_option(types.SimpleNamespace(polar_ray_frame=None)) == (None, "all", 1)
    for bad in ("yes", 2, -1, 0.5, [1]):
        with pytest.raises(ValueError, match="polar_ray_frame must be True or False"):
            _polar_loss_option(types.SimpleNamespace(polar_loss=(1, 1), polar_ray_frame=bad))


def test_the_reference_option_table_is_untouched():
    from manydepth.options import MonodepthOptions
    opts = MonodepthOptions().parse(["--data_path", "synthetic"])
    assert not hasattr(opts, "polar_ray_frame") and not hasattr(opts, "polar_loss")


def test_evaluation_reads_the_option_and_the_environment(monkeypatch):
    import inspect
    from manydepth.evaluation import Evaluation
    sig = inspect.signature(Evaluation.__init__)
    assert sig.parameters["polar_ray_frame"].default is None
    src = inspect.getsource(Evaluation.__init__)
    assert 'os.environ.get("PD_POLAR_RAY_FRAME") == "1"' in src
