"""pd_polar_normals_stats, host side (no GPU): the exported symbols, the defines, SIGNATURES, every refusal decided before the
device is touched, and the workspace query."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import polar_normals_ref as R
from polardepth import _lib
from polardepth import polar_normals_eval as PE

HEADER = os.path.join(ROOT, "include", "polardepth.h")
ALL = (ctypes.c_int * 2)(1, 0)                       # one class: every pixel
RANGED = (ctypes.c_int * 4)(1, 0, 20, 160)
INF = float("inf")
NAN = float("nan")


def test_symbols_defines_and_signatures():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert int(defs["PD_PNSTAT_NORMAL_BINS"]) == PE.NORMAL_BINS == R.NBINS == 720 == int(defs["PD_NSTAT_BINS"])
    assert int(defs["PD_PNSTAT_AZIMUTH_BINS"]) == PE.AZIMUTH_BINS == R.ABINS == 360
    assert int(defs["PD_PNSTAT_COUNTERS"]) == len(PE.NORMAL_COUNTERS) == len(PE.AZIMUTH_COUNTERS) == 4
    assert int(defs["PD_PNSTAT_SUMS"]) == len(PE.SUM_NAMES) == 4
    assert int(defs["PD_PNSTAT_NORMAL_RECORD_BYTES"]) == PE.NORMAL_RECORD_BYTES == 80 + 4 * 720
    assert int(defs["PD_PNSTAT_AZIMUTH_RECORD_BYTES"]) == PE.AZIMUTH_RECORD_BYTES == 80 + 4 * 360
    assert int(defs["PD_PNSTAT_MAX_CLASSES"]) == PE.MAX_CLASSES == 16
    assert PE.NORMAL_COUNTERS == R.NORMAL_COUNTERS and PE.AZIMUTH_COUNTERS == R.AZIMUTH_COUNTERS
    so = ctypes.CDLL(_lib.lib.path)
    for name in ("pd_polar_normals_stats", "pd_polar_normals_stats_workspace"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src
    assert len(_lib.SIGNATURES["pd_polar_normals_stats"][1]) == 26
    assert _lib.SIGNATURES["pd_polar_normals_stats_workspace"][0] is ctypes.c_size_t


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; none reaches the device (the pointers are dummies)."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only

    def call(pred=p, ld=4, pol=p, xolp=p, ldp=8, mask=None, classes=ALL, nk=1, valid=None, edges=p, rho_min=0.05, rho_max=1.0,
             tilt2=0.0076, sign=1, sn=p, sa=p, az=None, nd=None, choice=None, pn=None, ws=p, ws_bytes=1 << 40, N=1, H=8, W=8):
        return L.pd_polar_normals_stats(pred, ld, pol, xolp, ldp, mask, classes, nk, valid, edges, rho_min, rho_max, tilt2, sign,
                                        sn, sa, az, nd, choice, pn, ws, ws_bytes, N, H, W, None)

    for kw in ({"pred": None}, {"pol": None}, {"xolp": None}, {"classes": None}, {"edges": None}, {"ws": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    assert call(sn=None, sa=None) == -22 and b"both null" in err()
    assert call(sn=None, sa=None, az=p, nd=p, choice=p, pn=p) == -22 and b"both null" in err()
    for kw in ({"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -4}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for nk in (0, -1, 17, 1 << 20):
        assert call(nk=nk) == -22 and b"classes" in err(), nk
    assert call(classes=RANGED, nk=2) == -22 and b"mask is null" in err() and b"[20, 160]" in err()
    assert call(classes=(ctypes.c_int * 2)(0, 0)) == -22 and b"mask is null" in err()      # lo == hi is a range too
    for ld in (2, 0, -4):
        assert call(ld=ld) == -22 and b"pixel stride" in err(), ld
    for ldp in (7, 0, -8):
        assert call(ldp=ldp) == -22 and b"row pitch" in err(), ldp
    for sign in (0, 2, -2, 1 << 20):
        assert call(sign=sign) == -22 and b"aolp_sign" in err(), sign
    for lo, hi in ((NAN, 1.0), (0.05, NAN), (-INF, 1.0), (0.05, INF), (0.5, 0.25)):
        assert call(rho_min=lo, rho_max=hi) == -22 and b"finite and not inverted" in err(), (lo, hi)
    for t in (-0.1, 1.0, 1.5, NAN, INF):
        assert call(tilt2=t) == -22 and b"tilt2_min" in err(), t
    for kw in ({"pol": odd}, {"sn": odd}, {"sa": odd}, {"pn": odd}, {"ws": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    need = L.pd_polar_normals_stats_workspace(1, 8, 8, 1)
    assert call(ws_bytes=need - 1) == -22 and b"workspace too small" in err() and str(need).encode() in err()
    assert call(ws_bytes=0) == -22 and b"workspace too small" in err()
    assert call(H=1 << 15, W=(1 << 15) + 1, ldp=1 << 16) == -22 and b"too large" in err()   # offsets inside a frame are 32-bit
    # an empty batch is fine and touches nothing; either record set may be left out; every map may be asked for
    assert call(N=0) == 0 and call(N=0, sn=None) == 0 and call(N=0, sa=None) == 0
    assert call(N=0, az=p, nd=p, choice=p, pn=p, mask=p, valid=p, classes=RANGED, nk=2) == 0
    assert call(N=0, sign=-1) == 0 and call(N=0, tilt2=0.0) == 0 and call(N=0, rho_min=0.3, rho_max=0.3) == 0
    assert call(N=0, ld=3, pred=odd) == 0 and call(N=0, ldp=1 << 20) == 0
    assert call(N=0, ws=None) == -22                                               # but its arguments are still checked


def test_workspace_is_monotone_never_zero_and_a_multiple_of_16():
    ws = _lib.lib.pd_polar_normals_stats_workspace
    assert ws(0, 0, 0, 0) > 0 and ws(0, 512, 640, 12) > 0 and ws(-1, -1, -1, -1) > 0
    shapes = [(1, 1, 4, 1), (2, 5, 7, 1), (3, 33, 70, 12), (4, 64, 96, 12), (12, 320, 480, 12), (16, 512, 640, 16),
              (4096, 4096, 4096, 16), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]
    sizes = [ws(*s) for s in shapes]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[4] < sizes[5]
    assert ws(3, 40, 52, 12) == 2 * 3 * 3 * 12 * 4 * 8         # two sets of [N][G][K][4] doubles, G = ceil(40 * 52 / 1024)
    assert ws(1, 264, 256, 1) == 2 * 64 * 4 * 8                 # 66 workgroups' worth of pixels: the cap of 64


def test_python_layer_refuses_cpu_tensors_and_bad_options():
    pred, pol, xolp = torch.ones(1, 3, 4, 4), torch.ones(1, 9, 4, 4), torch.ones(1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PE.polar_normals_stats(pred, pol, xolp, classes=[("all", None)])
    assert len(PE.METRIC_NAMES) == 8 and len(PE.CHOICE_NAMES) == 7
    doc = PE.polar_normals_stats.__doc__
    assert doc.count("CONVENTION") == 2 and "not a measurement" in doc


def test_write_ply_with_normals(tmp_path):
    """nx ny nz sit behind x y z, follow the w == 1 selection and the viewer flip; without them the file is what it was."""
    import numpy as np
    from polardepth import pointcloud as PC
    rng = np.random.default_rng(4)
    pts = np.zeros((50, 4), np.float32)
    pts[:, :3] = rng.normal(size=(50, 3))
    pts[:, 3] = rng.choice([1.0, 0.0, -1.0], 50)
    nrm = rng.normal(size=(50, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    keep = pts[:, 3] == 1
    for flip in (True, False):
        path = tmp_path / "n.ply"
        assert PC.write_ply(str(path), torch.from_numpy(pts), rgb, flip=flip, normals=torch.from_numpy(nrm)) == keep.sum()
        head, payload = path.read_bytes().split(b"end_header\n", 1)
        props = [l.split()[-1] for l in head.decode("ascii").splitlines() if l.startswith("property")]
        assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
        rows = np.frombuffer(payload, dtype=[("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
        sign = np.array([1, -1, -1], np.float32) if flip else np.ones(3, np.float32)
        assert np.array_equal(rows["xyz"], pts[keep, :3] * sign) and np.array_equal(rows["n"], nrm[keep] * sign)
        assert np.array_equal(rows["rgb"], rgb[keep])
    plain, none = tmp_path / "a.ply", tmp_path / "b.ply"
    PC.write_ply(str(plain), pts, rgb)
    PC.write_ply(str(none), pts, rgb, normals=None)
    assert plain.read_bytes() == none.read_bytes() and b"nx" not in plain.read_bytes()
    with pytest.raises(ValueError, match="normals must be"):
        PC.write_ply(str(plain), pts, rgb, normals=nrm[:10])
