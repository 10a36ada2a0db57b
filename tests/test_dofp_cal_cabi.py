"""pd_frame_moments, pd_dofp_cal_solve and pd_dofp_calibrate, host side (no GPU): every refusal is decided before anything
touches the device, the header's constants, the Python layer's argument checks, Calibration.save / load, the PD_POL_CALIBRATION
mapping of manydepth/train.py and the loader, which the option leaves alone."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

from polardepth import _lib

HEADER = os.path.join(ROOT, "include", "polardepth.h")
U8, U16, F32 = 0, 1, 2
CELL, PIXEL = 0, 1
NEW = ("pd_frame_moments", "pd_dofp_cal_solve", "pd_dofp_calibrate")
P = ctypes.c_void_p(64)        # a non-null, 16-byte aligned dummy: never dereferenced on these paths
ODD = ctypes.c_void_p(72)      # 8-byte aligned only
D9 = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
D12 = (ctypes.c_double * 12)(*([0.5] * 12))


def test_header_constants_signatures_and_exports():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert defs["PD_DOFP_CAL_CELL"] == "0" and defs["PD_DOFP_CAL_PIXEL"] == "1"
    h = ctypes.CDLL(_lib.lib.path)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(h, name)
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    from polardepth import calibration
    assert calibration.KINDS == {"cell": CELL, "pixel": PIXEL}


def test_calibrate_refusals_need_no_gpu():
    L, err = _lib.lib, _lib.lib.pd_last_error

    def call(mosaic=P, dtype=U8, dark=P, gain=P, kind=CELL, out=P, B=1, H2=8, W2=8):
        return L.pd_dofp_calibrate(mosaic, dtype, dark, gain, kind, out, B, H2, W2, None)

    assert call(B=0) == 0
    assert call(B=0, mosaic=None, gain=None, out=None, dtype=9, kind=9, H2=3, W2=-1) == 0      # nothing is looked at
    assert call(B=-1) == -22 and b"bad shape" in err()
    for kw in ({"mosaic": None}, {"gain": None}, {"out": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for dtype in (-1, 3, 7):
        assert call(dtype=dtype) == -22 and b"unknown dtype" in err()
    for kind in (-1, 2):
        assert call(kind=kind) == -22 and b"unknown gain_kind" in err()
    for H2, W2 in ((7, 8), (8, 7), (0, 8), (8, 0), (1, 8), (-2, 8), (8, -4)):
        assert call(H2=H2, W2=W2) == -22 and b"even sides" in err(), (H2, W2)
    for kind in (CELL, PIXEL):
        for kw in ({"mosaic": ODD}, {"dark": ODD}, {"gain": ODD}, {"out": ODD}):
            assert call(kind=kind, **kw) == -22 and b"16-byte aligned" in err(), kw
        assert call(kind=kind, H2=65536, W2=32768) == -22 and b"too large" in err()          # 2^31 pixels in a frame
        assert call(kind=kind, H2=32768, W2=32770) == -22 and b"too large" in err()          # just past 2^30
        assert call(kind=kind, B=2048, H2=32768, W2=32768) == -22 and b"too large" in err()  # 2^41 in the batch
    assert call(W2=6, mosaic=ODD) == -22 and b"16-byte aligned" in err()                     # W2 = 6 itself is legal


def test_moments_refusals_need_no_gpu():
    L, err = _lib.lib, _lib.lib.pd_last_error

    def call(frames=P, dtype=U16, dark=P, weights=P, out=P, N=3, Q=3, H2=8, W2=8, accumulate=0):
        return L.pd_frame_moments(frames, dtype, dark, weights, out, N, Q, H2, W2, accumulate, None)

    for kw in ({"frames": None}, {"weights": None}, {"out": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for dtype in (-1, 3):
        assert call(dtype=dtype) == -22 and b"unknown dtype" in err()
    for Q in (0, 5, -1):
        assert call(Q=Q) == -22 and b"outside 1..4" in err() and str(Q).encode() in err()
    for N in (0, -3):
        assert call(N=N) == -22 and b"at least one frame" in err()
    for H2, W2 in ((7, 8), (8, 7), (0, 8), (8, -4)):
        assert call(H2=H2, W2=W2) == -22 and b"even sides" in err(), (H2, W2)
    for kw in ({"frames": ODD}, {"dark": ODD}, {"out": ODD}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    assert call(weights=ctypes.c_void_p(68)) == -22 and b"8-byte aligned" in err()
    assert call(H2=32768, W2=32770) == -22 and b"too large" in err()
    assert call(N=2048, H2=32768, W2=32768) == -22 and b"too large" in err()


def test_solve_refusals_need_no_gpu():
    L, err = _lib.lib, _lib.lib.pd_last_error

    def call(moments=P, rinv=D9, a_nom=D12, qmin=1e-3, gain=P, quality=P, H2=8, W2=8):
        return L.pd_dofp_cal_solve(moments, rinv, a_nom, qmin, gain, quality, H2, W2, None)

    for kw in ({"moments": None}, {"rinv": None}, {"a_nom": None}, {"gain": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for bad in (np.nan, np.inf, -np.inf):
        r = (ctypes.c_double * 9)(*D9)
        r[4] = bad
        assert call(rinv=r) == -22 and b"rinv[4]" in err() and b"not finite" in err()
        a = (ctypes.c_double * 12)(*D12)
        a[11] = bad
        assert call(a_nom=a) == -22 and b"a_nom[11]" in err() and b"not finite" in err()
        assert call(qmin=bad) == -22 and b"qmin" in err() and b"not finite" in err()
    for H2, W2 in ((7, 8), (8, 7), (0, 8), (8, -4)):
        assert call(H2=H2, W2=W2) == -22 and b"even sides" in err(), (H2, W2)
    for kw in ({"moments": ODD}, {"gain": ODD}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    assert call(H2=32768, W2=32770) == -22 and b"too large" in err()


def test_python_layer_names_the_offending_value():
    from polardepth import calibration as cal
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cal.apply(torch.zeros(1, 4, 4, dtype=torch.uint8), cal.Calibration(torch.ones(4, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cal.mean_frame(torch.zeros(2, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cal.fit(torch.zeros(3, 4, 4, dtype=torch.uint8), [0, 60, 120])
    with pytest.raises(ValueError, match=r"\(6, 12\).*\(6, 10\)"):
        cal.Calibration(torch.ones(3, 5, 4, 4), dark=torch.zeros(6, 12))
    with pytest.raises(ValueError, match=r"\(3, 5\)"):
        cal.Calibration(torch.ones(3, 5))
    with pytest.raises(ValueError, match="4 frames but 3 polarizer angles"):
        cal.fit(torch.zeros(4, 4, 4), [0, 60, 120])
    with pytest.raises(ValueError, match="'0,1,2,2'"):
        cal.nominal_matrix("0,1,2,2")
    with pytest.raises(ValueError, match=r"\[1, 2, 3\]"):
        cal.nominal_matrix(pol_angles=[1, 2, 3])
    with pytest.raises(TypeError, match="str"):
        cal.apply(torch.zeros(1, 4, 4), "cal.npz")
    # the host recipe is the NumPy statement's
    import dofp_cal_ref as C
    deg = C.polarizer_angles(7)
    assert np.array_equal(cal.fit_weights(deg, 0.97, np.linspace(1, 2, 7)), C.fit_weights(deg, 0.97, np.linspace(1, 2, 7)))
    for layout, ang in ((C.IMX250MZR, None), ((1, 3, 0, 2), [0.8, 44.1, 91.3, 134.6])):
        assert np.array_equal(cal.nominal_matrix(layout, ang), C.nominal_matrix(layout, ang))
    # from_flat_field is the statement's PIXEL gain
    sensor = C.Sensor((8, 12), 6)
    S = np.zeros((1, 3, 4, 6))
    S[:, 0] = 0.5 * sensor.full
    flat = sensor.measure(S)[0]
    c = cal.Calibration.from_flat_field(torch.from_numpy(flat), torch.from_numpy(sensor.dark))
    assert c.kind == "pixel" and c.shape == (8, 12) and c.bad_cells == 0
    assert np.array_equal(C.bits(c.gain.numpy()), C.bits(C.flat_field_gain(flat, sensor.dark)))
    with pytest.raises(ValueError, match=r"\(7, 12\)"):
        cal.Calibration.from_flat_field(torch.ones(7, 12))


def test_save_load_round_trip(tmp_path):
    from polardepth import calibration as cal
    rng = np.random.default_rng(0)
    gain = torch.from_numpy(rng.standard_normal((3, 5, 4, 4)).astype(np.float32))
    quality = torch.from_numpy(rng.random((3, 5)).astype(np.float32))
    quality[1, 2] = 0
    dark = torch.from_numpy(rng.random((6, 10)).astype(np.float32))
    a = cal.Calibration(gain, dark, quality, (1, 3, 0, 2), [0.8, 44.1, 91.3, 134.6])
    assert a.kind == "cell" and a.shape == (6, 10) and a.bad_cells == 1
    path = tmp_path / "cal.npz"
    a.save(str(path))
    with np.load(str(path)) as z:
        assert int(z["version"]) == cal.VERSION
    b = cal.Calibration.load(str(path))
    assert b.layout == (1, 3, 0, 2) and b.pol_angles == (0.8, 44.1, 91.3, 134.6) and b.shape == (6, 10) and b.bad_cells == 1
    for name in ("gain", "dark", "quality"):
        assert torch.equal(getattr(a, name), getattr(b, name))
    assert cal.parse(str(path)).shape == (6, 10) and cal.parse(a) is a and cal.parse(None) is None
    p = cal.Calibration(torch.ones(4, 6))                                  # PIXEL kind, nothing optional
    p.save(str(tmp_path / "p.npz"))
    q = cal.Calibration.load(str(tmp_path / "p.npz"))
    assert q.kind == "pixel" and q.dark is None and q.quality is None and q.pol_angles is None and q.layout == (2, 1, 3, 0)
    np.savez(str(tmp_path / "other.npz"), gain=np.ones((4, 6), np.float32))
    with pytest.raises(ValueError, match="other.npz.*version"):
        cal.Calibration.load(str(tmp_path / "other.npz"))


def test_train_maps_the_environment_variable():
    from manydepth.train import options_from_environment
    opts = options_from_environment(types.SimpleNamespace(), {"PD_POL_CALIBRATION": "/data/cal.npz", "PD_POL_LAYOUT": "2,1,3,0"})
    assert opts.pol_calibration == "/data/cal.npz" and opts.pol_layout == [2, 1, 3, 0]
    for env in ({}, {"PD_POL_CALIBRATION": ""}):
        assert not hasattr(options_from_environment(types.SimpleNamespace(), env), "pol_calibration")


def test_dataset_items_travel_raw(tmp_path, monkeypatch):
    """HAMMER_Dataset does not know the option: with PD_POL_CALIBRATION set, a pol_dofp item is what it was."""
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset
    from test_dofp_cabi import _tree, _mosaic
    _tree(tmp_path, ("pol_dofp",), lambda path, idx: Image.fromarray(_mosaic(idx, np.uint16)).save(path))
    mk = lambda: HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4, pol_dofp=True)[0]
    monkeypatch.delenv("PD_POL_CALIBRATION", raising=False)
    before = mk()
    monkeypatch.setenv("PD_POL_CALIBRATION", str(tmp_path / "cal.npz"))
    after = mk()
    assert set(before) == set(after)
    for k in before:
        assert before[k].dtype == after[k].dtype and torch.equal(before[k], after[k]), k
    assert after[("pol_dofp", 0, 0)].dtype == torch.uint16 and np.array_equal(after[("pol_dofp", 0, 0)].numpy()[0], _mosaic(3, np.uint16))


def test_a_calibration_is_checked_against_the_loaders_first_sensor_frame(tmp_path):
    """``check_dataset``, what the Trainer (three loaders) and Evaluation ask at construction: a tree of 192 x 256 sensor frames
    accepts a calibration of that size, refuses another with both sizes and the loader's name, and a loader without sensor
    frames reports that it serves none."""
    from PIL import Image
    from test_dofp_cabi import _tree, _mosaic
    from manydepth.datasets import HAMMER_Dataset
    from polardepth import calibration as cal
    _tree(tmp_path, ("pol_dofp",), lambda path, idx: Image.fromarray(_mosaic(idx, np.uint16)).save(path))
    ds = HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4, pol_dofp=True)
    assert cal.check_dataset(cal.Calibration(torch.ones(192, 256)), ds) is True
    assert cal.check_dataset(cal.Calibration(torch.ones(96, 128, 4, 4)), ds, "the validation loader") is True
    with pytest.raises(ValueError, match=r"64x96, the validation loader's .*pol_dofp.000003\.png is 192x256"):
        cal.check_dataset(cal.Calibration(torch.ones(64, 96)), ds, "the validation loader")
    synth = HAMMER_Dataset("synthetic", ["a"], 64, 96, [0], 4, pol_dofp=True)
    assert cal.check_dataset(cal.Calibration(torch.ones(64, 96)), synth) is False
    assert cal.check_dataset(cal.Calibration(torch.ones(64, 96)), HAMMER_Dataset("synthetic", ["a"], 64, 96, [0], 4)) is False


def test_mean_frame_needs_the_frame_count_of_a_generator():
    from polardepth import calibration as cal
    with pytest.raises(ValueError, match="count=N"):
        cal.mean_frame(iter([torch.zeros(2, 4, 4, dtype=torch.uint8)]))
    with pytest.raises(ValueError, match="at least one frame, got 0"):
        cal.mean_frame([])
