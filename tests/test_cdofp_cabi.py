"""pd_cdofp_demosaic, host side (no GPU): the header's declaration, every refusal decided before anything touches the device,
the Python layer's argument checks, and HAMMER_Dataset(pol_cdofp=True)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from polardepth import _lib

HEADER = os.path.join(ROOT, "include", "polardepth.h")
POL = (ctypes.c_int * 4)(2, 1, 3, 0)
RGGB = (ctypes.c_int * 4)(0, 1, 1, 2)
U8, U16, F32 = 0, 1, 2


def test_header_declares_the_entry_point():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert (defs["PD_POLAR_U8"], defs["PD_POLAR_U16"], defs["PD_POLAR_F32"]) == ("0", "1", "2")
    decl = re.search(r"int\s+pd_cdofp_demosaic\s*\(([^;]*)\)\s*;", src)
    assert decl, "pd_cdofp_demosaic is not declared in include/polardepth.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const void* mosaic", "int dtype", "const int* layout", "const int* bayer", "const double* gains",
                      "double color_scale", "void* planes", "void* color_u8", "void* rgb_planes", "int B", "int H4", "int W4",
                      "void* stream"]
    res, args = _lib.SIGNATURES["pd_cdofp_demosaic"]
    c = ctypes
    assert res is c.c_int and args == [c.c_void_p, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_double),
                                       c.c_double, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.lib.path), "pd_cdofp_demosaic")
    from polardepth import cdofp
    assert cdofp.IMX250MYR_POL == (2, 1, 3, 0) and cdofp.RGGB == (0, 1, 1, 2)
    assert cdofp.BAYER_ORDERS == {"RGGB": (0, 1, 1, 2), "BGGR": (2, 1, 1, 0), "GRBG": (1, 0, 2, 1), "GBRG": (1, 2, 0, 1)}


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; an empty batch returns 0 before anything is looked at."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only
    nan, inf = float("nan"), float("inf")

    def call(mosaic=p, dtype=U8, layout=POL, bayer=RGGB, gains=None, scale=1.0, planes=p, color=p, rgb=p, B=1, H4=8, W4=8):
        g = None if gains is None else (ctypes.c_double * 3)(*gains)
        return L.pd_cdofp_demosaic(mosaic, dtype, layout, bayer, g, scale, planes, color, rgb, B, H4, W4, None)

    assert call(B=0) == 0
    assert call(B=0, mosaic=None, layout=None, bayer=None, planes=None, color=None, rgb=None, dtype=9, scale=nan, H4=3) == 0
    assert call(B=-1) == -22 and b"bad shape" in err()
    for kw in ({"mosaic": None}, {"layout": None}, {"bayer": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    assert call(planes=None, color=None, rgb=None) == -22 and b"must not all be null" in err()
    for dtype in (-1, 3, 7):
        assert call(dtype=dtype) == -22 and b"unknown dtype" in err()
    for bad in ((0, 1, 2, 2), (0, 1, 2, 4), (-1, 0, 1, 2), (0, 0, 0, 0), (1, 2, 3, 4)):
        assert call(layout=(ctypes.c_int * 4)(*bad)) == -22 and b"not a permutation" in err(), bad
        assert ("(%d,%d,%d,%d)" % bad).encode() in err()
    for bad in ((0, 1, 2, 1), (1, 1, 0, 2), (0, 0, 1, 2), (0, 1, 1, 0), (0, 1, 1, 3), (0, 1, 1, -1), (1, 1, 1, 1), (0, 2, 2, 1),
                (4, 1, 1, 2)):
        assert call(bayer=(ctypes.c_int * 4)(*bad)) == -22 and b"not a Bayer order" in err(), bad
        assert ("(%d,%d,%d,%d)" % bad).encode() in err()
    for gains in ((nan, 1, 1), (1, inf, 1), (1, 1, -inf)):
        assert call(gains=gains) == -22 and b"gains must be finite" in err(), gains
    for scale in (nan, inf, -inf, 0.0, -1.0):
        assert call(scale=scale) == -22 and b"color_scale must be finite and greater than 0" in err(), scale
    for H4, W4 in ((6, 8), (8, 6), (0, 8), (8, 0), (2, 8), (-4, 8), (8, -4), (9, 8), (8, 10)):
        assert call(H4=H4, W4=W4) == -22 and b"multiples of 4" in err(), (H4, W4)
    for kw in ({"mosaic": odd}, {"planes": odd}, {"color": odd}, {"rgb": odd}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    assert call(H4=65536, W4=32768) == -22 and b"too large" in err()         # 2^31 pixels in a frame
    assert call(H4=32768, W4=32772) == -22 and b"too large" in err()         # just past 2^30
    assert call(B=2048, H4=32768, W4=32768) == -22 and b"too large" in err()  # 2^41 in the batch
    # every Bayer order, NULL outputs and odd-looking but legal sizes pass the checks above: refused here for alignment only
    for bayer in ((0, 1, 1, 2), (2, 1, 1, 0), (1, 0, 2, 1), (1, 2, 0, 1)):
        assert call(bayer=(ctypes.c_int * 4)(*bayer), W4=20, planes=None, rgb=None, color=odd, gains=(2.0, 1.0, 0.5)) == -22
        assert b"16-byte aligned" in err()


def test_python_layer_names_the_offending_value():
    from polardepth import cdofp
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cdofp.demosaic(torch.zeros(1, 4, 4, dtype=torch.uint8))
    assert cdofp.parse_bayer("RGGB") == (0, 1, 1, 2) and cdofp.parse_bayer("gbrg") == (1, 2, 0, 1)
    assert cdofp.parse_bayer("0,1,1,2") == (0, 1, 1, 2) and cdofp.parse_bayer([2, 1, 1, 0]) == (2, 1, 1, 0)
    for bad in ("RGBG", "0,1,2,1", (0, 1, 1), "a,b,c,d", (0, 1, 1, 3), 5):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            cdofp.parse_bayer(bad)
    assert cdofp.options() == ((2, 1, 3, 0), (0, 1, 1, 2), None, None)
    assert cdofp.options("0,1,2,3", "BGGR", "2,1,1.5", "0.0625") == ((0, 1, 2, 3), (2, 1, 1, 0), (2.0, 1.0, 1.5), 0.0625)
    for kw, match in (({"layout": "0,1,2,2"}, "permutation"), ({"bayer": "RGGG"}, "'RGGG'"), ({"gains": (1, 2)}, "three"),
                      ({"gains": "1,nan,1"}, "finite"), ({"color_scale": 0}, "greater than 0"),
                      ({"color_scale": float("inf")}, "finite"), ({"color_scale": "x"}, "'x'")):
        with pytest.raises(ValueError, match=match):
            cdofp.options(**kw)
    # expand leaves a batch alone unless the frame is there and both results are missing: no device is touched here
    for batch in ({}, {("pol", 0, 0): 1}, {cdofp.KEY: 1, ("pol", 0, 0): 2}, {cdofp.KEY: 1, ("color_raw", 0, 0): 2},
                  {cdofp.KEY: 1, ("pol", 0, 0): 2, ("color_raw", 0, 0): 3}):
        assert cdofp.expand(dict(batch)) == batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cdofp.expand({cdofp.KEY: torch.zeros(1, 1, 4, 4, dtype=torch.uint8)})


def test_wide_frames_need_a_color_scale():
    """The argument checks come before the device check, so they show on any machine: a uint16 / float32 frame with "color"
    wanted and no scale is a ValueError, with a scale (or without "color") it gets as far as the device check."""
    from polardepth import cdofp
    for dt in (torch.uint16, torch.float32):
        m = torch.zeros((1, 8, 8), dtype=dt)
        with pytest.raises(ValueError, match="needs color_scale"):
            cdofp.demosaic(m)
        with pytest.raises(ValueError, match="needs color_scale"):
            cdofp.expand({cdofp.KEY: m})
        for kw in ({"color_scale": 255 / 4095}, {"want": ("planes", "rgb_planes")}):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cdofp.demosaic(m, **kw)
    for bad, match in ((torch.zeros((1, 8, 8), dtype=torch.int32), "torch.int32"), (torch.zeros((1, 2, 8, 8)), r"\(1, 2, 8, 8\)"),
                       (torch.zeros((1, 6, 8)), "multiples of 4"), (torch.zeros((1, 8, 2)), "multiples of 4")):
        with pytest.raises(ValueError, match=match):
            cdofp.demosaic(bad, color_scale=1.0)
    with pytest.raises(ValueError, match="'colour'"):
        cdofp.demosaic(torch.zeros((1, 8, 8), dtype=torch.uint8), want=("colour",))


def _tree(root, writer, with_planes=False):
    from PIL import Image
    rng = np.random.default_rng(0)
    scene = root / "scene1_traj1_1" / "polarization"
    dirs = ("pol_cdofp", "_gt", "_instance") + (("rgb", "pol00", "pol01", "pol10", "pol11") if with_planes else ())
    for d in dirs:
        (scene / d).mkdir(parents=True)
    for idx in (3, 4):
        writer(scene / "pol_cdofp" / f"{idx:06d}.png", idx)
        Image.fromarray(rng.integers(300, 1800, (96, 128)).astype(np.uint16)).save(scene / "_gt" / f"{idx:06d}.png")
        Image.fromarray((rng.integers(0, 11, (96, 128)) * 20).astype(np.uint8)).save(scene / "_instance" / f"{idx:06d}.png")
        if with_planes:
            Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(scene / "rgb" / f"{idx:06d}.png")
            for d in ("pol00", "pol01", "pol10", "pol11"):
                Image.fromarray(rng.integers(0, 256, (96, 128), dtype=np.uint8)).save(scene / d / f"{idx:06d}.png")
    (scene / "intrinsics.txt").write_text("80 0 64\n0 82 48\n0 0 1\n")
    return scene


def _mosaic(idx, dtype):
    rng = np.random.default_rng(100 + idx)
    return rng.integers(0, 256 if dtype == np.uint8 else 4096, (192, 256)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_dataset_serves_the_raw_colour_frame(tmp_path, dtype):
    """A tree with pol_cdofp/, _gt/ and no rgb/ or pol*/ folder: the frame arrives as ("pol_cdofp", 0, 0) [1,H4,W4] of the
    file's depth, untouched, with the jitter row of the raw_color draw and intrinsics scaled by the frame's own size."""
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset, color_jitter_params
    from polardepth.color import pack_jitter
    _tree(tmp_path, lambda path, idx: Image.fromarray(_mosaic(idx, dtype)).save(path))
    ds = HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4, pol_cdofp=True)
    assert len(ds) == 2 and ds.pol_cdofp is True
    want = {("pol_cdofp", 0, 0), "color_jitter", "depth", "depth_gt", ("mask", 0, 0), "stereo_T"}
    for s in range(4):
        want |= {("K", s), ("inv_K", s)}
    for i, idx in enumerate((3, 4)):
        it = ds[i]
        assert set(it) == want
        m = it[("pol_cdofp", 0, 0)]
        assert m.dtype == getattr(torch, np.dtype(dtype).name) and m.shape == (1, 192, 256)
        assert np.array_equal(m.numpy()[0], _mosaic(idx, dtype))
        assert it["color_jitter"].dtype == torch.float64 and it["color_jitter"].shape == (8,) and not it["color_jitter"].any()
        # intrinsics.txt is in pixels of the 256 x 192 frame: fx 80 / 256 * 96, cy 48 / 192 * 64
        K = it[("K", 0)].numpy()
        assert np.allclose(K[:2, :3], [[80 / 256 * 96, 0, 64 / 256 * 96], [0, 82 / 192 * 64, 48 / 192 * 64]], rtol=1e-6)
        assert np.allclose(it[("K", 1)].numpy()[:2, :3], K[:2, :3] / 2, rtol=1e-6)
    # a training item draws like a raw_color item: the gate, then the four factors in their shuffled order
    train = HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4, is_train=True, pol_cdofp=True)
    seed = next(k for k in range(64) if random.Random(k).random() > 0.5)
    random.seed(seed)
    row = train[0]["color_jitter"].numpy()
    random.seed(seed)
    assert random.random() > 0.5
    assert row.any() and np.array_equal(row, pack_jitter(color_jitter_params()))
    synth = HAMMER_Dataset("synthetic", ["a"], 64, 96, [0], 4, pol_cdofp=True)[0]            # synthetic items are untouched
    assert ("pol", 0, 0) in synth and ("pol_cdofp", 0, 0) not in synth and "color_jitter" not in synth
    # the tree has neither rgb/ nor pol00 .. pol11: the default loader finds no frame in it
    with pytest.raises(FileNotFoundError, match="pol00/01/10/11"):
        HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4)


def test_dataset_option_defaults_and_refusals(tmp_path, monkeypatch):
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset
    rng = np.random.default_rng(1)
    _tree(tmp_path / "rgbfile", lambda path, idx: Image.fromarray(rng.integers(0, 256, (192, 256, 3), dtype=np.uint8)).save(path))
    ds = HAMMER_Dataset(str(tmp_path / "rgbfile"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_cdofp=True)
    with pytest.raises(ValueError, match=r"pol_cdofp.000003\.png.*'RGB'.*pol_cdofp serves"):
        ds[0]
    scene = _tree(tmp_path / "both", lambda path, idx: Image.fromarray(_mosaic(idx, np.uint16)).save(path), with_planes=True)
    monkeypatch.delenv("PD_POL_CDOFP", raising=False)
    monkeypatch.delenv("PD_POL_DOFP", raising=False)
    plain = HAMMER_Dataset(str(tmp_path / "both"), ["scene1_traj1_1"], 64, 96, [0], 4)
    assert plain.pol_cdofp is False and ("pol", 0, 0) in plain[0] and ("pol_cdofp", 0, 0) not in plain[0]
    monkeypatch.setenv("PD_POL_CDOFP", "1")
    assert ("pol_cdofp", 0, 0) in HAMMER_Dataset(str(tmp_path / "both"), ["scene1_traj1_1"], 64, 96, [0], 4)[0]
    assert HAMMER_Dataset(str(tmp_path / "both"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_cdofp=False).pol_cdofp is False
    with pytest.raises(ValueError, match="choose one"):
        HAMMER_Dataset(str(tmp_path / "both"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_dofp=True)
    monkeypatch.delenv("PD_POL_CDOFP")
    for f in (scene / "pol_cdofp").iterdir():
        f.unlink()
    with pytest.raises(FileNotFoundError, match="pol_cdofp"):
        HAMMER_Dataset(str(tmp_path / "both"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_cdofp=True)


def test_train_maps_the_environment_onto_the_options(monkeypatch):
    """train.py maps the PD_POL_* variables onto the options object the Trainer reads; the mapping itself needs no GPU."""
    import manydepth.train as train_mod
    seen = {}

    class _Stop(Exception):
        pass

    def fake_trainer(opts):
        seen["opts"] = opts
        raise _Stop

    monkeypatch.setattr(train_mod, "Trainer", fake_trainer)
    monkeypatch.setattr("sys.argv", ["train", "--data_path", "synthetic"])
    monkeypatch.setenv("PD_POL_BAYER", "GRBG")
    monkeypatch.setenv("PD_POL_GAINS", "1.5,1,2.25")
    monkeypatch.setenv("PD_POL_COLOR_SCALE", "0.0625")
    with pytest.raises(_Stop):
        train_mod.main()
    o = seen["opts"]
    assert o.pol_bayer == "GRBG" and o.pol_gains == [1.5, 1.0, 2.25] and o.pol_color_scale == 0.0625
    from polardepth import cdofp
    assert cdofp.options(getattr(o, "pol_layout", None), o.pol_bayer, o.pol_gains, o.pol_color_scale) == \
        ((2, 1, 3, 0), (1, 0, 2, 1), (1.5, 1.0, 2.25), 0.0625)
