"""pd_dofp_demosaic, host side (no GPU): every refusal is decided before anything touches the device, the header's constants,
the Python layer's argument checks, and HAMMER_Dataset(pol_dofp=True)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from polardepth import _lib

HEADER = os.path.join(ROOT, "include", "polardepth.h")
IMX = (ctypes.c_int * 4)(2, 1, 3, 0)
U8, U16, F32 = 0, 1, 2
SUPERPIXEL, BILINEAR = 0, 1


def test_header_constants():
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define\s+(PD_\w+)\s+\(?(-?\d+)\)?", src))
    assert defs["PD_DOFP_SUPERPIXEL"] == "0" and defs["PD_DOFP_BILINEAR"] == "1"
    assert (defs["PD_POLAR_U8"], defs["PD_POLAR_U16"], defs["PD_POLAR_F32"]) == ("0", "1", "2")
    assert "pd_dofp_demosaic" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.lib.path), "pd_dofp_demosaic")
    from polardepth import dofp
    assert dofp.IMX250MZR == (2, 1, 3, 0) and dofp.MODES == {"superpixel": SUPERPIXEL, "bilinear": BILINEAR}


def test_argument_validation_needs_no_gpu():
    """Each refusal returns PD_EINVAL (-22) with its message; an empty batch returns 0."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(72)    # 8-byte aligned only

    def call(mosaic=p, dtype=U8, planes=p, mode=BILINEAR, layout=IMX, B=1, H2=8, W2=8):
        return L.pd_dofp_demosaic(mosaic, dtype, planes, mode, layout, B, H2, W2, None)

    assert call(B=0) == 0
    assert call(B=0, mosaic=None, planes=None, layout=None) == 0                    # empty batch: nothing is looked at
    assert call(B=-1) == -22 and b"bad shape" in err()
    for kw in ({"mosaic": None}, {"planes": None}, {"layout": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for dtype in (-1, 3, 7):
        assert call(dtype=dtype) == -22 and b"unknown dtype" in err()
    for mode in (-1, 2):
        assert call(mode=mode) == -22 and b"unknown mode" in err()
    for bad in ((0, 1, 2, 2), (0, 1, 2, 4), (-1, 0, 1, 2), (0, 0, 0, 0), (1, 2, 3, 4)):
        assert call(layout=(ctypes.c_int * 4)(*bad)) == -22 and b"not a permutation" in err(), bad
        assert ("(%d,%d,%d,%d)" % bad).encode() in err()
    for H2, W2 in ((7, 8), (8, 7), (0, 8), (8, 0), (1, 8), (-2, 8), (8, -4)):
        assert call(H2=H2, W2=W2) == -22 and b"even sides" in err(), (H2, W2)
    for mode in (SUPERPIXEL, BILINEAR):
        for kw in ({"mosaic": odd}, {"planes": odd}):
            assert call(mode=mode, **kw) == -22 and b"16-byte aligned" in err(), kw
        assert call(mode=mode, H2=65536, W2=32768) == -22 and b"too large" in err()         # 2^31 pixels in a frame
        assert call(mode=mode, H2=32768, W2=32770) == -22 and b"too large" in err()         # just past 2^30
        assert call(mode=mode, B=2048, H2=32768, W2=32768) == -22 and b"too large" in err()  # 2^41 in the batch
    # legal shapes pass every check up to the launch: uint8 rows of 6 need no alignment of their own (refused only for
    # the reasons above)
    assert call(W2=6, mosaic=odd) == -22 and b"16-byte aligned" in err()


def test_python_layer_names_the_offending_value():
    from polardepth import dofp
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dofp.demosaic(torch.zeros(1, 4, 4, dtype=torch.uint8))
    assert dofp.parse_layout("2,1,3,0") == (2, 1, 3, 0) and dofp.parse_layout([3, 2, 1, 0]) == (3, 2, 1, 0)
    for bad in ("0,1,2,2", (0, 1, 2), "a,b,c,d", (0, 1, 2, 4), 5):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            dofp.parse_layout(bad)
    with pytest.raises(ValueError, match="'nearest'"):
        dofp.options(None, "nearest")
    assert dofp.options() == ((2, 1, 3, 0), "bilinear") and dofp.options("0,1,2,3", "superpixel") == ((0, 1, 2, 3), "superpixel")


def _tree(root, pol_dirs, pol_writer):
    from PIL import Image
    rng = np.random.default_rng(0)
    scene = root / "scene1_traj1_1" / "polarization"
    for d in ("rgb", "_gt", "_instance") + tuple(pol_dirs):
        (scene / d).mkdir(parents=True)
    for idx in (3, 4):
        Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(scene / "rgb" / f"{idx:06d}.png")
        for d in pol_dirs:
            pol_writer(scene / d / f"{idx:06d}.png", idx)
        Image.fromarray(rng.integers(300, 1800, (96, 128)).astype(np.uint16)).save(scene / "_gt" / f"{idx:06d}.png")
        Image.fromarray((rng.integers(0, 11, (96, 128)) * 20).astype(np.uint8)).save(scene / "_instance" / f"{idx:06d}.png")
    (scene / "intrinsics.txt").write_text("80 0 64\n0 82 48\n0 0 1\n")
    return scene


def _mosaic(idx, dtype):
    rng = np.random.default_rng(100 + idx)
    return rng.integers(0, 256 if dtype == np.uint8 else 4096, (192, 256)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_dataset_serves_the_raw_mosaic(tmp_path, dtype):
    """pol_dofp/%06d.png in mode L / I;16 arrives as ("pol_dofp", 0, 0) [1,H2,W2] of the file's depth, untouched; the item has
    no ("pol", 0, 0) and every other key of an ordinary item."""
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset
    _tree(tmp_path, ("pol_dofp",), lambda path, idx: Image.fromarray(_mosaic(idx, dtype)).save(path))
    ds = HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4, pol_dofp=True)
    assert len(ds) == 2
    for i, idx in enumerate((3, 4)):
        it = ds[i]
        m = it[("pol_dofp", 0, 0)]
        assert m.dtype == getattr(torch, np.dtype(dtype).name) and m.shape == (1, 192, 256)
        assert np.array_equal(m.numpy()[0], _mosaic(idx, dtype))
        assert ("pol", 0, 0) not in it
    synth = HAMMER_Dataset("synthetic", ["a"], 64, 96, [0], 4, pol_dofp=True)[0]            # synthetic items are untouched
    assert ("pol", 0, 0) in synth and ("pol_dofp", 0, 0) not in synth
    assert set(ds[0]) - {("pol_dofp", 0, 0)} == set(synth) - {("pol", 0, 0)}
    # the tree has no pol00 .. pol11: the default loader finds no frame in it
    with pytest.raises(FileNotFoundError, match="pol00/01/10/11"):
        HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4)


def test_dataset_refuses_other_modes_and_trees_without_the_folder(tmp_path):
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset
    rng = np.random.default_rng(1)
    _tree(tmp_path / "rgb", ("pol_dofp",),
          lambda path, idx: Image.fromarray(rng.integers(0, 256, (192, 256, 3), dtype=np.uint8)).save(path))
    ds = HAMMER_Dataset(str(tmp_path / "rgb"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_dofp=True)
    with pytest.raises(ValueError, match=r"pol_dofp.000003\.png.*'RGB'"):
        ds[0]
    plain = lambda path, idx: Image.fromarray(rng.integers(0, 256, (96, 128), dtype=np.uint8)).save(path)
    _tree(tmp_path / "planes", ("pol00", "pol01", "pol10", "pol11"), plain)
    with pytest.raises(FileNotFoundError, match="pol_dofp"):
        HAMMER_Dataset(str(tmp_path / "planes"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_dofp=True)


def test_default_constructor_is_unchanged(tmp_path, monkeypatch):
    """An ordinary tree through the default constructor: the keys, dtypes and shapes it has always had; PD_POL_DOFP=1 is the
    default of the new argument and nothing else."""
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset
    rng = np.random.default_rng(2)
    scene = _tree(tmp_path, ("pol00", "pol01", "pol10", "pol11"),
                  lambda path, idx: Image.fromarray(rng.integers(0, 256, (96, 128), dtype=np.uint8)).save(path))
    monkeypatch.delenv("PD_POL_DOFP", raising=False)
    ds = HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4)
    assert ds.pol_dofp is False
    it = ds[0]
    want = {("pol", 0, 0), "depth", "depth_gt", ("mask", 0, 0), "stereo_T"}
    for s in range(4):
        want |= {("color", 0, s), ("color_aug", 0, s), ("K", s), ("inv_K", s)}
    assert set(it) == want
    assert it[("pol", 0, 0)].dtype == torch.uint8 and it[("pol", 0, 0)].shape == (4, 64, 96)
    monkeypatch.setenv("PD_POL_DOFP", "1")
    assert HAMMER_Dataset("synthetic", ["a"], 64, 96, [0], 4).pol_dofp is True
    assert HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4, pol_dofp=False).pol_dofp is False
    (scene / "pol_dofp").mkdir()
    for idx in (3, 4):
        Image.fromarray(_mosaic(idx, np.uint16)).save(scene / "pol_dofp" / f"{idx:06d}.png")
    assert ("pol_dofp", 0, 0) in HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4)[0]
