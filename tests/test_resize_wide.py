"""LANCZOS resize of 16-bit and float polarizer planes, host side (no GPU): the NumPy restatement of Pillow's I;16 / F
arithmetic (tests/resize_wide_ref.py) against ``Image.resize(..., Image.LANCZOS)`` bit for bit, the double coefficient tables
of polardepth/resize.py against the restatement's, the argument checks of pd_resize_wide_pass, and the loader's
``pol_native`` hand-over on a temporary tree of 16-bit PNGs.

NaN and infinity are not compared: they follow IEEE through ``ss += in * k`` (a non-finite sample reaches every output whose
window holds it, also through a zero coefficient) and the inputs here are finite, |x| <= 1e4."""
import ctypes

import numpy as np
import pytest
import torch

import resize_wide_ref as R


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("case", R.CASES)
def test_restatement_equals_pillow_bit_for_bit(case, dtype):
    p = R.planes(case, dtype)
    got, stats = R.restate(p, case[2:4])
    ref = R.pil_planes(case, dtype)
    assert got.dtype == ref.dtype and got.shape == ref.shape == (2, 4) + case[2:4]
    print(f"{case} {dtype}: overshoots {stats['over']}  undershoots {stats['under']}")
    np.testing.assert_array_equal(R.bits(got), R.bits(ref))
    if dtype == "uint16" and case[4] == 65536:
        # the bytewise store is under test only if the sums really leave [0, 65535] on these inputs
        assert stats["over"] >= 1 and stats["under"] >= 1, stats
        assert (ref >= 0xff00).any() and (ref == 0).any()
    if dtype == "float32":
        assert (p < 0).any() and (p != np.trunc(p)).any() and np.isfinite(got).all()


def test_overshoot_wraps_the_low_byte_and_undershoot_is_zero():
    """The rule in numbers, on the restatement's store alone: 65836 = 0x1012c -> high byte clips to 255, low byte 0x2c stays."""
    st = {}
    ss = np.array([65836.0, 65535.4, 65535.5, -0.4, -0.6, -300.0, 4095.5, 255.49])
    np.testing.assert_array_equal(R._store(ss, np.uint16, st), np.array([0xff2c, 65535, 0xff00, 0, 0, 0, 4096, 255], np.uint16))
    assert st == {"over": 2, "under": 2}


@pytest.mark.parametrize("sizes", sorted({(c[1], c[3]) for c in R.CASES} | {(c[0], c[2]) for c in R.CASES} | {(1088, 612), (832, 512)}))
def test_double_tables_equal_the_restatement_and_share_the_integer_bounds(sizes):
    from polardepth import resize as pdresize
    kk, bounds = pdresize.lanczos_coeffs_f64(*sizes)
    rk, rb = R.coeffs(*sizes)
    assert kk.dtype == np.float64 and bounds.dtype == np.int32 and kk.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(kk.view(np.uint64), rk.view(np.uint64))
    np.testing.assert_array_equal(bounds, rb)
    ik, ib = pdresize.lanczos_coeffs(*sizes)
    np.testing.assert_array_equal(bounds, ib)
    assert ik.shape == kk.shape and ik.dtype == np.int32
    # every window lies inside the input and the table row
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= sizes[0]).all() and (bounds[:, 1] <= kk.shape[1]).all()


def test_resize_lanczos_refuses_other_dtypes_and_host_tensors():
    from polardepth import resize as pdresize
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdresize.resize_lanczos(torch.zeros((4, 8, 8), dtype=torch.float32), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdresize.resize_lanczos(np.zeros((4, 8, 8), np.uint16), (4, 4))


def test_argument_validation_of_the_wide_pass_needs_no_gpu():
    """Every refusal of pd_resize_wide_pass is decided before anything touches the device: PD_EINVAL (-22) with a message;
    an empty batch returns 0."""
    from polardepth import _lib
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, aligned dummy: never dereferenced on these paths
    U16, F32 = 1, 2

    def call(src=p, dst=p, dtype=U16, coeffs=p, bounds=p, ksize=7, P=1, Hs=8, Ws=8, out=4, vertical=0):
        return L.pd_resize_wide_pass(src, dst, dtype, coeffs, bounds, ksize, P, Hs, Ws, out, vertical, None)

    assert call(P=0, src=None, dst=None, coeffs=None, bounds=None) == 0
    for kw in ({"P": -1}, {"Hs": 0}, {"Ws": 0}, {"out": 0}, {"ksize": 0}, {"Hs": -3, "vertical": 1}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    for dt in (0, 3, -1):                                    # PD_POLAR_U8 has its own entry point
        assert call(dtype=dt) == -22 and b"dtype" in err(), dt
    for name in ("src", "dst", "coeffs", "bounds"):
        for dt in (U16, F32):
            assert call(dtype=dt, **{name: None}) == -22 and b"null pointer" in err(), name
    assert call(dtype=U16, src=ctypes.c_void_p(65)) == -22 and b"aligned" in err()
    assert call(dtype=F32, dst=ctypes.c_void_p(66)) == -22 and b"aligned" in err()
    assert call(coeffs=ctypes.c_void_p(68)) == -22 and b"aligned" in err()


def _write_tree(tmp_path, pol_arrays):
    """one HAMMER frame (96x128) whose four polarizer files hold `pol_arrays`"""
    from PIL import Image
    rng = np.random.default_rng(1)
    scene = tmp_path / "scene1_traj1_1" / "polarization"
    for d in ("rgb", "pol00", "pol01", "pol10", "pol11", "_gt"):
        (scene / d).mkdir(parents=True)
    Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(scene / "rgb" / "000003.png")
    for d, a in zip(("pol00", "pol01", "pol10", "pol11"), pol_arrays):
        Image.fromarray(a).save(scene / d / "000003.png")
    Image.fromarray(rng.integers(300, 1800, (96, 128)).astype(np.uint16)).save(scene / "_gt" / "000003.png")
    (scene / "intrinsics.txt").write_text("80 0 64\n0 82 48\n0 0 1\n")
    return scene


def test_loader_keeps_the_depth_of_16_bit_polarizer_files(tmp_path, monkeypatch):
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset
    monkeypatch.delenv("PD_POL_NATIVE", raising=False)
    monkeypatch.delenv("PD_DEVICE_RESIZE", raising=False)
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 4096, (4, 96, 128)).astype(np.uint16)          # 12-bit frames
    raw[:, :8, :8] = 200                                                 # a corner below 256: survives convert("L")
    _write_tree(tmp_path, raw)
    mk = lambda **kw: HAMMER_Dataset(str(tmp_path), ["scene1_traj1_1"], 64, 96, [0], 4, **kw)
    # default: today's convert("L"), which clips a 16-bit file at 255
    it = mk()[0]
    assert it[("pol", 0, 0)].dtype == torch.uint8 and it[("pol", 0, 0)].shape == (4, 64, 96)
    clipped = np.minimum(raw, 255).astype(np.uint8)
    host = np.stack([np.asarray(Image.fromarray(clipped[c], "L").resize((96, 64), Image.LANCZOS)) for c in range(4)])
    np.testing.assert_array_equal(it[("pol", 0, 0)].numpy(), host)
    it = mk(raw_pol=True)[0]
    assert it[("pol", 0, 0)].dtype == torch.uint8
    np.testing.assert_array_equal(it[("pol", 0, 0)].numpy(), clipped)
    # pol_native: uint16, PIL's I;16 resize in the worker ...
    it = mk(pol_native=True)[0]
    assert it[("pol", 0, 0)].dtype == torch.uint16 and it[("pol", 0, 0)].shape == (4, 64, 96)
    ref = np.stack([R.pil_resize(raw[c], (64, 96)) for c in range(4)])
    np.testing.assert_array_equal(it[("pol", 0, 0)].numpy(), ref)
    assert ref.max() > 255
    # ... or the raw frame for the device resize
    it = mk(pol_native=True, raw_pol=True)[0]
    assert it[("pol", 0, 0)].dtype == torch.uint16
    np.testing.assert_array_equal(it[("pol", 0, 0)].numpy(), raw)
    # default collation stacks such items
    batch = torch.utils.data.default_collate([it, it])
    assert batch[("pol", 0, 0)].dtype == torch.uint16 and batch[("pol", 0, 0)].shape == (2, 4, 96, 128)
    # the environment switch is read in the constructor
    monkeypatch.setenv("PD_POL_NATIVE", "1")
    assert mk().pol_native and mk()[0][("pol", 0, 0)].dtype == torch.uint16 and not mk(pol_native=False).pol_native
    monkeypatch.delenv("PD_POL_NATIVE")
    assert not mk().pol_native
    # synthetic items are untouched
    s = HAMMER_Dataset("synthetic", ["a"], 64, 96, [0], 4, pol_native=True)[0]
    assert s[("pol", 0, 0)].dtype == torch.uint8


def test_loader_native_modes_l_and_f_and_refusals(tmp_path):
    from PIL import Image
    from manydepth.datasets import HAMMER_Dataset
    rng = np.random.default_rng(3)
    mk = lambda root, **kw: HAMMER_Dataset(str(root), ["scene1_traj1_1"], 64, 96, [0], 4, pol_native=True, **kw)
    # 8-bit files stay uint8 and equal the default path
    a8 = rng.integers(0, 256, (4, 96, 128), dtype=np.uint8)
    _write_tree(tmp_path / "l", a8)
    it = mk(tmp_path / "l")[0]
    dflt = HAMMER_Dataset(str(tmp_path / "l"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_native=False)[0]
    assert it[("pol", 0, 0)].dtype == torch.uint8 and torch.equal(it[("pol", 0, 0)], dflt[("pol", 0, 0)])
    # float files (TIFF holds mode F; the loader looks the polarizer planes up as .png names, so write them under that name)
    af = rng.uniform(-50.0, 4000.0, (4, 96, 128)).astype(np.float32)
    scene = _write_tree(tmp_path / "f", a8)
    for d, a in zip(("pol00", "pol01", "pol10", "pol11"), af):
        Image.fromarray(a).save(scene / d / "000003.png", format="TIFF")
    it = mk(tmp_path / "f")[0]
    assert it[("pol", 0, 0)].dtype == torch.float32
    ref = np.stack([R.pil_resize(af[c], (64, 96)) for c in range(4)])
    np.testing.assert_array_equal(R.bits(it[("pol", 0, 0)].numpy()), R.bits(ref))
    np.testing.assert_array_equal(R.bits(mk(tmp_path / "f", raw_pol=True)[0][("pol", 0, 0)].numpy()), R.bits(af))
    # four planes of differing modes: the error names the file
    scene = _write_tree(tmp_path / "mixed", [a8[0], a8[1], a8[2].astype(np.uint16) * 16, a8[3]])
    with pytest.raises(ValueError, match=r"pol10.000003\.png.*one mode"):
        mk(tmp_path / "mixed")[0]
    # a mode K1 has no element type for
    scene = _write_tree(tmp_path / "rgb", a8)
    Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(scene / "pol01" / "000003.png")
    with pytest.raises(ValueError, match=r"pol01.000003\.png.*'RGB'"):
        mk(tmp_path / "rgb")[0]
    # without pol_native such a tree loads as before (everything goes through convert("L"))
    assert HAMMER_Dataset(str(tmp_path / "mixed"), ["scene1_traj1_1"], 64, 96, [0], 4, pol_native=False)[0][("pol", 0, 0)].dtype == torch.uint8
