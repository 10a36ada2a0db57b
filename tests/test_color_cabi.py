"""The colour path's host side, no GPU: pd_color_jitter_u8 is exported, declared and refuses bad arguments before anything
touches a device; pack_jitter's row layout; HAMMER_Dataset(raw_color=True) hands over the decoded frame and the jitter row
and consumes the ``random`` stream exactly as the PIL path does."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from conftest import ROOT

from polardepth import _lib
from polardepth import color as pdcolor

from color_cases import make_hammer_tree, dataset as _ds, gate_seeds as _seeds

EINVAL = -22


def test_symbol_is_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "polardepth.h")).read()
    assert "int pd_color_jitter_u8(const void* src, const void* params, void* dst_u8, void* dst_f32, void* sum_ws" in header
    assert hasattr(ctypes.CDLL(_lib.lib.path), "pd_color_jitter_u8")
    res, args = _lib.SIGNATURES["pd_color_jitter_u8"]
    assert res is ctypes.c_int and len(args) == 9


def test_bad_arguments_are_refused_without_a_device():
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(64)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    f = L.pd_color_jitter_u8
    assert f(None, None, p, p, None, 1, 4, 4, None) == EINVAL and b"pd_color_jitter_u8: null src" in err()
    assert f(p, None, None, None, None, 1, 4, 4, None) == EINVAL and b"both outputs are null" in err()
    assert f(p, p, None, None, p, 1, 4, 4, None) == EINVAL and b"both outputs are null" in err()
    assert f(p, None, p, p, None, -1, 4, 4, None) == EINVAL and b"bad shape" in err()
    for H, W in ((0, 4), (4, 0), (-3, 4), (4, -1)):
        assert f(p, None, p, p, None, 1, H, W, None) == EINVAL and b"bad shape" in err(), (H, W)
        assert f(p, None, p, p, None, 0, H, W, None) == EINVAL, (H, W)          # refused before the empty batch returns
    assert f(p, p, p, p, None, 1, 4, 4, None) == EINVAL and b"sum_ws" in err()   # a jitter needs its workspace
    assert f(p, ctypes.c_void_p(68), p, p, p, 1, 4, 4, None) == EINVAL and b"8-byte aligned" in err()
    assert f(None, None, None, None, None, 0, 4, 4, None) == 0                   # empty batch: nothing launched
    assert f(p, p, p, None, p, 0, 1, 1, None) == 0


def test_python_layer_has_no_cpu_fallback_and_checks_shapes():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdcolor.color_jitter_u8(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdcolor.color_pyramid(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), None, (4, 4), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdcolor.color_jitter_u8(torch.zeros(1, 3, 4, 4), None)


def test_pack_jitter_round_trips_codes_and_values():
    from manydepth import datasets
    assert pdcolor.CODES == {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4}
    z = pdcolor.pack_jitter(None)
    assert z.dtype == np.float64 and z.shape == (8,) and not z.any()
    names = {v: k for k, v in pdcolor.CODES.items()}
    orders = set()
    for seed in range(20):
        random.seed(seed)
        params = datasets.color_jitter_params()
        row = pdcolor.pack_jitter(params)
        assert row.dtype == np.float64 and row.shape == (8,)
        back = [(names[int(row[2 * k])], row[2 * k + 1]) for k in range(4)]
        assert back == params                       # the factors travel as the doubles they were drawn as
        orders.add(tuple(n for n, _ in params))
    assert len(orders) > 4
    short = pdcolor.pack_jitter([("hue", -0.037)])
    np.testing.assert_array_equal(short, [4, -0.037, 0, 0, 0, 0, 0, 0])
    with pytest.raises(KeyError):
        pdcolor.pack_jitter([("sharpness", 1.0)])


@pytest.fixture(scope="module")
def hammer_tree(tmp_path_factory):
    return make_hammer_tree(tmp_path_factory.mktemp("hammer"))


def test_raw_color_items_carry_the_frame_and_the_jitter_row(hammer_tree):
    from PIL import Image
    host, raw = _ds(hammer_tree, is_train=True), _ds(hammer_tree, is_train=True, raw_color=True)
    assert host.raw_color is False and raw.raw_color is True
    random.seed(0)
    it = raw[0]
    assert not [k for k in it if isinstance(k, tuple) and k[0] in ("color", "color_aug")]
    frame = it[("color_raw", 0, 0)]
    assert frame.dtype == torch.uint8 and frame.shape == (3, 96, 128) and frame.is_contiguous()
    png = np.asarray(Image.open(hammer_tree / "scene1_traj1_1" / "polarization" / "rgb" / "000003.png").convert("RGB"))
    np.testing.assert_array_equal(frame.numpy(), png.transpose(2, 0, 1))
    assert it["color_jitter"].dtype == torch.float64 and it["color_jitter"].shape == (8,)
    random.seed(0)
    h = host[0]
    assert set(h) - set(it) == {(n, 0, s) for n in ("color", "color_aug") for s in range(4)}
    assert set(it) - set(h) == {("color_raw", 0, 0), "color_jitter"}
    for k in set(h) & set(it):                       # polarizer planes, depth, mask, intrinsics: untouched
        assert torch.equal(h[k], it[k]), k
    batch = torch.utils.data.default_collate([raw[0], raw[1]])
    assert batch[("color_raw", 0, 0)].shape == (2, 3, 96, 128) and batch["color_jitter"].shape == (2, 8)


def test_raw_color_draws_from_random_like_the_host_path(hammer_tree):
    from manydepth import datasets
    host, raw = _ds(hammer_tree, is_train=True), _ds(hammer_tree, is_train=True, raw_color=True)
    aug, plain = _seeds()
    for seed, augmented in ((aug, True), (plain, False)):
        random.seed(seed)
        host[1]
        after_host = random.random()
        random.seed(seed)
        row = raw[1]["color_jitter"].numpy()
        assert random.random() == after_host, seed
        random.seed(seed)                            # the host draw, restated: the gate, then one get_params
        assert (random.random() > 0.5) == augmented
        want = pdcolor.pack_jitter(datasets.color_jitter_params() if augmented else None)
        np.testing.assert_array_equal(row, want)
        assert bool(row.any()) == augmented


def test_evaluation_items_carry_a_zero_row(hammer_tree):
    aug, _ = _seeds()
    ds = _ds(hammer_tree, is_train=False, raw_color=True)
    random.seed(aug)
    it = ds[0]
    assert not it["color_jitter"].any() and it[("color_raw", 0, 0)].shape == (3, 96, 128)
    random.seed(aug)
    first = random.random()
    random.seed(aug)
    ds[0]
    assert random.random() == first                  # and draw nothing


def test_switch_defaults_to_the_environment_variable(hammer_tree, monkeypatch):
    monkeypatch.delenv("PD_DEVICE_COLOR", raising=False)
    assert _ds(hammer_tree).raw_color is False
    monkeypatch.setenv("PD_DEVICE_COLOR", "1")
    assert _ds(hammer_tree).raw_color is True and _ds(hammer_tree, raw_color=False).raw_color is False
    from manydepth.datasets import HAMMER_Dataset
    s = HAMMER_Dataset("synthetic", ["a"], 64, 96, [0], 4, raw_color=True)[0]      # synthetic items are untouched
    assert ("color", 0, 0) in s and ("color_raw", 0, 0) not in s and "color_jitter" not in s
