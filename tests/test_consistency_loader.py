"""HAMMER_Dataset(neighbour_items=True) (no GPU): a three-frame HAMMER tree in a temporary directory, as
tests/test_reproj_loader.py builds it.  With the switch off an item is what it was; with it on every neighbour also arrives
as its complete single-frame item, and a missing neighbour as a zero item with ``frame_valid`` 0."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from manydepth.datasets import HAMMER_Dataset

H, W, FH, FW = 32, 64, 40, 72
SUBS = ("rgb", "pol00", "pol01", "pol10", "pol11", "_gt", "_instance")


@pytest.fixture()
def tree(tmp_path):
    rng = np.random.default_rng(7)
    folder = tmp_path / "scene_a" / "polarization"
    for sub in SUBS + ("_pose",):
        (folder / sub).mkdir(parents=True)
    for k in range(3):
        name = f"{k:06d}.png"
        Image.fromarray(rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8), "RGB").save(folder / "rgb" / name)
        for sub in ("pol00", "pol01", "pol10", "pol11", "_instance"):
            Image.fromarray(rng.integers(0, 256, (FH, FW), dtype=np.uint8), "L").save(folder / sub / name)
        Image.fromarray(rng.integers(0, 2500, (FH, FW), dtype=np.uint16)).save(folder / "_gt" / name)
        T = np.eye(4)
        T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        (folder / "_pose" / f"{k:06d}.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in T))
    (folder / "intrinsics.txt").write_text("70.5 0 36.2\n0 71.25 19.9\n0 0 1\n")
    return tmp_path, folder


def _ds(root, frame_idxs, **kw):
    return HAMMER_Dataset(str(root), ["scene_a"], H, W, frame_idxs, 4, is_train=False, offset=1, **kw)


def _same(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    for k, v in b.items():
        assert a[k].dtype == v.dtype and a[k].shape == v.shape and a[k].numpy().tobytes() == v.numpy().tobytes(), k


def test_without_the_switch_an_item_is_what_it_was(tree):
    root, _ = tree
    plain, off = _ds(root, [0, -1, 1]), _ds(root, [0, -1, 1], neighbour_items=False)
    single, single_on = _ds(root, [0]), _ds(root, [0], neighbour_items=True)
    for k in range(3):
        _same(off[k], plain[k])
        assert not any(isinstance(key, tuple) and key[0] == "neighbour" for key in off[k])
        _same(single_on[k], single[k])                       # no neighbours, nothing to add


def test_the_nested_item_is_the_single_frame_item_of_the_neighbour(tree):
    root, _ = tree
    on, plain, single = _ds(root, [0, -1, 1], neighbour_items=True), _ds(root, [0, -1, 1]), _ds(root, [0])
    for k in range(3):
        item = on[k]
        nested = {key: item.pop(key) for key in [("neighbour", -1), ("neighbour", 1)]}
        _same(item, plain[k])                                # everything else is untouched
        for i in (-1, 1):
            o = k + i
            if 0 <= o < 3:
                assert float(item[("frame_valid", i)]) == 1.0
                _same(nested[("neighbour", i)], single[o])
            else:                                            # a missing neighbour: the zero item
                assert float(item[("frame_valid", i)]) == 0.0
                z = nested[("neighbour", i)]
                assert set(z) == set(single[k])
                for key, v in single[k].items():
                    assert z[key].dtype == v.dtype and z[key].shape == v.shape and not z[key].any(), key
    batch = torch.utils.data.default_collate([on[0], on[1]])
    assert batch[("neighbour", 1)]["depth_gt"].shape == (2, 1, H, W) and batch[("neighbour", -1)][("K", 0)].shape == (2, 4, 4)
    assert batch[("neighbour", -1)][("pol", 0, 0)].dtype == torch.uint8 and batch[("frame_valid", -1)].tolist() == [0.0, 1.0]


def test_an_incomplete_or_poseless_neighbour_is_the_zero_item(tree):
    root, folder = tree
    os.remove(folder / "_gt" / "000002.png")                 # frame 2 keeps its picture and pose but is no complete frame
    on = _ds(root, [0, -1, 1], neighbour_items=True)
    assert len(on) == 2
    item = on[1]
    assert float(item[("frame_valid", 1)]) == 0.0 and not item[("neighbour", 1)]["depth_gt"].any()
    assert float(_ds(root, [0, -1, 1])[1][("frame_valid", 1)]) == 1.0        # without the switch the picture decides, as before
    os.remove(folder / "_pose" / "000000.txt")
    item = _ds(root, [0, -1, 1], neighbour_items=True)[1]
    assert float(item[("frame_valid", -1)]) == 0.0 and not item[("neighbour", -1)][("color", 0, 0)].any()


def test_synthetic_items_gain_the_same_keys_and_keep_everything_else():
    kw = dict(is_train=False)
    one = HAMMER_Dataset("synthetic", [], 32, 64, [0], 4, **kw)
    plain = HAMMER_Dataset("synthetic", [], 32, 64, [0, -1, 1], 4, **kw)
    on = HAMMER_Dataset("synthetic", [], 32, 64, [0, -1, 1], 4, neighbour_items=True, **kw)
    for idx in (0, 5):
        item = on[idx]
        again = on[idx]
        nested = {key: item.pop(key) for key in [("neighbour", -1), ("neighbour", 1)]}
        _same(item, plain[idx])
        for i in (-1, 1):
            n = nested[("neighbour", i)]
            assert set(n) == set(one[idx])
            for key, v in one[idx].items():
                assert n[key].dtype == v.dtype and n[key].shape == v.shape, key
            _same(n, again[("neighbour", i)])                # seeded
            assert not torch.equal(n[("color", 0, 0)], item[("color", 0, 0)])
            d = n["depth_gt"]
            assert 0.25 < d[d > 0].min() and d.max() < 1.85 and 0.05 < (d == 0).float().mean() < 0.15
