"""HAMMER_Dataset with neighbouring frames (no GPU): a three-frame HAMMER tree in a temporary directory.  The relative poses
equal the NumPy formula of hammer_dataset.py:104-132 bit for bit, the end frames' missing neighbours are flagged, and with
``frame_idxs=[0]`` an item is exactly what the single-frame loader has always returned -- compared against values the test
derives from the files itself."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from manydepth.datasets import HAMMER_Dataset

H, W, FH, FW = 32, 64, 40, 72
SUBS = ("rgb", "pol00", "pol01", "pol10", "pol11", "_gt", "_instance")


def _pose(rng):
    a = rng.uniform(-0.2, 0.2, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rx @ Ry @ Rz, rng.uniform(-0.5, 0.5, 3)
    return T


@pytest.fixture()
def tree(tmp_path):
    rng = np.random.default_rng(7)
    folder = tmp_path / "scene_a" / "polarization"
    for sub in SUBS + ("_pose",):
        (folder / sub).mkdir(parents=True)
    poses = []
    for k in range(3):
        name = f"{k:06d}.png"
        Image.fromarray(rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8), "RGB").save(folder / "rgb" / name)
        for sub in ("pol00", "pol01", "pol10", "pol11", "_instance"):
            Image.fromarray(rng.integers(0, 256, (FH, FW), dtype=np.uint8), "L").save(folder / sub / name)
        Image.fromarray(rng.integers(0, 2500, (FH, FW), dtype=np.uint16)).save(folder / "_gt" / name)
        poses.append(_pose(rng))
        (folder / "_pose" / f"{k:06d}.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in poses[-1]))
    (folder / "intrinsics.txt").write_text("70.5 0 36.2\n0 71.25 19.9\n0 0 1\n")
    return tmp_path, folder, poses


def _ds(root, frame_idxs, **kw):
    return HAMMER_Dataset(str(root), ["scene_a"], H, W, frame_idxs, 4, is_train=False, offset=1, **kw)


def _expected_single_frame_item(folder, k):
    """What the single-frame loader returns for frame k, derived here from the files (datasets/__init__.py as it stood)."""
    name = f"{k:06d}.png"
    to_t = lambda im: np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0
    want = {}
    prev = Image.open(folder / "rgb" / name).convert("RGB")
    for s in range(4):
        prev = prev.resize((W >> s, H >> s), Image.LANCZOS)
        want[("color", 0, s)] = to_t(prev)
        want[("color_aug", 0, s)] = to_t(prev)
    want[("pol", 0, 0)] = np.stack([np.asarray(Image.open(folder / d / name).convert("L").resize((W, H), Image.LANCZOS))
                                    for d in ("pol00", "pol01", "pol10", "pol11")]).astype(np.uint8)
    depth = (np.asarray(Image.open(folder / "_gt" / name).resize((W, H), Image.NEAREST)).astype(np.uint16) / 1000).astype(np.float32)
    want["depth"] = want["depth_gt"] = depth[None]
    want[("mask", 0, 0)] = np.asarray(Image.open(folder / "_instance" / name).convert("L").resize((W, H), Image.NEAREST)).astype(np.int32)[None]
    K0 = np.eye(4, dtype=np.float32)
    K0[:3, :3] = np.array("70.5 0 36.2 0 71.25 19.9 0 0 1".split(), dtype=np.float32).reshape(3, 3)
    K0[0, :] /= FW
    K0[1, :] /= FH
    for s in range(4):
        K = K0.copy()
        K[0, :] *= W // (2 ** s)
        K[1, :] *= H // (2 ** s)
        want[("K", s)] = K
        want[("inv_K", s)] = np.linalg.pinv(K)
    st = np.eye(4, dtype=np.float32)
    st[0, 3] = -0.0498921
    want["stereo_T"] = st
    return want


def _same(item, want):
    assert set(item) == set(want), set(item) ^ set(want)
    for k, v in want.items():
        got = item[k].numpy()
        assert got.dtype == v.dtype and got.shape == v.shape and got.tobytes() == v.tobytes(), k


def test_single_frame_items_keep_every_key_and_byte(tree):
    root, folder, _ = tree
    ds = _ds(root, [0])
    assert len(ds) == 3
    for k in range(3):
        _same(ds[k], _expected_single_frame_item(folder, k))


def test_neighbours_poses_and_validity(tree):
    root, folder, poses = tree
    ds = _ds(root, [0, -1, 1])
    single = _ds(root, [0])
    extra = {("color", -1, 0), ("color", 1, 0), ("poses", -1), ("poses", 1), ("frame_valid", -1), ("frame_valid", 1)}
    for k in range(3):
        item, base = ds[k], single[k]
        assert set(item) == set(base) | extra
        for key, v in base.items():                       # frame 0 is untouched by the neighbours
            assert item[key].numpy().tobytes() == v.numpy().tobytes(), key
        for i in (-1, 1):
            o = k + i
            ok = 0 <= o < 3
            assert item[("frame_valid", i)].dtype == torch.float32 and item[("frame_valid", i)].shape == ()
            assert float(item[("frame_valid", i)]) == (1.0 if ok else 0.0), (k, i)
            pose, color = item[("poses", i)].numpy(), item[("color", i, 0)].numpy()
            assert pose.dtype == np.float32 and pose.shape == (4, 4) and color.dtype == np.float32 and color.shape == (3, H, W)
            if ok:
                want = np.linalg.inv(np.linalg.inv(poses[k]) @ poses[o]).astype(np.float32)
                assert pose.tobytes() == want.tobytes(), (k, i)
                im = Image.open(folder / "rgb" / f"{o:06d}.png").convert("RGB").resize((W, H), Image.LANCZOS)
                assert color.tobytes() == (np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0).tobytes()
                assert color.tobytes() == single[o][("color", 0, 0)].numpy().tobytes()
            else:
                assert (color == 0).all() and np.array_equal(pose, np.eye(4, dtype=np.float32))
    # the pose takes frame 0's camera coordinates to the neighbour's: a world point seen from both
    X = np.array([0.3, -0.2, 2.0, 1.0])
    p0, p1 = np.linalg.inv(poses[1]) @ X, np.linalg.inv(poses[2]) @ X
    assert np.allclose(ds[1][("poses", 1)].numpy().astype(np.float64) @ p0, p1, atol=1e-6)
    # a neighbour whose pose file is missing is as good as a missing neighbour
    os.remove(folder / "_pose" / "000002.txt")
    item = _ds(root, [0, -1, 1])[1]
    assert float(item[("frame_valid", 1)]) == 0.0 and float(item[("frame_valid", -1)]) == 1.0
    assert (item[("color", 1, 0)] == 0).all() and torch.equal(item[("poses", 1)], torch.eye(4))
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert batch[("frame_valid", -1)].tolist() == [0.0, 1.0] and batch[("poses", 1)].shape == (2, 4, 4)


def test_offset_selects_the_neighbour(tree):
    root, _, poses = tree
    ds = HAMMER_Dataset(str(root), ["scene_a"], H, W, [0, -1, 1], 4, is_train=False, offset=2)
    item = ds[0]
    assert float(item[("frame_valid", 1)]) == 1.0 and float(item[("frame_valid", -1)]) == 0.0
    want = np.linalg.inv(np.linalg.inv(poses[0]) @ poses[2]).astype(np.float32)
    assert item[("poses", 1)].numpy().tobytes() == want.tobytes()
    assert float(ds[1][("frame_valid", 1)]) == 0.0 and float(ds[1][("frame_valid", -1)]) == 0.0


def test_raw_color_applies_to_frame_zero_only_and_cdofp_refuses_neighbours(tree):
    root, _, _ = tree
    item = _ds(root, [0, 1], raw_color=True)[0]
    assert ("color_raw", 0, 0) in item and ("color", 0, 0) not in item
    assert item[("color", 1, 0)].shape == (3, H, W) and float(item[("frame_valid", 1)]) == 1.0
    with pytest.raises(ValueError, match="pol_cdofp"):
        _ds(root, [0, -1, 1], pol_cdofp=True)


def test_synthetic_items_gain_seeded_smooth_neighbours_and_keep_frame_zero():
    kw = dict(is_train=False)
    one = HAMMER_Dataset("synthetic", [], 32, 64, [0], 4, **kw)
    three = HAMMER_Dataset("synthetic", [], 32, 64, [0, -1, 1], 4, **kw)
    for idx in (0, 5):
        a, b = one[idx], three[idx]
        assert set(b) == set(a) | {("color", -1, 0), ("color", 1, 0), ("poses", -1), ("poses", 1), ("frame_valid", -1),
                                   ("frame_valid", 1)}
        for k, v in a.items():
            assert b[k].numpy().tobytes() == v.numpy().tobytes(), k
        assert all(torch.equal(three[idx][k], b[k]) for k in b)                       # seeded
        for i in (-1, 1):
            c, T = b[("color", i, 0)], b[("poses", i)].double()
            assert c.dtype == torch.float32 and c.shape == (3, 32, 64) and 0 <= c.min() and c.max() <= 1
            assert (c[:, :, 1:] - c[:, :, :-1]).abs().mean() < 0.05 < (a[("color", 0, 0)][:, :, 1:] - a[("color", 0, 0)][:, :, :-1]).abs().mean()
            assert torch.allclose(T[:3, :3] @ T[:3, :3].T, torch.eye(3, dtype=torch.float64), atol=1e-6)      # rigid (fp32 storage)
            assert 0 < T[:3, 3].norm() < 0.1 and float(b[("frame_valid", i)]) == 1.0
