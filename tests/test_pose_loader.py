"""HAMMER_Dataset(need_poses=False) (no GPU): the loader of the Trainer's pose-network mode on a three-frame HAMMER tree that
ships NO ``_pose/`` folder -- the sequences that mode is for.  A neighbour is present as soon as its picture exists; with the
default ``need_poses=True`` the same tree flags every neighbour as missing, as before."""
import numpy as np
import pytest
import torch
from PIL import Image

from manydepth.datasets import HAMMER_Dataset

H, W, FH, FW = 32, 64, 40, 72


@pytest.fixture()
def tree(tmp_path):
    rng = np.random.default_rng(9)
    folder = tmp_path / "scene_a" / "polarization"
    for sub in ("rgb", "pol00", "pol01", "pol10", "pol11", "_gt", "_instance"):
        (folder / sub).mkdir(parents=True)
    for k in range(3):
        name = f"{k:06d}.png"
        Image.fromarray(rng.integers(1, 256, (FH, FW, 3), dtype=np.uint8), "RGB").save(folder / "rgb" / name)
        for sub in ("pol00", "pol01", "pol10", "pol11", "_instance"):
            Image.fromarray(rng.integers(0, 256, (FH, FW), dtype=np.uint8), "L").save(folder / sub / name)
        Image.fromarray(rng.integers(0, 2500, (FH, FW), dtype=np.uint16)).save(folder / "_gt" / name)
    (folder / "intrinsics.txt").write_text("70.5 0 36.2\n0 71.25 19.9\n0 0 1\n")
    return tmp_path, folder


def _ds(root, **kw):
    return HAMMER_Dataset(str(root), ["scene_a"], H, W, [0, -1, 1], 4, is_train=False, offset=1, lookup_aug=True, **kw)


def test_neighbours_are_present_without_pose_files(tree):
    root, folder = tree
    item = _ds(root, need_poses=False)[1]                              # the middle frame: both neighbours exist
    for i, k in ((-1, 0), (1, 2)):
        assert item[("frame_valid", i)].item() == 1.0
        im = Image.open(folder / "rgb" / f"{k:06d}.png").convert("RGB").resize((W, H), Image.LANCZOS)
        want = np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0
        assert item[("color", i, 0)].numpy().tobytes() == want.tobytes()
        assert item[("color_aug", i, 0)].abs().sum().item() > 0
        assert torch.equal(item[("color_aug", i, 0)], item[("color", i, 0)])          # not a training item: no jitter
        assert torch.equal(item[("poses", i)], torch.eye(4))                            # nothing to read: the identity
    first = _ds(root, need_poses=False)[0]                             # frame -1 of the first frame does not exist
    assert first[("frame_valid", -1)].item() == 0.0 and first[("frame_valid", 1)].item() == 1.0
    assert first[("color_aug", -1, 0)].abs().sum().item() == 0


def test_default_still_needs_both_pose_files(tree):
    root, _ = tree
    item = _ds(root)[1]
    for i in (-1, 1):
        assert item[("frame_valid", i)].item() == 0.0 and item[("color", i, 0)].abs().sum().item() == 0


def test_pose_files_are_still_read_where_they_exist(tree):
    root, folder = tree
    (folder / "_pose").mkdir()
    rng = np.random.default_rng(1)
    for k in range(3):
        T = np.eye(4)
        T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        (folder / "_pose" / f"{k:06d}.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in T))
    a, b = _ds(root, need_poses=False)[1], _ds(root)[1]
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a[("poses", 1)], torch.eye(4))
