"""Shared pieces of the colour-path tests (test_color_cabi.py, test_color_gpu.py): the temporary HAMMER tree, the PIL
references and the seeds of an augmented and of a plain item.  The oracle is Pillow as installed, through
``manydepth.datasets.apply_color_jitter`` and ``Image.resize(..., LANCZOS)``."""
import random

import numpy as np


def make_hammer_tree(root):
    """Two 96x128 frames (3 and 4) of scene1_traj1_1 under ``root``: the recipe of test_host_logic's loader test."""
    from PIL import Image
    rng = np.random.default_rng(0)
    scene = root / "scene1_traj1_1" / "polarization"
    for d in ("rgb", "pol00", "pol01", "pol10", "pol11", "_gt", "_instance"):
        (scene / d).mkdir(parents=True)
    for idx in (3, 4):
        Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)).save(scene / "rgb" / f"{idx:06d}.png")
        for d in ("pol00", "pol01", "pol10", "pol11"):
            Image.fromarray(rng.integers(0, 256, (96, 128), dtype=np.uint8)).save(scene / d / f"{idx:06d}.png")
        Image.fromarray(rng.integers(300, 1800, (96, 128)).astype(np.uint16)).save(scene / "_gt" / f"{idx:06d}.png")
        Image.fromarray((rng.integers(0, 11, (96, 128)) * 20).astype(np.uint8)).save(scene / "_instance" / f"{idx:06d}.png")
    (scene / "intrinsics.txt").write_text("80 0 64\n0 82 48\n0 0 1\n")
    return root


def dataset(root, **kw):
    from manydepth.datasets import HAMMER_Dataset
    return HAMMER_Dataset(str(root), ["scene1_traj1_1"], 64, 96, [0], 4, **kw)


def gate_seeds():
    """(first seed whose item is augmented, first seed whose item is plain): the loader's gate is random() > 0.5."""
    aug = plain = None
    for k in range(64):
        random.seed(k)
        if random.random() > 0.5:
            aug = k if aug is None else aug
        else:
            plain = k if plain is None else plain
    assert aug is not None and plain is not None
    return aug, plain


def pil_jitter(chw, params):
    """uint8 [3,H,W] -> uint8 [3,H,W] through PIL; params as color_jitter_params() returns them (None / [] = copy)."""
    from PIL import Image
    from manydepth import datasets
    img = Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0)))
    return np.asarray(datasets.apply_color_jitter(img, params or [])).transpose(2, 0, 1)


def to_t(hwc_u8):
    """The loader's to_t (manydepth/datasets: float32 of the bytes, transposed, / 255.0)."""
    return np.asarray(hwc_u8, dtype=np.float32).transpose(2, 0, 1) / 255.0


def pil_pyramid(frame_chw, params, size, num_scales=4):
    """The host loader's colour loop on one frame: successive LANCZOS resizes, jitter of every scale, to_t."""
    from PIL import Image
    from manydepth import datasets
    H, W = size
    prev = Image.fromarray(np.ascontiguousarray(frame_chw.transpose(1, 2, 0)))
    out = {}
    for s in range(num_scales):
        prev = prev.resize((W >> s, H >> s), Image.LANCZOS)
        out[("color", 0, s)] = to_t(prev)
        out[("color_aug", 0, s)] = to_t(datasets.apply_color_jitter(prev, params)) if params else out[("color", 0, s)]
    return out
