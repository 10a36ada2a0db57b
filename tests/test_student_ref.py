"""tests/student_ref.py (the NumPy restatement of csrc/student.hip) against fixture G14 -- the reference's own
compute_matching_mask, the is_multi branch of compute_losses, update_adaptive_depth_bins and compute_depth_bins, run on the
CPU by tests/golden/make_golden_student.py -- and the loader's opt-in ``lookup_aug`` keys.  No GPU.

Masks are exact.  Bins are bit-equal to polardepth.matching.depth_bins of the fixture's tracker values.  Losses: the reference
sums in fp32 in torch's order, student_ref in fp64; the bound is 4 x the difference the generator recorded, with a floor of
2^-20 relative for that fp32 summation."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN

import student_ref as S
from manydepth.datasets import HAMMER_Dataset, apply_color_jitter, color_jitter_params

CASES = {"mm": dict(motion_masking=True, avg=False), "nomm": dict(motion_masking=False, avg=False),
         "avg": dict(motion_masking=True, avg=True)}


@pytest.fixture(scope="module")
def g14():
    return dict(np.load(os.path.join(GOLDEN, "g14_student.npz")))


def test_masks_are_the_references_exactly(g14):
    for case, kw in CASES.items():
        m = S.masks(g14["lowest"], g14["confidence"], g14["mono_depth"], g14["aug"], kw["motion_masking"])
        assert np.array_equal(m["lowest_up"], g14["lowest_up"])                  # F.interpolate(mode="nearest") is (y>>2, x>>2)
        assert np.array_equal(m["conf"], g14["conf_up"] != 0)
        assert np.array_equal(m["mm"], g14["matching_mask"])
        want_c = g14["consistency_mask"] if kw["motion_masking"] else g14["conf_up"]
        assert m["cmask"].dtype == np.float32 and np.array_equal(m["cmask"], want_c), case
        assert m["rmask"].dtype == np.uint8 and np.array_equal(m["rmask"], g14[f"rmask_{case}"][:, 0].astype(np.uint8)), case
        assert (m["rmask"][1] == 0).all() and 0.05 < m["rmask"].mean() < 0.95    # item 1 is augmented
    assert not g14["matching_mask"][0, 1, 2] and not g14["matching_mask"][0, 2, 1]    # the ratios that are exactly 1
    flat = g14["mono_depth"].reshape(3, -1)
    assert np.array_equal(m["minmax"], np.stack([flat.min(1), flat.max(1)], 1))
    # without the augmentation vector item 1 is an item like the others
    assert S.masks(g14["lowest"], g14["confidence"], g14["mono_depth"], None, True)["rmask"][1].any()


@pytest.mark.parametrize("case", list(CASES))
def test_losses_against_the_reference(g14, case):
    kw = CASES[case]
    m = S.masks(g14["lowest"], g14["confidence"], g14["mono_depth"], g14["aug"], kw["motion_masking"])
    c = S.combine([g14["reproj0"], g14["reproj1"]], m["rmask"], g14["multi_depth"], g14["mono_depth"], avg=kw["avg"])
    n = m["rmask"].size
    got = {"reproj": c["sums"][0] / (c["sums"][1] + 1e-7), "consistency": c["sums"][2] / n}
    assert c["loss"].dtype == np.float32 and c["loss"][0] == np.float32(got["reproj"]) and c["loss"][1] == np.float32(got["consistency"])
    for name in ("reproj", "consistency"):
        ref = float(g14[f"{name}_loss_{case}"])
        tol = max(4.0 * float(g14[f"dev_{name}_{case}"]), 2.0 ** -20)
        err = abs(got[name] - ref) / abs(ref)
        print(f"{case} {name}: student_ref {got[name]!r} reference fp32 {ref!r} rel {err:.2e} tol {tol:.2e}")
        assert err <= tol, (case, name, got[name], ref)
    assert ((c["sel"] == 255) == (m["rmask"] == 0)).all()
    if kw["avg"]:
        assert set(np.unique(c["sel"])) <= {0, 255}


def test_combine_edges():
    """A tie goes to the earlier frame, an invalid frame never wins, an item without a valid frame counts as masked, and a NaN
    under the mask still reaches the sum (a real product)."""
    f32 = np.float32
    a = np.array([0.5, 0.25, 0.75, 0.5], f32).reshape(1, 1, 1, 4).repeat(4, 2)
    b = np.array([0.5, 0.5, 0.25, np.nan], f32).reshape(1, 1, 1, 4).repeat(4, 2)
    ones = np.ones((1, 4, 4), np.uint8)
    d = np.ones((1, 1, 4, 4), f32)
    c = S.combine([a, b], ones, d * 2, d)
    assert c["sel"][0, 0].tolist() == [0, 0, 1, 0] and c["sums"][2] == 0 and c["sums"][1] == 16
    c = S.combine([a, b], ones, d * 2, d, valid=np.array([[0, 1]], f32))
    assert c["sel"][0, 0].tolist() == [1, 1, 1, 1] and np.isnan(c["sums"][0])
    c = S.combine([a, b], ones, d * 2, d, valid=np.zeros((1, 2), f32))
    assert (c["sel"] == 255).all() and c["sums"].tolist() == [0.0, 0.0, 16.0] and c["loss"].tolist() == [0.0, 1.0]
    masked = ones.copy()
    masked[0, :, 3] = 0
    c = S.combine([b, b], masked, d * 2, d)
    assert np.isnan(c["sums"][0]) and c["sums"][2] == 4                         # NaN * 0 is NaN: the product is real
    g, gm = S.combine_grad([1.0, 2.0], c["sel"], np.array([1.0, 12.0, 4.0]), d * 2, d, None, 2)
    assert gm[0, 0, 0].tolist() == [0.0, 0.0, 0.0, f32(2.0 / 16)] and g[0][0, 0, 0, 3] == 0
    _, gm = S.combine_grad([1.0, 2.0], c["sel"], np.array([1.0, 12.0, 4.0]), d * np.nan, d, None, 2)
    assert (gm == 0).all()                                                       # sign(NaN) = 0, as torch.sign
    assert torch.sign(torch.tensor(float("nan"))).item() == 0


def test_tracker_and_bins_are_the_references(g14):
    from polardepth import matching
    tracker = tuple(g14["tracker_init"])
    for k in range(3):
        d = g14["tracker_depths"][k]
        flat = d.reshape(d.shape[0], -1)
        minmax = np.stack([flat.min(1), flat.max(1)], 1)
        for binning, D, key in (("linear", 96, "bins_linear"), ("inverse", 96, "bins_inverse"), ("linear", 2, "bins2_linear"),
                                ("inverse", 2, "bins2_inverse")):
            new, bins = S.bins_update(minmax, tracker, float(g14["tracker_floor"]), D, binning)
            assert new == tuple(g14["tracker"][k]), (k, new, g14["tracker"][k])   # the reference's Python floats, bit for bit
            assert bins.dtype == np.float32 and bins.tobytes() == g14[key][k].tobytes(), (k, key)
            assert bins.tobytes() == matching.depth_bins(new[0], new[1], D, binning).numpy().tobytes()
        tracker = new
    assert g14["tracker"][1, 0] < g14["tracker"][0, 0]       # the second batch's minima lie below the floor: pulled to it
    for binning in ("linear", "inverse"):                    # D == 1 as NumPy treats it
        assert S.bins_of(0.3, 7.0, 1, binning).tobytes() == matching.depth_bins(0.3, 7.0, 1, binning).numpy().tobytes()


# ------------------------------------------------------------------ the loader's lookup_aug switch
H, W, FH, FW = 32, 64, 40, 72


@pytest.fixture()
def tree(tmp_path):
    rng = np.random.default_rng(11)
    folder = tmp_path / "scene_a" / "polarization"
    for sub in ("rgb", "pol00", "pol01", "pol10", "pol11", "_gt", "_instance", "_pose"):
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


def _item(root, index, seed, **kw):
    ds = HAMMER_Dataset(str(root), ["scene_a"], H, W, [0, -1, 1], 4, is_train=True, offset=1, **kw)
    random.seed(seed)
    return ds[index]


def test_lookup_aug_adds_the_jittered_neighbours_and_nothing_else(tree):
    root, folder = tree
    seed = next(s for s in range(100) if random.Random(s).random() > 0.5)      # an item that is jittered
    random.seed(seed)
    assert random.random() > 0.5
    params = color_jitter_params()                                              # the item's own draw
    off, on = _item(root, 1, seed), _item(root, 1, seed, lookup_aug=True)
    new = {("color_aug", -1, 0), ("color_aug", 1, 0)}
    assert set(on) - set(off) == new and set(off) - set(on) == set()
    assert {k for k in off if isinstance(k, tuple) and k[0] == "color_aug"} == {("color_aug", 0, s) for s in range(4)}
    for k, v in off.items():                                                    # without the switch: the item as it was
        assert on[k].dtype == v.dtype and on[k].shape == v.shape and on[k].numpy().tobytes() == v.numpy().tobytes(), k
    for i in (-1, 1):
        im = Image.open(folder / "rgb" / f"{1 + i:06d}.png").convert("RGB").resize((W, H), Image.LANCZOS)
        plain = np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0
        want = np.asarray(apply_color_jitter(im, params), dtype=np.float32).transpose(2, 0, 1) / 255.0
        assert on[("color", i, 0)].numpy().tobytes() == plain.tobytes()
        assert on[("color_aug", i, 0)].numpy().tobytes() == want.tobytes() and not np.array_equal(want, plain), i
    # frame 0's own jitter is the same draw
    im0 = Image.open(folder / "rgb" / "000001.png").convert("RGB").resize((W, H), Image.LANCZOS)
    assert on[("color_aug", 0, 0)].numpy().tobytes() == (np.asarray(apply_color_jitter(im0, params), dtype=np.float32).transpose(2, 0, 1) / 255.0).tobytes()


def test_lookup_aug_without_jitter_and_with_a_missing_neighbour(tree):
    root, _ = tree
    seed = next(s for s in range(100) if random.Random(s).random() <= 0.5)     # an item that is not jittered
    on = _item(root, 0, seed, lookup_aug=True)                                  # frame 0 has no frame -1
    assert on[("frame_valid", -1)].item() == 0 and on[("frame_valid", 1)].item() == 1
    assert torch.equal(on[("color_aug", 1, 0)], on[("color", 1, 0)])
    assert on[("color_aug", -1, 0)].shape == (3, H, W) and not on[("color_aug", -1, 0)].any()
    seed = next(s for s in range(100) if random.Random(s).random() > 0.5)
    on = _item(root, 0, seed, lookup_aug=True)                                  # jittered item: the dummy frame stays blank
    assert not on[("color_aug", -1, 0)].any() and not torch.equal(on[("color_aug", 1, 0)], on[("color", 1, 0)])


def test_synthetic_items_get_the_same_keys():
    off = HAMMER_Dataset("synthetic", [], 32, 64, [0, -1, 1], 4, is_train=True)[3]
    on = HAMMER_Dataset("synthetic", [], 32, 64, [0, -1, 1], 4, is_train=True, lookup_aug=True)[3]
    assert set(on) - set(off) == {("color_aug", -1, 0), ("color_aug", 1, 0)}
    for k, v in off.items():
        assert torch.equal(on[k], v), k
    for i in (-1, 1):
        assert torch.equal(on[("color_aug", i, 0)], on[("color", i, 0)])
