"""Evaluation(multi_frame=True) on synthetic items (64 x 96, batch 2, 16 depth bins): predict_multi against the same modules
called by hand, from both pose sources; an absent lookup frame; checkpoints written the way the reference writes them;
test_depth(source="multi") and test_pose_chain; and an Evaluation without the arguments: the models and the bits it had."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=2)
MULTI = dict(multi_frame=True, num_depth_bins=16, **KW)


def _ev(seed, **kw):
    from manydepth.evaluation import Evaluation
    torch.manual_seed(seed)
    return Evaluation(**kw)


@pytest.fixture(scope="module")
def ev_files():
    return _ev(6, matching_ids=(0, -1, -2), multi_poses="files", **MULTI)


@pytest.fixture(scope="module")
def ev_net():
    return _ev(6, matching_ids=(0, -1), multi_poses="network", **MULTI)


def _batch(ev):
    return {k: v.to(ev.device) for k, v in next(iter(ev.multi_loader)).items()}


def _by_hand(ev, inputs, poses):
    from polardepth._lib import lib, check, ptr, stream_ptr
    ids = ev.matching_ids
    with torch.no_grad():
        lookups = torch.stack([inputs[("color", i, 0)].float() for i in ids[1:]], 1)
        feats, lowest, conf = ev.models["encoder"](inputs[("color_aug", 0, 0)].float(), lookups, poses, inputs[("K", 2)],
                                                   inputs[("inv_K", 2)])
        disp = ev.models["depth"](feats)[("disp", 0)].contiguous()
        depth = torch.empty((disp.shape[0], 1, ev.height, ev.width), device=disp.device)
        check(lib.pd_disp_to_depth(ptr(disp), ptr(depth), None, disp.shape[0], disp.shape[2], disp.shape[3], ev.height,
                                   ev.width, ev.min_depth, ev.max_depth, stream_ptr()), "pd_disp_to_depth")
    return {"depth": depth.clamp(ev.min_depth, ev.max_depth), "lowest_cost": lowest, "confidence": conf}


def _same(a, b):
    return set(a) == set(b) == {"depth", "lowest_cost", "confidence"} and all(torch.equal(a[k], b[k]) for k in a)


def test_predict_multi_from_both_pose_sources(ev_files, ev_net):
    from polardepth import matching
    for ev in (ev_files, ev_net):
        names = list(ev.models)
        assert names[-2:] == ["encoder", "depth"] and ("pose" in names) == (ev.multi_poses == "network")
        assert ev.models["encoder"].adaptive_bins and ev.models["encoder"].num_depth_bins == 16
        assert torch.equal(ev.models["encoder"].depth_bins.cpu(), matching.depth_bins(ev.min_depth, ev.max_depth, 16, "linear"))
        ds = ev.multi_loader.dataset
        assert ds.frame_idxs == [0] + ev.matching_ids[1:] and ds.need_poses is (ev.multi_poses == "files")
        inputs = _batch(ev)
        got = ev.predict_multi(dict(inputs))
        assert tuple(got["depth"].shape) == (2, 1, 64, 96)
        assert tuple(got["lowest_cost"].shape) == tuple(got["confidence"].shape) == (2, 16, 24)
        for v in got.values():
            assert torch.isfinite(v).all()
        assert got["depth"].min() >= ev.min_depth and got["depth"].max() <= ev.max_depth
        assert ((got["confidence"] == 0) | (got["confidence"] == 1)).all()
        ids = ev.matching_ids
        if ev.multi_poses == "files":
            poses = torch.stack([inputs[("poses", i)] for i in ids[1:]], 1)               # every synthetic frame is present
        else:
            rel, _ = matching.matching_poses(ev.models["pose_encoder"], ev.models["pose"],
                                             {i: inputs[("color", i, 0)] for i in ids}, ids,
                                             {i: inputs[("frame_valid", i)] for i in ids[1:]})
            poses = torch.stack([rel[i] for i in ids[1:]], 1)
        assert _same(got, _by_hand(ev, inputs, poses))
        assert _same(got, ev.predict_multi(dict(inputs)))


def test_an_absent_lookup_frame_reaches_the_sweep_as_a_zero_pose(ev_files):
    ev = ev_files
    inputs = _batch(ev)
    ids = ev.matching_ids
    # what the loader serves for a neighbour that does not exist: a black picture, the identity, frame_valid 0
    inputs[("color", -1, 0)][1] = 0
    inputs[("poses", -1)][1] = torch.eye(4, device=ev.device)
    inputs[("frame_valid", -1)][1] = 0
    got = ev.predict_multi(dict(inputs))
    left_in = torch.stack([inputs[("poses", i)] for i in ids[1:]], 1)
    zeroed = left_in.clone()
    zeroed[1, 0] = 0
    assert _same(got, _by_hand(ev, inputs, zeroed))
    other = _by_hand(ev, inputs, left_in)
    assert not torch.equal(got["depth"][1], other["depth"][1])                 # the black picture would have been matched
    assert torch.equal(got["depth"][0], other["depth"][0])                     # eval mode: the other item does not see it


def _write_folder(folder, ev, extras):
    os.makedirs(folder, exist_ok=True)
    for n, m in ev.models.items():
        sd = dict(m.state_dict())
        if n == "encoder":
            sd.update(extras)
        torch.save(sd, os.path.join(folder, f"{n}.pth"))


def test_checkpoints_written_the_reference_way(ev_files, tmp_path):
    from polardepth import matching
    src = ev_files
    folder = str(tmp_path / "weights_3")
    _write_folder(folder, src, {"height": 64, "width": 96, "min_depth_bin": 0.25, "max_depth_bin": 1.5})
    dst = _ev(7, matching_ids=(0, -1, -2), multi_poses="files", load_weights_folder=folder, **MULTI)
    assert not torch.equal(dst.models["encoder"].layer0[0].weight, src.models["encoder"].layer0[0].weight)
    dst.load_mono_model()
    for n in src.models:
        a, b = src.models[n].state_dict(), dst.models[n].state_dict()
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), n
    assert not any(k in dst.models["encoder"].state_dict() for k in ("height", "width", "min_depth_bin", "max_depth_bin"))
    assert torch.equal(dst.models["encoder"].depth_bins.cpu(), matching.depth_bins(0.25, 1.5, 16, "linear"))
    inputs = _batch(dst)
    assert torch.isfinite(dst.predict_multi(inputs)["depth"]).all()
    # without the stored range the bins stay those of the object's min_depth / max_depth
    plain = str(tmp_path / "weights_plain")
    _write_folder(plain, src, {"height": 64, "width": 96})
    dst2 = _ev(7, matching_ids=(0, -1, -2), multi_poses="files", load_weights_folder=plain, **MULTI)
    dst2.load_mono_model()
    assert torch.equal(dst2.models["encoder"].depth_bins.cpu(), matching.depth_bins(dst2.min_depth, dst2.max_depth, 16, "linear"))
    assert torch.equal(dst2.models["encoder"].layer0[0].weight, src.models["encoder"].layer0[0].weight)
    # another size: refused
    wrong = str(tmp_path / "weights_wrong")
    _write_folder(wrong, src, {"height": 128, "width": 96, "min_depth_bin": 0.25, "max_depth_bin": 1.5})
    dst3 = _ev(7, matching_ids=(0, -1, -2), multi_poses="files", load_weights_folder=wrong, **MULTI)
    with pytest.raises(ValueError, match="height"):
        dst3.load_mono_model()
    # a folder of a single-frame run: the two multi-frame modules keep their initialisation
    os.remove(os.path.join(plain, "encoder.pth"))
    os.remove(os.path.join(plain, "depth.pth"))
    dst4 = _ev(8, matching_ids=(0, -1, -2), multi_poses="files", load_weights_folder=plain, **MULTI)
    before = {n: {k: v.clone() for k, v in dst4.models[n].state_dict().items()} for n in ("encoder", "depth")}
    dst4.load_mono_model()
    for n, sd in before.items():
        assert all(torch.equal(v, dst4.models[n].state_dict()[k]) for k, v in sd.items()), n
    k0 = next(iter(src.models["rgb_encoder"].state_dict()))
    assert torch.equal(dst4.models["rgb_encoder"].state_dict()[k0], src.models["rgb_encoder"].state_dict()[k0])


def test_reports(ev_net):
    from polardepth import depth_eval
    multi = ev_net.test_depth(source="multi")
    mono = ev_net.test_depth()
    assert set(multi) == set(mono) and "all" in multi
    for r in multi.values():
        assert set(r) == {"per_image", "pooled", "bad"} and len(r["per_image"]) == len(depth_eval.METRIC_NAMES)
    assert np.isfinite(multi["all"]["pooled"]).all() and not np.array_equal(multi["all"]["pooled"], mono["all"]["pooled"])
    chain = ev_net.test_pose_chain(2)
    assert set(chain) == {-1, -2, "all"}
    for r in chain.values():
        assert set(r) == {"pairs", "missing", "bad", "rot_deg", "trans_mm", "scale_ratio_median"}
    assert chain[-1]["pairs"] == chain[-2]["pairs"] == 8 and chain["all"]["missing"] == chain["all"]["bad"] == 0
    assert np.isfinite(chain[-2]["rot_deg"]["mean"]) and chain[-2]["trans_mm"]["mean"] > 0
    with pytest.raises(ValueError, match="source"):
        ev_net.test_depth(source="student")


def test_plain_evaluation_is_what_it_was(ev_files):
    plain = [_ev(6, **KW) for _ in range(2)]
    for ev in plain:
        assert list(ev.models) == ["rgb_encoder", "normals_encoder", "xolp_encoder", "joint_encoder", "mono_depth"]
        assert not hasattr(ev, "multi_loader") and not ev.multi_frame
        with pytest.raises(ValueError, match="multi_frame"):
            ev.predict_multi({})
        with pytest.raises(ValueError, match="multi_frame"):
            ev.test_depth(source="multi")
        with pytest.raises(ValueError, match="pose_network"):
            ev.test_pose_chain(2)
    batch = next(iter(plain[0].test_loader))
    depths = [ev.predict({k: v.to(ev.device) for k, v in batch.items()}) for ev in plain + [ev_files]]
    assert torch.equal(depths[0], depths[1]) and torch.equal(depths[0], depths[2])     # the shared modules draw first
