"""Evaluation(pose_network=True).test_pose() on synthetic items against tests/pose_loss_ref.py applied to the matrices the
networks return, and an Evaluation without the argument: no pose models, and the bits it returned before."""
import numpy as np
import pytest
import torch

import pose_loss_ref as L

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=4)


def _flat(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _flat(v, f"{prefix}{k}.")
        else:
            yield f"{prefix}{k}", v


def test_pose_report_is_the_statement_on_the_networks_matrices():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(5)
    ev = Evaluation(pose_network=True, **KW)
    ev.load_mono_model()                                               # no folder: every module keeps its initialisation
    assert {"pose_encoder", "pose"} <= set(ev.models) and ev.pose_loader.dataset.need_poses is True
    assert ev.pose_loader.dataset.frame_idxs == [0, -1, 1] and ev.test_loader.dataset.frame_idxs == [0]
    got = ev.test_pose()
    Tp, Tg, valid = {-1: [], 1: []}, {-1: [], 1: []}, []
    for inputs in ev.pose_loader:
        inputs = {k: v.to(ev.device) for k, v in inputs.items()}
        T = ev.predict_poses(inputs)
        for i in (-1, 1):
            Tp[i].append(T[i].cpu().numpy())
            Tg[i].append(inputs[("poses", i)].cpu().numpy())
        valid.append(torch.stack([inputs[("frame_valid", i)] for i in (-1, 1)], 1).cpu().numpy())
    rec = L.pose_records([np.concatenate(Tp[i]) for i in (-1, 1)], [np.concatenate(Tg[i]) for i in (-1, 1)])
    want = L.metrics(rec, np.concatenate(valid), [-1, 1])
    assert set(got) == {-1, 1, "all"} and want["all"]["pairs"] == 2 * rec.shape[1] > 0
    a, b = dict(_flat(got)), dict(_flat(want))
    assert set(a) == set(b)
    for k in a:
        if isinstance(b[k], int):
            assert a[k] == b[k], k
        else:
            np.testing.assert_allclose(a[k], b[k], rtol=1e-9, err_msg=k)
    assert got["all"]["rot_deg"]["max"] > 0 and got["all"]["trans_mm"]["mean"] > 0


def test_metrics_from_records_counts_missing_and_bad():
    """polardepth.pose_eval.metrics_from_records against the statement on records with missing and non-finite pairs."""
    from polardepth import pose_eval
    rng = np.random.default_rng(8)
    Tp = [L.head_matrices(rng, 9, 0.2) for _ in range(2)]
    Tg = [L.head_matrices(rng, 9, 0.2) for _ in range(2)]
    rec = L.pose_records(Tp, Tg)
    rec[0, 2, 6] = np.nan
    valid = np.ones((9, 2), np.float32)
    valid[4, 1] = valid[2, 1] = 0
    got = pose_eval.metrics_from_records(torch.from_numpy(rec).cuda(), torch.from_numpy(valid).cuda(), [-1, 1])
    want = L.metrics(rec, valid, [-1, 1])
    assert (got["all"]["pairs"], got["all"]["missing"], got["all"]["bad"]) == (15, 2, 1)
    a, b = dict(_flat(got)), dict(_flat(want))
    for k in b:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-12, err_msg=k)


def test_plain_evaluation_is_what_it_was():
    from manydepth.evaluation import Evaluation
    evs = []
    for _ in range(2):
        torch.manual_seed(6)
        evs.append(Evaluation(**KW))
    torch.manual_seed(6)
    with_pose = Evaluation(pose_network=True, **KW)                    # the shared modules draw before the pose modules
    for ev in evs:
        assert "pose_encoder" not in ev.models and "pose" not in ev.models and not hasattr(ev, "pose_loader")
        with pytest.raises(ValueError, match="pose_network"):
            ev.test_pose()
    batch = next(iter(evs[0].test_loader))
    depths = [ev.predict({k: v.to(ev.device) for k, v in batch.items()}) for ev in evs + [with_pose]]
    assert torch.equal(depths[0], depths[1]) and torch.equal(depths[0], depths[2])
    r0, r1 = evs[0].test(), evs[1].test()
    assert set(r0) == set(r1) and all(np.array_equal(r0[k], r1[k]) for k in r0)
