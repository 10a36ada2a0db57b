"""Evaluation(uncertainty=True) on the GPU with synthetic items: ``test_uncertainty`` totals equal ``uncertainty_stats`` called
directly on the same predictions, its pooled figures come from the sum of the per-image tables, ``predict_all`` hands out the
scale, and a weights folder without the heads is refused."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=2)


@pytest.fixture(scope="module")
def ev():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    return Evaluation(uncertainty=True, **KW)


def test_report_equals_direct_calls_and_the_pool_is_the_sum_of_the_tables(ev, capsys):
    from polardepth import uncertainty_eval as ue
    res = ev.test_uncertainty()
    text = capsys.readouterr().out
    assert "uncertainty (b from 0.5 to 500 mm)" in text and "pooled" in text and "per-image" in text and "ause_mm" in text
    assert list(res) == [n for n, _ in ue.DEFAULT_CLASSES] and len(res) == 12
    recs, tabs, per = [], [], []
    with torch.no_grad():
        for inputs in ev.test_loader:
            inputs = {k: v.to(ev.device) for k, v in inputs.items()}
            out = ev.predict_all(inputs)
            assert tuple(out["uncertainty"].shape) == tuple(out["depth"].shape) == (2, 1, 64, 96)
            u = out["uncertainty_u"]
            assert float(u.min()) >= 0 and float(u.max()) <= 1
            assert torch.equal(out["uncertainty"], ue.scale_of(u, ev.uncertainty_range))
            assert 0.0005 <= float(out["uncertainty"].min()) and float(out["uncertainty"].max()) <= 0.5
            st = ue.uncertainty_stats(out["depth"], inputs["depth_gt"], u, mask=inputs[("mask", 0, 0)], b_range=ev.uncertainty_range,
                                      min_depth=ev.min_depth, max_depth=ev.max_depth)
            recs.append({k: getattr(st, k).cpu().numpy() for k in ("n", "bad", "cover", "sums", "hist")})
            tabs.append(st.tables.cpu().numpy())
            per.append(st.metrics())
    assert len(recs) >= 2
    cat = {k: np.concatenate([r[k] for r in recs], 0) for k in recs[0]}
    tables = np.concatenate(tabs, 0).astype(object).sum(0)                   # Python integers: the exact sum of the per-image tables
    pooled = ue.metrics_from_fields(cat["n"].sum(0), cat["cover"].sum(0), cat["sums"].sum(0), cat["hist"].sum(0), tables)
    per = np.concatenate(per, 0)
    valid = per[..., 9] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        per_image = np.where(valid[..., None], per, 0.0).sum(0) / valid.sum(0)[:, None]
    for k, name in enumerate(res):
        r = res[name]
        assert set(r) == {"per_image", "pooled", "bad"} and r["pooled"].shape == (10,)
        assert r["pooled"][9] == cat["n"][:, k].sum() and r["bad"] == cat["bad"][:, k].sum()
        assert np.array_equal(r["pooled"][3:10], pooled[k][3:10], equal_nan=True), name      # integer figures: equal
        assert np.allclose(r["pooled"][:3], pooled[k][:3], rtol=1e-12, atol=0.0, equal_nan=True), name
        assert np.allclose(r["per_image"], per_image[k], rtol=1e-12, atol=0.0, equal_nan=True), name
    assert res["all"]["pooled"][9] > 0 and res["all"]["bad"] == 0 and np.isfinite(res["all"]["pooled"]).all()


def test_options_and_refusals(tmp_path, monkeypatch):
    from manydepth.evaluation import Evaluation
    plain = Evaluation(**KW)
    assert not plain.uncertainty and not plain.models["mono_depth"].uncertainty
    with pytest.raises(ValueError, match="uncertainty=True"):
        plain.test_uncertainty()
    with torch.no_grad():
        inputs = {k: v.to(plain.device) for k, v in next(iter(plain.test_loader)).items()}
        assert "uncertainty" not in plain.predict_all(inputs)
    with pytest.raises(ValueError, match="uncertainty=True"):
        Evaluation(uncertainty_range=(0.001, 0.1), **KW)
    with pytest.raises(ValueError, match="b_lo < b_hi"):
        Evaluation(uncertainty=True, uncertainty_range=(0.1, 0.001), **KW)
    assert Evaluation(uncertainty=True, uncertainty_range="0.001,0.25", **KW).uncertainty_range == (0.001, 0.25)
    monkeypatch.setenv("PD_UNCERTAINTY", "1")
    assert Evaluation(**KW).uncertainty and not Evaluation(uncertainty=False, **KW).uncertainty
    monkeypatch.delenv("PD_UNCERTAINTY")
    # a weights folder of a run without the heads
    folder = tmp_path / "weights"
    os.makedirs(folder)
    for n, m in plain.models.items():
        torch.save(m.state_dict(), folder / f"{n}.pth")
    Evaluation(load_weights_folder=str(folder), **KW).load_mono_model()
    ev = Evaluation(load_weights_folder=str(folder), uncertainty=True, **KW)
    with pytest.raises(ValueError, match="holds no unc_conv weights"):
        ev.load_mono_model()
    # with the heads, and the range the trainer stored with them
    with_heads = Evaluation(uncertainty=True, **KW)
    torch.save(with_heads.models["mono_depth"].state_dict(), folder / "mono_depth.pth")
    torch.save({"uncertainty_range": [0.002, 0.2]}, folder / "trainer_state.pth")
    ev = Evaluation(load_weights_folder=str(folder), uncertainty=True, **KW)
    ev.load_mono_model()
    assert ev.uncertainty_range == (0.002, 0.2)
    for k, v in with_heads.models["mono_depth"].state_dict().items():
        assert torch.equal(ev.models["mono_depth"].state_dict()[k], v), k
    own = Evaluation(load_weights_folder=str(folder), uncertainty=True, uncertainty_range=(0.001, 0.1), **KW)
    assert own.uncertainty_range == (0.001, 0.1)
