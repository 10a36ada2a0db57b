"""Evaluation.test_polar_normals on the GPU, on the synthetic loader at its smallest size: both sources return every class with
finite figures where a class holds pixels, the pooled n and the counters add up to the class's pixel count, the report
equals the NumPy statement (tests/polar_normals_ref.py) applied to what the device holds, and nothing else moves: test()
prints what it printed before."""
import math

import numpy as np
import pytest
import torch

import polar_normals_ref as R

pytestmark = pytest.mark.gpu

KW = dict(data_path="synthetic", height=64, width=96, batch_size=4)


@pytest.fixture(scope="module")
def ev():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    return Evaluation(**KW)


def _batches(ev):
    for inputs in ev.test_loader:
        yield {k: v.cuda() for k, v in inputs.items()}


def _class_pixels(ev, source):
    """[K] the pixels of each default class over the loader (for "gt": those whose 3x3 window is inside the depth range)."""
    from polardepth import normals_eval as ne
    import normals_stats_ref as NR
    tot = np.zeros(len(ne.DEFAULT_CLASSES), np.int64)
    for inputs in _batches(ev):
        mask = inputs[("mask", 0, 0)][:, 0].cpu().numpy()
        live = np.ones(mask.shape, bool)
        if source == "gt":
            live = NR.window_ok(inputs["depth_gt"][:, 0].float().cpu().numpy(), np.float32(0.1), np.float32(2.0), 1)
        for k, (_, r) in enumerate(ne.DEFAULT_CLASSES):
            lo, hi = (1, 0) if r is None else r
            tot[k] += (R.in_class(mask, lo, hi) & live).sum()
    return tot


@pytest.mark.parametrize("source", ["depth", "gt"])
def test_every_class_reports_and_the_counts_add_up(ev, source, capsys):
    from polardepth import normals_eval as ne
    from polardepth import polar_normals_eval as pe
    res = ev.test_polar_normals(source=source)
    text = capsys.readouterr().out
    assert f"polar normal ({source})" in text and f"polar azimuth ({source})" in text and "pooled" in text and "dolp_out" in text
    names = [n for n, _ in ne.DEFAULT_CLASSES]
    assert list(res) == names and len(names) == 12
    pixels = _class_pixels(ev, source)
    assert pixels[0] > 0 and pixels[1] > 0
    for k, name in enumerate(names):
        for sname, counters in (("normal", pe.NORMAL_COUNTERS), ("azimuth", pe.AZIMUTH_COUNTERS)):
            r = res[name][sname]
            assert r["per_image"].shape == (8,) and r["pooled"].shape == (8,) and set(counters) <= set(r)
            n = int(r["pooled"][6])
            gates = r["bad"] + r["dolp_out"] + (r["frontal"] if sname == "azimuth" else 0)
            print(source, name, sname, "n", n, {c: r[c] for c in counters}, "of", int(pixels[k]))
            assert n + gates == pixels[k], (source, name, sname)
            assert r["spec"] <= n and (sname == "azimuth" or r["flipped"] <= n)
            if n > 0:
                assert np.isfinite(r["pooled"][:7]).all() and np.isfinite(r["per_image"][:7]).all(), (source, name, sname)
                assert 0.0 <= r["pooled"][0] <= (180.0 if sname == "normal" else 90.0)
    assert res["all"]["normal"]["pooled"][6] > 0 and res["all"]["azimuth"]["pooled"][6] > 0


def test_the_report_equals_the_statement(ev):
    """The wiring of source="depth": which tensors are scored, the classes, the conventions' defaults."""
    from polardepth import normals_eval as ne
    from polardepth import polar as pdpolar
    from polardepth._lib import lib, check, ptr, stream_ptr
    res = ev.test_polar_normals(source="depth")
    big = float(np.finfo(np.float32).max)
    lohi = [(1, 0) if r is None else r for _, r in ne.DEFAULT_CLASSES]
    parts = []
    for inputs in _batches(ev):
        depth = ev.predict(inputs).contiguous()
        pol = pdpolar.polar_inputs(inputs, (64, 96), ("xolp", "normals"), ev.pol_angles)
        K = inputs[("K", 0)].float().contiguous()
        N, _, H, W = depth.shape
        pn = torch.empty((N, H, W, 4), device="cuda")
        check(lib.pd_gt_normals(ptr(depth), ptr(K), ptr(pn), N, H, W, -big, big, stream_ptr()), "pd_gt_normals")
        parts.append(R.stats(pn.cpu().numpy(), pol.cpu().numpy(), inputs["xolp", 0, 0].cpu().numpy(),
                             inputs[("mask", 0, 0)][:, 0].cpu().numpy(), lohi, ne.cos_edges_numpy(),
                             tilt2_min=math.sin(math.radians(5.0)) ** 2))
    for sname in ("normal", "azimuth"):
        n = sum(p[sname]["n"].sum(0) for p in parts)
        s = sum(p[sname]["sums"].sum(0) for p in parts)
        for k, name in enumerate(res):
            r = res[name][sname]
            assert int(r["pooled"][6]) == n[k], (sname, name)
            for c in R.NORMAL_COUNTERS if sname == "normal" else R.AZIMUTH_COUNTERS:
                assert r[c] == sum(p[sname][c].sum(0) for p in parts)[k], (sname, name, c)
            if n[k]:
                assert np.isclose(r["pooled"][0], s[k, 0] / n[k], rtol=1e-9) and np.isclose(r["pooled"][7], s[k, 2] / s[k, 3], rtol=1e-9)


def test_nothing_else_moves(ev, capsys, monkeypatch):
    from manydepth.evaluation import Evaluation
    a = ev.test()
    before = capsys.readouterr().out
    ev.test_polar_normals(source="gt")
    ev.test_polar_normals()
    capsys.readouterr()
    b = ev.test()
    assert capsys.readouterr().out == before and before.startswith("all ")
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError, match="source must be"):
        ev.test_polar_normals(source="xolp")
    with pytest.raises(ValueError, match="normals_decoder=True"):
        ev.test_polar_normals(source="decoder")
    # the handedness: an argument, or the environment, and it changes the azimuth set only through the candidates' y
    assert ev.aolp_sign == 1
    monkeypatch.setenv("PD_POL_AOLP_SIGN", "-1")
    torch.manual_seed(0)
    other = Evaluation(**KW)
    assert other.aolp_sign == -1 and Evaluation(aolp_sign=1, **KW).aolp_sign == 1
    monkeypatch.delenv("PD_POL_AOLP_SIGN")
    with pytest.raises(ValueError, match="aolp_sign"):
        Evaluation(aolp_sign=0, **KW)
    x, y = ev.test_polar_normals(source="gt"), other.test_polar_normals(source="gt")
    assert x["all"]["azimuth"]["pooled"][6] == y["all"]["azimuth"]["pooled"][6]
    assert x["all"]["azimuth"]["pooled"][0] != y["all"]["azimuth"]["pooled"][0]


def test_export_writes_the_disambiguated_normals(tmp_path):
    """tools/export_pointcloud.py --normals: pred.ply carries nx ny nz -- the depth map's normals, or with "polar" the
    winning polarisation candidate wherever the measurement gives one; gt.ply is unchanged."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_pointcloud as E

    def read(path, with_normals):
        head, payload = open(path, "rb").read().split(b"end_header\n", 1)
        props = [l.split()[-1] for l in head.decode("ascii").splitlines() if l.startswith("property")]
        assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + ["red", "green", "blue"]
        dt = [("xyz", "<f4", 3)] + ([("n", "<f4", 3)] if with_normals else []) + [("rgb", "u1", 3)]
        return np.frombuffer(payload, dtype=dt)

    rows = {}
    for kind in (None, "depth", "polar"):
        torch.manual_seed(0)
        out = str(tmp_path / str(kind))
        written = E.export("synthetic", None, 0, out, height=64, width=96, normals=kind)
        rows[kind] = read(os.path.join(out, "pred.ply"), kind is not None)
        assert written[os.path.join(out, "pred.ply")] == len(rows[kind]) > 0
        assert len(read(os.path.join(out, "gt.ply"), False)) > 0
    assert np.array_equal(rows[None]["xyz"], rows["depth"]["xyz"]) and np.array_equal(rows[None]["xyz"], rows["polar"]["xyz"])
    changed = (rows["depth"]["n"] != rows["polar"]["n"]).any(1)
    assert 0 < changed.sum() <= len(changed)
    norm = np.linalg.norm(rows["polar"]["n"][changed], axis=1)
    assert np.allclose(norm, 1.0, atol=1e-4)                       # K1's candidates are unit vectors
    # on the depth normal's side: the angle to it is at most 90 degrees (flipped file: y and z negated in both)
    assert ((rows["depth"]["n"][changed] * rows["polar"]["n"][changed]).sum(1) >= -1e-6).all()
    with pytest.raises(ValueError, match="--normals"):
        E.export("synthetic", None, 0, str(tmp_path / "x"), height=64, width=96, normals="xolp")
