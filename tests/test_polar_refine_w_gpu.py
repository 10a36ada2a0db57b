"""The per-pixel weight of the prior on the GPU: pd_polar_refine_setup_w, _table_w, _weights and polar_refine(weight=,
uncertainty=, robust=) against tests/polar_refine_w_ref.py, on the five shapes of tests/test_polar_refine_gpu.py (shared with it,
as its cached inputs and its unweighted reference are).

Weight == 1: the bits of the scalar route, device against device.  A random map with every special value: the edges, p, q and
1/diag bit for bit, rhs within the scalar test's bound with lam_i for lam, A the exact minimum of the device's own planes, the
table from that A bit for bit.  The weights kernel: NumPy's bits in its four input modes.  End to end: within the tolerance that
the reference's own response to a zeta0 perturbed by LOG_ULP gives (times 4), touched and the copied pixels bit for bit, the
fused route the one-step route's bits.  Two calls and a replayed capture return the eager bits."""
import numpy as np
import pytest
import torch

import polar_refine_ref as R
import polar_refine_w_ref as RW
import test_polar_refine_gpu as G
from test_polar_refine_gpu import CASES, IDS, LOG_ULP, EXP_ULP, bits, case, lib

pytestmark = pytest.mark.gpu

F64 = np.float64
_CACHE = {}


def wild(i):
    """A weight map for CASES[i] with every population of the clamp, about 5 % each: NaN, 0, negative, +inf, below weight_min,
    above weight_max; the rest in 1/16 .. 1.  Computed once, never written to."""
    if ("wild", i) not in _CACHE:
        N, H, W = CASES[i][:3]
        rng = np.random.default_rng(4000 + i)
        w = rng.uniform(RW.WEIGHT_MIN, RW.WEIGHT_MAX, (N, H, W)).astype(np.float32)
        sel = rng.random((N, H, W))
        for k, v in enumerate((np.nan, 0.0, -0.7, np.inf, 0.01, 3.0)):
            w[(sel >= 0.05 * k) & (sel < 0.05 * (k + 1))] = v
        _CACHE["wild", i] = (w, torch.from_numpy(w).cuda())
    return _CACHE["wild", i]


def scale_b(i):
    """A Laplace scale b for CASES[i]: 1 .. 40 mm, with NaN, 0 and negatives."""
    if ("b", i) not in _CACHE:
        N, H, W = CASES[i][:3]
        rng = np.random.default_rng(5000 + i)
        b = np.exp(rng.uniform(np.log(0.001), np.log(0.04), (N, H, W))).astype(np.float32)
        sel = rng.random((N, H, W))
        for k, v in enumerate((np.nan, 0.0, -0.003, np.inf)):
            b[(sel >= 0.04 * k) & (sel < 0.04 * (k + 1))] = v
        _CACHE["b", i] = (b, torch.from_numpy(b).cuda())
    return _CACHE["b", i]


def dev_setup_w(i, weight, lam=R.LAM, iters=R.ITERS):
    """pd_polar_refine_setup_w + _table_w on CASES[i] with the device tensor ``weight`` -> dict of host arrays."""
    L, check, ptr = lib()
    c, _, t = case(i)
    N, H, W = c["depth"].shape
    f64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    zeta0, coef, pq, A, table = f64(N, H, W), f64(N, 4, H, W), f64(N, 2, H, W), f64(N), f64(N, iters, 2)
    ws = torch.empty(int(L.pd_polar_refine_workspace(N, H, W)), dtype=torch.uint8, device="cuda")
    check(L.pd_polar_refine_setup_w(ptr(t["depth"]), ptr(t["K"]), ptr(t["normal"]), ptr(t["xolp"]), c["ldp"], ptr(t["valid"]), lam,
                                    R.EDGE_MAX, R.cos_inc_of(R.INCIDENCE_MAX_DEG), ptr(weight), RW.WEIGHT_MIN, RW.WEIGHT_MAX,
                                    ptr(zeta0), ptr(coef), ptr(pq), ptr(ws), ws.numel(), N, H, W, None), "pd_polar_refine_setup_w")
    check(L.pd_polar_refine_table_w(ptr(ws), ws.numel(), iters, ptr(A), ptr(table), N, H, W, None), "pd_polar_refine_table_w")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in (("zeta0", zeta0), ("coef", coef), ("pq", pq), ("A", A), ("table", table))}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_a_weight_of_one_returns_the_scalar_routes_bits(i):
    from polardepth import refine
    c, _, t = case(i)
    want = G.dev_setup(i)
    got = dev_setup_w(i, torch.ones_like(t["depth"]))
    for k in ("zeta0", "coef", "pq", "table"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    a = np.where(want["S"] > 0, R.LAM / (R.LAM + want["S"]), 0.0)
    assert np.array_equal(bits(got["A"]), bits(a))
    xolp = t["xolp"][..., :c["depth"].shape[2]]
    plain = refine.polar_refine(t["depth"], t["K"], None, xolp, valid=t["valid"], normals=t["normal"], iters=20)
    ones, wmap = refine.polar_refine(t["depth"], t["K"], None, xolp, valid=t["valid"], normals=t["normal"], iters=20,
                                     weight=torch.ones_like(t["depth"])[:, None], return_weight=True)
    torch.cuda.synchronize()
    for name, x, y in zip(("depth", "residual", "touched"), ones[:3], plain[:3]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name
    assert wmap.shape == t["depth"].shape and (wmap == 1).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_setup_and_table_with_a_random_weight(i):
    c, st0, _ = case(i)
    w, wd = wild(i)
    got = dev_setup_w(i, wd)
    st = RW.setup(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], w)
    assert st["dz_margin"] > 1e-9                                               # no gate decision within reach of an ulp
    m = st["margin"][np.isfinite(st["margin"])]
    assert m.size == 0 or np.abs(m).min() > 1e-9
    if w.size > 500:
        for pop in (np.isnan(w), w == 0, w < 0, np.isposinf(w), (w > 0) & (w < RW.WEIGHT_MIN), np.isfinite(w) & (w > RW.WEIGHT_MAX)):
            assert 0.02 < pop.mean() < 0.08
    wE, wS, rhs, idiag = (got["coef"][:, j] for j in range(4))
    for name, a, b in (("wE", wE, st["wE"]), ("wS", wS, st["wS"]), ("p", got["pq"][:, 0], st["p"]), ("q", got["pq"][:, 1], st["q"]),
                       ("idiag", idiag, st["idiag"])):
        assert np.array_equal(bits(a), bits(b)), name
    assert np.array_equal(bits(got["zeta0"]), bits(G.dev_setup(i)["zeta0"]))    # the weight does not reach zeta0
    if w.size > 500:
        assert not np.array_equal(idiag, st0["idiag"])
    # the scalar test's bound with lam_i for lam: only lam_i zeta0 sees the logarithm, then five roundings
    lam_i = st["lam_i"]
    wgE, wgS = np.abs(st["wE"] * st["gE"]), np.abs(st["wS"] * st["gS"])
    big = lam_i * np.abs(st["zeta0"]) + wgE + R._shift(wgE, -1, 0) + wgS + R._shift(wgS, 0, -1)
    bound = lam_i * LOG_ULP * np.spacing(np.abs(st["zeta0"])) + 5 * np.spacing(big)
    err = np.abs(rhs - st["rhs"])
    print("rhs: largest error / bound", (err / bound).max())
    assert (err <= bound).all()
    # A: the exact minimum over the device's own planes and the clamped map; the table from that A
    s = ((wE + R._shift(wE, -1, 0)) + wS) + R._shift(wS, 0, -1)
    a = np.where(s > 0, lam_i / (lam_i + np.where(s > 0, s, 1.0)), np.inf)
    assert np.array_equal(bits(got["A"]), bits(RW.lower_end(a)))
    assert np.array_equal(bits(got["table"]), bits(RW.table(got["A"])))
    dead = CASES[i][4]
    if dead is not None:
        assert got["A"][dead] == 0 and (got["table"][dead] == 0).all() and (got["A"][[0, 2]] > 0).all()
        assert (got["A"][[0, 2]] < R.LAM / (R.LAM + G.dev_setup(i)["S"][[0, 2]])).all()      # a small weight lowers the end
    if CASES[i][1] * CASES[i][2] == 1:
        assert got["A"][0] == 0 and (got["table"] == 0).all()                   # one pixel has no edge


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_weights_kernel_returns_numpys_bits(i):
    from polardepth import refine
    c, _, t = case(i)
    b, bd = scale_b(i)
    N, H, W = c["depth"].shape
    rng = np.random.default_rng(6000 + i)
    z0 = rng.uniform(0.0, 1.0, (N, H, W))
    zp = z0 + rng.choice([0.0, 1e-4, -0.004, 0.005, -0.005, 0.0050001, 0.02, -0.3, np.nan], (N, H, W))
    z0d, zpd = torch.from_numpy(z0).cuda(), torch.from_numpy(zp).cuda()
    for name, kw, ref in (("plain", {}, {}), ("b", dict(uncertainty=bd, unc_ref=0.003), dict(b=b, unc_ref=0.003)),
                          ("zeta_prev", dict(zeta_prev=zpd, zeta0=z0d, robust=0.005), dict(zeta_prev=zp, zeta0=z0, c=0.005)),
                          ("both", dict(uncertainty=bd, zeta_prev=zpd, zeta0=z0d, robust=0.005), dict(b=b, zeta_prev=zp, zeta0=z0, c=0.005))):
        got = refine.weights(t["depth"], **kw).cpu().numpy()
        want = RW.weights(c["depth"], **ref)
        assert got.dtype == np.float32 and got.shape == want.shape
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), name
        assert np.array_equal(bits(got[~nan]), bits(want[~nan])), name
        if name == "plain":
            assert (got == 1).all()
        elif got.size > 500:
            assert nan.any() == ("b" in ref) and (got[~nan] != 1).any()


def _tolerance(c, ref, kw, samples=4):
    """The scalar test's rule: 4 x the largest change of the reference's zeta and residual when zeta0 moves by LOG_ULP ulp in
    random directions."""
    rng = np.random.default_rng(99)
    z0 = ref["setup"]["zeta0"]
    worst = 0.0
    for _ in range(samples):
        moved = z0 + rng.choice([-1.0, 1.0], z0.shape) * LOG_ULP * np.spacing(np.abs(z0))
        o = RW.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], zeta0=moved, **kw)
        worst = max(worst, float(np.abs(o["zeta"] - ref["zeta"]).max()), float(np.abs(o["residual"] - ref["residual"]).max()))
    return 4 * worst


@pytest.mark.parametrize("mode", ["weight", "uncertainty-robust"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_end_to_end(i, mode):
    from polardepth import refine
    c, _, t = case(i)
    N, H, W = c["depth"].shape
    if mode == "weight":
        kw, dkw = dict(weight=wild(i)[0]), dict(weight=wild(i)[1])
    else:
        kw, dkw = dict(uncertainty=scale_b(i)[0], unc_ref=0.004, robust=0.005, rounds=2), \
            dict(uncertainty=scale_b(i)[1][:, None], unc_ref=0.004, robust=0.005, rounds=2)
    ref = RW.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], **kw)
    tol = _tolerance(c, ref, kw)
    xolp = t["xolp"][..., :W]                                                   # ldp > W: a view, read in place
    out, wmap = refine.polar_refine(t["depth"], t["K"], None, xolp, valid=t["valid"], normals=t["normal"], return_weight=True, **dkw)
    _, _, _, zeta = refine.solve(t["depth"], t["K"], t["normal"], xolp, c["ldp"], t["valid"], R.LAM, R.ITERS, R.EDGE_MAX,
                                 R.INCIDENCE_MAX_DEG, weight=wmap)
    torch.cuda.synchronize()
    assert out.choice is None and out.depth.shape == t["depth"].shape and wmap.shape == (N, H, W) and wmap.dtype == torch.float32
    depth, touched, res, zeta = out.depth.cpu().numpy(), out.touched.cpu().numpy(), out.residual.cpu().numpy(), zeta.cpu().numpy()
    assert np.array_equal(touched, ref["touched"])
    un = touched == 0
    assert np.array_equal(bits(depth[un]), bits(c["depth"][un]))                # the copied pixels, NaN payloads included
    ez = float(np.abs(zeta - ref["zeta"]).max())
    on = ~un
    want = ref["depth"][on].astype(F64)
    ed = (np.abs(depth[on].astype(F64) - want) / np.spacing(ref["depth"][on]).astype(F64)).max() if on.any() else 0.0
    er = float(np.abs(res - ref["residual"]).max())
    print(f"tolerance {tol:.3g}; zeta off by {ez:.3g}, depth by {ed:.3g} fp32 ulp, residual by {er:.3g} (residual {ref['residual']})")
    assert ez <= tol and er <= tol
    assert ed <= EXP_ULP + tol / 2.0 ** -24                                     # an fp32 ulp is at least 2^-24 relative
    dead = CASES[i][4]
    if dead is not None:
        assert res[dead] == 0 and not touched[dead].any()
    if on.any():
        assert (depth[on] != c["depth"][on]).any() and np.isfinite(depth[on]).all()
        plain = refine.polar_refine(t["depth"], t["K"], None, xolp, valid=t["valid"], normals=t["normal"])
        assert torch.equal(plain.touched, out.touched)
        assert depth.size < 500 or not torch.equal(plain.depth, out.depth)      # a handful of pixels may all clamp to 1
    if mode == "weight":
        assert np.array_equal(bits(wmap.cpu().numpy()[~np.isnan(kw["weight"])]), bits(kw["weight"][~np.isnan(kw["weight"])]))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_fused_route_returns_the_one_step_routes_bits_from_weighted_coefficients(i):
    """iters = 11 is no multiple of T: the last launch takes what is left."""
    from polardepth import refine
    c, _, t = case(i)
    args = (t["depth"], t["K"], t["normal"], t["xolp"], c["ldp"], t["valid"], R.LAM, 11, R.EDGE_MAX, R.INCIDENCE_MAX_DEG)
    kw = dict(weight=wild(i)[1], weight_min=1 / 32, weight_max=2.0)
    want = refine.solve(*args, fused=0, **kw)
    for T in (1, 3, 8):
        got = refine.solve(*args, fused=T, **kw)
        torch.cuda.synchronize()
        for name, a, b in zip(("depth", "residual", "touched", "zeta"), got, want):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (T, name)
    if c["depth"][0].size > 1:
        assert want[2].any()
    if c["depth"].size > 500:
        other = refine.solve(*args, fused=0, weight=wild(i)[1])                 # the clamp is read
        assert not torch.equal(want[3], other[3])
    z0 = torch.full_like(want[3], float("nan"))                                 # zeta0 comes back where it is asked for
    refine.solve(*args, zeta0_out=z0, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(bits(z0.cpu().numpy()), bits(G.dev_setup(i)["zeta0"]))


def test_two_calls_and_a_replayed_capture_return_the_same_bits():
    from polardepth import refine
    depth, K, pol, xolp = G._full_inputs()
    b = (0.002 + 0.02 * torch.rand(depth.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)))
    b[0, 0, :3] = float("nan")
    kw = dict(iters=11, uncertainty=b, robust=0.005, rounds=2, weight=torch.full_like(depth, 0.75), return_weight=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires
        a, wa = refine.polar_refine(depth, K, pol, xolp, **kw)
        b2, wb = refine.polar_refine(depth, K, pol, xolp, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(tuple(a) + (wa,), tuple(b2) + (wb,)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        g, wg = refine.polar_refine(depth, K, pol, xolp, **kw)
    g.depth.zero_()
    g.touched.zero_()
    g.residual.fill_(-1.0)
    wg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(tuple(a) + (wa,), tuple(g) + (wg,)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert a.touched.any() and (wa[~wa.isnan()] < 0.75).any() and wa.isnan().any()
    one = refine.polar_refine(depth, K, pol, xolp, iters=11, rounds=2)
    assert not torch.equal(one.depth, a.depth)
    with pytest.raises(ValueError, match="rounds >= 2"):
        refine.polar_refine(depth, K, pol, xolp, robust=0.005)
    with pytest.raises(ValueError, match="uncertainty must be"):
        refine.polar_refine(depth, K, pol, xolp, uncertainty=b[..., :-1])
    with pytest.raises(ValueError, match="weight must be"):
        refine.polar_refine(depth, K, pol, xolp, weight=b[:, 0, :-1])


# ---- Evaluation and the export tool

def test_evaluation_weights_the_prior_with_its_own_uncertainty():
    from manydepth.evaluation import Evaluation
    from polardepth import polar as pdpolar
    from polardepth import refine
    torch.manual_seed(0)
    plain = Evaluation(uncertainty=True, polar_refine=dict(iters=20), **G.KW)
    torch.manual_seed(0)
    ev = Evaluation(uncertainty=True, polar_refine={"uncertainty": True, "iters": 20}, **G.KW)
    assert ev.polar_refine == {"uncertainty": True, "iters": 20}
    inputs = G._first(ev)
    out, base = ev.predict_all(inputs), plain.predict_all(G._first(plain))
    assert set(out) == set(base)
    for k in base:                                                              # the same networks: only the refinement moves
        same = torch.equal(out[k].view(torch.int32), base[k].view(torch.int32)) if out[k].dtype == torch.float32 else torch.equal(out[k], base[k])
        assert same == (k not in ("depth_refined", "refine_residual")), k
    touched = out["refine_touched"].bool()[:, None]
    assert touched.any() and torch.isfinite(out["depth_refined"][touched]).all()
    pol = pdpolar.polar_inputs(inputs, (64, 96), ("xolp", "normals"), ev.pol_angles)
    hand = refine.polar_refine(out["depth"], inputs[("K", 0)], pol, inputs["xolp", 0, 0], iters=20, aolp_sign=ev.aolp_sign,
                               ray_frame=ev.polar_ray_frame, uncertainty=out["uncertainty"])
    assert torch.equal(out["depth_refined"].view(torch.int32), hand.depth.view(torch.int32))
    rep = ev.test_depth(source="refined")
    assert rep["all"]["pooled"][-1] > 0 and not np.array_equal(rep["all"]["pooled"], plain.test_depth(source="refined")["all"]["pooled"])
    with pytest.raises(ValueError, match=r"needs Evaluation\(uncertainty=True\)"):
        Evaluation(polar_refine={"uncertainty": True}, **G.KW)


def test_export_writes_points_with_both_new_flags(tmp_path):
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_pointcloud as E

    def xyz(path):
        _, payload = open(path, "rb").read().split(b"end_header\n", 1)
        return np.frombuffer(payload, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])

    rows = {}
    for name, kw in (("refined", dict(refine=True, refine_iters=20)),
                     ("weighted", dict(refine=True, refine_iters=20, refine_uncertainty=True, refine_robust=0.005)),
                     ("tau", dict(refine=True, refine_iters=20, refine_uncertainty=0.004))):
        torch.manual_seed(0)
        out = str(tmp_path / name)
        E.export("synthetic", None, 0, out, height=64, width=96, **kw)
        rows[name] = xyz(os.path.join(out, "pred.ply"))
    assert len(rows["refined"]) > 0 and len(rows["weighted"]) == len(rows["refined"]) == len(rows["tau"])
    assert np.isfinite(rows["weighted"]["xyz"]).all()
    assert not np.array_equal(rows["weighted"]["xyz"], rows["refined"]["xyz"])
    assert not np.array_equal(rows["tau"]["xyz"], rows["weighted"]["xyz"])
    for kw in (dict(refine_uncertainty=True), dict(refine_robust=0.005)):
        with pytest.raises(ValueError, match="--refine"):
            E.export("synthetic", None, 0, str(tmp_path / "x"), height=64, width=96, **kw)
