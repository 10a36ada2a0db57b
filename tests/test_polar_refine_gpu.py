"""pd_polar_refine_* and polardepth.refine.polar_refine on the GPU against tests/polar_refine_ref.py.

Setup: the live edges, wE, wS, p, q and 1/diag bit for bit (they hold only IEEE + x / sqrt, and no gate decision of the cases
lies within 1e-9 of its threshold); zeta0 within LOG_ULP of np.log, rhs within the bound that follows from it.  Table: bit for
bit from the device's own S, and S is the maximum of the device's own weights.  Step: from the reference's coefficients, zeta and
d bit for bit after 1, 2 and 7 steps.  End to end: zeta, depth and residual within the tolerance that the reference's own
response to a zeta0 perturbed by LOG_ULP gives (times 4, the perturbation is sampled); touched and the copied pixels bit for
bit.  The fused route (T steps per launch) returns the one-step route's bits.  Two calls and a captured, replayed call return the
eager bits.  Measured on the MI355X: the device's log at most 1.0 ulp from np.log (97.8 % of 13,517 depths exact), rhs at 0.35 of
its bound, the end-to-end tolerance 2.2e-16 .. 9.8e-15 with zeta 0 .. 2.6e-15 off, depth 0 fp32 ulp off."""
import numpy as np
import pytest
import torch

import polar_refine_ref as R

pytestmark = pytest.mark.gpu

F64 = np.float64
LOG_ULP = 1                 # the largest |device log - np.log| measured on the cases' depths, in fp64 ulp
EXP_ULP = 1                 # fp32 ulp: the device's exp(zeta) rounded to fp32 against np.exp's (tests/test_unc_loss_gpu.py)
# N, H, W, ldp (None = W), the item without polarisation
CASES = [(1, 1, 1, None, None), (1, 1, 7, None, None), (1, 5, 1, None, None), (2, 13, 67, 72, None), (3, 37, 130, None, 1)]
IDS = ["1x1x1", "1x1x7", "1x5x1", "2x13x67-ldp72", "3x37x130-dead1"]
_CACHE = {}


def lib():
    from polardepth._lib import lib as L, check, ptr
    return L, check, ptr


def case(i):
    """The inputs of CASES[i] on the host and on the device, and the reference's setup: computed once, never written to."""
    if i not in _CACHE:
        N, H, W, ldp, dead = CASES[i]
        c = R.case(N, H, W, ldp=ldp, dead_item=dead)
        st = R.setup(c["depth"], c["K"], c["normal"], c["rho"], c["valid"])
        t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("depth", "K", "normal", "xolp", "valid")}
        _CACHE[i] = (c, st, t)
    return _CACHE[i]


def dev_setup(i, lam=R.LAM):
    """pd_polar_refine_setup + _table on CASES[i] -> dict of host arrays (zeta0, coef, pq, S, table) ."""
    key = ("setup", i)
    if key not in _CACHE:
        L, check, ptr = lib()
        c, _, t = case(i)
        N, H, W = c["depth"].shape
        f64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
        zeta0, coef, pq, S, table = f64(N, H, W), f64(N, 4, H, W), f64(N, 2, H, W), f64(N), f64(N, R.ITERS, 2)
        ws = torch.empty(int(L.pd_polar_refine_workspace(N, H, W)), dtype=torch.uint8, device="cuda")
        check(L.pd_polar_refine_setup(ptr(t["depth"]), ptr(t["K"]), ptr(t["normal"]), ptr(t["xolp"]), c["ldp"], ptr(t["valid"]), lam,
                                      R.EDGE_MAX, R.cos_inc_of(R.INCIDENCE_MAX_DEG), ptr(zeta0), ptr(coef), ptr(pq), ptr(ws),
                                      ws.numel(), N, H, W, None), "pd_polar_refine_setup")
        check(L.pd_polar_refine_table(ptr(ws), ws.numel(), lam, R.ITERS, ptr(S), ptr(table), N, H, W, None), "pd_polar_refine_table")
        torch.cuda.synchronize()
        _CACHE[key] = {k: v.cpu().numpy() for k, v in (("zeta0", zeta0), ("coef", coef), ("pq", pq), ("S", S), ("table", table))}
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_setup(i):
    c, st, _ = case(i)
    got = dev_setup(i)
    # no gate decision within reach of an ulp
    assert st["dz_margin"] > 1e-9
    m = st["margin"][np.isfinite(st["margin"])]
    assert m.size == 0 or np.abs(m).min() > 1e-9
    wE, wS, rhs, idiag = (got["coef"][:, j] for j in range(4))
    assert np.array_equal(wE > 0, st["wE"] > 0) and np.array_equal(wS > 0, st["wS"] > 0)
    for name, a, b in (("wE", wE, st["wE"]), ("wS", wS, st["wS"]), ("p", got["pq"][:, 0], st["p"]), ("q", got["pq"][:, 1], st["q"]),
                       ("idiag", idiag, st["idiag"])):
        assert np.array_equal(bits(a), bits(b)), name
    good = np.isfinite(c["depth"]) & (c["depth"] > 0)
    assert (got["zeta0"][~good] == 0).all() and not np.signbit(got["zeta0"][~good]).any()
    ulps = np.abs(got["zeta0"] - st["zeta0"])[good] / np.spacing(np.abs(st["zeta0"][good]))
    print("device log vs np.log on", int(good.sum()), "depths: max", ulps.max() if ulps.size else 0.0, "ulp; exact share",
          (ulps == 0).mean() if ulps.size else 1.0)
    assert ulps.size == 0 or ulps.max() <= LOG_ULP
    # rhs = (((lam zeta0 - wE gE) + wW gW) - wS gS) + wN gN: only the first product sees the logarithm; it is off by at most
    # lam LOG_ULP ulp(zeta0), and each of the five roundings may then fall the other way: one spacing of the largest
    # intermediate each
    wgE, wgS = np.abs(st["wE"] * st["gE"]), np.abs(st["wS"] * st["gS"])
    big = R.LAM * np.abs(st["zeta0"]) + wgE + R._shift(wgE, -1, 0) + wgS + R._shift(wgS, 0, -1)
    bound = R.LAM * LOG_ULP * np.spacing(np.abs(st["zeta0"])) + 5 * np.spacing(big)
    err = np.abs(rhs - st["rhs"])
    print("rhs: largest error / bound", (err / bound).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_table(i):
    got = dev_setup(i)
    wE, wS = got["coef"][:, 0], got["coef"][:, 1]
    s = ((wE + R._shift(wE, -1, 0)) + wS) + R._shift(wS, 0, -1)
    assert np.array_equal(bits(got["S"]), bits(s.reshape(len(s), -1).max(1)))
    assert np.array_equal(bits(got["table"]), bits(R.table(got["S"])))
    dead = CASES[i][4]
    if dead is not None:
        assert got["S"][dead] == 0 and (got["table"][dead] == 0).all() and (got["S"][[0, 2]] > 0).all()
    if CASES[i][1] * CASES[i][2] == 1:
        assert got["S"][0] == 0                                                 # one pixel has no edge


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_steps_are_the_references_bit_for_bit(i):
    L, check, ptr = lib()
    c, st, _ = case(i)
    N, H, W = c["depth"].shape
    coef_h, tab_h = R.coef_planes(st), R.table(st["S"], iters=9)
    coef, tab = torch.from_numpy(coef_h).cuda(), torch.from_numpy(tab_h).cuda()
    z = [torch.from_numpy(st["zeta0"].copy()).cuda(), torch.full((N, H, W), float("nan"), dtype=torch.float64, device="cuda")]
    d = torch.full((N, H, W), float("nan"), dtype=torch.float64, device="cuda")      # step 0 must not read it
    zr, dr = st["zeta0"].copy(), np.zeros_like(st["zeta0"])
    for k in range(7):
        check(L.pd_polar_refine_step(ptr(coef), ptr(tab), 9, k, ptr(z[k % 2]), ptr(z[(k + 1) % 2]), ptr(d), N, H, W, None),
              "pd_polar_refine_step")
        zr, dr = R.step(coef_h, tab_h, k, zr, dr)
        if k + 1 in (1, 2, 7):
            torch.cuda.synchronize()
            assert np.array_equal(bits(z[(k + 1) % 2].cpu().numpy()), bits(zr)), k
            assert np.array_equal(bits(d.cpu().numpy()), bits(dr)), k
    touched = R.residual(coef_h, zr)[1]
    assert np.array_equal(bits(zr[~touched]), bits(st["zeta0"][~touched]))
    assert not touched.any() or (zr[touched] != st["zeta0"][touched]).any()
    dead = CASES[i][4]
    if dead is not None:                                                        # S = 0: the item stays where it was
        assert np.array_equal(bits(z[1].cpu().numpy()[dead]), bits(st["zeta0"][dead])) and (d.cpu().numpy()[dead] == 0).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_fused_route_returns_the_one_step_routes_bits(i):
    """iters = 11 is no multiple of T: the last launch takes what is left.  The images smaller than the rim are among the cases."""
    from polardepth import refine
    c, _, t = case(i)
    N, H, W = c["depth"].shape
    args = (t["depth"], t["K"], t["normal"], t["xolp"], c["ldp"], t["valid"], R.LAM, 11, R.EDGE_MAX, R.INCIDENCE_MAX_DEG)
    want = refine.solve(*args, fused=0)
    for T in (1, 3, 8):
        got = refine.solve(*args, fused=T)
        torch.cuda.synchronize()
        for name, a, b in zip(("depth", "residual", "touched", "zeta"), got, want):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (T, name)
    if H * W > 1:
        assert want[2].any() and not torch.equal(want[0], t["depth"])
    # d as well: one launch of T = 8 against eight one-step launches, from the reference's coefficients
    L, check, ptr = lib()
    st = case(i)[1]
    coef, tab = torch.from_numpy(R.coef_planes(st)).cuda(), torch.from_numpy(R.table(st["S"], iters=16)).cuda()
    nan = lambda: torch.full((N, H, W), float("nan"), dtype=torch.float64, device="cuda")
    z = [torch.from_numpy(st["zeta0"].copy()).cuda(), nan()]
    d = nan()
    for k in range(16):
        check(L.pd_polar_refine_step(ptr(coef), ptr(tab), 16, k, ptr(z[k % 2]), ptr(z[(k + 1) % 2]), ptr(d), N, H, W, None), "step")
    zf, df = [z[0].new_tensor(st["zeta0"]), nan(), nan()], [nan(), nan()]
    check(L.pd_polar_refine_steps(ptr(coef), ptr(tab), 16, 0, 8, ptr(zf[0]), ptr(zf[1]), None, ptr(df[0]), N, H, W, None), "steps")
    check(L.pd_polar_refine_steps(ptr(coef), ptr(tab), 16, 8, 8, ptr(zf[1]), ptr(zf[2]), ptr(df[0]), ptr(df[1]), N, H, W, None), "steps")
    torch.cuda.synchronize()
    assert zf[2].cpu().numpy().tobytes() == z[0].cpu().numpy().tobytes()
    assert df[1].cpu().numpy().tobytes() == d.cpu().numpy().tobytes()


def _tolerance(c, ref, samples=4):
    """4 x the largest change of the reference's zeta and residual when zeta0 moves by LOG_ULP ulp in random directions."""
    rng = np.random.default_rng(99)
    z0 = ref["setup"]["zeta0"]
    worst = 0.0
    for _ in range(samples):
        moved = z0 + rng.choice([-1.0, 1.0], z0.shape) * LOG_ULP * np.spacing(np.abs(z0))
        o = R.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"], zeta0=moved)
        worst = max(worst, float(np.abs(o["zeta"] - ref["zeta"]).max()), float(np.abs(o["residual"] - ref["residual"]).max()))
    return 4 * worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_end_to_end(i):
    from polardepth import refine
    c, _, t = case(i)
    N, H, W = c["depth"].shape
    ref = R.refine(c["depth"], c["K"], c["normal"], c["rho"], c["valid"])
    tol = _tolerance(c, ref)
    xolp = t["xolp"][..., :W]                                                   # ldp > W: a view, read in place
    assert refine._dolp_pitch(xolp, H, W)[0] is xolp and refine._dolp_pitch(xolp, H, W)[1] == c["ldp"]
    out = refine.polar_refine(t["depth"], t["K"], None, xolp, valid=t["valid"], normals=t["normal"])
    _, _, _, zeta = refine.solve(t["depth"], t["K"], t["normal"], xolp, c["ldp"], t["valid"], R.LAM, R.ITERS, R.EDGE_MAX,
                                 R.INCIDENCE_MAX_DEG)
    torch.cuda.synchronize()
    assert out.choice is None and out.depth.shape == t["depth"].shape
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


def _full_inputs(N=2, H=21, W=70):
    """A depth prior, K1's nine candidate planes and the DoLP for the whole path (disambiguation included)."""
    c = R.case(N, H, W, seed=3)
    rng = np.random.default_rng(8)
    depth = np.where(np.isfinite(c["depth"]) & (c["depth"] > 0), c["depth"], 1.5).astype(np.float32)
    v = rng.standard_normal((N, 3, 3, H, W)) + np.array([0, 0, 1.5]).reshape(1, 1, 3, 1, 1)
    pol = (v / np.linalg.norm(v, axis=2, keepdims=True)).reshape(N, 9, H, W).astype(np.float32)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return cuda(depth)[:, None], cuda(c["K"]), cuda(pol), cuda(c["xolp"])


def test_the_whole_path_is_the_disambiguation_then_the_solve():
    from polardepth import polar_normals_eval as pe
    from polardepth import refine, ops
    depth, K, pol, xolp = _full_inputs()
    out = refine.polar_refine(depth, K, pol, xolp, iters=11, ray_frame=True, aolp_sign=-1)
    st = pe.polar_normals_stats(depth, pol, xolp, K=K, classes=(("all", None),), maps=True, ray_frame=True, aolp_sign=-1)
    by_hand = refine.polar_refine(depth, K, None, xolp, iters=11, normals=st.pol_normal)
    assert out.depth.shape == depth.shape and torch.equal(out.choice, st.choice) and (out.choice != 0).any()
    assert torch.equal(out.depth.view(torch.int32), by_hand.depth.view(torch.int32))
    assert torch.equal(out.touched, by_hand.touched) and torch.equal(out.residual, by_hand.residual)
    assert out.touched.any() and not out.touched[(st.choice == 0)].any()        # no normal, no edge
    alias = ops.polar_refine(depth, K, pol, xolp, iters=11, ray_frame=True, aolp_sign=-1)
    assert torch.equal(alias.depth.view(torch.int32), out.depth.view(torch.int32))
    # a second round disambiguates against the refined depth and starts again from the prior
    two = refine.polar_refine(depth, K, pol, xolp, iters=11, rounds=2)
    one = refine.polar_refine(depth, K, pol, xolp, iters=11)
    st2 = pe.polar_normals_stats(one.depth, pol, xolp, K=K, classes=(("all", None),), maps=True)
    again = refine.polar_refine(depth, K, None, xolp, iters=11, normals=st2.pol_normal)
    assert torch.equal(two.depth.view(torch.int32), again.depth.view(torch.int32)) and torch.equal(two.choice, st2.choice)
    # an [N,H,W] prior comes back as [N,H,W]; an empty batch is a no-op
    flat = refine.polar_refine(depth[:, 0], K, pol, xolp, iters=11)
    assert flat.depth.shape == depth[:, 0].shape and torch.equal(flat.depth, one.depth[:, 0])
    empty = refine.polar_refine(depth[:0], K[:0], pol[:0], xolp[:0])
    assert empty.depth.shape == (0,) + tuple(depth.shape[1:]) and empty.residual.shape == (0,)
    for bad in (dict(lam=0.0), dict(iters=0), dict(edge_max=float("nan")), dict(incidence_max_deg=90.0), dict(rounds=0)):
        with pytest.raises(ValueError):
            refine.polar_refine(depth, K, pol, xolp, **bad)
    with pytest.raises(ValueError, match="xolp must be"):
        refine.polar_refine(depth, K, pol, xolp[..., :-1])
    with pytest.raises(ValueError, match="pol_normals must be"):
        refine.polar_refine(depth, K, pol[:, :8], xolp)
    with pytest.raises(ValueError, match="normals must be"):
        refine.polar_refine(depth, K, None, xolp, normals=pol)
    with pytest.raises(ValueError, match="K must be"):
        refine.polar_refine(depth, K[:, :3], pol, xolp)


def test_two_calls_and_a_replayed_capture_return_the_same_bits():
    from polardepth import refine
    depth, K, pol, xolp = _full_inputs()
    kw = dict(iters=11)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires (builds the table)
        a = refine.polar_refine(depth, K, pol, xolp, **kw)
        b = refine.polar_refine(depth, K, pol, xolp, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(a[:3], b[:3]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        g = refine.polar_refine(depth, K, pol, xolp, **kw)
    g.depth.zero_()
    g.touched.zero_()
    g.residual.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, g):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert a.touched.any()


# ---- Evaluation

KW = dict(data_path="synthetic", height=64, width=96, batch_size=4)


@pytest.fixture(scope="module")
def evs():
    from manydepth.evaluation import Evaluation
    torch.manual_seed(0)
    plain = Evaluation(**KW)
    torch.manual_seed(0)
    return plain, Evaluation(polar_refine=dict(iters=20), **KW)


def _first(ev):
    return {k: v.cuda() for k, v in next(iter(ev.test_loader)).items()}


def test_evaluation_returns_the_refined_depth(evs):
    from polardepth import polar as pdpolar
    from polardepth import refine
    plain, ev = evs
    assert plain.polar_refine is None and ev.polar_refine == {"iters": 20}
    inputs = _first(ev)
    out = ev.predict_all(inputs)
    base = plain.predict_all(_first(plain))
    assert "depth_refined" not in base and "refine_residual" not in base and "refine_touched" not in base
    assert set(out) == set(base) | {"depth_refined", "refine_residual", "refine_touched"}
    for k in base:                                                              # the other outputs do not move
        assert torch.equal(out[k].view(torch.int32), base[k].view(torch.int32)), k
    pol = pdpolar.polar_inputs(inputs, (64, 96), ("xolp", "normals"), ev.pol_angles)
    hand = refine.polar_refine(out["depth"], inputs[("K", 0)], pol, inputs["xolp", 0, 0], iters=20, aolp_sign=ev.aolp_sign,
                               ray_frame=ev.polar_ray_frame)
    assert out["depth_refined"].shape == out["depth"].shape
    assert torch.equal(out["depth_refined"].view(torch.int32), hand.depth.view(torch.int32))
    assert torch.equal(out["refine_touched"], hand.touched) and torch.equal(out["refine_residual"], hand.residual)
    assert out["refine_touched"].any() and not torch.equal(out["depth_refined"], out["depth"])
    assert torch.equal(plain.predict(_first(plain)).view(torch.int32), ev.predict(_first(ev)).view(torch.int32))


def test_evaluation_scores_the_refined_depth(evs, capsys, monkeypatch):
    from manydepth.evaluation import Evaluation
    plain, ev = evs
    mono, refined = ev.test_depth(source="mono"), ev.test_depth(source="refined")
    assert list(mono) == list(refined)
    for name in mono:
        assert mono[name]["pooled"][-1] == refined[name]["pooled"][-1], name                     # n: the same pixels are scored
    assert mono["all"]["pooled"][-1] > 0 and not np.array_equal(mono["all"]["pooled"], refined["all"]["pooled"])
    a, b = plain.test_depth(), ev.test_depth()
    assert all(np.array_equal(a[k]["pooled"], b[k]["pooled"]) and np.array_equal(a[k]["per_image"], b[k]["per_image"]) for k in a)
    nd, nr = ev.test_normals(source="depth"), ev.test_normals(source="refined")
    assert nd["all"]["pooled"][6] > 0 and nr["all"]["pooled"][6] > 0 and not np.array_equal(nd["all"]["pooled"], nr["all"]["pooled"])
    pn = plain.test_normals(source="depth")
    assert all(np.array_equal(pn[k]["pooled"], nd[k]["pooled"]) for k in pn)
    for call in (plain.test_depth, plain.test_normals):
        with pytest.raises(ValueError, match="polar_refine=True"):
            call(source="refined")
    with pytest.raises(ValueError, match="source must be"):
        ev.test_depth(source="polar")
    # the environment: "1" = the conventions, "lam,iters" = those two; the argument wins
    capsys.readouterr()
    monkeypatch.setenv("PD_POLAR_REFINE", "1")
    assert Evaluation(**KW).polar_refine == {}
    monkeypatch.setenv("PD_POLAR_REFINE", "0.05,30")
    assert Evaluation(**KW).polar_refine == {"lam": 0.05, "iters": 30}
    assert Evaluation(polar_refine=False, **KW).polar_refine is None
    monkeypatch.delenv("PD_POLAR_REFINE")
    assert Evaluation(polar_refine=True, **KW).polar_refine == {} and Evaluation(**KW).polar_refine is None
    for bad in ({"lam": -1.0}, {"steps": 3}, "fast", 3):
        with pytest.raises(ValueError):
            Evaluation(polar_refine=bad, **KW)


def test_export_writes_the_refined_points(tmp_path):
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_pointcloud as E

    def xyz(path, with_normals):
        _, payload = open(path, "rb").read().split(b"end_header\n", 1)
        dt = [("xyz", "<f4", 3)] + ([("n", "<f4", 3)] if with_normals else []) + [("rgb", "u1", 3)]
        return np.frombuffer(payload, dtype=dt)

    rows = {}
    for name, kw in (("plain", {}), ("refined", dict(refine=True, refine_iters=20)),
                     ("both", dict(refine=True, refine_iters=20, normals="polar"))):
        torch.manual_seed(0)
        out = str(tmp_path / name)
        E.export("synthetic", None, 0, out, height=64, width=96, **kw)
        rows[name] = xyz(os.path.join(out, "pred.ply"), "normals" in kw)
    assert len(rows["plain"]) > 0 and len(rows["refined"]) > 0
    assert not np.array_equal(rows["plain"]["xyz"], rows["refined"]["xyz"])      # other depths
    assert np.array_equal(rows["both"]["xyz"], rows["refined"]["xyz"])          # --normals polar composes
    with pytest.raises(ValueError, match="--refine"):
        E.export("synthetic", None, 0, str(tmp_path / "x"), height=64, width=96, refine_lam=0.1)
