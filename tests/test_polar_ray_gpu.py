"""The per-pixel viewing-ray frame on the GPU: pd_polar_normals_stats_ray, pd_polar_loss_fwd_ray / _bwd_ray and their Python
layers against the NumPy statement (tests/polar_ray_ref.py, pinned by tests/test_polar_ray_ref.py) applied to the very arrays
handed to the kernels.  Per-item intrinsics throughout (polar_ray_ref.intrinsics): fx != fy, an off-centre principal point, item
0's principal point exactly on a pixel, the last item with a short focal length (fx = 0.3 W).

Evaluator: n, every counter, both histograms, choice, the NaN / zero patterns equal; pol_normal bit-equal; the eight sums to
rtol 1e-11 and the degree maps to 1e-5 degrees, the bounds tests/test_polar_normals_gpu.py derives.  Loss, forward: p is taken
from pd_gt_normals on the device; state, counters and maps bit-equal, the four sums within (n - 1) 2^-53 of math.fsum, the
values the fp32 rounding of the ratio.  Backward: against the fp64 autograd reference with the DEVICE's own state, by the rule of
loss_cases.py: |dev - ref64| <= 4 max|ref32 - ref64| + 1e-6 max|ref64|, elementwise.  With ray_frame = 0 the new entry points
give the bytes of the old ones."""
import functools
import math

import numpy as np
import pytest
import torch

import loss_cases as LC
import polar_loss_cases as C
import polar_loss_ref as LR
import polar_normals_ref as NR
import polar_ray_ref as RR

pytestmark = pytest.mark.gpu

F32_MAX = float(np.finfo(np.float32).max)
# (N, H, W, ldp, ld): less than a wave | padded rows, both pixel strides | 2080 pixels: more than one workgroup per image
SHAPES = [(1, 1, 4, 4, 3), (2, 5, 20, 24, 3), (2, 5, 20, 24, 4), (3, 40, 52, 52, 4)]
TILT_DEG = 5.0
TILT2 = math.sin(math.radians(TILT_DEG)) ** 2
OPTS = dict(rho_min=C.RHO_MIN, rho_max=C.RHO_MAX, tilt_min_deg=C.TILT_DEG)
# (2,9,65), (1,17,129): straddle the 8 x 64 tile; (1,2,2): smaller than a Sobel window; (1,32808,17): more pixels than a forward
# trip and more tiles than a backward trip
LOSS_GEOMS = [(2, 9, 65), (1, 17, 129), (2, 21, 70), C.PITCHED, (1, 2, 2), (1, 32808, 17)]


def PE():
    from polardepth import polar_normals_eval
    return polar_normals_eval


def OPS():
    from polardepth import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a writable copy


def _edges():
    from polardepth import normals_eval
    return normals_eval.cos_edges_numpy()


def _classes(K):
    from polardepth import normals_eval
    return [("all", None)] if K == 1 else list(normals_eval.DEFAULT_CLASSES)


def _lohi(classes):
    return [(1, 0) if r is None else tuple(r) for _, r in classes]


# ------------------------------------------------------------------ the evaluator

@functools.lru_cache(maxsize=None)
def ecase(N, H, W, ldp, ld):
    # seeds for which every counter and all six choices are reached in the ray frame too (checked on the statement below)
    c = NR.random_case(1000 + 100 * N + H + W + ld, N, H, W, ldp, ld, masked=True)
    c["K"] = RR.intrinsics(N, H, W)
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ereference(shape, K, ray=True):
    c = ecase(*shape)
    return RR.stats(c["pred"], c["pol"], c["xolp"], c["mask"] if K > 1 else None, _lohi(_classes(K)), _edges(), K=c["K"],
                    ray_frame=ray, valid=c["valid"], tilt2_min=TILT2)


def etensors(shape, K):
    N, H, W, ldp, ld = shape
    c = ecase(*shape)
    pred = _dev(c["pred"]).permute(0, 3, 1, 2)[:, :3]
    pol, xolp = _dev(c["pol"])[..., :W], _dev(c["xolp"])[..., :W]
    mask = _dev(c["mask"])[:, None] if K > 1 else None
    return pred, pol, xolp, mask, _dev(c["valid"])[:, None], _dev(c["K"])


def erun(shape, K, maps=True, ray=True):
    pred, pol, xolp, mask, valid, Km = etensors(shape, K)
    return PE().polar_normals_stats(pred, pol, xolp, K=Km, mask=mask, valid=valid, classes=_classes(K), tilt_min_deg=TILT_DEG,
                                    maps=maps, ray_frame=ray)


def fields(st):
    torch.cuda.synchronize()
    out = {}
    for name, rs in (("normal", st.normal), ("azimuth", st.azimuth)):
        out[name] = {"n": rs.n.cpu().numpy(), "sums": rs.sums.cpu().numpy(), "hist": rs.hist.cpu().numpy().astype(np.int64)}
        for c in rs.counter_names:
            out[name][c] = getattr(rs, c).cpu().numpy()
    for m in ("az_deg", "n_deg", "choice", "pol_normal"):
        out[m] = None if getattr(st, m) is None else getattr(st, m).cpu().numpy()
    return out


def compare(got, ref, what):
    for name in ("normal", "azimuth"):
        for k in ref[name]:
            if k == "sums":
                rel = np.abs(got[name][k] - ref[name][k]) / np.maximum(np.abs(ref[name][k]), 1e-300)
                print(what, name, "sums: max rel err", rel.max())
                assert np.allclose(got[name][k], ref[name][k], rtol=1e-11, atol=0.0), (what, name, rel.max())
            else:
                assert np.array_equal(got[name][k], ref[name][k]), (what, name, k)
    assert np.array_equal(got["choice"], ref["choice"]), what
    assert np.array_equal(got["pol_normal"].view(np.int32), ref["pol_normal"].view(np.int32)), what
    for m in ("az_deg", "n_deg"):
        assert np.array_equal(np.isnan(got[m]), np.isnan(ref[m])), (what, m)
        ok = ~np.isnan(ref[m])
        d = np.abs(got[m][ok].astype(np.float64) - ref[m][ok])
        print(what, m, "max abs err", d.max() if d.size else 0.0)
        assert (d <= 1e-5).all(), (what, m, d.max())


def _bytes(st):
    return [t.cpu().numpy().tobytes() for t in (st.normal.records, st.azimuth.records, st.az_deg, st.n_deg, st.choice, st.pol_normal)]


def test_the_evaluator_cases_reach_every_counter_and_choice_in_the_ray_frame():
    """Asserted on the statement, before anything runs on the device."""
    for shape in SHAPES[1:]:
        ref = ereference(shape, 12)
        for name, counters in (("normal", NR.NORMAL_COUNTERS), ("azimuth", NR.AZIMUTH_COUNTERS)):
            for c in counters:
                assert ref[name][c][:, 0].sum() > 0, (shape, name, c)
        assert set(np.unique(ref["choice"])) == set(range(7)), shape
        assert not np.array_equal(ref["choice"], ereference(shape, 12, False)["choice"])       # the frame decides differently


@pytest.mark.parametrize("K", [1, 12])
@pytest.mark.parametrize("shape", SHAPES)
def test_evaluator_equals_the_statement(shape, K):
    compare(fields(erun(shape, K)), ereference(shape, K), (shape, K))


def _cabi_eval(shape, entry, ray, Km, which=("normal", "azimuth"), fill=0x5A):
    """The C call on a case -> (rec_n, rec_a, az, nd, ch, pn); entry "old" | "ray"."""
    from polardepth._lib import lib, check, ptr, stream_ptr
    from polardepth import normals_eval as ne
    pe = PE()
    N, H, W, ldp, ld = shape
    pred, pol, xolp, mask, valid, _ = etensors(shape, 12)
    names, table = ne.class_table(_classes(12))
    pred_pm, ld_pm = ne.pixel_major(pred)
    assert ld_pm == ld
    mask_i, valid_u = mask[:, 0].contiguous(), valid[:, 0].contiguous()
    ws = torch.empty(int(lib.pd_polar_normals_stats_workspace(N, H, W, 12)), dtype=torch.uint8, device="cuda")
    rec_n = torch.full((N, 12, pe.NORMAL_RECORD_BYTES), fill, dtype=torch.uint8, device="cuda")
    rec_a = torch.full((N, 12, pe.AZIMUTH_RECORD_BYTES), fill, dtype=torch.uint8, device="cuda")
    az, nd = torch.full((N, H, W), 7.0, device="cuda"), torch.full((N, H, W), 7.0, device="cuda")
    ch, pn = torch.full((N, H, W), 9, dtype=torch.uint8, device="cuda"), torch.full((N, H, W, 4), 7.0, device="cuda")
    tail = (ptr(pol), ptr(xolp), ldp, ptr(mask_i), table, 12, ptr(valid_u), ptr(ne.cos_edges("cuda")), 0.05, 1.0, TILT2, 1,
            ptr(rec_n) if "normal" in which else None, ptr(rec_a) if "azimuth" in which else None, ptr(az), ptr(nd), ptr(ch),
            ptr(pn), ptr(ws), ws.numel(), N, H, W, stream_ptr())
    if entry == "old":
        check(lib.pd_polar_normals_stats(ptr(pred_pm), ld, *tail), "old")
    else:
        check(lib.pd_polar_normals_stats_ray(ptr(pred_pm), ld, ptr(Km) if Km is not None else None, ray, *tail), "ray")
    torch.cuda.synchronize()
    return rec_n, rec_a, az, nd, ch, pn


def test_either_record_set_may_be_null_in_the_ray_frame():
    shape = SHAPES[3]
    full = erun(shape, 12)
    Km = etensors(shape, 12)[5]
    for which in ("normal", "azimuth"):
        rec_n, rec_a, az, nd, ch, pn = _cabi_eval(shape, "ray", 1, Km, which=(which,))
        assert torch.equal(rec_n if which == "normal" else rec_a, getattr(full, which).records), which
        assert bool(((rec_a if which == "normal" else rec_n) == 0x5A).all())
        got = [t.cpu().numpy().tobytes() for t in (az, nd, ch, pn)]
        assert got == _bytes(full)[2:], which


def test_ray_frame_0_through_the_new_evaluator_entry_is_the_old_entry():
    for shape in (SHAPES[2], SHAPES[3]):
        old = _cabi_eval(shape, "old", 0, None)
        new = _cabi_eval(shape, "ray", 0, None)                       # K is ignored and may be NULL
        with_k = _cabi_eval(shape, "ray", 0, etensors(shape, 12)[5])
        for a, b, c in zip(old, new, with_k):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
        # and the Python layer without the flag is the orthographic statement
        compare(fields(erun(shape, 12, ray=False)), ereference(shape, 12, False), (shape, "frame off"))


def test_evaluator_two_calls_and_a_captured_call_give_identical_bytes():
    pe = PE()
    shape = SHAPES[3]
    a = erun(shape, 12)
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")      # whatever the allocator hands out next is dirty
    del junk
    assert _bytes(erun(shape, 12)) == _bytes(a)
    pred, pol, xolp, mask, valid, Km = etensors(shape, 12)
    kw = dict(K=Km, mask=mask, valid=valid, tilt_min_deg=TILT_DEG, maps=True, ray_frame=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        st = pe.polar_normals_stats(pred, pol, xolp, **kw)
    for t in (st.normal.records, st.azimuth.records, st.choice, st.pol_normal, st.az_deg, st.n_deg):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _bytes(st) == _bytes(a)


def test_normals_need_the_intrinsics_in_the_ray_frame():
    pred, pol, xolp, mask, valid, Km = etensors(SHAPES[1], 12)
    with pytest.raises(ValueError, match="ray_frame=True needs the intrinsics"):
        PE().polar_normals_stats(pred, pol, xolp, mask=mask, ray_frame=True)
    with pytest.raises(ValueError, match=r"K must be \[2,4,4\]"):
        PE().polar_normals_stats(pred, pol, xolp, K=Km[:1], mask=mask, ray_frame=True)


# ------------------------------------------------------------------ the loss

def lcase(geom, mirrored=False):
    return RR.loss_case(*geom, mirrored=mirrored) if len(geom) == 3 else RR.loss_case(*geom)


def ltensors(c):
    W = c["W"]
    return _dev(c["depth"]), _dev(c["K"]), _dev(c["pol"])[..., :W], _dev(c["xolp"])[..., :W], _dev(c["valid"])[:, None]


def device_normals(depth, K):
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, _, H, W = depth.shape
    pn = torch.empty((N, H, W, 4), device="cuda")
    check(lib.pd_gt_normals(ptr(depth), ptr(K), ptr(pn), N, H, W, -F32_MAX, F32_MAX, stream_ptr()), "pd_gt_normals")
    return pn.cpu().numpy()


def lrun(c, sign=1, weighted=True, g=None, ray=True):
    depth, K, pol, xolp, valid = ltensors(c)
    depth.requires_grad_(g is not None)
    L_n, L_a, det = OPS().polar_loss(depth, K, pol, xolp, valid, aolp_sign=sign, dolp_weighted=weighted, details=True,
                                     ray_frame=ray, **OPTS)
    if g is not None:
        (g[0] * L_n + g[1] * L_a).backward()
    torch.cuda.synchronize()
    return dict(values=torch.stack([L_n, L_a]).detach().cpu().numpy(), state=det.state.cpu().numpy(), sums=det.sums.cpu().numpy(),
                counters=det.counters.cpu().numpy(), maps=det.maps.cpu().numpy(), record=det.record.cpu().numpy(),
                gdepth=None if g is None else depth.grad.cpu())


@functools.lru_cache(maxsize=None)
def lforward(geom, sign=1, weighted=True, mirrored=False):
    c = lcase(geom, mirrored)
    depth, K = ltensors(c)[:2]
    ref = RR.terms(device_normals(depth, K), c["pol"], c["xolp"], c["valid"], K=c["K"], ray_frame=True, rho_min=C.RHO_MIN,
                   rho_max=C.RHO_MAX, tilt2_min=C.TILT2, aolp_sign=sign, dolp_weighted=weighted)
    return lrun(c, sign, weighted), ref


def check_forward(got, ref, what):
    assert np.array_equal(got["state"], ref["state"]), what
    assert got["counters"].tolist() == [ref["counters"][k] for k in LR.COUNTERS], what
    for k, name in enumerate(("l_n", "l_a")):
        want = ref[name].astype(np.float32)
        assert np.array_equal(np.isnan(got["maps"][..., k]), np.isnan(want)), (what, name)
        ok = ~np.isnan(want)
        assert np.array_equal(got["maps"][..., k][ok].view(np.int32), want[ok].view(np.int32)), (what, name)
    n = (ref["n_terms"][0],) * 2 + (ref["n_terms"][1],) * 2
    for k in range(4):
        bound = max(n[k] - 1, 0) * 2.0 ** -53 * abs(ref["sums"][k])
        err = abs(got["sums"][k] - ref["sums"][k])
        print(what, f"sum {k}: err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, k, err, bound)
    s = got["sums"]
    want = np.array([s[0] / s[1] if s[1] > 0 else 0.0, s[2] / s[3] if s[3] > 0 else 0.0]).astype(np.float32)
    assert np.array_equal(got["values"].view(np.int32), want.view(np.int32)), what
    assert got["record"][88:].tolist() == [0] * 8


@pytest.mark.parametrize("geom", LOSS_GEOMS, ids=str)
def test_forward_equals_the_statement_on_the_device_normals(geom):
    got, ref = lforward(geom)
    check_forward(got, ref, str(geom))
    if geom == (2, 9, 65):
        assert not np.array_equal(got["state"], lrun(lcase(geom), ray=False)["state"])     # the frame decides differently


def test_forward_options_and_the_mirrored_camera():
    for sign, weighted in ((-1, True), (1, False)):
        got, ref = lforward((2, 9, 65), sign, weighted)
        check_forward(got, ref, f"sign {sign} weighted {weighted}")
    got, ref = lforward((2, 9, 65), mirrored=True)
    check_forward(got, ref, "mirrored")
    assert ((got["state"][1] & LR.NEGATED) != 0).sum() > 100


@pytest.mark.parametrize("geom", [(2, 21, 70), C.PITCHED, (1, 2, 2)], ids=str)
def test_the_winner_is_the_evaluators_choice(geom):
    depth, K, pol, xolp, valid = ltensors(lcase(geom))
    st = PE().polar_normals_stats(depth, pol, xolp, K=K, valid=valid, classes=[("all", None)], maps=True, ray_frame=True, **OPTS)
    got = lforward(geom)[0]
    assert np.array_equal(got["state"] & LR.WINNER, st.choice.cpu().numpy())
    k = dict(zip(LR.COUNTERS, got["counters"].tolist()))
    assert k["n_normal"] == int(st.normal.n.sum()) and k["n_azimuth"] == int(st.azimuth.n.sum())
    assert k["dolp_out"] == int(st.normal.dolp_out.sum()) and k["bad"] == int(st.normal.bad.sum())
    assert k["frontal"] == int(st.azimuth.frontal.sum()) and k["spec"] == int(st.normal.spec.sum())
    assert k["flipped"] == int(st.normal.flipped.sum())
    assert np.array_equal(np.isnan(got["maps"][..., 1]), np.isnan(st.az_deg.cpu().numpy()))


def check_backward(c, g, sign=1, weighted=True):
    got = lrun(c, sign, weighted, g)
    kw = dict(g=g, aolp_sign=sign, dolp_weighted=weighted, ray_frame=True)
    r64, _ = RR.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], got["state"], torch.float64, **kw)
    r32, _ = RR.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], got["state"], torch.float32, **kw)
    err, tol = LC.assert_elem(got["gdepth"], r32, r64, f"gdepth g = {g} sign {sign} weighted {weighted}")
    print(f"{c['N'], c['H'], c['W']} g = {g}: max err {err:.3e}, tol {tol:.3e}, max |ref| {r64.abs().max().item():.3e}")
    assert r64.abs().max() > 0
    return got


@pytest.mark.parametrize("geom", LOSS_GEOMS, ids=str)
def test_backward_both_terms(geom):
    got = check_backward(lcase(geom), (1.3, 0.7))
    # not the orthographic gradient
    if geom == (2, 9, 65):
        assert not torch.equal(got["gdepth"], lrun(lcase(geom), g=(1.3, 0.7), ray=False)["gdepth"])


@pytest.mark.parametrize("g", [(1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("sign,weighted", [(1, True), (1, False), (-1, True)])
def test_backward_each_term_alone_and_options(g, sign, weighted):
    check_backward(lcase((2, 9, 65)), g, sign, weighted)
    check_backward(lcase((1, 17, 129)), g, sign, weighted)


def test_backward_of_negated_pixels():
    """A mirrored camera (fx < 0) makes the depth map's own normals look away from their rays: the NEGATED path."""
    for g in ((1.3, 0.7), (1.0, 0.0), (0.0, 1.0)):
        got = check_backward(lcase((2, 9, 65), mirrored=True), g)
    assert ((got["state"][1] & LR.NEGATED) != 0).sum() > 100


@functools.lru_cache(maxsize=None)
def disp_case(N, H, W, zoom):
    m = LC.ms_case(N, H, W, [zoom])
    depth = LC.ol.upsample_disp_to_depth(m["disps"][0], H, W, LC.MIN_D, LC.MAX_D)
    c = C.build(depth.numpy(), RR.intrinsics(N, H, W), 9100 * N + 17 * H + W + zoom, None, False)
    c.update(disp=m["disps"][0].numpy(), zoom=zoom)
    return c


def disp_grad(c, state, dt, g=(1.3, 0.7)):
    d = torch.from_numpy(c["disp"]).to(dt).requires_grad_(True)
    depth = LC.ol.upsample_disp_to_depth(d, c["H"], c["W"], LC.MIN_D, LC.MAX_D)
    L_n, L_a = RR.torch_loss(depth, c["K"], c["pol"], c["xolp"], state, dt, ray_frame=True)
    gt = torch.tensor(g, dtype=torch.float32).to(dt)
    (gt[0] * L_n + gt[1] * L_a).backward()
    return d.grad


@pytest.mark.parametrize("zoom", C.ZOOMS)
def test_backward_through_disp_depth(zoom):
    from polardepth import functional as PF
    from polardepth._lib import lib, check, ptr, stream_ptr
    c = disp_case(*C.DISP_GEOM, zoom)
    N, H, W = c["N"], c["H"], c["W"]
    _, K, pol, xolp, valid = ltensors(c)
    disp = _dev(c["disp"]).requires_grad_(True)
    depth = torch.empty((N, 1, H, W), device="cuda")
    check(lib.pd_disp_to_depth(ptr(disp.detach()), ptr(depth), None, N, H // zoom, W // zoom, H, W, LC.MIN_D, LC.MAX_D,
                               stream_ptr()), "pd_disp_to_depth")
    cfg = PF.LossCfg([0], LC.MIN_D, LC.MAX_D, 0.0, 0.0, H, W)
    (L_n, L_a), = PF.polarimetric_loss(cfg, [disp], [depth], K, pol, xolp, valid, ray_frame=True, **OPTS)
    (1.3 * L_n + 0.7 * L_a).backward()
    state = OPS().polar_loss(depth, K, pol, xolp, valid, details=True, ray_frame=True, **OPTS)[2].state.cpu().numpy()
    r32, r64 = (disp_grad(c, state, dt) for dt in (torch.float32, torch.float64))
    err, tol = LC.assert_elem(disp.grad, r32, r64, f"gdisp zoom {zoom}")
    print(f"zoom {zoom}: max err {err:.3e}, tol {tol:.3e}")


def _cabi_loss(c, entry, ray):
    """Forward + backward through the C ABI -> bytes of (state, record, values, maps, gdepth); entry "old" | "ray"."""
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, H, W = c["N"], c["H"], c["W"]
    depth, K, pol, xolp, valid = ltensors(c)
    valid = valid[:, 0].contiguous()
    state = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
    record = torch.zeros(96, dtype=torch.uint8, device="cuda")
    values, gdepth = torch.zeros(2, device="cuda"), torch.zeros_like(depth)
    maps = torch.zeros((N, H, W, 2), device="cuda")
    ws = torch.empty((lib.pd_polar_loss_rows(N, H, W), 11), dtype=torch.float64, device="cuda")
    g = torch.tensor([1.3, 0.7], device="cuda")
    ldp = pol.stride(2)

    def both():
        st = stream_ptr()
        head = (ptr(depth), ptr(K), ptr(pol), ptr(xolp), ldp, ptr(valid), C.RHO_MIN, C.RHO_MAX, C.TILT2, 1, 1)
        ftail = (ptr(state), ptr(record), ptr(values), ptr(maps), ptr(ws), ws.numel() * 8, N, H, W, st)
        bhead = (ptr(depth), ptr(K), ptr(pol), ptr(xolp), ldp, ptr(state), ptr(g), ptr(record), 1, 1)
        btail = (ptr(gdepth), N, H, W, st)
        if entry == "old":
            check(lib.pd_polar_loss_fwd(*head, *ftail), "fwd")
            check(lib.pd_polar_loss_bwd(*bhead, *btail), "bwd")
        else:
            check(lib.pd_polar_loss_fwd_ray(*head, ray, *ftail), "fwd_ray")
            check(lib.pd_polar_loss_bwd_ray(*bhead, ray, *btail), "bwd_ray")

    outs = (state, record, values, maps, gdepth)
    return both, outs


def _out_bytes(outs):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in outs]


def test_ray_frame_0_through_the_new_loss_entries_is_the_old_entries():
    for geom in ((2, 9, 65), C.PITCHED):
        c = lcase(geom)
        res = []
        for entry in ("old", "ray"):
            both, outs = _cabi_loss(c, entry, 0)
            both()
            res.append(_out_bytes(outs))
        assert res[0] == res[1]
        both, outs = _cabi_loss(c, "ray", 1)
        both()
        assert _out_bytes(outs)[0] != res[0][0]


def test_loss_two_calls_and_a_captured_forward_and_backward_give_identical_bytes():
    c = lcase((1, 17, 129))
    a = lrun(c, g=(1.3, 0.7))
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
    del junk
    b = lrun(c, g=(1.3, 0.7))
    for k in ("values", "state", "record", "maps"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["gdepth"].numpy().tobytes() == b["gdepth"].numpy().tobytes()
    both, outs = _cabi_loss(c, "ray", 1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        both()
    for t in outs:
        t.zero_()
    graph.replay()
    got = _out_bytes(outs)
    assert got == [a["state"].tobytes(), a["record"].tobytes(), a["values"].tobytes(), a["maps"].tobytes(),
                   a["gdepth"].numpy().tobytes()]


def test_empty_batch_and_all_gated_images():
    depth = torch.zeros((0, 1, 8, 8), device="cuda", requires_grad=True)
    K, pol, xolp = torch.zeros((0, 4, 4), device="cuda"), torch.zeros((0, 9, 8, 8), device="cuda"), torch.zeros((0, 2, 8, 8), device="cuda")
    L_n, L_a, det = OPS().polar_loss(depth, K, pol, xolp, details=True, ray_frame=True)
    (L_n + L_a).backward()
    assert float(L_n) == 0.0 and float(L_a) == 0.0 and tuple(depth.grad.shape) == (0, 1, 8, 8) and not det.record.any()
    c = lcase((2, 9, 65))
    for how in ("dolp_out", "invalid", "bad"):
        depth, K, pol, xolp, valid = ltensors(c)
        pol, xolp = pol.contiguous(), xolp.contiguous()
        if how == "dolp_out":
            xolp[:, 0] = 1.5
        elif how == "invalid":
            valid.zero_()
        elif how == "bad":
            pol.zero_()
        depth.requires_grad_(True)
        L_n, L_a, det = OPS().polar_loss(depth, K, pol, xolp, valid, details=True, ray_frame=True, **OPTS)
        (1.3 * L_n + 0.7 * L_a).backward()
        assert float(L_n) == 0.0 and float(L_a) == 0.0, how
        assert not depth.grad.any() and torch.isfinite(depth.grad).all(), how
        assert torch.isnan(det.maps).all() and not det.sums.any(), how
        k = dict(zip(LR.COUNTERS, det.counters.tolist()))
        assert k["n_normal"] == 0 and k["n_azimuth"] == 0 and k["frontal"] == 0
    # a zero focal length under the evaluator, with finite normals: every pixel of that item is `bad`, the other item is not
    shape = SHAPES[2]
    pred, pol, xolp, mask, valid, Km = etensors(shape, 12)
    Km[1, 0, 0] = 0.0
    st = PE().polar_normals_stats(pred, pol, xolp, K=Km, mask=mask, valid=valid, tilt_min_deg=TILT_DEG, maps=True, ray_frame=True)
    kz = np.array(ecase(*shape)["K"])
    kz[1, 0, 0] = 0.0
    c2 = ecase(*shape)
    ref = RR.stats(c2["pred"], c2["pol"], c2["xolp"], c2["mask"], _lohi(_classes(12)), _edges(), K=kz, ray_frame=True,
                   valid=c2["valid"], tilt2_min=TILT2)
    compare(fields(st), ref, "fx = 0")
    assert ref["normal"]["n"][1, 0] == 0 and ref["normal"]["n"][0, 0] > 0 and ref["normal"]["bad"][1, 0] > 0


# ------------------------------------------------------------------ the perspective plane

def test_the_perspective_plane_is_flat_only_in_the_ray_frame():
    """polar_ray_ref.plane_scene(): a camera with fx = 0.58 W looks at a plane tilted by 20 degrees whose one normal, expressed
    exactly in each pixel's ray frame, is the diffuse candidate.  In the ray frame the evaluator's two means and the loss's two
    values are below the statement's measured figures times 4 (polar_ray_ref.PLANE_*: 6.0e-7 / 5.2e-7 degrees for the normal
    itself, 4.0e-5 / 6.2e-5 degrees and L_n = 3.3e-13, L_a = 2.8e-12 for the depth map); orthographically they are 13.2 and 22.3
    degrees, L_n = 0.033 and L_a = 0.180: more than 100 times the bounds.  Fails without the ray frame."""
    s = RR.plane_scene()
    H, W = s["normals"].shape[1:3]
    inner = torch.zeros((1, 1, H, W), dtype=torch.uint8, device="cuda")
    inner[..., 1:-1, 1:-1] = 1
    K, pol, xolp = _dev(s["K"]), _dev(s["pol"]), _dev(s["xolp"])
    normals = _dev(s["normals"]).permute(0, 3, 1, 2)[:, :3]
    depth = _dev(s["depth"])
    for pred, bound in ((normals, RR.PLANE_NORMALS_DEG), (depth, RR.PLANE_DEPTH_DEG)):
        for ray in (True, False):
            st = PE().polar_normals_stats(pred, pol, xolp, K=K, valid=inner, classes=[("all", None)], tilt_min_deg=TILT_DEG,
                                          ray_frame=ray)
            means = [float(rs.sums[0, 0, 0] / rs.n[0, 0]) for rs in (st.normal, st.azimuth)]
            print("ray" if ray else "orthographic", "mean n_deg, az_deg", means)
            assert int(st.normal.n[0, 0]) == int(inner.sum())
            assert (max(means) <= bound) if ray else (min(means) >= 100 * bound)
    for ray in (True, False):
        L_n, L_a = OPS().polar_loss(depth, K, pol, xolp, inner, tilt_min_deg=TILT_DEG, ray_frame=ray)
        print("ray" if ray else "orthographic", "L_n, L_a", float(L_n), float(L_a))
        for v, b in zip((float(L_n), float(L_a)), RR.PLANE_LOSS):
            assert (v <= b) if ray else (v >= 100 * b)
