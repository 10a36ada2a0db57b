"""pd_polar_loss_fwd / _bwd and polardepth.ops.polar_loss on the GPU.

Forward: p is taken from pd_gt_normals on the device and fed to the NumPy statement (tests/polar_loss_ref.py): the state map,
the counters and the per-pixel maps must be equal bit for bit; the four ordered fp64 sums within (n - 1) 2^-53 relative of
math.fsum (the bound of any summation order of n terms, the evaluator tests' rule); the values the fp32 rounding of the ratio.
Backward: against the fp64 autograd reference with the DEVICE's own state as the fixed decisions, by the project's rule
(loss_cases.py): |dev - ref64| <= 4 max|ref32 - ref64| + 1e-6 max|ref64|, elementwise.  tests/test_polar_loss_ref.py caps the
conditioning max|ref32 - ref64| / max|ref64| of these inputs at 5e-4."""
import functools

import numpy as np
import pytest
import torch

import loss_cases as LC
import polar_loss_cases as C
import polar_loss_ref as R

pytestmark = pytest.mark.gpu

F32_MAX = float(np.finfo(np.float32).max)
GRAD_GEOMS = [g for g in C.GEOMS if g[1] > 1]          # a one-row frame has no fp64 reference gradient (test_polar_loss_ref.py)
OPTS = dict(rho_min=C.RHO_MIN, rho_max=C.RHO_MAX, tilt_min_deg=C.TILT_DEG)


def OPS():
    from polardepth import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def tensors(c):
    """The case on the device as the Python layer takes it: pol_normals and xolp views of row pitch ldp."""
    W = c["W"]
    return _dev(c["depth"]), _dev(c["K"]), _dev(c["pol"])[..., :W], _dev(c["xolp"])[..., :W], _dev(c["valid"])[:, None]


def device_normals(depth, K):
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, _, H, W = depth.shape
    pn = torch.empty((N, H, W, 4), device="cuda")
    check(lib.pd_gt_normals(ptr(depth), ptr(K), ptr(pn), N, H, W, -F32_MAX, F32_MAX, stream_ptr()), "pd_gt_normals")
    return pn.cpu().numpy()


def run(c, sign=1, weighted=True, g=None):
    """ops.polar_loss with details; with g also d (g[0] L_n + g[1] L_a) / d depth."""
    depth, K, pol, xolp, valid = tensors(c)
    depth.requires_grad_(g is not None)
    L_n, L_a, det = OPS().polar_loss(depth, K, pol, xolp, valid, aolp_sign=sign, dolp_weighted=weighted, details=True, **OPTS)
    if g is not None:
        (g[0] * L_n + g[1] * L_a).backward()
    torch.cuda.synchronize()
    return dict(values=torch.stack([L_n, L_a]).detach().cpu().numpy(), state=det.state.cpu().numpy(), sums=det.sums.cpu().numpy(),
                counters=det.counters.cpu().numpy(), maps=det.maps.cpu().numpy(), record=det.record.cpu().numpy(),
                gdepth=None if g is None else depth.grad.cpu())


@functools.lru_cache(maxsize=None)
def forward(geom, sign=1, weighted=True):
    """(device results, the statement on the device's normals): computed once per case, never modified."""
    c = C.case(*geom)
    depth, K = tensors(c)[:2]
    ref = C.terms_of(c, p=device_normals(depth, K), aolp_sign=sign, dolp_weighted=weighted)
    return run(c, sign, weighted), ref


def check_forward(got, ref, what):
    assert np.array_equal(got["state"], ref["state"]), what
    assert got["counters"].tolist() == [ref["counters"][k] for k in R.COUNTERS], what
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


@pytest.mark.parametrize("geom", C.GEOMS + [C.PITCHED], ids=str)
def test_forward_equals_the_statement_on_the_device_normals(geom):
    got, ref = forward(geom)
    check_forward(got, ref, str(geom))


@pytest.mark.parametrize("sign,weighted", [(-1, True), (1, False), (-1, False)])
def test_forward_options(sign, weighted):
    got, ref = forward((2, 9, 65), sign, weighted)
    check_forward(got, ref, f"sign {sign} weighted {weighted}")
    assert not np.array_equal(got["values"], forward((2, 9, 65))[0]["values"])


@pytest.mark.parametrize("geom", [(2, 21, 70), (3, 1, 40), (2, 40, 1), C.PITCHED], ids=str)
def test_the_winner_is_the_evaluators_choice(geom):
    from polardepth import polar_normals_eval as PE
    depth, K, pol, xolp, valid = tensors(C.case(*geom))
    st = PE.polar_normals_stats(depth, pol, xolp, K=K, valid=valid, classes=[("all", None)], maps=True, **OPTS)
    got = forward(geom)[0]
    assert np.array_equal(got["state"] & R.WINNER, st.choice.cpu().numpy())
    k = dict(zip(R.COUNTERS, got["counters"].tolist()))
    assert k["n_normal"] == int(st.normal.n.sum()) and k["n_azimuth"] == int(st.azimuth.n.sum())
    assert k["dolp_out"] == int(st.normal.dolp_out.sum()) and k["bad"] == int(st.normal.bad.sum())
    assert k["frontal"] == int(st.azimuth.frontal.sum()) and k["spec"] == int(st.normal.spec.sum())
    assert k["flipped"] == int(st.normal.flipped.sum())
    assert np.array_equal(np.isnan(got["maps"][..., 1]), np.isnan(st.az_deg.cpu().numpy()))


def check_backward(c, g, sign=1, weighted=True):
    got = run(c, sign, weighted, g)
    kw = dict(g=g, aolp_sign=sign, dolp_weighted=weighted)
    r64, _ = R.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], got["state"], torch.float64, **kw)
    r32, _ = R.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], got["state"], torch.float32, **kw)
    err, tol = LC.assert_elem(got["gdepth"], r32, r64, f"gdepth g = {g} sign {sign} weighted {weighted}")
    print(f"{c['N'], c['H'], c['W']} g = {g}: max err {err:.3e}, tol {tol:.3e}, max |ref| {r64.abs().max().item():.3e}")
    return got


@pytest.mark.parametrize("geom", GRAD_GEOMS + [C.PITCHED], ids=str)
def test_backward_both_terms(geom):
    got = check_backward(C.case(*geom), (1.3, 0.7))
    if geom[2] == 1:
        assert not got["gdepth"].any()


@pytest.mark.parametrize("g", [(1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("sign,weighted", [(1, True), (1, False), (-1, True)])
def test_backward_each_term_alone_and_options(g, sign, weighted):
    check_backward(C.case(2, 9, 65), g, sign, weighted)
    check_backward(C.case(1, 17, 129), g, sign, weighted)


@pytest.mark.parametrize("zoom", C.ZOOMS)
def test_backward_through_disp_depth(zoom):
    """d loss / d disp: the depth map goes on the tape through DispDepthFn, as functional.polarimetric_loss does it."""
    from polardepth import functional as PF
    from polardepth._lib import lib, check, ptr, stream_ptr
    c = C.disp_case(*C.DISP_GEOM, zoom)
    N, H, W = c["N"], c["H"], c["W"]
    _, K, pol, xolp, valid = tensors(c)
    disp = _dev(c["disp"]).requires_grad_(True)
    depth = torch.empty((N, 1, H, W), device="cuda")
    check(lib.pd_disp_to_depth(ptr(disp.detach()), ptr(depth), None, N, H // zoom, W // zoom, H, W, LC.MIN_D, LC.MAX_D,
                               stream_ptr()), "pd_disp_to_depth")
    cfg = PF.LossCfg([0], LC.MIN_D, LC.MAX_D, 0.0, 0.0, H, W)
    (L_n, L_a), = PF.polarimetric_loss(cfg, [disp], [depth], K, pol, xolp, valid, **OPTS)
    (1.3 * L_n + 0.7 * L_a).backward()
    state = OPS().polar_loss(depth, K, pol, xolp, valid, details=True, **OPTS)[2].state.cpu().numpy()
    r32, r64 = (C.disp_grad(c, state, dt) for dt in (torch.float32, torch.float64))
    err, tol = LC.assert_elem(disp.grad, r32, r64, f"gdisp zoom {zoom}")
    print(f"zoom {zoom}: max err {err:.3e}, tol {tol:.3e}")


def test_autograd_with_upstream_gradients_on_each_value():
    c = C.case(2, 9, 65)
    depth, K, pol, xolp, valid = tensors(c)
    depth.requires_grad_(True)
    L_n, L_a = OPS().polar_loss(depth, K, pol, xolp, valid, **OPTS)
    assert L_n.requires_grad and L_a.requires_grad and L_n.dim() == 0
    (2.5 * L_n * L_n + torch.exp(-L_a)).backward()                    # upstream: 5 L_n on the first value, -e^{-L_a} on the second
    g = (5.0 * L_n.item(), -float(np.exp(-L_a.item())))
    st = forward((2, 9, 65))[0]["state"]
    r64, _ = R.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], st, torch.float64, g=g)
    r32, _ = R.torch_grad(c["depth"], c["K"], c["pol"], c["xolp"], st, torch.float32, g=g)
    LC.assert_elem(depth.grad, r32, r64, "autograd")
    with pytest.raises(ValueError, match="aolp_sign"):
        OPS().polar_loss(depth, K, pol, xolp, aolp_sign=0)
    with pytest.raises(ValueError, match=r"\[N,1,H,W\]"):
        OPS().polar_loss(depth[:, 0], K, pol, xolp)


def test_two_calls_give_identical_bytes():
    c = C.case(1, 17, 129)
    a = run(c, g=(1.3, 0.7))
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")      # whatever the allocator hands out next is dirty
    del junk
    b = run(c, g=(1.3, 0.7))
    for k in ("values", "state", "record", "maps"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["gdepth"].numpy().tobytes() == b["gdepth"].numpy().tobytes()


def test_captured_forward_and_backward_replay_the_eager_bytes():
    from polardepth._lib import lib, check, ptr, stream_ptr
    c = C.case(1, 17, 129)
    N, H, W = c["N"], c["H"], c["W"]
    eager = run(c, g=(1.3, 0.7))
    depth, K, pol, xolp, valid = tensors(c)
    valid = valid[:, 0].contiguous()
    state = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
    record = torch.zeros(96, dtype=torch.uint8, device="cuda")
    values, gdepth = torch.zeros(2, device="cuda"), torch.zeros_like(depth)
    maps = torch.zeros((N, H, W, 2), device="cuda")
    ws = torch.empty((lib.pd_polar_loss_rows(N, H, W), 11), dtype=torch.float64, device="cuda")
    g = torch.tensor([1.3, 0.7], device="cuda")
    tilt2 = C.TILT2

    def both():
        st = stream_ptr()
        check(lib.pd_polar_loss_fwd(ptr(depth), ptr(K), ptr(pol), ptr(xolp), pol.stride(2), ptr(valid), C.RHO_MIN, C.RHO_MAX, tilt2,
                                    1, 1, ptr(state), ptr(record), ptr(values), ptr(maps), ptr(ws), ws.numel() * 8, N, H, W, st),
              "pd_polar_loss_fwd")
        check(lib.pd_polar_loss_bwd(ptr(depth), ptr(K), ptr(pol), ptr(xolp), pol.stride(2), ptr(state), ptr(g), ptr(record), 1, 1,
                                    ptr(gdepth), N, H, W, st), "pd_polar_loss_bwd")

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        both()
    for t in (state, record, values, gdepth, maps):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, t in (("state", state), ("record", record), ("values", values), ("maps", maps)):
        assert t.cpu().numpy().tobytes() == eager[k].tobytes(), k
    assert gdepth.cpu().numpy().tobytes() == eager["gdepth"].numpy().tobytes()


def test_empty_batch():
    depth = torch.zeros((0, 1, 8, 8), device="cuda", requires_grad=True)
    K, pol, xolp = torch.zeros((0, 4, 4), device="cuda"), torch.zeros((0, 9, 8, 8), device="cuda"), torch.zeros((0, 2, 8, 8), device="cuda")
    L_n, L_a, det = OPS().polar_loss(depth, K, pol, xolp, details=True)
    (L_n + L_a).backward()
    assert float(L_n) == 0.0 and float(L_a) == 0.0 and tuple(depth.grad.shape) == (0, 1, 8, 8)
    assert not det.record.any() and tuple(det.state.shape) == (0, 8, 8)


def test_an_image_with_every_pixel_gated():
    """Values 0, the gradient all zero, no NaN: by rho out of range, by valid == 0 and by zero candidates."""
    c = C.case(2, 9, 65)
    for how in ("dolp_out", "invalid", "bad"):
        depth, K, pol, xolp, valid = tensors(c)
        pol, xolp = pol.contiguous(), xolp.contiguous()
        if how == "dolp_out":
            xolp[:, 0] = 1.5
        elif how == "invalid":
            valid.zero_()
        else:
            pol.zero_()
        depth.requires_grad_(True)
        L_n, L_a, det = OPS().polar_loss(depth, K, pol, xolp, valid, details=True, **OPTS)
        (1.3 * L_n + 0.7 * L_a).backward()
        assert float(L_n) == 0.0 and float(L_a) == 0.0, how
        assert not depth.grad.any() and torch.isfinite(depth.grad).all(), how
        assert torch.isnan(det.maps).all() and not det.sums.any(), how
        k = dict(zip(R.COUNTERS, det.counters.tolist()))
        assert k["n_normal"] == 0 and k["n_azimuth"] == 0 and k["frontal"] == 0
        live = int(c["valid"].sum())
        assert {"dolp_out": k["dolp_out"] == live, "invalid": k["dolp_out"] + k["bad"] == 0, "bad": k["dolp_out"] + k["bad"] == live}[how]


def test_one_row_and_one_column_frames():
    """W = 1: every normal is the zero vector, every pixel `bad`, values 0 and a zero gradient.  H = 1: pd_gt_normals gives
    normals made of rounding noise (tests/test_polar_loss_ref.py); the forward pass scores them as the statement does
    (test_forward_equals_the_statement_on_the_device_normals) and the gradient is finite and reproducible."""
    got = run(C.case(2, 40, 1), g=(1.3, 0.7))
    assert got["values"].tolist() == [0.0, 0.0] and not got["gdepth"].any() and not got["sums"].any()
    assert (got["state"] >> R.GATE_SHIFT != R.GATE_NONE).all()
    a, b = run(C.case(3, 1, 40), g=(1.3, 0.7)), run(C.case(3, 1, 40), g=(1.3, 0.7))
    assert torch.isfinite(a["gdepth"]).all() and np.isfinite(a["values"]).all()
    assert a["gdepth"].numpy().tobytes() == b["gdepth"].numpy().tobytes()
