"""pd_unc_loss_fwd / _bwd and polardepth.ops.uncertainty_loss on the GPU against the NumPy statement (tests/unc_loss_ref.py,
pinned to a torch restatement by tests/test_unc_loss_ref.py) applied to the very arrays handed to the kernels.

Maps: the NaN pattern equal, every value within one fp32 ulp of the statement's (the device rounds an fp64 value that may
differ from the statement's in its last bits).  Sums: the summation-order bound of the evaluator tests, (n - 1) 2^-53 sum|term|,
plus what the device's exp may add: no accuracy statement for the device library's fp64 exp is at hand, so its largest distance
from NumPy's on these tests' own arguments is measured (test_device_exp_...; recorded in DESIGN.md, section 4) and twice that is
allowed; the division is IEEE, half an ulp per term.  Value: the fp32 rounding of the device's own sums, bit for bit.
Gradients: the project's rule, |dev - ref64| <= 4 max|ref32 - ref64| + 1e-6 max|ref64|."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import unc_cases as C
import unc_loss_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EXP_ULP = 1                 # the largest |device exp - np.exp| measured on these arguments, in ulp
EPS = 2.0 ** -53


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _gt_dev(case):
    """The ground truth on the device with the case's pitch: a view of a wider tensor where the case says so."""
    gt = case["gt"]
    if gt.base is not None and gt.strides[1] != gt.shape[2] * 4:
        return torch.from_numpy(np.array(gt.base)).cuda()[:, :, :gt.shape[2]]
    return _dev(gt)


@functools.lru_cache(maxsize=None)
def refs(name):
    case = C.loss_case(name)
    args = (case["depth"], case["gt"], case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, case["valid"])
    return R.statement(*args), R.evaluate(*args, dtype=F32), R.evaluate(*args, dtype=F64)


def run(name, detach=False, details=True, backward=True):
    from polardepth import ops
    case = C.loss_case(name)
    depth = _dev(case["depth"])[:, None].requires_grad_(True)
    unc = _dev(case["unc"])[:, None].requires_grad_(True)
    gt = _gt_dev(case)
    out = ops.uncertainty_loss(depth, gt, unc, C.B_RANGE, C.MIN_D, C.MAX_D, valid=_dev(case["valid"]), detach_depth=detach,
                               details=details)
    value, det = out if details else (out, None)
    if backward:
        value.backward()
    torch.cuda.synchronize()
    return value, det, depth.grad, unc.grad


@pytest.mark.parametrize("name", list(C.LOSS_CASES))
def test_maps_sums_and_value_equal_the_statement(name):
    st, _, _ = refs(name)
    value, det, _, _ = run(name, backward=False)
    maps = det.maps.cpu().numpy()
    assert maps.shape == st["m"].shape + (2,)
    for j, key in enumerate(("term", "b")):
        got, want = maps[..., j], st[key].astype(F32)
        assert np.array_equal(np.isnan(got), ~st["m"]), (name, key)
        d = np.abs(got[st["m"]] - want[st["m"]])
        print(name, key, "max distance in fp32 ulp", (d / np.spacing(np.abs(want[st["m"]]))).max())
        assert (d <= np.spacing(np.abs(want[st["m"]]))).all(), (name, key)
    sums = det.sums.cpu().numpy()
    m = st["m"]
    n = int(m.sum())
    ratio, l2b, b = st["ratio"][m], st["l2b"][m], st["b"][m]
    order = (n - 1) * EPS
    # an ulp is at most 2 EPS relative; log 2b holds no exp and no division
    bounds = [(order + 2 * EXP_ULP * 2 * EPS + EPS) * ratio.sum(), order * np.abs(l2b).sum(), 0.0,
              (order + 2 * EXP_ULP * 2 * EPS) * b.sum()]
    for j, bound in enumerate(bounds):
        err = abs(sums[j] - st["sums"][j])
        print(name, "sum", j, "error", err, "bound", bound)
        assert err <= bound, (name, j, err, bound)
    assert sums[2] == n
    want = F32((sums[0] + sums[1]) / sums[2])
    assert value.dtype == torch.float32 and value.item() == want and np.float32(value.item()).tobytes() == want.tobytes()
    assert abs(value.item() - st["value"]) <= 2.0 ** -23 * abs(st["value"])


@pytest.mark.parametrize("name", list(C.LOSS_CASES))
def test_gradients_follow_the_rule(name):
    import loss_cases as lc
    _, r32, r64 = refs(name)
    _, _, gdepth, gunc = run(name)
    t = lambda a: torch.from_numpy(np.asarray(a))
    e, tol = lc.assert_elem(gdepth[:, 0], t(r32["gdepth"]), t(r64["gdepth"]), f"{name} d/d depth")
    print(name, "d/d depth: err", e, "tol", tol)
    e, tol = lc.assert_elem(gunc[:, 0], t(r32["gunc"]), t(r64["gunc"]), f"{name} d/d u")
    print(name, "d/d u: err", e, "tol", tol)
    m = refs(name)[0]["m"]
    assert not gdepth[:, 0].cpu().numpy()[~m].any()                          # nothing outside the mask, the NaN depth included
    case = C.loss_case(name)
    same = m & (case["depth"] == case["gt"])
    assert same.any() and not gdepth[:, 0].cpu().numpy()[same].any()         # 0 at depth == gt


@pytest.mark.parametrize("name", ["ratio_1.8", "head_2", "identity"])
def test_detached_depth_gets_no_gradient_and_u_the_same_bits(name):
    _, _, gdepth, gunc = run(name)
    value_d, _, gdepth_d, gunc_d = run(name, detach=True)
    assert gdepth is not None and gdepth_d is None
    assert gunc_d.cpu().numpy().tobytes() == gunc.cpu().numpy().tobytes()
    assert value_d.item() == run(name, backward=False)[0].item()


@pytest.mark.parametrize("name", ["ratio_1.8", "head_1", "pitched"])
def test_two_runs_give_identical_bytes(name):
    a = run(name)
    junk = torch.full((1 << 22,), 0x5A, dtype=torch.uint8, device="cuda")      # whatever the allocator hands out next is dirty
    del junk
    b = run(name)
    assert a[0].item() == b[0].item()
    for x, y in ((a[1].sums, b[1].sums), (a[1].maps, b[1].maps), (a[2], b[2]), (a[3], b[3])):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_empty_mask_and_empty_batch():
    from polardepth import ops
    case = C.loss_case("head_1")
    depth = _dev(case["depth"])[:, None].requires_grad_(True)
    unc = _dev(case["unc"])[:, None].requires_grad_(True)
    value, det = ops.uncertainty_loss(depth, torch.zeros_like(depth), unc, C.B_RANGE, C.MIN_D, C.MAX_D, details=True)
    value.backward()
    torch.cuda.synchronize()
    assert value.item() == 0.0 and det.sums.tolist() == [0, 0, 0, 0] and bool(det.maps.isnan().all())
    assert not depth.grad.any() and not unc.grad.any()
    d0, u0 = depth.detach()[:0].requires_grad_(True), unc.detach()[:0].requires_grad_(True)
    v0 = ops.uncertainty_loss(d0, d0.detach(), u0, C.B_RANGE, C.MIN_D, C.MAX_D)
    v0.backward()
    assert v0.item() == 0.0 and d0.grad.shape == d0.shape


def test_functional_wrapper_runs_every_scale_through_the_tape():
    """functional.uncertainty_loss: DispDepthFn -> ops.uncertainty_loss per scale; detached, no disparity receives a gradient."""
    import types
    from polardepth import functional as PF, ops
    from polardepth._lib import lib, check, ptr, stream_ptr
    cfg = types.SimpleNamespace(min_depth=C.MIN_D, max_depth=C.MAX_D)
    N, H, W = 2, 24, 40
    case = C.loss_case("head_1")
    g = torch.Generator().manual_seed(5)
    sizes = [(24, 40), (12, 20), (6, 10)]
    disps = [torch.rand(N, 1, h, w, generator=g).cuda().requires_grad_(True) for h, w in sizes]
    uncs = [torch.rand(N, 1, h, w, generator=g).cuda().requires_grad_(True) for h, w in sizes]
    depths = []
    for d in disps:
        full = torch.empty(N, 1, H, W, device="cuda")
        check(lib.pd_disp_to_depth(ptr(d.detach()), ptr(full), None, N, d.shape[2], d.shape[3], H, W, C.MIN_D, C.MAX_D,
                                   stream_ptr()), "pd_disp_to_depth")
        depths.append(full)
    gt = _dev(case["gt"])[:, None]
    losses = PF.uncertainty_loss(cfg, disps, depths, uncs, gt)
    assert len(losses) == 3
    for i, l in enumerate(losses):
        assert l.item() == ops.uncertainty_loss(depths[i], gt, uncs[i].detach(), None, C.MIN_D, C.MAX_D).item()
    sum(losses).backward()
    assert all(d.grad is not None and d.grad.abs().sum() > 0 for d in disps) and all(u.grad.abs().sum() > 0 for u in uncs)
    kept = [u.grad.clone() for u in uncs]
    for t in disps + uncs:
        t.grad = None
    sum(PF.uncertainty_loss(cfg, disps, depths, uncs, gt, detach_depth=True)).backward()
    assert all(d.grad is None for d in disps) and all(torch.equal(u.grad, k) for u, k in zip(uncs, kept))
    with pytest.raises(ValueError, match="one uncertainty map per scale"):
        PF.uncertainty_loss(cfg, disps, depths, uncs[:2], gt)


def test_forward_and_backward_capture_into_a_graph_and_replay_the_same_bits():
    from polardepth import ops
    case = C.loss_case("ratio_1.8")
    depth = _dev(case["depth"])[:, None].requires_grad_(True)
    unc = _dev(case["unc"])[:, None].requires_grad_(True)
    gt, valid = _dev(case["gt"]), _dev(case["valid"])

    def step():
        value = ops.uncertainty_loss(depth, gt, unc, C.B_RANGE, C.MIN_D, C.MAX_D, valid=valid)
        gd, gu = torch.autograd.grad(value, (depth, unc))
        return value, gd, gu

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires
        eager = step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        captured = step()
    for t in captured:
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()
    assert eager[1].abs().sum() > 0 and eager[2].abs().sum() > 0


def device_exp(u):
    """exp(fma(u, log(b_hi / b_lo), log b_lo)) in fp64 as the device forms it, for fp32 values u [n]: one pd_unc_loss_fwd call
    per value on a 1 x 1 frame with depth == gt, whose sums[3] is that pixel's b."""
    from polardepth._lib import lib, check, ptr, stream_ptr
    n = u.size
    ud = _dev(u.astype(F32))
    one = torch.ones(1, device="cuda")
    sums = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    value = torch.zeros(1, device="cuda")
    ws = torch.empty(4, dtype=torch.float64, device="cuda")
    st = stream_ptr()
    for i in range(n):
        check(lib.pd_unc_loss_fwd(ptr(one), ptr(one), 1, ctypes.c_void_p(ud.data_ptr() + 4 * i), 1, 1, None, C.MIN_D, C.MAX_D,
                                  C.B_RANGE[0], C.B_RANGE[1], ctypes.c_void_p(sums.data_ptr() + 32 * i), ptr(value), None, ptr(ws),
                                  32, 1, 1, 1, st), "pd_unc_loss_fwd")
    torch.cuda.synchronize()
    return sums[:, 3].cpu().numpy()


def test_device_exp_stays_within_the_recorded_distance_from_numpy():
    """The allowance of the sum bounds: on the sampled u of every loss case and the u of every evaluator case (up to 4096 of
    the distinct values, evenly spread, with 0 and 1), the device's b is within EXP_ULP ulp of np.exp of the exactly rounded
    argument."""
    import math
    vals = [np.array([0.0, 1.0], F32)]
    for name in C.LOSS_CASES:
        st = refs(name)[0]
        case = C.loss_case(name)
        vals.append(R.upsample(case["unc"], *case["shape"][1:])[st["m"]])
    for shape in C.STATS_SHAPES:
        u = C.stats_case(*shape)[2]
        vals.append(u[(u >= 0) & (u <= 1)])
    u = np.unique(np.concatenate(vals))
    u = np.unique(np.concatenate([u[:: max(1, u.size // 4094)], np.array([0.0, 1.0], F32)]))
    got = device_exp(u)
    want = np.exp(R.fma64(u.astype(F64), math.log(C.B_RANGE[1] / C.B_RANGE[0]), math.log(C.B_RANGE[0])))
    ulps = np.abs(got - want) / np.spacing(want)
    print("device exp vs np.exp on", u.size, "arguments: max", ulps.max(), "ulp; share of exact results", (ulps == 0).mean())
    assert ulps.max() <= EXP_ULP
