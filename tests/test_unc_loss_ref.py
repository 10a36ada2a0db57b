"""tests/unc_loss_ref.py on the CPU: the NumPy statement of the depth-uncertainty loss equals a restatement in torch fp64
(F.interpolate bilinear, align_corners=False; autograd for the gradients), and the inputs of tests/unc_cases.py are well
conditioned for the project's gradient rule."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unc_cases as C
import unc_loss_ref as R

F32, F64 = np.float32, np.float64
# max|ref32 - ref64| / max|ref64| of every quantity the GPU test bounds by the rule.  The largest the cases give is 1.6e-6
# (the gradients of "ratio_1.8"; every other case stays below 6e-7): an fp32 evaluation of terms of order one to a hundred.
# The cap is three times that: a case that lets |g - d| / b run away, or cancels in the sums, would exceed it.
CONDITIONING_CAP = 5e-6


def _torch_loss(case, detach=False):
    depth = torch.from_numpy(np.array(case["depth"])).double()[:, None].requires_grad_(True)
    unc = torch.from_numpy(np.array(case["unc"])).double()[:, None].requires_grad_(True)
    gt = torch.from_numpy(np.array(case["gt"])).double()[:, None]
    H, W = gt.shape[2:]
    # which pixels a NaN u reaches is the kernel's rule (a zero weight on a NaN neighbour is NaN; torch copies at ratio 1), so
    # that set comes from the statement's sampler; the values come from F.interpolate with the NaN replaced
    finite = torch.from_numpy(np.isfinite(R.upsample(case["unc"], H, W, F64)))[:, None]
    up = F.interpolate(torch.nan_to_num(unc), size=(H, W), mode="bilinear", align_corners=False)
    m = (gt >= float(F32(C.MIN_D))) & (gt <= float(F32(C.MAX_D))) & finite
    if case["valid"] is not None:
        m = m & (torch.from_numpy(np.array(case["valid"]))[:, None] != 0)
    lo, hi = C.B_RANGE
    logb = math.log(lo) + torch.where(m, up, torch.zeros_like(up)) * math.log(hi / lo)
    d = depth.detach() if detach else depth
    e = torch.where(m, (gt - d).abs(), torch.zeros_like(gt))
    term = torch.where(m, e / torch.exp(logb) + logb + math.log(2.0), torch.zeros_like(gt))
    value = term.sum() / m.sum()
    value.backward()
    return value, depth.grad, unc.grad, m


@pytest.mark.parametrize("name", list(C.LOSS_CASES))
def test_statement_equals_the_torch_restatement(name):
    case = C.loss_case(name)
    value, gdepth, gunc, m = _torch_loss(case)
    ref = R.evaluate(case["depth"], case["gt"], case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, case["valid"], F64)
    st = R.statement(case["depth"], case["gt"], case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, case["valid"])
    assert np.array_equal(ref["m"], m[:, 0].numpy()) and 0 < m.sum() < m.numel()
    assert abs(float(ref["value"]) - value.item()) <= 1e-13 * abs(value.item())
    # the statement samples u in fp32: it differs from the fp64 evaluation by that rounding only
    assert np.array_equal(st["m"], ref["m"]) and abs(float(st["value"]) - value.item()) <= 2e-6 * abs(value.item())
    scale = gdepth.abs().max().item()
    assert np.abs(ref["gdepth"] - gdepth[:, 0].numpy()).max() <= 1e-13 * scale
    assert np.abs(ref["gunc"] - np.nan_to_num(gunc[:, 0].numpy())).max() <= 1e-12 * np.abs(ref["gunc"]).max()
    _, none, gunc_d, _ = _torch_loss(case, detach=True)
    assert none is None and torch.equal(gunc_d, gunc)
    det = R.evaluate(case["depth"], case["gt"], case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, case["valid"], F64, detach=True)
    assert det["gdepth"] is None and np.array_equal(det["gunc"], ref["gunc"])


@pytest.mark.parametrize("name", list(C.LOSS_CASES))
def test_cases_hold_what_they_promise_and_are_well_conditioned(name):
    case = C.loss_case(name)
    st = R.statement(case["depth"], case["gt"], case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, case["valid"])
    m, gt, depth = st["m"], case["gt"], case["depth"]
    assert (depth[m] == gt[m]).any()                                         # a pixel with d == g under the mask
    assert (case["unc"] == 0).any() and (case["unc"] == 1).any() and np.isnan(case["unc"]).any()
    assert np.isnan(depth[~m]).any() and not np.isnan(depth[m]).any()        # a NaN depth, on a hole only
    assert np.isnan(gt).any() and (gt == 0).any() and (gt > F32(C.MAX_D)).any()
    assert (gt[m] == F32(C.MIN_D)).any() or (gt[m] == F32(C.MAX_D)).any()    # the mask is inclusive
    up = R.upsample(case["unc"], *gt.shape[1:])
    gate = (gt >= F32(C.MIN_D)) & (gt <= F32(C.MAX_D))
    assert (np.isnan(up) & gate).any() and not np.isnan(up[m]).any()         # a NaN u under the gate takes its pixels out
    ratio = st["ratio"][m]
    print(name, "|g - d| / b: min > 0", ratio[ratio > 0].min(), "max", ratio.max())
    assert ratio.max() < 1e3
    r32 = R.evaluate(depth, gt, case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, case["valid"], F32)
    r64 = R.evaluate(depth, gt, case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, case["valid"], F64)
    for key in ("value", "gdepth", "gunc", "gup"):
        a, b = np.asarray(r32[key], F64), np.asarray(r64[key], F64)
        cond = np.abs(a - b).max() / np.abs(b).max()
        print(name, key, "conditioning", cond)
        assert cond <= CONDITIONING_CAP, (name, key, cond)


def test_an_empty_mask_gives_zero_everywhere():
    case = C.loss_case("row")
    gt = np.zeros_like(case["gt"])
    for dtype in (F32, F64):
        r = R.evaluate(case["depth"], gt, case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D, None, dtype)
        assert r["value"] == 0 and not r["gdepth"].any() and not r["gunc"].any()
    st = R.statement(case["depth"], gt, case["unc"], C.B_RANGE, C.MIN_D, C.MAX_D)
    assert st["value"] == 0 and st["sums"].tolist() == [0, 0, 0, 0] and np.isnan(st["term"]).all()


def test_the_fma_of_the_statement_is_exactly_rounded():
    u = np.array([0.0, 1.0, 0.5, np.float32(0.3), np.float32(0.7)], F64)
    lo, ratio = math.log(0.0005), math.log(1000.0)
    got = R.fma64(u, ratio, lo)
    assert got[0] == lo and got[2] == 0.5 * ratio + lo                      # exact products: the fma is the sum
    long = (np.longdouble(u) * np.longdouble(ratio) + np.longdouble(lo)).astype(F64)
    assert np.abs(got - long).max() <= np.spacing(np.abs(got)).max()        # within an ulp of the extended evaluation
    assert math.isnan(R.fma64(np.array([np.nan]), ratio, lo)[0])
