"""oracle/attention.py pinned on the CPU, and the proof that the comparison rule of tests/test_attention_gpu.py has teeth.

1. attention / attention_bwd against torch.softmax attention and autograd in fp64.
2. The three staging models against the fp64 truth within the first-order effect of rounding the operands: a product
   q~ k~ is off by at most rho = 2 h + h^2 + 4 u relative (h for each bf16 operand; 4 u: fl32(q c32), c32 itself and the
   fp32 constant log2 e), a score by rho * Sabs (log2 units), a normalised probability by expm1(2 ln2 rho max_j Sabs_ij)
   relative -- the factor 2: numerator and denominator -- which is expm1(2 * 2 h * max_j Sabs_ij) with Sabs in natural
   units; carried through the remaining products, each of which adds the h of its own rounded operand.  h = 2^-9 here: half
   the unit roundoff of bf16 (2^-8, see tests/test_attention_gpu.py).  The guaranteed worst case needs 2^-8; the stricter
   figure holds for these fixed seeds because no row has all its rounding errors at the bottom of their binades and
   aligned, and it is kept.
3. A torch-fp32 emulation of the bf16 kernels' arithmetic (tests/attention_cases.py: bf16 operands, fp32 products and sums,
   P / dS rounded to bf16, the plain and the lazy running maximum) stays inside BOTH tiers of the rule at every shape and
   scale the GPU tests use.
4. Faults planted in that emulation -- two rows swapped inside a block, one row times 1.25, one row dropped, the output
   times 1 + 2^-6, a maximum that moves without rescaling O -- each break tier 2.  This is what shows that the GPU criteria
   would notice a subtly wrong kernel; it is not to be loosened to make a GPU case pass.
"""
import math

import pytest
import torch

import attention_cases as ac
from oracle import attention as oa

F64 = torch.float64
U = ac.U
UB = 2.0 ** -9            # half the unit roundoff of bf16: the stricter figure, which the fixed seeds below do satisfy


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("scale", [ac.SCALE0] + ac.SCALES)
def test_attention_and_backward_match_torch_softmax_and_autograd(scale):
    N, T = 2, 96
    q, k, v, do = (t.double() for t in ac.make_case("peaky", N, T, scale))
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    S = (qr @ kr.transpose(1, 2)) * scale
    P = torch.softmax(S, -1)
    O = P @ vr
    (O * do).sum().backward()
    r = oa.attention(q, k, v, scale)
    assert _rel(r["O"], O.detach()) < 1e-13 and _rel(r["P"], P.detach()) < 1e-13
    assert _rel(r["lse"], torch.logsumexp(S.detach(), -1)) < 1e-13
    b = oa.attention_bwd(q, k, v, r["O"], r["lse"], do, scale)
    assert _rel(b["dq"], qr.grad) < 1e-12 and _rel(b["dk"], kr.grad) < 1e-12 and _rel(b["dv"], vr.grad) < 1e-12
    assert _rel(b["delta"], (do * O.detach()).sum(-1)) < 1e-13 and _rel(b["P"], P.detach()) < 1e-12
    # the magnitudes dominate what they are the magnitudes of
    for val, A, R in (("O", "A_O", "R_O"),):
        assert (r[val].abs() <= r[A] * (1 + 1e-12)).all() and (r[R] <= r[A] * (1 + 1e-12)).all()
    for val, A, R in (("dq", "A_dQ", "R_dQ"), ("dk", "A_dK", "R_dK"), ("dv", "A_dV", "R_dV")):
        assert (b[val].abs() <= b[A] * (1 + 1e-12)).all() and (b[R] <= b[A] * (1 + 1e-12)).all()
    assert (b["dS"].abs() <= b["A_dS"] * (1 + 1e-12)).all() and (b["delta"].abs() <= b["A_delta"] * (1 + 1e-12)).all()
    assert (r["S2"].abs() <= r["Sabs"] * (1 + 1e-12)).all()


def test_backward_is_defined_for_whatever_o_and_lse_the_caller_feeds():
    """o and lse are inputs: shifting lse by ln 2 halves P, and with it dv; delta follows the o that was given."""
    q, k, v, do = ac.make_case("plain", 1, 32)
    r = oa.attention(q, k, v, ac.SCALE0)
    b0 = oa.attention_bwd(q, k, v, r["O"], r["lse"], do, ac.SCALE0)
    b1 = oa.attention_bwd(q, k, v, 2 * r["O"], r["lse"] + math.log(2.0), do, ac.SCALE0)
    assert _rel(b1["dv"], 0.5 * b0["dv"]) < 1e-13 and _rel(b1["delta"], 2 * b0["delta"]) < 1e-13


@pytest.mark.parametrize("kind,scale", [("plain", ac.SCALE0), ("peaky", ac.SCALE0), ("plain", 0.25), ("peaky", ac.SCALES[1])])
def test_staging_models_within_first_order_operand_rounding_of_the_truth(kind, scale):
    N, T = 2, 160
    q, k, v, do = ac.make_case(kind, N, T, scale, seed=3)
    rho = 2 * UB + UB * UB + 4 * U
    t = oa.attention(q, k, v, scale)
    m = oa.fwd_bf16_model(q, k, v, scale)
    sab = torch.maximum(t["Sabs"], m["Sabs"]).amax(-1, keepdim=True)
    assert ((m["S2"] - t["S2"]).abs() <= rho * torch.maximum(t["Sabs"], m["Sabs"])).all()
    relP = torch.expm1(2 * oa.LN2 * rho * sab)
    assert ((m["P"] - t["P"]).abs() <= relP * t["P"]).all()
    assert ((m["O"] - t["O"]).abs() <= ((1 + relP) * (1 + UB) - 1) * t["A_O"]).all()
    assert ((m["lse"] - t["lse"]).abs() <= (oa.LN2 * rho * sab).squeeze(-1)).all()
    # backward: P = exp2(S2 - lse2) is not normalised (one factor), lse2 is rounded to fp32 in the models
    o32, lse32 = t["O"].float(), t["lse"].float()
    bt = oa.attention_bwd(q, k, v, o32, lse32, do, scale)
    relP1 = torch.expm1(oa.LN2 * (rho * sab + U * bt["lse2"].abs().unsqueeze(-1)))
    rds = (1 + relP1) * (1 + 2 * UB + UB * UB) - 1          # dS: P, and dP = bf16(dO) . bf16(v); delta is not rounded
    mq = oa.dq_bf16_model(q, k, v, o32, lse32, do, scale)
    mk = oa.dkv_bf16_model(q, k, v, o32, lse32, do, scale)
    for mm in (mq, mk):
        assert ((mm["P"] - bt["P"]).abs() <= relP1 * bt["P"]).all()
        assert ((mm["dS"] - bt["dS"]).abs() <= rds * bt["A_dS"]).all()
        assert torch.equal(mm["delta"], bt["delta"])
    assert ((mq["dq"] - bt["dq"]).abs() <= ((1 + rds) * (1 + UB) - 1) * bt["A_dQ"]).all()
    # rows differ in their bound: carry the row factor through the transposed sums
    s = abs(scale)
    Adk = s * ((bt["A_dS"] * ((1 + rds) * (1 + UB) - 1)).transpose(1, 2) @ q.double().abs())
    Adv = (bt["P"] * ((1 + relP1) * (1 + UB) - 1)).transpose(1, 2) @ do.double().abs()
    assert ((mk["dk"] - bt["dk"]).abs() <= Adk).all()
    assert ((mk["dv"] - bt["dv"]).abs() <= Adv).all()


# ------------------------------------------------------------------------------------------------ emulation vs the rule
def _mode(T):
    return "lazy" if T % 128 == 0 else "plain"


def emulated_ratios(q, k, v, do, scale, fault_fwd=None, fault_bwd=None, mode=None):
    """Worst err / bound of the emulation against the staging models, per output and tier, over the images of a case."""
    N, T = q.shape[:2]
    out = {}
    for n in range(N):
        O, lse = ac.emulate_fwd(q[n], k[n], v[n], scale, mode or _mode(T), fault_fwd)
        m = oa.fwd_bf16_model(q[n], k[n], v[n], scale)
        fb = ac.fwd_bounds(m, T, ac.BF16)
        res = {"O": ac.worst(O, m["O"], fb["O"]), "O2": ac.worst(O, m["O"], fb["O2"]), "lse": ac.worst(lse, m["lse"], fb["lse"])}
        dq, dk, dv, delta = ac.emulate_bwd(q[n], k[n], v[n], O, lse, do[n], scale, fault_bwd)
        mq = oa.dq_bf16_model(q[n], k[n], v[n], O, lse, do[n], scale)
        mk = oa.dkv_bf16_model(q[n], k[n], v[n], O, lse, do[n], scale)
        bq, bk = ac.bwd_bounds(mq, T, ac.BF16), ac.bwd_bounds(mk, T, ac.BF16)
        res.update(dq=ac.worst(dq, mq["dq"], bq["dq"]), dq2=ac.worst(dq, mq["dq"], bq["dq2"]),
                   dk=ac.worst(dk, mk["dk"], bk["dk"]), dk2=ac.worst(dk, mk["dk"], bk["dk2"]),
                   dv=ac.worst(dv, mk["dv"], bk["dv"]), dv2=ac.worst(dv, mk["dv"], bk["dv2"]),
                   delta=ac.worst(delta, mq["delta"], bq["delta"]))
        for key, val in res.items():
            out[key] = max(out.get(key, 0.0), val)
    return out


def _cases():
    for N, T in ac.BF16_SHAPES:
        for kind in ("plain", "peaky", "onehot"):
            yield kind, N, T, ac.SCALE0
    for T in (256, 384):
        yield "staircase", 1, T, ac.SCALE0
    for s in ac.SCALES:
        for N, T in ((3, 96), (2, 128)):
            yield "peaky", N, T, s


@pytest.mark.parametrize("kind,N,T,scale", list(_cases()))
def test_emulated_bf16_arithmetic_stays_inside_both_tiers(kind, N, T, scale):
    worst = {}
    for seed in (0, 1):
        q, k, v, do = ac.make_case(kind, N, T, scale, seed)
        for key, val in emulated_ratios(q, k, v, do, scale).items():
            worst[key] = max(worst.get(key, 0.0), val)
    print(f"emulation {kind} N={N} T={T} scale={scale:.4g}: " + " ".join(f"{a}={b:.3f}" for a, b in worst.items()))
    assert all(val <= 1.0 for val in worst.values()), worst


@pytest.mark.parametrize("T,kind", [(32, "plain"), (96, "peaky"), (256, "plain"), (640, "plain"), (640, "peaky")])
@pytest.mark.parametrize("fault", [f for f in ac.FAULTS if f != "norescale"])
def test_planted_faults_break_tier_two(T, kind, fault):
    q, k, v, do = ac.make_case(kind, 1, T)
    f = emulated_ratios(q, k, v, do, ac.SCALE0, fault_fwd=fault)
    assert f["O2"] > 1.0, f"forward fault '{fault}' passes tier 2: worst err / bound {f['O2']:.3f}"
    b = emulated_ratios(q, k, v, do, ac.SCALE0, fault_bwd=fault)
    for key in ("dq2", "dk2", "dv2"):
        assert b[key] > 1.0, f"backward fault '{fault}' passes tier 2 of {key}: worst err / bound {b[key]:.3f}"
    print(f"fault {fault} T={T} {kind}: O {f['O2']:.1f} dq {b['dq2']:.1f} dk {b['dk2']:.1f} dv {b['dv2']:.1f} times the bound")


@pytest.mark.parametrize("T,kind,mode", [(96, "plain", "plain"), (640, "peaky", "plain"), (256, "staircase", "lazy"),
                                         (384, "staircase", "lazy")])
def test_a_maximum_that_moves_without_rescaling_breaks_tier_two(T, kind, mode):
    q, k, v, do = ac.make_case(kind, 1, T)
    ok = emulated_ratios(q, k, v, do, ac.SCALE0, mode=mode)
    bad = emulated_ratios(q, k, v, do, ac.SCALE0, fault_fwd="norescale", mode=mode)
    assert ok["O2"] <= 1.0 and bad["O2"] > 1.0, (ok["O2"], bad["O2"])


@pytest.mark.parametrize("T", [256, 384])
def test_staircase_case_holds_the_four_kinds_of_query_in_one_wave(T):
    """On the fp64 scores of the staged operands: see attention_cases._staircase."""
    q, k, v, _ = ac.make_case("staircase", 1, T)
    ac.assert_staircase(oa.fwd_bf16_model(q, k, v, ac.SCALE0)["S2"][0])


def test_onehot_case_separates_the_scores_by_more_than_150():
    for N, T in ((1, 32), (1, 640)):
        q, k, v, _ = ac.make_case("onehot", N, T)
        S2 = oa.fwd_bf16_model(q, k, v, ac.SCALE0)["S2"][0]
        top = S2.topk(2, -1)
        assert (top.indices[:, 0] == ac.onehot_target(T)).all() and (top.values[:, 0] - top.values[:, 1] > 150.0).all()
