"""The nine fused attention kernels (csrc/attention.hip, csrc/attention_bf16.hip) called through the C ABI, against the fp64
oracles of oracle/attention.py (which tests/test_oracle_attention.py pins to torch.softmax / autograd on the CPU, and
whose comparison rule it proves sensitive by planting faults in an emulation of the kernels' arithmetic).

Every element of every output is compared; nothing is masked, nothing is scaled by the tensor's maximum.  The rule is
code in tests/attention_cases.py (fwd_bounds, bwd_bounds); this is its derivation.

Notation
--------
u = 2^-24, the unit roundoff of fp32.  u_b = 2^-8, the unit roundoff of bf16: 8 significant bits, round to nearest even
(the (__bf16) casts compile to that), so |bf16(x) - x| <= 2^-8 |x|, attained just above a power of two.  (2^-9, which is
sometimes quoted, is the error at the top of a binade; as a worst case it is false, and the CPU emulation, whose
roundings are exact, exceeds a tier 1 built on it at T = 32.)  The library is built with -ffp-contract=off: every
product and sum written in the source is a rounding of its own.  A, R, Sabs, S2, G are the oracle's magnitudes (docstring
of oracle/attention.py); all scores are in log2 units; D_i = max_j S2_ij - min_j S2_ij is the score range of a row.

The score argument, E_i
-----------------------
A probability is p = exp2(s - m) (forward) or exp2(s - lse2) (backward).  An absolute error E in its argument is a relative
error ln2 * E in p.  Counting the roundings on the way to the argument:
  fp32 kernels    a score is a chain of 128 MFMA accumulation steps: term j passes through 129 - j roundings, at most 128 u
                  Sabs; + 1 for fl(q * c32) (attention.hip:51), + 1 for c32 = fl(scale * log2e) (:382), whose constant is
                  itself 0.22 u off (inside the slack 128 u Sabs - u sum_j (129 - j)|t_j| unless four fifths of Sabs sit in
                  the first product): e_i = (128 + 2) u max_j Sabs_ij.
                  Forward: s - m_new is one rounding of at most u D_i (:109); the rescales multiply O and l by
                  exp2(m_run - m_new) (:106), whose arguments telescope to at most D_i in all: 2 u D_i.
                  Backward: s - lse2 is one rounding of at most u (D_i + log2 T) (:229, :337) and lse2 = fl(lse * log2e)
                  (:179, :295) one of u |lse2| which the truth does not have.
  bf16 kernels    products of bf16 numbers are exact in fp32, the chain has 128 steps; the pipelined kernels start the
                  accumulator at a statistic instead of zero (-m: attention_bf16.hip:344; -lse2: :552, :574, :832, :857 via
                  init_rows), one more term of size at most max_j |S2_ij| + log2 T:
                  e_i = (128 + 1) u (max_j Sabs_ij + max_j |S2_ij| + log2 T).  The plain kernels satisfy it a fortiori.
                  Forward: the subtraction (:192; pipelined: inside the chain), the shift of the tile in flight (:369, :396)
                  and the telescoping rescales (:189, :365): 3 u D_i.  Backward: the subtraction (:475, :698), u (D_i +
                  log2 T); lse2 is rounded identically in the model (oracle: lse2_32), no term.
  E_i = e_i + (2 | 3) u D_i  (forward),   E_i = e_i + u (D_i + log2 T) [+ u |lse2_i|, fp32 kernels]  (backward).
In the forward pass P = p / l and l carries the same relative error: 2 ln2 E_i.  The backward P is not normalised by the
kernel: ln2 E_i.

fp32 terms (the whole bound of the fp32 kernels, which are compared with the fp64 truth on the same fp32 operands)
----------
  O        ((T + 4) u + 2 ln2 E_i) A_O + floor         n = T: the chain of P.V over all keys; + 4: exp2, 1 / l, * inv, and
                                                       the product inside the MFMA step
  lse      ln2 E_i + (T + 4) u + 4 u A_lse             m is a score (E_i); l a sum of T positive terms, (T + 4) u relative,
                                                       the same absolute on ln l; log2f, the sum m + log2 l and * ln2
                                                       against A_lse = ln2 (|m| + |log2 l|)
  delta    (128 + 4) u A_delta                         n = 128 (attn_delta_kernel: 4 products, 2 + 5 additions per term)
  dS       (ln2 E_i + (128 + 4 + 4) u) A_dS            dP is a chain of 128 and delta is off by (128 + 4) u A_delta: both
                                                       inside A_dS = P (sum |dO||v| + A_delta); + 4: exp2, dP - delta,
                                                       P * (.), and the MFMA product
  dQ       (T + 4) u A_dQ + sum_j [dS term] + floor    n = T; + 4 holds the final * scale.  The dS term is constant along a
                                                       row of dQ and varies along the sums of dK and dV, so it is carried
  dK       (T + 4) u A_dK + sum_i [dS term] + floor    inside them: scale sum_i (ln2 E_i + 136 u) A_dS,ij |q_ic|
  dV       (T + 4) u A_dV + sum_i (ln2 E_i + 2 u) P_ij |dO_ic| + floor
  floor    2^-126 * (sum_j |v_jc|  |  scale sum_j G_ij |k_jc|  |  scale sum_i G_ij |q_ic|  |  sum_i |dO_ic|):
           fast_exp2 (attention_bf16.hip:46) returns zero where the probability is subnormal, and exp2f loses relative
           precision there; the scores of the one-hot case are more than 150 apart.  As in pd_softmax_rows.
These are first-order worst cases of the chains named; they are kept at n = T although l (forward) adds a second chain of T
to O -- the stricter form.  A kernel beyond them is a finding, not a reason to scale them.

bf16 kernels: compared with their staging model (the same formulas on the operands as the kernel rounds them; oracle
docstring for the rounding points), so that what remains is ONE bf16 rounding per term -- P in front of P.V and P^T.dO, dS in
front of dS.K and dS^T.Q (acc_frag, attention_bf16.hip:58) -- and fp32 arithmetic:
  tier 1, deterministic     |got - model| <= (r u_b + fp32 terms) A,  r = 1 for O, dV (P) and for dQ, dK (dS)
  tier 2, concentration     |got - model| <= 7 * 2^-9 R + (fp32 terms) A
                            The rounding errors x_j of the terms are treated as independent and zero-mean.  A rounding error
                            is uniform on +-half an ulp, at most +-u_b |a_j|: sub-Gaussian with variance proxy (u_b a_j)^2 / 3,
                            so P(|sum x_j| > 3.5 u_b R) <= 2 exp(-3 * 3.5^2 / 2) = 2e-8 per element if EVERY term sat just
                            above a power of two, and 2 exp(-36) for mantissas spread over the binade (mean square half-ulp
                            0.52 u_b^2).  Sums of up to 12 terms cannot exceed it at all (12 u_b a < 3.5 u_b sqrt(12) a).
                            The seeds are fixed.  Tier 2 is the sharper one wherever many keys share the mass, tier 1
                            where one does.
  lse of the forward        against the model's lse within the fp32 terms only: no bf16 rounding lies between them.
  delta                     fp32, as above.
Both tiers must hold for 100 % of the elements.  test_oracle_attention.py records what the exact emulation reaches (at
most 0.55 of tier 2, 0.83 of tier 1) and that a key scaled by 1.25 lands 4 to 18 times beyond tier 2, a gain of 1 + 2^-6
1.7 to 4.3 times.

Which kernel runs at which token count (dispatch: attention_bf16.hip:978, :1034, :1050)
------------------------------------
   T     forward                          dQ                            dK / dV                 last workgroup
   32    plain, one key block             plain                         plain                   one live wave
   64    plain                            pipelined, 1 unrolled pair    plain                   two live waves
   96    plain                            plain                         plain                   three live waves
  128    pipelined, 1 iteration of 4      pipelined                     pipelined               full
  160    plain                            plain                         plain                   one live wave of four
  192    plain                            pipelined                     plain                   two live waves
  256    pipelined, 2 iterations          pipelined                     pipelined               full
  320    plain                            pipelined                     plain                   two live waves
  384    pipelined, 3 iterations (odd)    pipelined                     pipelined               full
  640    pipelined, 5 iterations          pipelined                     pipelined               full
fp32 kernels (one kernel each): T = 32, 96, 160, 288 (= 2 * 128 + 32: one live wave).
pd_attn_bf16_bwd_parts issues delta + packing (1), dK / dV (2) and dQ (4) separately.

Data: plain (randn), peaky (q * 2.5), one-hot (scores more than 150 apart: O is one row of v, which tests the key and
channel permutations of the transposed tiles directly), and the staircase (attention_cases._staircase: in ONE wave, queries
whose maximum moves by more than 9 in every key block -- all four unroll positions, consecutive moves, the rescale of the
tile in flight --, queries that never move, queries that move by less than the threshold, queries that see their peak
first; asserted on the fp64 scores).  scale in {1/sqrt(128), 0.25, 0.03}.  The backward runs once on the kernel's own (o,
lse) and once on the fp64 truth rounded to fp32; the oracles take them as given.  Every output and the workspace sit in
buffers with a sentinel tail.

Observed on the MI355X: DESIGN.md section 4.
"""
import pytest
import torch

import attention_cases as ac
from oracle import attention as oa

pytestmark = pytest.mark.gpu

C = 128
SENT = -77.25            # behind the last token of every output
WS_SENT = 0xA5           # behind the last byte of the workspace
PAD_TOK = 3
PAD_WS = 256
HEADROOM = {}            # kernel -> (worst err / bound, case)


def _L():
    from polardepth._lib import lib, check, ptr, stream_ptr
    return lib, check, ptr, stream_ptr


class Buf:
    """A flat fp32 output of `ntok` tokens x `width` with PAD_TOK sentinel tokens behind it."""

    def __init__(self, ntok, width):
        self.n = ntok * width
        self.t = torch.full(((ntok + PAD_TOK) * width,), SENT, dtype=torch.float32, device="cuda")

    def val(self, *shape):
        return self.t[:self.n].view(*shape)

    def tail_ok(self):
        return bool((self.t[self.n:] == SENT).all())

    def untouched(self):
        return bool((self.t == SENT).all())


class Ws:
    def __init__(self, N, T, backward):
        lib = _L()[0]
        self.bytes = lib.pd_attn_bf16_workspace(N, T, C, backward)
        self.t = torch.full((self.bytes + PAD_WS,), WS_SENT, dtype=torch.uint8, device="cuda")

    def tail_ok(self):
        return bool((self.t[self.bytes:] == WS_SENT).all())


def _cuda(*ts):
    return [t.to("cuda").contiguous() for t in ts]


def fwd_f32(q, k, v, scale):
    lib, check, ptr, sp = _L()
    N, T = q.shape[:2]
    o, lse = Buf(N * T, C), Buf(N * T, 1)
    check(lib.pd_attn_fwd(ptr(q), ptr(k), ptr(v), ptr(o.t), ptr(lse.t), N, T, C, scale, sp()), "pd_attn_fwd")
    torch.cuda.synchronize()
    return o, lse


def bwd_f32(q, k, v, o, do, lse, scale):
    lib, check, ptr, sp = _L()
    N, T = q.shape[:2]
    out = {"delta": Buf(N * T, 1), "dq": Buf(N * T, C), "dk": Buf(N * T, C), "dv": Buf(N * T, C)}
    check(lib.pd_attn_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(out["delta"].t), ptr(out["dq"].t),
                          ptr(out["dk"].t), ptr(out["dv"].t), N, T, C, scale, sp()), "pd_attn_bwd")
    torch.cuda.synchronize()
    return out


def fwd_bf16(q, k, v, scale):
    lib, check, ptr, sp = _L()
    N, T = q.shape[:2]
    o, lse, ws = Buf(N * T, C), Buf(N * T, 1), Ws(N, T, 0)
    check(lib.pd_attn_bf16_fwd(ptr(q), ptr(k), ptr(v), ptr(o.t), ptr(lse.t), ptr(ws.t), ws.bytes, N, T, C, scale, sp()),
          "pd_attn_bf16_fwd")
    torch.cuda.synchronize()
    return o, lse, ws


def bwd_bf16(q, k, v, o, do, lse, scale, parts=(7,), entry="parts"):
    """parts: the sequence of pd_attn_bf16_bwd_parts calls, all on the same fresh sentinel buffers; entry 'whole' calls
    pd_attn_bf16_bwd instead."""
    lib, check, ptr, sp = _L()
    N, T = q.shape[:2]
    out = {"delta": Buf(N * T, 1), "dq": Buf(N * T, C), "dk": Buf(N * T, C), "dv": Buf(N * T, C), "ws": Ws(N, T, 1)}
    args = (ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(out["delta"].t), ptr(out["dq"].t), ptr(out["dk"].t),
            ptr(out["dv"].t), ptr(out["ws"].t), out["ws"].bytes, N, T, C, scale)
    if entry == "whole":
        check(lib.pd_attn_bf16_bwd(*args, sp()), "pd_attn_bf16_bwd")
    else:
        for p in parts:
            check(lib.pd_attn_bf16_bwd_parts(*args, p, sp()), f"pd_attn_bf16_bwd_parts({p})")
    torch.cuda.synchronize()
    return out


def _kernels(T):
    return {"fwd": "fwd_bf16_pipe" if T % 128 == 0 else "fwd_bf16", "dq": "dq_bf16_pipe" if T % 64 == 0 else "dq_bf16",
            "dkv": "dkv_bf16_pipe" if T % 128 == 0 else "dkv_bf16"}


def _judge(kernel, what, case, got, ref, bound, failures):
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, f"{case} {what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not torch.isfinite(got).all():
        failures.append(f"{case} {what}: non-finite output")
        return
    ratio = ac.worst(got, ref, bound)
    key = f"{kernel} {what}"
    if ratio > HEADROOM.get(key, (0.0, ""))[0]:
        HEADROOM[key] = (ratio, case)
    print(f"  {case:<44s} {key:<28s} worst err / bound {ratio:.3f}")
    if not ratio <= 1.0:
        err = (got - ref).abs()
        bad = err > bound
        kk = int((err - bound).argmax())
        failures.append(f"{case} {key}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst err / bound {ratio:.3f} at flat "
                        f"index {kk}: got {got.flatten()[kk].item()!r} ref {ref.flatten()[kk].item()!r} "
                        f"bound {bound.expand_as(err).flatten()[kk].item():.3e}")


@pytest.fixture(scope="module", autouse=True)
def _headroom_report():
    yield
    print("\nworst err / bound per kernel and output over this run:")
    for key in sorted(HEADROOM):
        print(f"  {key:<30s} {HEADROOM[key][0]:.3f}   ({HEADROOM[key][1]})")


def _tails(case, bufs, failures):
    for name, b in bufs.items():
        if not b.tail_ok():
            failures.append(f"{case}: the sentinel behind {name} was overwritten")


# ====================================================================================================== fp32 kernels
F32_CASES = [(N, T, kind, ac.SCALE0) for N, T in ac.F32_SHAPES for kind in ("plain", "peaky", "onehot")] + \
            [(3, 96, "peaky", s) for s in ac.SCALES]


@pytest.mark.parametrize("N,T,kind,scale", F32_CASES)
def test_fp32_kernels_against_the_fp64_truth(N, T, kind, scale):
    case = f"f32 {kind} N={N} T={T} scale={scale:.4g}"
    failures = []
    q, k, v, do = ac.make_case(kind, N, T, scale)
    qd, kd, vd, dod = _cuda(q, k, v, do)
    o, lse = fwd_f32(qd, kd, vd, scale)
    t = oa.attention(q, k, v, scale)
    fb = ac.fwd_bounds(t, T, ac.F32)
    _judge("attn_fwd", "O", case, o.val(N, T, C), t["O"], fb["O"], failures)
    _judge("attn_fwd", "lse", case, lse.val(N, T), t["lse"], fb["lse"], failures)
    o2, lse2 = fwd_f32(qd, kd, vd, scale)
    assert torch.equal(o.t, o2.t) and torch.equal(lse.t, lse2.t), case + ": the same call twice gives different bits"
    _tails(case, {"o": o, "lse": lse}, failures)
    pairs = (("own", o.val(N, T, C).clone(), lse.val(N, T).clone()),
             ("truth", t["O"].float().cuda(), t["lse"].float().cuda()))
    for tag, od, lsed in pairs:
        g = bwd_f32(qd, kd, vd, od, dod, lsed, scale)
        b = oa.attention_bwd(q, k, v, od, lsed, do, scale)
        bb = ac.bwd_bounds(b, T, ac.F32)
        c2 = f"{case} [{tag} o, lse]"
        _judge("attn_delta", "delta", c2, g["delta"].val(N, T), b["delta"], bb["delta"], failures)
        _judge("attn_bwd_dq", "dq", c2, g["dq"].val(N, T, C), b["dq"], bb["dq"], failures)
        _judge("attn_bwd_dkv", "dk", c2, g["dk"].val(N, T, C), b["dk"], bb["dk"], failures)
        _judge("attn_bwd_dkv", "dv", c2, g["dv"].val(N, T, C), b["dv"], bb["dv"], failures)
        _tails(c2, g, failures)
    assert not failures, "\n".join(failures)


# ====================================================================================================== bf16 kernels
BF16_CASES = [(N, T, kind, ac.SCALE0) for N, T in ac.BF16_SHAPES for kind in ("plain", "peaky", "onehot")] + \
             [(1, T, "staircase", ac.SCALE0) for T in (256, 384)] + \
             [(N, T, "peaky", s) for s in ac.SCALES for N, T in ((3, 96), (2, 128))]


def _judge_bf16_fwd(case, kern, q, k, v, scale, o, lse, failures, images=None):
    T = q.shape[1]
    m = oa.fwd_bf16_model(q, k, v, scale)
    fb = ac.fwd_bounds(m, T, ac.BF16)
    sel = (lambda x: x) if images is None else (lambda x: x[images])
    _judge(kern["fwd"], "O tier 1", case, sel(o), m["O"], fb["O"], failures)
    _judge(kern["fwd"], "O tier 2", case, sel(o), m["O"], fb["O2"], failures)
    _judge(kern["fwd"], "lse", case, sel(lse), m["lse"], fb["lse"], failures)
    return m


def _judge_bf16_bwd(case, kern, q, k, v, o, lse, do, scale, g, failures, images=None):
    """g: name -> [N, T, ..] device tensors of the kernel; o, lse: what the kernel was given (CPU or device)."""
    T = q.shape[1]
    sel = (lambda x: x) if images is None else (lambda x: x[images])
    mq = oa.dq_bf16_model(q, k, v, o, lse, do, scale)
    mk = oa.dkv_bf16_model(q, k, v, o, lse, do, scale)
    bq, bk = ac.bwd_bounds(mq, T, ac.BF16), ac.bwd_bounds(mk, T, ac.BF16)
    _judge("attn_delta_bf16", "delta", case, sel(g["delta"]), mq["delta"], bq["delta"], failures)
    for tier, sfx in (("tier 1", ""), ("tier 2", "2")):
        _judge(kern["dq"], "dq " + tier, case, sel(g["dq"]), mq["dq"], bq["dq" + sfx], failures)
        _judge(kern["dkv"], "dk " + tier, case, sel(g["dk"]), mk["dk"], bk["dk" + sfx], failures)
        _judge(kern["dkv"], "dv " + tier, case, sel(g["dv"]), mk["dv"], bk["dv" + sfx], failures)


@pytest.mark.parametrize("N,T,kind,scale", BF16_CASES)
def test_bf16_kernels_against_their_staging_models(N, T, kind, scale):
    case = f"bf16 {kind} N={N} T={T} scale={scale:.4g}"
    kern = _kernels(T)
    failures = []
    q, k, v, do = ac.make_case(kind, N, T, scale)
    qd, kd, vd, dod = _cuda(q, k, v, do)
    o, lse, ws = fwd_bf16(qd, kd, vd, scale)
    m = _judge_bf16_fwd(case, kern, q, k, v, scale, o.val(N, T, C), lse.val(N, T), failures)
    _tails(case, {"o": o, "lse": lse, "the forward workspace": ws}, failures)
    if kind == "staircase":
        for n in range(N):
            ac.assert_staircase(m["S2"][n])
    if kind == "onehot":          # O is one row of v: bf16(v) exactly where the probability rounds to 1, within u_b |v| of v
        assert (m["S2"].topk(2, -1).values.diff(dim=-1) < -150.0).all(), case + ": the scores are not 150 apart"
        want = v.double()[:, ac.onehot_target(T), :]
        got = o.val(N, T, C).cpu().double()
        if not ((got - want).abs() <= ac.UB * want.abs() + ac.FLOOR * v.double().abs().sum(1, keepdim=True)).all():
            failures.append(case + ": O is not the designated row of v within u_b |v|")
    t = oa.attention(q, k, v, scale)
    pairs = (("own", o.val(N, T, C).clone(), lse.val(N, T).clone()),
             ("truth", t["O"].float().cuda(), t["lse"].float().cuda()))
    for tag, od, lsed in pairs:
        g = bwd_bf16(qd, kd, vd, od, dod, lsed, scale, entry="whole")
        c2 = f"{case} [{tag} o, lse]"
        _judge_bf16_bwd(c2, kern, q, k, v, od, lsed, do, scale,
                        {"delta": g["delta"].val(N, T), "dq": g["dq"].val(N, T, C), "dk": g["dk"].val(N, T, C),
                         "dv": g["dv"].val(N, T, C)}, failures)
        _tails(c2, {"delta": g["delta"], "dq": g["dq"], "dk": g["dk"], "dv": g["dv"], "the backward workspace": g["ws"]}, failures)
    assert not failures, "\n".join(failures)


# ====================================================================================================== parts, streams, determinism
def _same_bits(a, b, names=("delta", "dq", "dk", "dv")):
    return [n for n in names if not torch.equal(a[n].t, b[n].t)]


@pytest.mark.parametrize("N,T", [(3, 96), (2, 64), (2, 128), (1, 160), (1, 256)])
def test_bf16_backward_parts_give_the_bits_of_the_whole_and_write_nothing_else(N, T):
    q, k, v, do = ac.make_case("peaky", N, T, seed=2)
    qd, kd, vd, dod = _cuda(q, k, v, do)
    o, lse, _ = fwd_bf16(qd, kd, vd, ac.SCALE0)
    od, lsed = o.val(N, T, C).clone(), lse.val(N, T).clone()
    run = lambda **kw: bwd_bf16(qd, kd, vd, od, dod, lsed, ac.SCALE0, **kw)
    whole = run(parts=(7,))
    assert not _same_bits(whole, run(parts=(7,))), "parts = 7 twice gives different bits"
    assert not _same_bits(whole, run(entry="whole")), "pd_attn_bf16_bwd differs from parts = 7"
    for seq in ((1, 2, 4), (1, 4, 2), (3, 4)):
        got = run(parts=seq)
        assert not _same_bits(whole, got), f"parts {seq}: {_same_bits(whole, got)} differ from parts = 7"
        assert all(got[n].tail_ok() for n in got), f"parts {seq}: a sentinel tail was overwritten"
    assert all(whole[n].tail_ok() for n in whole), "parts = 7: a sentinel tail was overwritten"
    p1 = run(parts=(1,))
    assert torch.equal(p1["delta"].t, whole["delta"].t), "parts = 1: delta"
    assert p1["dq"].untouched() and p1["dk"].untouched() and p1["dv"].untouched(), "parts = 1 wrote a gradient"
    assert p1["ws"].tail_ok()
    p12 = run(parts=(1, 2))
    assert p12["dq"].untouched(), "parts = 2 wrote dq"
    assert not _same_bits(whole, p12, ("delta", "dk", "dv"))
    p14 = run(parts=(1, 4))
    assert p14["dk"].untouched() and p14["dv"].untouched(), "parts = 4 wrote dk or dv"
    assert not _same_bits(whole, p14, ("delta", "dq"))
    # parts 2 and 4 on two streams behind part 1, as FlashAttentionFn.backward enqueues them
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    lib, check, ptr, sp = _L()
    out = {"delta": Buf(N * T, 1), "dq": Buf(N * T, C), "dk": Buf(N * T, C), "dv": Buf(N * T, C), "ws": Ws(N, T, 1)}
    args = (ptr(qd), ptr(kd), ptr(vd), ptr(od), ptr(dod), ptr(lsed), ptr(out["delta"].t), ptr(out["dq"].t), ptr(out["dk"].t),
            ptr(out["dv"].t), ptr(out["ws"].t), out["ws"].bytes, N, T, C, ac.SCALE0)
    torch.cuda.synchronize()
    check(lib.pd_attn_bf16_bwd_parts(*args, 1, sp()), "parts 1")
    side.wait_stream(main)
    check(lib.pd_attn_bf16_bwd_parts(*args, 2, sp()), "parts 2")
    with torch.cuda.stream(side):
        check(lib.pd_attn_bf16_bwd_parts(*args, 4, sp()), "parts 4")
    main.wait_stream(side)
    torch.cuda.synchronize()
    assert not _same_bits(whole, out), f"two streams: {_same_bits(whole, out)} differ from parts = 7"
    assert all(out[n].tail_ok() for n in out)


@pytest.mark.parametrize("N,T", [(3, 96), (2, 128)])
def test_bf16_forward_is_deterministic(N, T):
    q, k, v, _ = ac.make_case("peaky", N, T, seed=4)
    qd, kd, vd = _cuda(q, k, v)
    a, b = fwd_bf16(qd, kd, vd, ac.SCALE0), fwd_bf16(qd, kd, vd, ac.SCALE0)
    assert torch.equal(a[0].t, b[0].t) and torch.equal(a[1].t, b[1].t)


# ====================================================================================================== pack grid-stride
def test_pack_kernel_grid_stride_beyond_4096_blocks():
    """N = 1026, T = 128: 4104 blocks of 32 tokens, attn_pack_multi_kernel launches 4096 and strides (image 1024 straddles
    block 4096).  About 0.5 GB of operands and outputs and 0.24 GB of workspace per run, from the launch code."""
    N, T, H = 1026, 128, 513
    kern = _kernels(T)
    g = torch.Generator(device="cuda").manual_seed(11)
    qd, kd, vd, dod = (torch.randn(N, T, C, generator=g, device="cuda") for _ in range(4))
    qd *= 2.0
    o, lse, ws = fwd_bf16(qd, kd, vd, ac.SCALE0)
    od, lsed = o.val(N, T, C), lse.val(N, T)
    gb = bwd_bf16(qd, kd, vd, od, dod, lsed, ac.SCALE0, entry="whole")
    for h in (0, 1):
        s = slice(H * h, H * h + H)
        o2, lse2, ws2 = fwd_bf16(qd[s], kd[s], vd[s], ac.SCALE0)
        assert torch.equal(o2.val(H, T, C), od[s]) and torch.equal(lse2.val(H, T), lsed[s]), f"forward, half {h}"
        g2 = bwd_bf16(qd[s], kd[s], vd[s], od[s], dod[s], lsed[s], ac.SCALE0, entry="whole")
        for name, shape in (("delta", (T,)), ("dq", (T, C)), ("dk", (T, C)), ("dv", (T, C))):
            assert torch.equal(g2[name].val(H, *shape), gb[name].val(N, *shape)[s]), f"{name}, half {h}"
        assert o2.tail_ok() and lse2.tail_ok() and ws2.tail_ok() and all(g2[n].tail_ok() for n in g2)
        del o2, lse2, ws2, g2
    assert o.tail_ok() and lse.tail_ok() and ws.tail_ok() and all(gb[n].tail_ok() for n in gb)
    img = [0, 1024, 1025]
    failures = []
    q, k, v, do, oc, lc = (t[img].cpu() for t in (qd, kd, vd, dod, od, lsed))
    case = "bf16 grid-stride N=1026 T=128 images 0, 1024, 1025"
    _judge_bf16_fwd(case, kern, q, k, v, ac.SCALE0, oc, lc, failures)
    _judge_bf16_bwd(case, kern, q, k, v, oc, lc, do, ac.SCALE0,
                    {"delta": gb["delta"].val(N, T)[img], "dq": gb["dq"].val(N, T, C)[img], "dk": gb["dk"].val(N, T, C)[img],
                     "dv": gb["dv"].val(N, T, C)[img]}, failures)
    assert not failures, "\n".join(failures)


# ====================================================================================================== empty batch
def test_empty_batch_returns_ok_and_touches_nothing():
    lib, check, ptr, sp = _L()
    T = 96
    bufs = [Buf(T, C) for _ in range(4)] + [Buf(T, 1) for _ in range(2)]
    o, dq, dk, dv, lse, delta = bufs
    ws = Ws(1, T, 1)
    x = torch.zeros(T, C, device="cuda")
    assert lib.pd_attn_bf16_fwd(ptr(x), ptr(x), ptr(x), ptr(o.t), ptr(lse.t), ptr(ws.t), ws.bytes, 0, T, C, ac.SCALE0, sp()) == 0
    assert lib.pd_attn_bf16_fwd(None, None, None, None, None, None, 0, 0, T, C, ac.SCALE0, sp()) == 0
    a = (ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), ptr(delta.t), ptr(dq.t), ptr(dk.t), ptr(dv.t), ptr(ws.t), ws.bytes, 0, T, C,
         ac.SCALE0)
    assert lib.pd_attn_bf16_bwd(*a, sp()) == 0
    for parts in (1, 2, 4, 7):
        assert lib.pd_attn_bf16_bwd_parts(*a, parts, sp()) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs) and bool((ws.t == WS_SENT).all())
