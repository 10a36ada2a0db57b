"""Shared by tests/test_oracle_attention.py (CPU) and tests/test_attention_gpu.py (GPU): the input cases, the comparison
rule of the attention kernels as code, and a CPU emulation of the bf16 kernels' arithmetic in which faults can be planted.
The derivation of every constant is in the docstring of tests/test_attention_gpu.py; nothing here is fitted to a result."""
import math

import torch

from oracle import attention as oa

U = 2.0 ** -24            # unit roundoff of fp32
UB = 2.0 ** -8            # unit roundoff of bf16: 8 significant bits, round to nearest even (half of ulp(1) = 2^-7)
TIER2 = 7.0 * 2.0 ** -9   # tier 2: 7 * 2^-9 * R (= 3.5 unit roundoffs; see tests/test_attention_gpu.py)
FLOOR = 2.0 ** -126       # smallest normal fp32: fast_exp2 flushes what lies below
C = 128
F32_SHAPES = [(1, 32), (3, 96), (2, 160), (1, 288)]
BF16_SHAPES = [(1, 32), (2, 64), (3, 96), (2, 128), (1, 160), (2, 192), (1, 256), (1, 320), (2, 384), (1, 640)]
SCALE0 = float(torch.tensor(1.0 / math.sqrt(128.0), dtype=torch.float32))
SCALES = [float(torch.tensor(s, dtype=torch.float32)) for s in (0.25, 0.03)]

# per kernel family: roundings of a score (chain), whether an accumulator starts at a statistic, subtractions of the order
# of the row's score range in the forward pass, whether lse * log2 e is rounded on the kernel's side only
F32 = dict(chain=130, acc_init=False, sub=2, lse=1)
BF16 = dict(chain=129, acc_init=True, sub=3, lse=0)


# ====================================================================================================== cases
def _gen(N, T, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, T, C, generator=g) for _ in range(4)]


def onehot_target(T):
    return (7 * torch.arange(T) + 3) % T


def make_case(kind, N, T, scale=SCALE0, seed=0):
    """q, k, v, do: fp32 [N, T, 128] on the CPU."""
    q, k, v, do = _gen(N, T, 1000 * seed + 7 * T + N)
    if kind == "plain":
        pass
    elif kind == "peaky":
        q = q * 2.5
    elif kind == "onehot":
        # keys are sign vectors, query i is a multiple of key pi(i): its own score is 128 s c, any other at most |<k, k'>| s c
        g = torch.Generator().manual_seed(seed + T)
        k = torch.where(torch.rand(N, T, C, generator=g) < 0.5, -1.0, 1.0)
        s = float(2 ** math.ceil(math.log2(320.0 / (scale * oa.LOG2E * 64.0))))
        q = s * k[:, onehot_target(T), :]
    elif kind == "staircase":
        q, k = _staircase(q, k, T, scale)
    else:
        raise ValueError(kind)
    return q.contiguous(), k.contiguous(), v.contiguous(), do.contiguous()


STAIR_A, STAIR_B, STAIR_C, STAIR_D = slice(0, 8), slice(8, 16), slice(16, 24), slice(24, 32)


def _staircase(q, k, T, scale):
    """The first wave (queries 0..31 of every image) holds four kinds of query, each steered through a channel of its own:
      A  0..7    meets a new maximum by 12 log2 units in EVERY key block (the lazy maximum moves at each unroll position, and
                 in consecutive blocks)
      B  8..15   its maximum never moves: the largest score is in block 0, later blocks stay 5 units below
      C  16..23  its maximum moves by 3 units per block (between 0 and 8: below the threshold of its own)
      D  24..31  sees its peak first (key 0, 40 units up) and only far smaller scores afterwards
    Everything else is noise of about +-1 unit.  Key 32 b + 5 carries the steps of block b."""
    c = scale * oa.LOG2E
    q, k = 0.3 * q, 0.3 * k
    q[:, :, :4] = 0.0
    k[:, :, :4] = 0.0
    nkb = T // 32
    amp = 8.0
    q[:, STAIR_A, 0] = amp
    q[:, STAIR_B, 1] = amp
    q[:, STAIR_C, 2] = amp
    q[:, STAIR_D, 3] = amp
    for b in range(nkb):
        k[:, 32 * b + 5, 0] = 12.0 * b / (amp * c)
        k[:, 32 * b + 5, 2] = 3.0 * b / (amp * c)
    k[:, 5, 1] = 8.0 / (amp * c)
    k[:, 0, 3] = 40.0 / (amp * c)
    return q, k


def block_maxima(S2):
    """[.., T, nkb] maximum of every 32-key block and the running maximum BEFORE each block (from block 1 on)."""
    bm = S2.reshape(*S2.shape[:-1], S2.shape[-1] // 32, 32).amax(-1)
    run = torch.cummax(bm, -1).values
    return bm, run


def assert_staircase(S2):
    bm, run = block_maxima(S2)
    step = bm[:, 1:] - run[:, :-1]                       # what block b >= 1 adds to the running maximum before it
    assert (step[STAIR_A] > 9.0).all(), "A: a new maximum by more than 9 in every block"
    assert (step[STAIR_B] < 0.0).all(), "B: the maximum never moves"
    assert ((step[STAIR_C] > 0.0) & (step[STAIR_C] < 8.0)).all(), "C: moves by between 0 and 8 in every block"
    assert (step[STAIR_D] < -20.0).all() and (S2[STAIR_D].argmax(-1) == 0).all(), "D: peak first, far smaller afterwards"


# ====================================================================================================== the comparison rule
def _row_terms(r, T, fam):
    S2, Sabs = r["S2"], r["Sabs"]
    base = Sabs.amax(-1, keepdim=True)
    if fam["acc_init"]:
        base = base + S2.abs().amax(-1, keepdim=True) + math.log2(T)
    D = S2.amax(-1, keepdim=True) - S2.amin(-1, keepdim=True)
    return fam["chain"] * U * base, D


def fwd_bounds(r, T, fam):
    """r: oracle.attention (fam F32) or fwd_bf16_model (fam BF16).  {'O': tier 1 or the fp32 bound, 'O2': tier 2, 'lse'}."""
    e, D = _row_terms(r, T, fam)
    E = e + fam["sub"] * U * D
    f32 = (T + 4) * U + 2.0 * oa.LN2 * E
    floor = FLOOR * r["vabs_sum"]
    out = {"lse": (oa.LN2 * E + (T + 4) * U).squeeze(-1) + 4 * U * r["A_lse"]}
    if fam is F32:
        out["O"] = f32 * r["A_O"] + floor
    else:
        out["O"] = (UB + f32) * r["A_O"] + floor
        out["O2"] = TIER2 * r["R_O"] + f32 * r["A_O"] + floor
    return out


def bwd_bounds(r, T, fam):
    """r: oracle.attention_bwd (fam F32), dq_bf16_model or dkv_bf16_model (fam BF16).  Keys 'dq', 'dk', 'dv' (tier 1 or the
    fp32 bound), 'dq2', 'dk2', 'dv2' (tier 2), 'delta' -- those the result holds."""
    e, D = _row_terms(r, T, fam)
    E = e + U * (D + math.log2(T)) + fam["lse"] * U * r["lse2"].abs().unsqueeze(-1)
    w = oa.LN2 * E                                   # relative error of P[i, :]
    dsrel = w + (128 + 4 + 4) * U                    # of dS[i, :], in units of A_dS
    n = (T + 4) * U
    s = abs(r["scale"])
    out = {"delta": (128 + 4) * U * r["A_delta"]}
    tr = lambda x: x.transpose(-1, -2)
    if "dq" in r:
        f = (n + dsrel) * r["A_dQ"] + FLOOR * s * (r["G"] @ r["k_dq"].abs())
        if fam is F32:
            out["dq"] = f
        else:
            out["dq"], out["dq2"] = UB * r["A_dQ"] + f, TIER2 * r["R_dQ"] + f
    if "dk" in r:
        fk = n * r["A_dK"] + s * (tr(r["A_dS"] * dsrel) @ r["q_dk"].abs()) + FLOOR * s * (tr(r["G"]) @ r["q_dk"].abs())
        fv = n * r["A_dV"] + tr(r["P"] * (w + 2 * U)) @ r["dO_dv"].abs() + FLOOR * r["dO_dv"].abs().sum(-2, keepdim=True)
        if fam is F32:
            out["dk"], out["dv"] = fk, fv
        else:
            out["dk"], out["dk2"] = UB * r["A_dK"] + fk, TIER2 * r["R_dK"] + fk
            out["dv"], out["dv2"] = UB * r["A_dV"] + fv, TIER2 * r["R_dV"] + fv
    return out


def worst(got, ref, bound):
    """max err / bound over all elements (0 / 0 counts as 0, x / 0 as inf)."""
    err = (got.detach().to("cpu", torch.float64) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max())


# ====================================================================================================== emulation
def _b(x):
    return x.to(torch.bfloat16).float()


FAULTS = ("swap", "scale_row", "drop", "gain", "norescale")


def emulate_fwd(q, k, v, scale, mode="plain", fault=None):
    """The bf16 forward kernels' arithmetic on one image [T, 128] in torch fp32: bf16-rounded operands, fp32 products and
    sums, exp2 in fp32, P rounded to bf16 in front of P.V, 32-key blocks with the running maximum of the plain kernel
    (mode 'plain': attn_fwd_bf16_kernel) or the lazy one of the pipelined kernel (mode 'lazy': threshold 8, decided per
    group of 32 queries, shift max(t, 0) per query).  `fault` plants one defect (FAULTS)."""
    T = q.shape[0]
    c = torch.tensor(oa.c32(scale), dtype=torch.float32)
    qt, kb, vb = _b(q.float() * c), _b(k.float()), _b(v.float()).clone()
    if fault == "swap":                                  # two V rows of key block 1 (block 0 when there is one block) trade places
        j = 32 if T > 32 else 0
        vb[[j + 3, j + 4]] = vb[[j + 4, j + 3]]
    elif fault == "scale_row":
        vb[5] = vb[5] * 1.25
    elif fault == "drop":
        vb[5] = 0.0
    O = torch.zeros(T, C)
    l = torch.zeros(T, 1)
    m = torch.full((T, 1), -math.inf)
    for b in range(T // 32):
        S = qt @ kb[32 * b:32 * b + 32].T
        if mode == "plain":
            m_new = torch.maximum(m, S.amax(-1, keepdim=True))
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(S - m_new)
            l = l * alpha + p.sum(-1, keepdim=True)
            if fault != "norescale":
                O = O * alpha
            m = m_new
        else:
            if b == 0:
                m = S.amax(-1, keepdim=True)
            S = S - m
            t = S.amax(-1, keepdim=True)
            hot = (t > 8.0).reshape(T // 32, 32).any(-1).repeat_interleave(32).unsqueeze(-1)
            shift = torch.where(hot, t.clamp_min(0.0), torch.zeros_like(t))
            a = torch.exp2(-shift)
            m = m + shift
            l = l * a
            S = S - shift
            if fault != "norescale":
                O = O * a
            p = torch.exp2(S)
            l = l + p.sum(-1, keepdim=True)
        O = O + _b(p) @ vb[32 * b:32 * b + 32]
    O = O * (1.0 / l)
    if fault == "gain":
        O = O * (1.0 + 2.0 ** -6)
    lse = (m + torch.log2(l)) * torch.tensor(oa.LN2, dtype=torch.float32)
    return O, lse.squeeze(-1)


def emulate_bwd(q, k, v, o, lse, do, scale, fault=None):
    """The bf16 backward kernels' arithmetic on one image in torch fp32: (dq, dk, dv, delta).  P and dS are rounded to bf16
    in front of the second products; lse * log2 e, delta and the final * scale are fp32."""
    c = torch.tensor(oa.c32(scale), dtype=torch.float32)
    s32 = torch.tensor(scale, dtype=torch.float32)
    q, k, v, o, lse, do = (t.float() for t in (q, k, v, o, lse, do))
    lse2 = (lse * torch.tensor(oa.LOG2E32, dtype=torch.float32)).unsqueeze(-1)
    delta = (do * o).sum(-1, keepdim=True)
    qt, qb, kt, kb, vb, dob = _b(q * c), _b(q), _b(k * c), _b(k), _b(v), _b(do)
    kq, qk, dov = kb.clone(), qb.clone(), dob.clone()          # the operands of the second products
    if fault == "swap":
        kq[[3, 4]] = kq[[4, 3]]; qk[[3, 4]] = qk[[4, 3]]; dov[[3, 4]] = dov[[4, 3]]
    elif fault == "scale_row":
        kq[5] *= 1.25; qk[5] *= 1.25; dov[5] *= 1.25
    elif fault == "drop":
        kq[5] = 0.0; qk[5] = 0.0; dov[5] = 0.0
    dP = dob @ vb.T - delta
    dSq = _b(torch.exp2(qt @ kb.T - lse2) * dP)
    dq = (dSq @ kq) * s32
    P = torch.exp2(qb @ kt.T - lse2)
    dk = (_b(P * dP).T @ qk) * s32
    dv = _b(P).T @ dov
    if fault == "gain":
        dq, dk, dv = (x * (1.0 + 2.0 ** -6) for x in (dq, dk, dv))
    return dq, dk, dv, delta.squeeze(-1)
