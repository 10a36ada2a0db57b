"""fp64 restatements of the fused single-head attention (csrc/attention.hip, csrc/attention_bf16.hip).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  q, k, v, o, do: [..., T, C] tokens, lse, delta: [..., T]; `scale` is the
fp32 value the C ABI receives.  Everything is evaluated in fp64 with plain matmul / exp2 / sum; nothing here calls
torch.softmax or autograd, so that tests/test_oracle_attention.py can pin every function to them independently.

Two kinds of function:

* attention / attention_bwd: the operation itself on the operands as given (the truth the fp32 kernels are compared with).
  attention_bwd takes `o` and `lse` as INPUTS, like pd_attn_bwd, so it is defined for whatever the caller feeds:
      P = exp(scale q k^T - lse),  delta = sum_c do o,  dS = P (do v^T - delta),
      dq = scale dS k,  dk = scale dS^T q,  dv = P^T do.
* fwd_bf16_model / dq_bf16_model / dkv_bf16_model: the same formulas with the operands rounded to bf16 exactly where
  the bf16 kernels round them when they stage them, and with the two fp32 constants the kernels form on the way
  (c32 = fl32(scale * fl32(log2 e)), lse2 = fl32(lse * fl32(log2 e))) formed the same way.  Rounding points, as the source
  stands (csrc/attention_bf16.hip):
      forward (plain :164, pipelined :301)   q~ = bf16(fl32(q * c32))  own_frags :110 -> cvt8 :51-54, c32 from :980 / :983
                                             bf16(k) rows, bf16(v) transposed: attn_pack_multi_kernel :126 -> store_rows :89,
                                             store_transposed :96-99 (jobs :973-974)
      dQ (plain :450-451, pipelined :531-532) q~ as above with c32 = scale * kLog2e formed in the kernel, bf16(dO) (scale 1.f);
                                             bf16(k) rows + transposed, bf16(v) rows (jobs :1025-1026)
      dK / dV (plain :656-657, pipe :774-775) k~ = bf16(fl32(k * c32)), bf16(v) from the wave's own tokens; bf16(q), bf16(dO)
                                             rows + transposed from the packed images (jobs :1027-1028)
      left in fp32                           lse (times fl32(log2 e): :452, :533, :669, :940), delta and dO . O
                                             (attn_delta_bf16_kernel :928-942)
  The three paths see three slightly different score matrices (q~ k, q~ k, q k~), hence three models.  The models do NOT
  round P or dS to bf16 (acc_frag :58-63): that rounding is what the bound of the GPU tests covers.

Every function returns a dict.  Beside the values it holds the magnitudes the comparison rule of
tests/test_attention_gpu.py is built from:
  A_*      the same sums on absolute values:  A_O = sum_j P |v|,  A_dV = sum_i P |dO|,  A_delta = sum_c |dO||O|,
           A_dS = P (sum_c |dO||v| + A_delta),  A_dQ = scale sum_j A_dS |k|,  A_dK = scale sum_i A_dS |q|
  R_*      the root-sum-square of the terms that carry a bf16-rounded factor (P or dS):
           R_O = sqrt(sum_j P^2 v^2)  (P normalised: the 1 / l is inside),  R_dV = sqrt(sum_i P^2 dO^2),
           R_dQ = scale sqrt(sum_j dS^2 k^2),  R_dK = scale sqrt(sum_i dS^2 q^2)
  S2, Sabs the scores in log2 units and the same products on absolute values, sum_c |q~||k~|
  G        sum_c |dO||v| + A_delta  (A_dS without the factor P: the scale of the flush-to-zero floor)
"""
import math

import numpy as np
import torch

F64 = torch.float64
LOG2E = 1.4426950408889634
LOG2E32 = float(np.float32(LOG2E))
LN2 = math.log(2.0)


def _d(t):
    return torch.as_tensor(t).detach().to("cpu", F64)


def bf16(x):
    """Round to bf16 (nearest even) what is already an fp32 value; returned in fp64."""
    return torch.as_tensor(x).detach().to("cpu").float().to(torch.bfloat16).double()


def c32(scale):
    """fl32(scale * fl32(log2 e)): the factor the kernels fold into the operand they pre-scale."""
    return float(np.float32(scale) * np.float32(LOG2E))


def _prescaled32(x, scale):
    """fl32(x * c32) elementwise, fp32 tensor."""
    return torch.as_tensor(x).detach().to("cpu").float() * torch.tensor(c32(scale), dtype=torch.float32)


def lse2_32(lse):
    """fl32(lse * fl32(log2 e)) in fp64: the log-sum-exp in log2 units as the backward kernels form it."""
    return (torch.as_tensor(lse).detach().to("cpu").float() * torch.tensor(LOG2E32, dtype=torch.float32)).double()


def _T(x):
    return x.transpose(-1, -2)


# ------------------------------------------------------------------------------------------------ forward
def _forward(S2, Sabs, v):
    m2 = S2.amax(-1, keepdim=True)
    E = torch.exp2(S2 - m2)
    l = E.sum(-1, keepdim=True)
    P = E / l
    log2l = torch.log2(l)
    return {"O": P @ v, "lse": ((m2 + log2l) * LN2).squeeze(-1), "P": P, "A_O": P @ v.abs(),
            "R_O": torch.sqrt((P * P) @ (v * v)), "S2": S2, "Sabs": Sabs, "vabs_sum": v.abs().sum(-2, keepdim=True),
            "A_lse": ((m2.abs() + log2l.abs()) * LN2).squeeze(-1)}


def attention(q, k, v, scale):
    """O = softmax(scale q k^T) v, lse = logsumexp(scale q k^T), P: the truth on the operands as given."""
    q, k, v = _d(q), _d(k), _d(v)
    c = float(scale) * LOG2E
    return _forward((q @ _T(k)) * c, (q.abs() @ _T(k.abs())) * abs(c), v)


def fwd_bf16_model(q, k, v, scale):
    """The forward on the operands as pd_attn_bf16_fwd stages them: bf16(fl32(q c32)), bf16(k), bf16(v)."""
    qt, kb, vb = bf16(_prescaled32(q, scale)), bf16(k), bf16(v)
    return _forward(qt @ _T(kb), qt.abs() @ _T(kb.abs()), vb)


# ------------------------------------------------------------------------------------------------ backward
def _backward(S2, Sabs, lse2, do_sum, o, dO, v, scale, k_for_dq=None, q_for_dk=None):
    """do_sum: the fp32 dO of the row sums delta = sum_c dO O (never rounded to bf16); dO, v: the operands of dP = dO v^T."""
    out = {"S2": S2, "Sabs": Sabs, "lse2": lse2, "scale": float(scale)}
    P = torch.exp2(S2 - lse2.unsqueeze(-1))
    delta = (do_sum * o).sum(-1)
    A_delta = (do_sum.abs() * o.abs()).sum(-1)
    dP = dO @ _T(v)
    G = dO.abs() @ _T(v.abs()) + A_delta.unsqueeze(-1)
    dS = P * (dP - delta.unsqueeze(-1))
    out.update(P=P, dS=dS, delta=delta, A_delta=A_delta, G=G, A_dS=P * G)
    s = float(scale)
    if k_for_dq is not None:
        kk = k_for_dq
        out.update(dq=s * (dS @ kk), A_dQ=abs(s) * (out["A_dS"] @ kk.abs()), R_dQ=abs(s) * torch.sqrt((dS * dS) @ (kk * kk)),
                   k_dq=kk)
    if q_for_dk is not None:
        qq = q_for_dk
        out.update(dk=s * (_T(dS) @ qq), A_dK=abs(s) * (_T(out["A_dS"]) @ qq.abs()),
                   R_dK=abs(s) * torch.sqrt(_T(dS * dS) @ (qq * qq)), q_dk=qq,
                   dv=_T(P) @ dO, A_dV=_T(P) @ dO.abs(), R_dV=torch.sqrt(_T(P * P) @ (dO * dO)), dO_dv=dO)
    return out


def attention_bwd(q, k, v, o, lse, do, scale):
    """dq, dk, dv, delta of the attention whose forward returned (o, lse): the truth on the operands as given."""
    q, k, v, o, lse, do = _d(q), _d(k), _d(v), _d(o), _d(lse), _d(do)
    c = float(scale) * LOG2E
    return _backward((q @ _T(k)) * c, (q.abs() @ _T(k.abs())) * abs(c), lse * LOG2E, do, o, do, v, scale, k_for_dq=k, q_for_dk=q)


def dq_bf16_model(q, k, v, o, lse, do, scale):
    """dq (and delta) on the operands as the bf16 dQ kernels stage them: bf16(fl32(q c32)), bf16(k), bf16(v), bf16(dO)."""
    qt, kb, vb, dob = bf16(_prescaled32(q, scale)), bf16(k), bf16(v), bf16(do)
    return _backward(qt @ _T(kb), qt.abs() @ _T(kb.abs()), lse2_32(lse), _d(do), _d(o), dob, vb, scale, k_for_dq=kb)


def dkv_bf16_model(q, k, v, o, lse, do, scale):
    """dk, dv (and delta) on the operands as the bf16 dK / dV kernels stage them: bf16(q), bf16(fl32(k c32)), bf16(v), bf16(dO)."""
    qb, kt, vb, dob = bf16(q), bf16(_prescaled32(k, scale)), bf16(v), bf16(do)
    return _backward(qb @ _T(kt), qb.abs() @ _T(kt.abs()), lse2_32(lse), _d(do), _d(o), dob, vb, scale, q_for_dk=qb)
