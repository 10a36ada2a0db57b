"""fp64 restatements of the K3 glue kernels (csrc/elementwise.hip), one function per operation.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Each function follows the contract of its C entry point in
include/polardepth.h and takes the same operands: NHWC tensors, the fp32 coefficient vectors as given (promoted to
fp64, never recomputed), and an explicit dropout mask (already scaled by 1/(1-p), on the OUTPUT grid) instead of a
Philox seed.  Everything is evaluated in fp64 with plain torch indexing; nothing here calls torch.nn.functional, so
that tests/test_oracle_glue.py can pin every function to torch.nn.functional / autograd independently.

Where an operation sums terms, the function also returns ``A``: the same formula evaluated on the absolute values of
its terms.  ``A`` is the scale of the rounding-error bound the GPU tests use: |got - ref| <= (n + 4) * 2^-24 * A for a
sum of n fp32 products.
"""
import math

import torch

F64 = torch.float64


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", F64)


# ------------------------------------------------------------------------------------------------ BN-apply chain
def _affine(x, scale, shift):
    return x if scale is None else x * scale + shift


def _windows(z, Ho, Wo):
    """The four members of every 2x2 window in scan order: [4][N,Ho,Wo,C] (a trailing odd row / column is dropped)."""
    return [z[:, dh:2 * Ho:2, dw:2 * Wo:2, :] for dh in (0, 1) for dw in (0, 1)]


def chain_fwd(x, scale, shift, res, relu_pre, pool, mask, relu_post):
    """out = relu_post(dropout(pool2x2(relu_pre(x * scale + shift))) + res), (out, A).  scale None = identity; mask None
    = no dropout."""
    x, scale, shift, res, mask = _d(x), _d(scale), _d(shift), _d(res), _d(mask)
    z = _affine(x, scale, shift)
    za = x.abs() if scale is None else x.abs() * scale.abs() + shift.abs()
    if relu_pre:
        z = z.clamp_min(0.0)
    if pool:
        Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
        v = _windows(z, Ho, Wo)
        va = _windows(za, Ho, Wo)
        z = torch.maximum(torch.maximum(v[0], v[1]), torch.maximum(v[2], v[3]))
        za = torch.maximum(torch.maximum(va[0], va[1]), torch.maximum(va[2], va[3]))
    if mask is not None:
        z, za = z * mask, za * mask
    if res is not None:
        z, za = z + res, za + res.abs()
    if relu_post:
        z = z.clamp_min(0.0)
    return z, za


def chain_bwd(dy, x, out, scale, shift, mean, invstd, coef, relu_pre, pool, mask, relu_post):
    """The two-pass backward of chain_fwd.  Returns a dict:
      g        dL/dz on the INPUT grid (z = x * scale + shift): dy gated by the post-add ReLU through `out`, times the
               dropout mask, routed to the first maximum of its 2x2 window in scan order, gated by the pre-ReLU; zero on
               a dropped odd row / column;
      sum_g, sum_gx, A_sum_g, A_sum_gx   per-channel sums of g and g * xhat, xhat = (x - mean) * invstd (None without
               mean);
      dx, A_dx scale * (g - c1 - xhat * c2) for the GIVEN coef = [c1 | c2], or g * scale when mean is None;
      dres     dy * (out > 0) (None without relu_post)."""
    dy, x, out, scale, shift, mean, invstd, coef, mask = (_d(t) for t in (dy, x, out, scale, shift, mean, invstd, coef, mask))
    N, H, W, C = x.shape
    gy = dy
    dres = None
    if relu_post:
        gy = gy * (out > 0).to(F64)
        dres = gy
    if mask is not None:
        gy = gy * mask
    z = _affine(x, scale, shift)
    if pool:
        Ho, Wo = H // 2, W // 2
        v = _windows(z.clamp_min(0.0) if relu_pre else z, Ho, Wo)
        best, arg = v[0].clone(), torch.zeros_like(v[0], dtype=torch.int64)
        for j in (1, 2, 3):                                 # strict >: the first maximum in scan order keeps the gradient
            up = v[j] > best
            best = torch.where(up, v[j], best)
            arg = torch.where(up, torch.full_like(arg, j), arg)
        g = torch.zeros_like(x)
        for j in range(4):
            g[:, (j >> 1):2 * Ho:2, (j & 1):2 * Wo:2, :] = gy * (arg == j).to(F64)
    else:
        g = gy.clone()
    if relu_pre:
        g = g * (z > 0).to(F64)
    r = {"g": g, "dres": dres, "sum_g": None, "sum_gx": None, "A_sum_g": None, "A_sum_gx": None}
    one = torch.ones(C, dtype=F64) if scale is None else scale
    if mean is not None:
        xhat = (x - mean) * invstd
        xhat_a = (x.abs() + mean.abs()) * invstd.abs()
        r["sum_g"], r["A_sum_g"] = g.sum((0, 1, 2)), g.abs().sum((0, 1, 2))
        r["sum_gx"], r["A_sum_gx"] = (g * xhat).sum((0, 1, 2)), (g.abs() * xhat_a).sum((0, 1, 2))
        c1, c2 = coef[:C], coef[C:]
        r["dx"] = one * (g - c1 - xhat * c2)
        r["A_dx"] = one.abs() * (g.abs() + c1.abs() + xhat_a * c2.abs())
    else:
        r["dx"] = g * one
        r["A_dx"] = (g * one).abs()
    return r


# ------------------------------------------------------------------------------------------------ 3x3 / stride 2 / pad 1 max-pool
def maxpool3s2(x):
    """(y, idx): idx = window position dh * 3 + dw of the first in-bounds maximum in scan order."""
    x = _d(x)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((N, H + 2, W + 2, C), -math.inf, dtype=F64)
    xp[:, 1:H + 1, 1:W + 1, :] = x
    y = torch.full((N, Ho, Wo, C), -math.inf, dtype=F64)
    idx = torch.zeros((N, Ho, Wo, C), dtype=torch.int64)
    for dh in range(3):
        for dw in range(3):
            t = xp[:, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2, :]
            up = t > y
            y = torch.where(up, t, y)
            idx = torch.where(up, torch.full_like(idx, dh * 3 + dw), idx)
    return y, idx.to(torch.uint8)


def maxpool3s2_bwd(idx, dy, H, W, addend=None):
    """(dx, A): every dy goes to the input pixel its idx names; addend (shape of dx) is summed on top."""
    dy, addend = _d(dy), _d(addend)
    idx = torch.as_tensor(idx).to("cpu", torch.int64)
    N, Ho, Wo, C = dy.shape
    dxp = torch.zeros((N, H + 2, W + 2, C), dtype=F64)
    dxa = torch.zeros_like(dxp)
    for dh in range(3):
        for dw in range(3):
            sel = (idx == dh * 3 + dw).to(F64)
            dxp[:, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2, :] += dy * sel
            dxa[:, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2, :] += dy.abs() * sel
    dx, A = dxp[:, 1:H + 1, 1:W + 1, :].clone(), dxa[:, 1:H + 1, 1:W + 1, :].clone()
    if addend is not None:
        dx, A = dx + addend, A + addend.abs()
    return dx, A


# ------------------------------------------------------------------------------------------------ bilinear x2
def _interp_matrix(n_in, align_corners):
    """[2 n_in, n_in] fp64 weights of 1-D linear interpolation by 2, torch's source-index rules."""
    n_out = 2 * n_in
    M = torch.zeros((n_out, n_in), dtype=F64)
    for o in range(n_out):
        if align_corners:
            src = (o * (n_in - 1)) / (n_out - 1) if n_out > 1 else 0.0
        else:
            src = max(0.5 * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = src - i0
        M[o, i0] += 1.0 - l1
        M[o, i1] += l1
    return M


def _up(a, align_corners):
    My, Mx = _interp_matrix(a.shape[1], align_corners), _interp_matrix(a.shape[2], align_corners)
    return torch.einsum("yh,nhwc,xw->nyxc", My, a, Mx)


def _up_t(g, align_corners):
    My, Mx = _interp_matrix(g.shape[1] // 2, align_corners), _interp_matrix(g.shape[2] // 2, align_corners)
    return torch.einsum("yh,nyxc,xw->nhwc", My, g, Mx)


def upcat(a, skip=None):
    """(out, A): out[..., :Ca] = bilinear x2 of a (align_corners=False), out[..., Ca:] = skip."""
    a, skip = _d(a), _d(skip)
    up, upa = _up(a, False), _up(a.abs(), False)
    if skip is None or skip.shape[-1] == 0:
        return up, upa
    return torch.cat([up, skip], -1), torch.cat([upa, skip.abs()], -1)


def up_bwd(dout, elu_y=None):
    """(da, A): gradient of the upsampled part; dout holds exactly the Ca channels of it.  elu_y: da is multiplied by
    ELU'(.) through the ELU output, (y > 0 ? 1 : y + 1)."""
    dout, elu_y = _d(dout), _d(elu_y)
    da, A = _up_t(dout, False), _up_t(dout.abs(), False)
    if elu_y is not None:
        f = torch.where(elu_y > 0, torch.ones_like(elu_y), elu_y + 1.0)
        da, A = da * f, A * f.abs()
    return da, A


def up2x_ac(a):
    a = _d(a)
    return _up(a, True), _up(a.abs(), True)


def up2x_ac_bwd(dout):
    dout = _d(dout)
    return _up_t(dout, True), _up_t(dout.abs(), True)


def _tap_matrix(n_in):
    """[2 n_in, n_in]: 1 where input index i is within one of the exact first tap of output o (align_corners=True): every
    input an evaluation of the source index in lower precision can touch."""
    n_out = 2 * n_in
    T = torch.zeros((n_out, n_in), dtype=F64)
    for o in range(n_out):
        i0 = (o * (n_in - 1)) // (n_out - 1) if n_out > 1 else 0
        T[o, max(i0 - 1, 0):min(i0 + 2, n_in)] = 1.0
    return T


def up2x_ac_reach(a):
    """B [N,2H,2W,C]: sum of |a| over the 3x3 input neighbourhood of every output's first tap -- the scale of the error that
    a perturbed source index (interpolation weights off by eps) causes in up2x_ac: at most eps * B."""
    a = _d(a)
    return torch.einsum("yh,nhwc,xw->nyxc", _tap_matrix(a.shape[1]), a.abs(), _tap_matrix(a.shape[2]))


def up2x_ac_bwd_reach(dout):
    """The same for the gradient: sum of |dout| over every output whose neighbourhood holds the input pixel."""
    dout = _d(dout)
    return torch.einsum("yh,nyxc,xw->nhwc", _tap_matrix(dout.shape[1] // 2), dout.abs(), _tap_matrix(dout.shape[2] // 2))


# ------------------------------------------------------------------------------------------------ BatchNorm finalize
def bn_finalize_fwd(partial, count, gamma, beta, running_mean, running_var, momentum, eps, training=True):
    """partial [R][C][2] (sum, sum of squares).  Returns dict(scale, shift, mean, invstd, running_mean, running_var):
    torch.nn.BatchNorm2d semantics (biased variance for the normalisation, unbiased for the running estimate)."""
    partial, gamma, beta, rm, rv = _d(partial), _d(gamma), _d(beta), _d(running_mean), _d(running_var)
    if training:
        s = partial.sum(0)
        mean = s[:, 0] / count
        var = (s[:, 1] / count - mean * mean).clamp_min(0.0)
        invstd = 1.0 / torch.sqrt(var + eps)
        if rm is not None:
            unbiased = var * count / (count - 1.0) if count > 1 else var
            rm = (1.0 - momentum) * rm + momentum * mean
            rv = (1.0 - momentum) * rv + momentum * unbiased
    else:
        mean, invstd = rm, 1.0 / torch.sqrt(rv + eps)
    g = torch.ones_like(mean) if gamma is None else gamma
    b = torch.zeros_like(mean) if beta is None else beta
    scale = g * invstd
    return {"scale": scale, "shift": b - mean * scale, "mean": mean, "invstd": invstd, "running_mean": rm, "running_var": rv}


def bn_finalize_bwd(partial, count, dgamma=None, dbeta=None, accumulate=False):
    """partial [R][C][2] (sum g, sum g * xhat) -> (dgamma, dbeta, coef = [mean g | mean g * xhat])."""
    s = _d(partial).sum(0)
    dg, db = s[:, 1].clone(), s[:, 0].clone()
    if accumulate:
        dg, db = dg + _d(dgamma), db + _d(dbeta)
    return dg, db, torch.cat([s[:, 0], s[:, 1]]) / count


# ------------------------------------------------------------------------------------------------ Adam
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """torch.optim.Adam (L2 weight decay added to the gradient; the gradient pre-multiplied by grad_scale).
    Returns dict(p, m, v, update, A_m, A_v, A_update)."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    gr = g * grad_scale + weight_decay * p
    gr_a = (g * grad_scale).abs() + (weight_decay * p).abs()
    m2 = beta1 * m + (1.0 - beta1) * gr
    A_m = (beta1 * m).abs() + abs(1.0 - beta1) * gr_a
    v2 = beta2 * v + (1.0 - beta2) * gr * gr
    A_v = (beta2 * v).abs() + abs(1.0 - beta2) * gr_a * gr_a
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    den = torch.sqrt(v2) / math.sqrt(bc2) + eps
    update = (lr / bc1) * (m2 / den)
    return {"p": p - update, "m": m2, "v": v2, "update": update, "A_m": A_m, "A_v": A_v,
            "A_update": abs(lr / bc1) * (A_m / den)}


# ------------------------------------------------------------------------------------------------ small ones
def softmax_rows(x, scale):
    z = _d(x) * scale
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_rows_bwd(p, dp, scale):
    """(ds, A): ds = scale * p * (dp - sum_j dp_j p_j)."""
    p, dp = _d(p), _d(dp)
    s = (p * dp).sum(-1, keepdim=True)
    sa = (p * dp).abs().sum(-1, keepdim=True)
    return scale * p * (dp - s), abs(scale) * p.abs() * (dp.abs() + sa)


def act_bwd(dy, y, act):
    """dz = dy * f'(.) through the activation OUTPUT y: act 1 ReLU, 2 ELU(alpha=1), 3 sigmoid."""
    dy, y = _d(dy), _d(y)
    if act == 1:
        return dy * (y > 0).to(F64)
    if act == 2:
        return torch.where(y > 0, dy, dy * (y + 1.0))
    if act == 3:
        return dy * y * (1.0 - y)
    raise ValueError(act)


def relu_add(x, res, relu):
    x, res = _d(x), _d(res)
    v = x.clamp_min(0.0) if relu else x
    return v if res is None else v + res


def reflect_fold(dxp, pad):
    """(dx, A): gradient of ReflectionPad2d(pad), dxp [N,H+2p,W+2p,C] -> dx [N,H,W,C]: every padded row / column is
    added to the row / column it mirrors."""
    dxp = _d(dxp)
    N, Hp, Wp, C = dxp.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad

    def src(n, size):
        i = torch.arange(size + 2 * pad) - pad
        i = i.abs()
        return torch.where(i >= size, 2 * (size - 1) - i, i)

    out = []
    for t in (dxp, dxp.abs()):
        rows = torch.zeros((N, H, Wp, C), dtype=F64).index_add_(1, src(Hp, H), t)
        out.append(torch.zeros((N, H, W, C), dtype=F64).index_add_(2, src(Wp, W), rows))
    return out[0], out[1]
