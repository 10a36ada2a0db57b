"""oracle/glue.py (the fp64 restatements the K3 GPU tests compare the kernels with) pinned to torch.nn.functional and
autograd in fp64 on the CPU: a mistake in a restatement cannot go unnoticed and then excuse the same mistake in a
kernel.  No GPU."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import glue

F64 = torch.float64


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def _grid(g, shape, lo=-256, hi=257):
    return torch.randint(lo, hi, shape, generator=g).to(F64) / 64.0


@pytest.mark.parametrize("shape", [(3, 2, 2, 4), (2, 6, 8, 8), (1, 5, 7, 4), (2, 9, 4, 8)])
def test_chain_matches_batch_norm_relu_pool_dropout_add_relu_autograd(shape):
    """Every flag combination against F.batch_norm(training=True) -> relu -> max_pool2d(2) -> * mask -> + res -> relu and
    its autograd: out, dx, dres, the two sums (as dbeta / dgamma) -- on tie-rich inputs (multiples of 2^-6, many all-zero
    windows), where the first-maximum routing matters."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    for relu_pre, pool, relu_post, has_res, drop in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        x = _grid(g, shape).requires_grad_(True)
        gamma = (torch.tensor([-0.5, 2.0, 1.0, -1.0], dtype=F64).repeat(C // 4)).requires_grad_(True)
        beta = _grid(g, (C,), -32, 33).requires_grad_(True)
        Ho, Wo = (H // 2, W // 2) if pool else (H, W)
        res = _grid(g, (N, Ho, Wo, C)).requires_grad_(True) if has_res else None
        mask = (torch.randint(0, 2, (N, Ho, Wo, C), generator=g).to(F64) * 2.0) if drop else None
        dy = _grid(g, (N, Ho, Wo, C))
        # torch
        z = F.batch_norm(_nchw(x), None, None, gamma, beta, True, 0.0, 1e-5)
        v = F.relu(z) if relu_pre else z
        if pool:
            v = F.max_pool2d(v, 2)
        if drop:
            v = v * _nchw(mask)
        if has_res:
            v = v + _nchw(res)
        out_t = F.relu(v) if relu_post else v
        out_t.backward(_nchw(dy))
        # the kernels' operands: scale / shift / mean / invstd of the batch, as pd_bn_fwd_finalize emits them
        xd = x.detach()
        mean = xd.mean((0, 1, 2))
        invstd = 1.0 / torch.sqrt(xd.var((0, 1, 2), unbiased=False) + 1e-5)
        scale = gamma.detach() * invstd
        shift = beta.detach() - mean * scale
        out, A = glue.chain_fwd(xd, scale, shift, res, relu_pre, pool, mask, relu_post)
        _close(out, _nhwc(out_t.detach()), 1e-11)
        assert (A >= out.abs() - 1e-9).all()
        cnt = N * H * W
        r0 = glue.chain_bwd(dy, xd, out, scale, shift, mean, invstd, torch.zeros(2 * C, dtype=F64), relu_pre, pool, mask,
                            relu_post)
        coef = torch.cat([r0["sum_g"], r0["sum_gx"]]) / cnt
        r = glue.chain_bwd(dy, xd, out, scale, shift, mean, invstd, coef, relu_pre, pool, mask, relu_post)
        _close(r["sum_g"], beta.grad, 1e-10)
        _close(r["sum_gx"], gamma.grad, 1e-10)
        _close(r["dx"], x.grad, 1e-9)
        assert (r["A_dx"] >= r["dx"].abs() - 1e-9).all() and (r["A_sum_gx"] >= r["sum_gx"].abs() - 1e-9).all()
        if has_res and relu_post:
            _close(r["dres"], res.grad, 1e-12)
        if pool and (H % 2 or W % 2):
            assert (r["g"][:, 2 * Ho:, :, :] == 0).all() and (r["g"][:, :, 2 * Wo:, :] == 0).all()
        # eval-mode form: no statistics, dx = g * scale
        re = glue.chain_bwd(dy, xd, out, scale, shift, None, None, None, relu_pre, pool, mask, relu_post)
        _close(re["dx"], r["g"] * scale)
        assert re["sum_g"] is None


def test_chain_identity_scale_is_the_plain_chain():
    g = torch.Generator().manual_seed(5)
    x, res = _grid(g, (2, 4, 6, 4)), _grid(g, (2, 2, 3, 4))
    out, _ = glue.chain_fwd(x, None, None, res, 0, 1, None, 1)
    _close(out, _nhwc(F.relu(F.max_pool2d(_nchw(x), 2) + _nchw(res))))


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 2, 3, 4), (1, 5, 7, 4), (2, 8, 8, 4), (1, 9, 6, 4)])
def test_maxpool3s2_matches_max_pool2d_with_indices(shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(H * 16 + W)
    for x in (torch.randint(0, 3, shape, generator=g).to(F64) * torch.randint(0, 2, shape, generator=g).to(F64),
              torch.full(shape, -1.0, dtype=F64)):
        xr = _nchw(x).clone().requires_grad_(True)
        y_t, ind = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
        y, idx = glue.maxpool3s2(x)
        _close(y, _nhwc(y_t.detach()), 0.0)
        # torch's flat input index -> window position
        Ho, Wo = y.shape[1], y.shape[2]
        ho = torch.arange(Ho).view(1, 1, Ho, 1)
        wo = torch.arange(Wo).view(1, 1, 1, Wo)
        pos = (ind // W - (2 * ho - 1)) * 3 + (ind % W - (2 * wo - 1))
        assert torch.equal(_nhwc(pos), idx.to(torch.int64))
        dy = _grid(g, y.shape)
        add = _grid(g, shape)
        y_t.backward(_nchw(dy))
        dx, A = glue.maxpool3s2_bwd(idx, dy, H, W)
        _close(dx, _nhwc(xr.grad), 0.0)
        dx2, _ = glue.maxpool3s2_bwd(idx, dy, H, W, add)
        _close(dx2, dx + add, 0.0)
        assert (A >= dx.abs()).all()


@pytest.mark.parametrize("align", [False, True])
def test_bilinear_x2_matches_interpolate_and_its_autograd(align):
    g = torch.Generator().manual_seed(11)
    shapes = [(1, h, w, 2) for h in range(1, 12) for w in (1, 2, 5)] + [(2, 3, 5, 4), (1, 33, 7, 2)]
    for shape in shapes:
        a = torch.randn(shape, generator=g, dtype=F64)
        ar = _nchw(a).clone().requires_grad_(True)
        up_t = F.interpolate(ar, scale_factor=2, mode="bilinear", align_corners=align)
        go = torch.randn(up_t.shape, generator=g, dtype=F64)
        up_t.backward(go)
        if align:
            up, A = glue.up2x_ac(a)
            da, Ab = glue.up2x_ac_bwd(_nhwc(go))
        else:
            skip = torch.randn(shape[0], 2 * shape[1], 2 * shape[2], 3, generator=g, dtype=F64)
            cat, A = glue.upcat(a, skip)
            assert torch.equal(cat[..., shape[3]:], skip)
            up, A = cat[..., :shape[3]], A[..., :shape[3]]
            da, Ab = glue.up_bwd(_nhwc(go))
        _close(up, _nhwc(up_t.detach()), 1e-12)
        _close(da, _nhwc(ar.grad), 1e-12)
        assert (A >= up.abs() - 1e-12).all() and (Ab >= da.abs() - 1e-12).all()


def test_align_corners_rows_that_read_an_input_row_lie_within_two_of_twice_its_index():
    """Output row o reads input row h only for 2h - 2 <= o <= 2h + 2 (exact arithmetic, every H): the +-3 gather window of
    up2x_ac_bwd_kernel has one row of margin, and a window of +-2 would compute the same gradient -- only +-1 loses terms."""
    for H in range(1, 130):
        o, h = torch.nonzero(glue._interp_matrix(H, True), as_tuple=True)
        assert int((o - 2 * h).abs().max()) <= 2
        if H > 2:
            assert int((o - 2 * h).max()) == 2          # ... and row 2h + 2 is needed
        T = glue._tap_matrix(H)
        assert bool((T[o, h] == 1).all())                # the reach of a perturbed source index covers every exact tap


def test_up_bwd_with_the_elu_derivative():
    g = torch.Generator().manual_seed(12)
    z = torch.randn(2, 3, 5, 4, generator=g, dtype=F64)
    z[0, 0, 0, 0] = 0.0
    zr = _nchw(z).clone().requires_grad_(True)
    y = F.elu(zr)
    up = F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=False)
    go = torch.randn(up.shape, generator=g, dtype=F64)
    up.backward(go)
    da, _ = glue.up_bwd(_nhwc(go), _nhwc(y.detach()))
    _close(da, _nhwc(zr.grad), 1e-12)


def test_bn_finalize_matches_batch_norm_module():
    g = torch.Generator().manual_seed(13)
    N, H, W, C = 3, 4, 5, 6
    x = torch.randn(N, H, W, C, generator=g, dtype=F64) * 2 + 1
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g, dtype=F64))
        bn.bias.copy_(torch.randn(C, generator=g, dtype=F64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=F64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    # partial rows as a conv epilogue would emit them: two rows of per-tile sums
    flat = x.reshape(-1, C)
    part = torch.stack([torch.stack([t.sum(0), (t * t).sum(0)], -1) for t in (flat[:17], flat[17:])])
    r = glue.bn_finalize_fwd(part, float(N * H * W), bn.weight, bn.bias, rm0, rv0, 0.1, bn.eps, True)
    xr = _nchw(x).clone().requires_grad_(True)
    y = bn(xr)
    _close(_nhwc(y.detach()), x * r["scale"] + r["shift"], 1e-11)
    _close(r["running_mean"], bn.running_mean, 1e-12)
    _close(r["running_var"], bn.running_var, 1e-12)
    go = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(go)
    gh = _nhwc(go)
    xhat = (x - r["mean"]) * r["invstd"]
    bpart = torch.stack([gh.sum((0, 1, 2)), (gh * xhat).sum((0, 1, 2))], -1)[None]
    dg, db, coef = glue.bn_finalize_bwd(bpart, float(N * H * W))
    _close(dg, bn.weight.grad, 1e-11)
    _close(db, bn.bias.grad, 1e-11)
    dg2, db2, _ = glue.bn_finalize_bwd(bpart, float(N * H * W), torch.ones(C), torch.ones(C), True)
    _close(dg2, dg + 1)
    _close(db2, db + 1)
    dx = glue.chain_bwd(gh, x, None, r["scale"], r["shift"], r["mean"], r["invstd"], coef, 0, 0, None, 0)["dx"]
    _close(dx, _nhwc(xr.grad), 1e-10)
    # eval mode: coefficients of the running statistics, which stay as they are
    bn.eval()
    e = glue.bn_finalize_fwd(None, 1.0, bn.weight, bn.bias, bn.running_mean, bn.running_var, 0.1, bn.eps, False)
    _close(_nhwc(bn(_nchw(x)).detach()), x * e["scale"] + e["shift"], 1e-11)
    assert torch.equal(e["running_mean"], bn.running_mean.detach()) and torch.equal(e["running_var"], bn.running_var.detach())


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_matches_torch_optim_adam_over_several_steps(wd):
    g = torch.Generator().manual_seed(14)
    p0 = torch.randn(37, generator=g, dtype=F64)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(37, dtype=F64), torch.zeros(37, dtype=F64)
    for step in range(1, 6):
        grad = torch.randn(37, generator=g, dtype=F64)
        pt.grad = grad.clone() * 0.125            # the gradient Adam sees = grad_scale * the accumulated one
        opt.step()
        r = glue.adam_step(p, grad, m, v, 1e-3, 0.9, 0.999, 1e-8, wd, step, 0.125)
        p, m, v = r["p"], r["m"], r["v"]
        _close(p, pt.detach(), 1e-12)
        assert (r["A_m"] >= m.abs() - 1e-15).all() and (r["A_update"] >= r["update"].abs() - 1e-15).all()
    st = opt.state[pt]
    _close(m, st["exp_avg"], 1e-13)
    _close(v, st["exp_avg_sq"], 1e-13)


def test_softmax_act_relu_add():
    g = torch.Generator().manual_seed(15)
    x = torch.randn(3, 9, generator=g, dtype=F64) * 40
    xr = x.clone().requires_grad_(True)
    p_t = F.softmax(0.5 * xr, -1)
    dp = torch.randn(3, 9, generator=g, dtype=F64)
    p_t.backward(dp)
    p = glue.softmax_rows(x, 0.5)
    _close(p, p_t.detach(), 1e-14)
    ds, A = glue.softmax_rows_bwd(p, dp, 0.5)
    _close(ds, xr.grad, 1e-14)
    assert (A >= ds.abs()).all()
    z = torch.randn(50, generator=g, dtype=F64)
    z[:3] = 0.0
    for act, f in ((1, F.relu), (2, F.elu), (3, torch.sigmoid)):
        zr = z.clone().requires_grad_(True)
        y = f(zr)
        go = torch.randn(50, generator=g, dtype=F64)
        y.backward(go)
        _close(glue.act_bwd(go, y.detach(), act), zr.grad, 1e-14)
    a, b = torch.randn(8, generator=g, dtype=F64), torch.randn(8, generator=g, dtype=F64)
    assert torch.equal(glue.relu_add(a, b, 1), F.relu(a) + b) and torch.equal(glue.relu_add(a, None, 0), a)
    assert torch.equal(glue.relu_add(a, b, 0), a + b) and torch.equal(glue.relu_add(a, None, 1), F.relu(a))


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_reflect_fold_matches_reflection_pad_autograd(pad):
    g = torch.Generator().manual_seed(16 + pad)
    for H, W in ((pad + 1, pad + 1), (5, 9), (pad + 1, 7)):
        x = torch.zeros(2, 3, H, W, dtype=F64, requires_grad=True)
        xp = F.pad(x, (pad,) * 4, mode="reflect")
        go = _grid(g, tuple(xp.shape))
        xp.backward(go)
        dx, A = glue.reflect_fold(_nhwc(go), pad)
        _close(dx, _nhwc(x.grad), 0.0)
        assert (A >= dx.abs()).all()
