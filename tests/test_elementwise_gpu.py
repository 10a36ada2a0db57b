"""The K3 glue kernels (csrc/elementwise.hip) called through the C ABI, one by one, against the fp64 restatements of
oracle/glue.py (which tests/test_oracle_glue.py pins to torch.nn.functional / autograd on the CPU).

Comparison rule
---------------
u = 2^-24 (unit roundoff of fp32, round to nearest).  An output that is a sum of n terms with fp32 products must satisfy

    |got - ref64| <= (n + 4) * u * A        elementwise, 100 % of the elements, nothing masked out,

where ref64 is the fp64 oracle on the SAME fp32 operands and A is the oracle's own formula evaluated on the absolute
values of its terms.  (n - 1) u A is the first-order bound of a sum of n terms in any order, one more u A covers the
rounding of each product, and the remaining + 4 the roundings of the weights (bilinear weights, 1 - l1, wy * wx, the ELU
factor).  The library is built with -ffp-contract=off, so there is no hidden FMA on the device and the bound counts every
rounding.  Where a case is pure selection / copy, or is built on exactly representable arithmetic, the requirement is
torch.equal with the fp64 result rounded to fp32.

Exact inputs: the chain and pooling cases draw x, shift, res, dy (and the BatchNorm mean) from multiples of 2^-6 in
[-4, 4] and scale from {+-0.25, +-0.5, +-1, +-2} (channel 0 always negative, about half of the others), so z = x * scale
+ shift is exact in fp32 and in fp64: ReLU gates and arg-max decisions are identical on both sides although ties are
frequent (with relu_pre many 2x2 windows are all zero).  Dropout p = 0.5 has the exact scale 2; p = 0.25 scales by
fl(4/3), one more rounding, and uses the bound.

n per kernel
  pd_chain_fwd                exact (p in {0, 0.5}); n = 2 for p = 0.25 (v * mask + res)
  pd_chain_bwd_reduce         n = N*H*W per channel (sum of the partial rows in fp64; valid for any summation order)
  pd_chain_bwd_apply          n = 3 (g - c1 - xhat * c2), + 1 for p = 0.25 (g = dy * mask is rounded); mean == NULL: g * scale
                              is exact for p in {0, 0.5}, n = 1 otherwise; dres exact
  pd_maxpool3s2_*             exact (selection; sums of at most four multiples of 2^-6, + the addend)
  pd_upcat_fwd                n = 4; the skip channels exact
  pd_up_bwd / _elu            n = 16
  pd_up2x_ac_fwd / _bwd       n = 4 / n = 25, plus a term for the source index.  The kernel evaluates src = fl(fl((H-1)/(2H-1)) * o)
                              in fp32 (like torch's area_pixel_compute_source_index for float tensors); the oracle uses the
                              exact rational.  Two roundings: |src_f - src| <= 2 u src <= 2 u (H - 1) ABSOLUTE, and the weight
                              l1 = src - floor(src) inherits it: at H = 33 that is 64 u, which no n in (n + 4) u A covers (A is
                              weighted by l0, l1 and says nothing about the difference of the two taps).  The bilinear
                              interpolant is continuous and piecewise linear in src, also across a tap switch, so the value
                              moves by at most eps_y * |row difference| + eps_x * |column difference| with eps_y = 2 u (H - 1),
                              eps_x = 2 u (W - 1); both differences are bounded by B = the sum of |a| over the 3x3
                              neighbourhood of the exact first tap (oracle: up2x_ac_reach).  Bound:
                              (n + 4) u A + 2 u ((H - 1) + (W - 1)) B, and the transposed statement for the gradient
                              (up2x_ac_bwd_reach).  Derived from the arithmetic above, not fitted.
  pd_bn_*_finalize            fp64 sums rounded once: the rtol / atol of the existing large-R test (test_prodsize_gpu.py)
  pd_adam_step                m within 4 u, p within 2 u |p| + 8 u |update|, v within 4 u without weight decay and 7 u with it.
                              "Relative" is taken against the oracle's A (A_m = |beta1 m| + |1 - beta1| A_gr with A_gr = |g grad_scale|
                              + |wd p|, A_v = |beta2 v| + |1 - beta2| A_gr^2, A_update likewise): it IS |m|, v, |update| whenever the
                              terms do not cancel, and no fp32 evaluation can be 4 u-relative to a result that has cancelled (the
                              inputs have mixed signs so that a sign error in the weight decay would show).
                              Derivation (first order; 1 - beta is exact in fp32 by Sterbenz): gr = fl(fl(g gs) + fl(wd p)) is off by
                              e_gr A_gr, e_gr <= 2 u, and e_gr = 0 when wd = 0 and gs is a power of two (the cases here).
                                m = fl(fl(b1 m) + fl((1-b1) gr)):      u |b1 m| + (e_gr + u) (1-b1) A_gr + u |m|          <= 4 u A_m
                                v = fl(fl(b2 v) + fl(fl((1-b2) gr) gr)): u |b2 v| + (2 e_gr + 2 u) (1-b2) A_gr^2 + u v   <= 3 u A_v (wd = 0)
                                                                                                                         <= 7 u A_v (wd > 0)
                              The 4 u the issue names for v is therefore not a property of this operation order once the weight
                              decay rounds gr, which v squares: n re-derived as the rule above asks, not fitted -- 7 is the worst
                              case of the arithmetic, 4 stays wherever the arithmetic supports it.
  pd_softmax_rows_fwd         relative u * (2 max|scale x| + ceil(L/256) + 16), plus the absolute floor 2^-126 (the smallest normal
                              fp32: e^-160 of the +-80 row is not representable, so no relative statement is possible below
                              it); rows sum to 1 within (L/256 + 16) u
  pd_softmax_rows_bwd         n = L, plus the same floor 2^-126: the +-80 row has probabilities down to the subnormal range, whose
                              products underflow in fp32
  pd_act_bwd                  n = 1 (ReLU exact);  pd_relu_add, pd_reflect_fold_pad exact (multiples of 2^-6)

Dropout: the mask of a site is recovered from pd_chain_fwd itself (scale NULL, x = 1, no ReLU, no residual, same pool, seed,
offset, step_state) and handed to the oracle; forward with real data and all three backward index expressions (even-grid window
branch, odd-grid / unpooled chain_grad) must then reproduce the oracle with that SAME mask.
"""
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import glue

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64 = torch.float64
SENT = -77.25            # sentinel in the padding of strided buffers and behind the end of flat ones
EINVAL = -22


def _L():
    from polardepth._lib import lib, check, ptr, stream_ptr
    return lib, check, ptr, stream_ptr


def _dev(t):
    return torch.as_tensor(t).to(torch.float32).to("cuda").contiguous()


def _wide(t, pad):
    """Device fp32 copy of NHWC `t` inside a buffer whose rows are `pad` floats longer (sentinel in the padding): (buf, ld)."""
    t = torch.as_tensor(t)
    C = t.shape[-1]
    buf = torch.full(tuple(t.shape[:-1]) + (C + pad,), SENT, dtype=torch.float32, device="cuda")
    buf[..., :C] = t.to(torch.float32).to("cuda")
    return buf, C + pad


def _cpu64(t):
    return t.detach().to("cpu", F64)


def _within(got, ref, A, n, what, extra=None):
    """The comparison rule: |got - ref64| <= (n + 4) u A elementwise (+ extra, where the module docstring derives one)."""
    got, ref, A = _cpu64(got), _cpu64(ref), _cpu64(A)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bound = (n + 4) * U * A
    if extra is not None:
        bound = bound + extra
    if not (err <= bound).all():
        excess = err - bound
        k = int(excess.argmax())
        raise AssertionError(f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond (n+4) u A, n = {n}; worst at flat "
                             f"index {k}: got {got.flatten()[k].item()!r} ref {ref.flatten()[k].item()!r} "
                             f"err {err.flatten()[k].item():.3e} bound {bound.flatten()[k].item():.3e}")


def _exact(got, ref, what):
    got, ref = got.detach().cpu(), _cpu64(ref).to(torch.float32)
    assert got.shape == ref.shape, f"{what}: shape"
    if not torch.equal(got, ref):
        bad = got != ref
        k = int(bad.flatten().to(torch.int64).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at flat index {k}: "
                             f"got {got.flatten()[k].item()!r} ref {ref.flatten()[k].item()!r}")


def _grid(g, shape, lo=-256, hi=257):
    """Multiples of 2^-6 in [-4, 4] (fp64)."""
    return torch.randint(lo, hi, tuple(shape), generator=g).to(F64) / 64.0


def _scales(g, C):
    s = torch.tensor([0.25, 0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 4, (C,), generator=g)]
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).to(F64)
    sign[0] = -1.0
    if C >= 8:
        sign[1] = 1.0
    return s * sign


# ====================================================================================================== chain
def _chain_fwd(x, scale, shift, res, ld_res, out, ld_out, shape, relu_pre, pool, p, seed, offset, state, relu_post):
    lib, check, ptr, sp = _L()
    N, H, W, C = shape
    check(lib.pd_chain_fwd(ptr(x), ptr(scale), ptr(shift), ptr(res), ptr(out), N, H, W, C, ld_res, ld_out, int(relu_pre),
                           int(pool), float(p), seed, offset, ptr(state), int(relu_post), sp()), "pd_chain_fwd")


def _mask(shape, pool, p, seed, offset, state=None):
    """The dropout mask (times 1/(1-p)) of a site on the output grid, recovered from the forward kernel: fp64 on the CPU."""
    N, H, W, C = shape
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    ones = torch.ones(shape, dtype=torch.float32, device="cuda")
    out = torch.full((N, Ho, Wo, C), SENT, dtype=torch.float32, device="cuda")
    _chain_fwd(ones, None, None, None, 0, out, C, shape, 0, pool, p, seed, offset, state, 0)
    torch.cuda.synchronize()
    m = _cpu64(out)
    keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    assert ((m == 0) | (m == keep)).all(), "mask values other than 0 and 1/(1-p)"
    return m


def _chain_case(shape, relu_pre, pool, relu_post, has_res, p, pad=0, scale_null=False, mean_null=False, fwd=True, bwd=True,
                seed=0x1234ABCD5678, offset=3, rng_seed=0):
    """One configuration of the chain through forward, reduce and apply against the oracle (see the module docstring)."""
    lib, check, ptr, sp = _L()
    N, H, W, C = shape
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    what = f"chain {shape} relu_pre={relu_pre} pool={pool} relu_post={relu_post} res={has_res} p={p} pad={pad}"
    g = torch.Generator().manual_seed(1000 * rng_seed + N * H * W + C + 2 * relu_pre + 4 * pool + 8 * relu_post + 16 * has_res)
    x = _grid(g, shape)
    scale, shift = (None, None) if scale_null else (_scales(g, C), _grid(g, (C,)))
    res = _grid(g, (N, Ho, Wo, C)) if has_res else None
    mask = _mask(shape, pool, p, seed, offset) if p > 0 else None
    exact_p = p in (0.0, 0.5)
    xd, sd, bd = _dev(x), (None if scale_null else _dev(scale)), (None if scale_null else _dev(shift))
    resd, ld_res = _wide(res, pad) if has_res else (None, 0)
    outd, ld_out = _wide(torch.full((N, Ho, Wo, C), SENT, dtype=F64), pad)
    ref_out, A_out = glue.chain_fwd(x, scale, shift, res, relu_pre, pool, mask, relu_post)
    _chain_fwd(xd, sd, bd, resd, ld_res, outd, ld_out, shape, relu_pre, pool, p, seed, offset, None, relu_post)
    torch.cuda.synchronize()
    if fwd:
        if exact_p:
            _exact(outd[..., :C], ref_out, what + " out")
        else:
            _within(outd[..., :C], ref_out, A_out, 2, what + " out")
        assert (outd[..., C:] == SENT).all(), what + ": the padding of out was written"
    if not bwd:
        return
    # the gate of the post-add ReLU reads `out`: hand the kernels the oracle's (the same bits when the forward is exact; the
    # same sign always, a positive number does not round to zero here)
    outd[..., :C] = ref_out.to(torch.float32).to("cuda")
    dy = _grid(g, (N, Ho, Wo, C))
    dyd, ld_dy = _wide(dy, pad)
    mean = None if mean_null else _grid(g, (C,), -64, 65)
    invstd = None if mean_null else torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)]
    coef = None if mean_null else torch.randn(2 * C, generator=g).to(F64)       # arbitrary: apply is tested independently of reduce
    md, isd, cd = (None, None, None) if mean_null else (_dev(mean), _dev(invstd), _dev(coef))
    r = glue.chain_bwd(dy, x, ref_out, scale, shift, mean, invstd, None if coef is None else _cpu64(cd), relu_pre, pool, mask,
                       relu_post)
    args = (N, H, W, C, int(relu_pre), int(pool), float(p), seed, offset, None, int(relu_post), sp())
    if not mean_null:
        rows = lib.pd_chain_bwd_rows(N, H, W, C)
        part = torch.full((rows, C, 2), float("nan"), dtype=torch.float32, device="cuda")
        check(lib.pd_chain_bwd_reduce(ptr(dyd), ld_dy, ptr(xd), ptr(outd), ld_out, ptr(sd), ptr(bd), ptr(md), ptr(isd), ptr(part),
                                      *args), "pd_chain_bwd_reduce")
        torch.cuda.synchronize()
        assert torch.isfinite(part).all(), what + ": a partial row was left unwritten"
        s = _cpu64(part).sum(0)
        _within(s[:, 0], r["sum_g"], r["A_sum_g"], N * H * W, what + " sum g")
        _within(s[:, 1], r["sum_gx"], r["A_sum_gx"], N * H * W, what + " sum g*xhat")
    dxd = torch.full(shape, SENT, dtype=torch.float32, device="cuda")
    dresd = torch.full((N, Ho, Wo, C), SENT, dtype=torch.float32, device="cuda") if relu_post else None
    check(lib.pd_chain_bwd_apply(ptr(dyd), ld_dy, ptr(xd), ptr(outd), ld_out, ptr(sd), ptr(bd), ptr(md), ptr(isd), ptr(cd),
                                 ptr(dxd), ptr(dresd), *args), "pd_chain_bwd_apply")
    torch.cuda.synchronize()
    if mean_null and exact_p:
        _exact(dxd, r["dx"], what + " dx (eval)")
    else:
        _within(dxd, r["dx"], r["A_dx"], (1 if mean_null else 3) + (0 if exact_p else 1), what + " dx")
    if relu_post:
        _exact(dresd, r["dres"], what + " dres")
    if not mean_null:
        # g itself: the eval-mode form of apply returns g * scale, and the scales are powers of two
        gd = torch.full(shape, SENT, dtype=torch.float32, device="cuda")
        check(lib.pd_chain_bwd_apply(ptr(dyd), ld_dy, ptr(xd), ptr(outd), ld_out, ptr(sd), ptr(bd), None, None, None, ptr(gd),
                                     None, *args), "pd_chain_bwd_apply")
        torch.cuda.synchronize()
        got_g = _cpu64(gd) / (1.0 if scale_null else scale)
        if exact_p:
            _exact(got_g.to(torch.float32), r["g"], what + " g")
        else:
            _within(got_g, r["g"], r["g"].abs(), 1, what + " g")
    assert (outd[..., C:] == SENT).all() and (dyd[..., C:] == SENT).all()


@pytest.mark.parametrize("p", [0.0, 0.5, 0.25])
@pytest.mark.parametrize("shape", [(2, 6, 8, 64), (1, 5, 7, 16)])
def test_chain_every_flag_combination_with_padded_row_strides(shape, p):
    """relu_pre x pool x relu_post x {no res, res} x drop_p {0, 0.5, 0.25} on the even grid (window branch of the backward) and
    the odd grid (chain_grad, dropped row / column), with ld_res = ld_out = ld_dy = C + 8."""
    for k, (rp, pool, rpost, has_res) in enumerate(itertools.product((0, 1), (0, 1), (0, 1), (0, 1))):
        _chain_case(shape, rp, pool, rpost, has_res, p, pad=8, rng_seed=k)


@pytest.mark.parametrize("shape", [(3, 2, 2, 4), (2, 9, 4, 128), (1, 4, 6, 1024)])
def test_chain_production_combinations_at_the_channel_extremes_and_odd_grids(shape):
    """C/4 = 1 on the smallest poolable grid, C/4 = 256, and a second odd grid: ConvBlock (relu_pre, [pool], dropout, [res]),
    the BasicBlock tail (no relu_pre, res, relu_post), the inference chain (scale NULL) and the eval-mode backward (mean
    NULL), tight and padded strides."""
    for pool, has_res, p in itertools.product((0, 1), (0, 1), (0.0, 0.5, 0.25)):
        _chain_case(shape, 1, pool, 0, has_res, p, pad=0 if has_res else 8, rng_seed=1)
    _chain_case(shape, 0, 0, 1, 1, 0.0, rng_seed=2)
    _chain_case(shape, 0, 0, 1, 1, 0.0, pad=8, rng_seed=3)
    for pool in (0, 1):
        _chain_case(shape, 0, pool, 1, 1, 0.0, scale_null=True, mean_null=True, rng_seed=4)
        _chain_case(shape, 1, pool, 0, 0, 0.5, mean_null=True, rng_seed=5)
        _chain_case(shape, 1, pool, 1, 1, 0.25, pad=8, mean_null=True, rng_seed=6)
        _chain_case(shape, 1, pool, 0, 1, 0.5, scale_null=True, rng_seed=7)


def test_chain_forward_grid_stride_loop_iterates():
    """(2,128,160,128) unpooled: 1.3 M quads > 4096 x 256, so chain_fwd_kernel's loop runs twice for part of the grid; with
    dropout, whose index is the loop variable."""
    assert 2 * 128 * 160 * 32 > 4096 * 256
    _chain_case((2, 128, 160, 128), 1, 0, 0, 1, 0.5, bwd=False)
    _chain_case((2, 128, 160, 128), 0, 0, 1, 1, 0.0, bwd=False)


def test_chain_backward_grid_stride_loop_iterates():
    """(1,64,80,256): 327680 quads > 1024 x 256 -- the per-pixel loop of chain_bwd_kernel iterates (unpooled), and the pooled
    even grid takes the window branch at a production size."""
    assert 64 * 80 * 64 > 1024 * 256
    _chain_case((1, 64, 80, 256), 1, 0, 0, 1, 0.5, fwd=False)
    _chain_case((1, 64, 80, 256), 1, 1, 0, 0, 0.5, fwd=False)
    _chain_case((1, 64, 80, 256), 0, 0, 1, 1, 0.0, fwd=False)


def test_dropout_mask_statistics_and_the_step_state_offset_rule():
    lib, check, ptr, sp = _L()
    shape, seed = (2, 16, 16, 64), 0xC0FFEE
    n = 2 * 16 * 16 * 64
    for p in (0.5, 0.25):
        m3, m4 = _mask(shape, 0, p, seed, 3), _mask(shape, 0, p, seed, 4)
        keep = (m3 != 0).double().mean().item()
        assert abs(keep - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), f"p={p}: keep fraction {keep}"
        agree = ((m3 != 0) == (m4 != 0)).double().mean().item()
        q = p * p + (1 - p) * (1 - p)
        assert abs(agree - q) <= 5 * math.sqrt(q * (1 - q) / n), f"p={p}: masks of two offsets agree at {agree}"
        assert torch.equal(_mask(shape, 0, p, seed, 3), m3)
        assert not torch.equal(_mask(shape, 0, p, seed + 1, 3), m3)
    # step_state[0] = k and offset o  ==  step_state NULL and offset o + (k << 12): pooled even, pooled odd, unpooled
    for shp, pool in (((2, 6, 8, 64), 1), ((1, 5, 7, 16), 1), ((1, 5, 7, 16), 0)):
        for k in (1, 5):
            state = torch.tensor([k, 9, 0, 0], dtype=torch.int64, device="cuda")
            assert torch.equal(_mask(shp, pool, 0.5, seed, 7, state), _mask(shp, pool, 0.5, seed, 7 + (k << 12)))
            assert not torch.equal(_mask(shp, pool, 0.5, seed, 7, state), _mask(shp, pool, 0.5, seed, 7))
    state = torch.tensor([4, 9, 123, 0], dtype=torch.int64, device="cuda")
    check(lib.pd_step_tick(ptr(state), 1, 0, sp()), "pd_step_tick")
    torch.cuda.synchronize()
    assert state.tolist() == [5, 9, 123, 0]


def test_chain_backward_follows_the_step_state_too():
    """The backward kernels add step_state[0] << 12 like the forward: with the counter at k they must match the oracle fed with
    the mask of offset o + (k << 12), on all three index expressions."""
    lib, check, ptr, sp = _L()
    seed, o, k = 99, 11, 5
    state = torch.tensor([k, 0, 0, 0], dtype=torch.int64, device="cuda")
    for shape, pool in (((2, 6, 8, 64), 1), ((1, 5, 7, 16), 1), ((1, 5, 7, 16), 0)):
        N, H, W, C = shape
        Ho, Wo = (H // 2, W // 2) if pool else (H, W)
        g = torch.Generator().manual_seed(H + pool)
        x, scale, shift, dy = _grid(g, shape), _scales(g, C), _grid(g, (C,)), _grid(g, (N, Ho, Wo, C))
        mask = _mask(shape, pool, 0.5, seed, o + (k << 12))
        r = glue.chain_bwd(dy, x, None, scale, shift, None, None, None, 1, pool, mask, 0)
        dxd = torch.empty(shape, dtype=torch.float32, device="cuda")
        xd, sd, bd, dyd = _dev(x), _dev(scale), _dev(shift), _dev(dy)
        check(lib.pd_chain_bwd_apply(ptr(dyd), C, ptr(xd), None, C, ptr(sd), ptr(bd), None, None, None, ptr(dxd), None, N, H, W, C,
                                     1, pool, 0.5, seed, o, ptr(state), 0, sp()), "pd_chain_bwd_apply")
        torch.cuda.synchronize()
        _exact(dxd, r["dx"], f"step_state backward {shape} pool={pool}")


def test_chain_dres_is_refused_without_relu_post_and_empty_batches_are_no_ops():
    lib, check, ptr, sp = _L()
    t = torch.full((1, 2, 2, 4), SENT, dtype=torch.float32, device="cuda")
    c = torch.zeros(8, dtype=torch.float32, device="cuda")
    rc = lib.pd_chain_bwd_apply(ptr(t), 4, ptr(t), ptr(t), 4, ptr(c), ptr(c), ptr(c), ptr(c), ptr(c), ptr(t), ptr(t), 1, 2, 2, 4, 1, 0,
                                0.0, 0, 0, None, 0, sp())
    assert rc == EINVAL and b"dres" in lib.pd_last_error()
    out = t.clone()
    assert lib.pd_chain_fwd(ptr(t), ptr(c), ptr(c), None, ptr(out), 0, 2, 2, 4, 0, 4, 1, 1, 0.5, 1, 2, None, 0, sp()) == 0
    assert lib.pd_chain_bwd_reduce(ptr(t), 4, ptr(t), ptr(t), 4, ptr(c), ptr(c), ptr(c), ptr(c), ptr(out), 0, 2, 2, 4, 1, 0, 0.0, 0, 0,
                                   None, 0, sp()) == 0
    assert lib.pd_chain_bwd_apply(ptr(t), 4, ptr(t), ptr(t), 4, ptr(c), ptr(c), ptr(c), ptr(c), ptr(c), ptr(out), None, 0, 2, 2, 4, 1, 0,
                                  0.0, 0, 0, None, 0, sp()) == 0
    torch.cuda.synchronize()
    assert (out == SENT).all()


def test_conv_bn_chain_with_dropout_matches_fp64_autograd_with_the_recovered_mask():
    """End to end through PF.conv_bn_chain (1x1 identity convolution -> BatchNorm(train) -> ReLU -> 2x2 max-pool -> dropout
    0.5) at (2,6,8,64): pd_chain_bwd_reduce, pd_bn_bwd_finalize and pd_chain_bwd_apply together against fp64 autograd of
    F.batch_norm(training=True) with the mask the forward kernel drew -- the backward really regenerates the forward's mask.

    Bounds (u = 2^-24, n = N*H*W = 96).  Unlike the direct cases, mean and invstd come from the convolution epilogue's fp32
    partial sums, so their own error enters (sum of n terms in any order, first order):
      dm  = n u mean|x|                                      error of the batch mean
      ri  = ((n + 1) u mean(x^2) + 2 |mean| dm) / (2 (var + eps)) + 2 u      relative error of invstd (and of scale)
      e_xhat = invstd dm + |xhat| ri                         error of xhat = (x - mean) invstd
      out     |scale| e_xhat + (4 + 4) u (|x| |scale| + |mean| |scale| + |beta|), through the max-pool (window maximum) and mask;
      dbeta   (n + 4) u sum |g|                              (the sum of g does not read the statistics)
      dgamma  (n + 8) u sum |g| xa + sum |g| e_xhat,         xa = (|x| + |mean|) invstd >= |xhat|
      dx      (2 n + 16) u A + ri A + |scale| (e_xhat |c2| + |xhat| E_dgamma / n),  A = |scale| (|g| + mean|g| + xa mean(|g| xa)).
    All of them are ~1e-5 or below against errors of order 1 from a mask that differs between forward and backward."""
    import torch.nn.functional as F
    from polardepth import functional as PF
    N, H, W, C = 2, 6, 8, 64
    g = torch.Generator().manual_seed(2024)
    conv = torch.nn.Conv2d(C, C, 1, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.eye(C).view(C, C, 1, 1))
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    conv.weight.requires_grad_(False)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    gamma = torch.randn(C, generator=g) + 0.5
    gamma[::4] = -gamma[::4].abs() - 0.1                    # negative scale in front of the max-pool in a quarter of the channels
    beta = torch.randn(C, generator=g) * 0.5
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    x = torch.randn(N, C, H, W, generator=g)
    dy = torch.randn(N, C, H // 2, W // 2, generator=g)
    xc = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    cfg = PF.ChainCfg(stride=1, pad=0, relu_pre=True, pool=True, drop_p=0.5, relu_post=False)
    # manual_seed also zeroes word 0 of every device's step words: save and restore them with the host side of the stream
    saved = (PF.DropoutState.seed, PF.DropoutState.site)
    saved_steps = {i: int(st[0].item()) for i, st in PF.DropoutState._state.items()}
    PF.DropoutState.manual_seed(77)
    try:
        out = PF.conv_bn_chain(xc, conv, bn, cfg, training=True)
        mask = _mask((N, H, W, C), 1, 0.5, cfg.seed, cfg.offset, PF.DropoutState.state(xc.device))
        assert 0.3 < (mask != 0).double().mean().item() < 0.7
        out.backward(dy.cuda().contiguous(memory_format=torch.channels_last))
        torch.cuda.synchronize()
    finally:
        PF.DropoutState.seed, PF.DropoutState.site = saved
        for i, k in saved_steps.items():
            PF.DropoutState._state[i][0] = k
    # fp64 autograd
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(x64, None, None, g64, b64, True, 0.0, bn.eps)
    ref = F.max_pool2d(F.relu(z), 2) * mask.permute(0, 3, 1, 2)
    ref.backward(dy.double())
    # scales of the bounds, from the oracle on the fp64 coefficients
    xh = x.double().permute(0, 2, 3, 1)
    n = N * H * W
    mean = xh.mean((0, 1, 2))
    var = xh.var((0, 1, 2), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + bn.eps)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    dm = n * U * xh.abs().mean((0, 1, 2))                                           # error of the batch mean
    ri = ((n + 1) * U * (xh * xh).mean((0, 1, 2)) + 2 * mean.abs() * dm) / (2 * (var + bn.eps)) + 2 * U      # relative, of invstd
    xhat = (xh - mean) * invstd
    e_xhat = invstd * dm + xhat.abs() * ri
    r = glue.chain_bwd(dy.double().permute(0, 2, 3, 1), xh, None, scale, shift, mean, invstd, torch.zeros(2 * C, dtype=F64), 1, 1,
                       mask, 0)
    E_z = scale.abs() * e_xhat + 8 * U * (xh.abs() * scale.abs() + mean.abs() * scale.abs() + beta.double().abs())
    w = glue._windows(E_z, H // 2, W // 2)
    E_out = torch.maximum(torch.maximum(w[0], w[1]), torch.maximum(w[2], w[3])) * mask
    zero = torch.zeros(1, dtype=F64)
    _within(out.detach().permute(0, 2, 3, 1), ref.detach().permute(0, 2, 3, 1), zero, 0, "conv_bn_chain out", extra=E_out)
    _within(bn.bias.grad, b64.grad, r["A_sum_g"], n, "dbeta")
    E_dgamma = (n + 8) * U * r["A_sum_gx"] + (r["g"].abs() * e_xhat).sum((0, 1, 2))
    _within(bn.weight.grad, g64.grad, zero, 0, "dgamma", extra=E_dgamma)
    xa = (xh.abs() + mean.abs()) * invstd
    A_dx = scale.abs() * (r["g"].abs() + r["A_sum_g"] / n + xa * r["A_sum_gx"] / n)
    E_dx = (2 * n + 16) * U * A_dx + ri * A_dx + scale.abs() * (e_xhat * r["sum_gx"].abs() / n + xhat.abs() * E_dgamma / n)
    _within(xc.grad.permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1), zero, 0, "dx", extra=E_dx)


# ====================================================================================================== 3x3 / s2 max-pool
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 2, 3, 8), (1, 5, 7, 16), (2, 8, 8, 64), (1, 9, 6, 4)])
def test_maxpool3s2_values_index_bytes_and_gradient_are_exact(shape):
    lib, check, ptr, sp = _L()
    N, H, W, C = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(H * 100 + W)
    post_relu = (torch.randint(1, 9, shape, generator=g).to(F64) / 8.0) * (torch.rand(shape, generator=g) < 0.5).to(F64)
    for name, x in (("post-ReLU", post_relu), ("all -1", torch.full(shape, -1.0, dtype=F64))):
        what = f"maxpool3s2 {shape} {name}"
        xd = _dev(x)
        y = torch.full((N, Ho, Wo, C), SENT, dtype=torch.float32, device="cuda")
        idx = torch.full((N, Ho, Wo, C), 255, dtype=torch.uint8, device="cuda")
        check(lib.pd_maxpool3s2_fwd(ptr(xd), ptr(y), ptr(idx), N, H, W, C, sp()), "pd_maxpool3s2_fwd")
        y2 = torch.full_like(y, SENT)
        check(lib.pd_maxpool3s2_fwd(ptr(xd), ptr(y2), None, N, H, W, C, sp()), "pd_maxpool3s2_fwd")      # idx NULL is accepted
        torch.cuda.synchronize()
        ref_y, ref_idx = glue.maxpool3s2(x)
        _exact(y, ref_y, what + " y")
        _exact(y2, ref_y, what + " y (no idx)")
        assert torch.equal(idx.cpu(), ref_idx), what + ": idx bytes"
        dy = _grid(g, (N, Ho, Wo, C))
        add = _grid(g, shape)
        dyd = _dev(dy)
        addd, ld_add = _wide(add, 4)
        dx = torch.full(shape, SENT, dtype=torch.float32, device="cuda")
        dx2 = torch.full(shape, SENT, dtype=torch.float32, device="cuda")
        check(lib.pd_maxpool3s2_bwd(ptr(idx), ptr(dyd), ptr(dx), N, H, W, C, sp()), "pd_maxpool3s2_bwd")
        check(lib.pd_maxpool3s2_bwd_add(ptr(idx), ptr(dyd), ptr(addd), ld_add, ptr(dx2), N, H, W, C, sp()), "pd_maxpool3s2_bwd_add")
        torch.cuda.synchronize()
        _exact(dx, glue.maxpool3s2_bwd(ref_idx, dy, H, W)[0], what + " dx")
        _exact(dx2, glue.maxpool3s2_bwd(ref_idx, dy, H, W, add)[0], what + " dx + addend")
        assert _cpu64(dx).sum().item() == dy.sum().item(), what + ": the gradient is not conserved"


# ====================================================================================================== decoder upsampling
@pytest.mark.parametrize("dims", [(1, 1, 1, 4, 0), (2, 1, 5, 8, 4), (1, 4, 1, 4, 8), (2, 3, 5, 16, 16), (1, 8, 8, 64, 64)])
def test_upcat_and_its_gradient(dims):
    lib, check, ptr, sp = _L()
    N, H, W, Ca, Cs = dims
    Ct = Ca + Cs
    g = torch.Generator().manual_seed(sum(dims))
    a = torch.randn(N, H, W, Ca, generator=g).to(F64)
    skip = torch.randn(N, 2 * H, 2 * W, Cs, generator=g).to(F64) if Cs else None
    ad = _dev(a)
    skd, ld_skip = _wide(skip, 4) if Cs else (None, 0)
    out = torch.full((N, 2 * H, 2 * W, Ct), SENT, dtype=torch.float32, device="cuda")
    check(lib.pd_upcat_fwd(ptr(ad), ptr(skd), ld_skip, ptr(out), N, H, W, Ca, Cs, sp()), "pd_upcat_fwd")
    torch.cuda.synchronize()
    ref, A = glue.upcat(_cpu64(ad), None if skip is None else _cpu64(skd[..., :Cs]))
    _within(out[..., :Ca], ref[..., :Ca], A[..., :Ca], 4, f"upcat {dims} upsampled part")
    if Cs:
        _exact(out[..., Ca:], ref[..., Ca:], f"upcat {dims} skip part")
    # backward on the gradient of the CONCATENATED tensor (ld_d = Ca + Cs), with and without the ELU derivative
    dout = torch.randn(N, 2 * H, 2 * W, Ct, generator=g).to(F64)
    elu_y = torch.randn(N, H, W, Ca, generator=g).to(F64).clamp_min(-0.999)
    elu_y.view(-1)[::5] = 0.0
    dd, ed = _dev(dout), _dev(elu_y)
    da = torch.full((N, H, W, Ca), SENT, dtype=torch.float32, device="cuda")
    da_elu, da_null = torch.full_like(da, SENT), torch.full_like(da, SENT)
    check(lib.pd_up_bwd(ptr(dd), Ct, ptr(da), N, H, W, Ca, sp()), "pd_up_bwd")
    check(lib.pd_up_bwd_elu(ptr(dd), Ct, ptr(ed), ptr(da_elu), N, H, W, Ca, sp()), "pd_up_bwd_elu")
    check(lib.pd_up_bwd_elu(ptr(dd), Ct, None, ptr(da_null), N, H, W, Ca, sp()), "pd_up_bwd_elu")
    torch.cuda.synchronize()
    rb, Ab = glue.up_bwd(_cpu64(dd)[..., :Ca])
    re, Ae = glue.up_bwd(_cpu64(dd)[..., :Ca], _cpu64(ed))
    _within(da, rb, Ab, 16, f"up_bwd {dims}")
    _within(da_elu, re, Ae, 16, f"up_bwd_elu {dims}")
    assert torch.equal(da_null, da)
    # adjoint identity on the returned tensors, positive operands (no cancellation in either inner product)
    ap = torch.rand(N, H, W, Ca, generator=g).to(F64) + 0.5
    gp = torch.rand(N, 2 * H, 2 * W, Ct, generator=g).to(F64) + 0.5
    apd, gpd = _dev(ap), _dev(gp)
    up = torch.empty((N, 2 * H, 2 * W, Ct), dtype=torch.float32, device="cuda")
    back = torch.empty((N, H, W, Ca), dtype=torch.float32, device="cuda")
    check(lib.pd_upcat_fwd(ptr(apd), ptr(skd), ld_skip, ptr(up), N, H, W, Ca, Cs, sp()), "pd_upcat_fwd")
    check(lib.pd_up_bwd(ptr(gpd), Ct, ptr(back), N, H, W, Ca, sp()), "pd_up_bwd")
    torch.cuda.synchronize()
    lhs = (_cpu64(up)[..., :Ca] * _cpu64(gpd)[..., :Ca]).sum().item()
    rhs = (_cpu64(apd) * _cpu64(back)).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs), f"upcat {dims}: <up(a), g> = {lhs!r} but <a, up_bwd(g)> = {rhs!r}"


def _up2x_ac_case(N, H, W, C, g):
    lib, check, ptr, sp = _L()
    what = f"up2x_ac ({N},{H},{W},{C})"
    a = torch.randn(N, H, W, C, generator=g).to(F64)
    dout = torch.randn(N, 2 * H, 2 * W, C, generator=g).to(F64)
    ap = torch.rand(N, H, W, C, generator=g).to(F64) + 0.5
    gp = torch.rand(N, 2 * H, 2 * W, C, generator=g).to(F64) + 0.5
    res = []
    for src, grad in ((a, dout), (ap, gp)):
        sd, gd = _dev(src), _dev(grad)
        up = torch.full((N, 2 * H, 2 * W, C), SENT, dtype=torch.float32, device="cuda")
        back = torch.full((N, H, W, C), SENT, dtype=torch.float32, device="cuda")
        check(lib.pd_up2x_ac_fwd(ptr(sd), ptr(up), N, H, W, C, sp()), "pd_up2x_ac_fwd")
        check(lib.pd_up2x_ac_bwd(ptr(gd), ptr(back), N, H, W, C, sp()), "pd_up2x_ac_bwd")
        res.append((sd, gd, up, back))
    torch.cuda.synchronize()
    sd, gd, up, back = res[0]
    eps = 2 * U * ((H - 1) + (W - 1))         # absolute error of the fp32 source indices, see the module docstring
    ref, A = glue.up2x_ac(_cpu64(sd))
    _within(up, ref, A, 4, what + " fwd", extra=eps * glue.up2x_ac_reach(_cpu64(sd)))
    rb, Ab = glue.up2x_ac_bwd(_cpu64(gd))
    _within(back, rb, Ab, 25, what + " bwd", extra=eps * glue.up2x_ac_bwd_reach(_cpu64(gd)))
    sd, gd, up, back = res[1]
    lhs, rhs = (_cpu64(up) * _cpu64(gd)).sum().item(), (_cpu64(sd) * _cpu64(back)).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs), f"{what}: <up(a), g> = {lhs!r} but <a, up_bwd(g)> = {rhs!r}"


def test_up2x_align_corners_for_every_height_up_to_33():
    """Values against the fp64 interpolation matrices and the adjoint identity <up(a), g> == <a, up_bwd(g)> for every H in 1..33
    and W in {1, 2, 7, 20}: the identity holds only if the gather window of up2x_ac_bwd_kernel covers every output row / column
    that reads an input row / column, for every size."""
    g = torch.Generator().manual_seed(7)
    for H in range(1, 34):
        for W in (1, 2, 7, 20):
            _up2x_ac_case(1, H, W, 4, g)
        _up2x_ac_case(1, 3, H, 4, g)                     # and every width: the column taps are code of their own
    _up2x_ac_case(2, 12, 16, 64, g)


# ====================================================================================================== BatchNorm finalize, R <= 4096
@pytest.mark.parametrize("C", [4, 36, 64])
def test_batchnorm_finalize_single_workgroup_kernels(C):
    """pd_bn_fwd_finalize / pd_bn_bwd_finalize at R <= 4096 (bn_stats_small_kernel: the branch every layer below 256x320 takes)
    against fp64, tolerances of test_batchnorm_finalize_ticket_kernels; C = 36 leaves a 32-channel group partly empty."""
    lib, check, ptr, sp = _L()
    dev = torch.device("cuda")
    acc = torch.zeros(2 * C + 2, dtype=F64, device=dev)
    for R, count in [(R, float(R * 128)) for R in (1, 31, 32, 33, 97, 128, 129, 4096)] + [(1, 1.0)]:
        rng = np.random.default_rng(R + C)
        part = rng.standard_normal((R, C, 2)).astype(np.float32)
        part[:, :, 1] = np.abs(part[:, :, 1]) * 3 + 2.0
        if count == 1.0:
            part[:, :, 1] = part[:, :, 0] ** 2                 # one sample: variance 0, and no n / (n - 1)
        gamma = rng.standard_normal(C).astype(np.float32); beta = rng.standard_normal(C).astype(np.float32)
        rm0 = rng.standard_normal(C).astype(np.float32); rv0 = (rng.random(C) + 0.5).astype(np.float32)
        o = glue.bn_finalize_fwd(part, count, gamma, beta, rm0, rv0, float(np.float32(0.1)), float(np.float32(1e-5)), True)
        o = {k: v.numpy() for k, v in o.items()}
        pd_ = torch.from_numpy(part).to(dev)
        gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
        rm, rv = torch.from_numpy(rm0.copy()).to(dev), torch.from_numpy(rv0.copy()).to(dev)
        scale, shift, smean, sinv = (torch.full((C + 4,), SENT, device=dev) for _ in range(4))
        check(lib.pd_bn_fwd_finalize(ptr(pd_), R, C, count, ptr(gd), ptr(bd), ptr(rm), ptr(rv), 0.1, 1e-5, ptr(acc), acc.numel(),
                                     ptr(scale), ptr(shift), ptr(smean), ptr(sinv), 1, sp()), "pd_bn_fwd_finalize")
        torch.cuda.synchronize()
        for t in (scale, shift, smean, sinv):
            assert (t[C:] == SENT).all(), "written past C channels"
        np.testing.assert_allclose(smean[:C].cpu().numpy(), o["mean"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(sinv[:C].cpu().numpy(), o["invstd"], rtol=1e-6)
        np.testing.assert_allclose(scale[:C].cpu().numpy(), o["scale"], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(shift[:C].cpu().numpy(), o["shift"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rm.cpu().numpy(), o["running_mean"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(rv.cpu().numpy(), o["running_var"], rtol=1e-6, atol=1e-7)
        assert acc.abs().max().item() == 0.0, "accumulator not left zero"
        # eval mode: coefficients of the running statistics, which stay untouched; no partials, no accumulator
        e = glue.bn_finalize_fwd(None, 1.0, gamma, beta, rm0, rv0, 0.1, float(np.float32(1e-5)), False)
        rm, rv = torch.from_numpy(rm0.copy()).to(dev), torch.from_numpy(rv0.copy()).to(dev)
        check(lib.pd_bn_fwd_finalize(None, 0, C, 1.0, ptr(gd), ptr(bd), ptr(rm), ptr(rv), 0.1, 1e-5, None, 0, ptr(scale), ptr(shift),
                                     None, None, 0, sp()), "pd_bn_fwd_finalize")
        torch.cuda.synchronize()
        np.testing.assert_allclose(scale[:C].cpu().numpy(), e["scale"].numpy(), rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(shift[:C].cpu().numpy(), e["shift"].numpy(), rtol=1e-5, atol=1e-6)
        assert np.array_equal(rm.cpu().numpy(), rm0) and np.array_equal(rv.cpu().numpy(), rv0)
        # backward: accumulate 0 / 1, dgamma / dbeta NULL
        for accumulate in (0, 1):
            dgamma, dbeta = torch.ones(C, device=dev), torch.ones(C, device=dev)
            coef = torch.full((2 * C + 4,), SENT, device=dev)
            check(lib.pd_bn_bwd_finalize(ptr(pd_), R, C, count, ptr(acc), acc.numel(), ptr(dgamma), ptr(dbeta), ptr(coef), accumulate,
                                         sp()), "pd_bn_bwd_finalize")
            torch.cuda.synchronize()
            dg, db, cf = glue.bn_finalize_bwd(part, count, np.ones(C), np.ones(C), bool(accumulate))
            np.testing.assert_allclose(dbeta.cpu().numpy(), db.numpy(), rtol=1e-6, atol=1e-4)
            np.testing.assert_allclose(dgamma.cpu().numpy(), dg.numpy(), rtol=1e-6, atol=1e-4)
            np.testing.assert_allclose(coef[:2 * C].cpu().numpy(), cf.numpy(), rtol=1e-6, atol=1e-9)
            assert (coef[2 * C:] == SENT).all() and acc.abs().max().item() == 0.0
        coef = torch.full((2 * C,), SENT, device=dev)
        check(lib.pd_bn_bwd_finalize(ptr(pd_), R, C, count, ptr(acc), acc.numel(), None, None, ptr(coef), 0, sp()), "pd_bn_bwd_finalize")
        torch.cuda.synchronize()
        np.testing.assert_allclose(coef.cpu().numpy(), cf.numpy(), rtol=1e-6, atol=1e-9)


# ====================================================================================================== Adam
def _f32(v):
    return float(np.float32(v))


def _adam_case(n, step, wd, gs, zero_grad, g):
    lib, check, ptr, sp = _L()
    what = f"adam n={n} step={step} wd={wd} grad_scale={gs} zero_grad={zero_grad}"
    lr, b1, b2, eps, wd = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(1e-8), _f32(wd)
    p0 = torch.randn(n, generator=g)
    g0 = torch.randn(n, generator=g)
    if step == 1:                                   # the state of a fresh optimizer
        m0, v0 = torch.zeros(n), torch.zeros(n)
    else:
        m0, v0 = torch.randn(n, generator=g) * 0.3, torch.rand(n, generator=g) + 1e-3

    def bufs():
        out = []
        for t in (p0, g0, m0, v0):
            b = torch.full((n + 8,), SENT, dtype=torch.float32, device="cuda")
            b[:n] = t.cuda()
            out.append(b)
        return out

    P, G, M, V = bufs()
    check(lib.pd_adam_step(ptr(P), ptr(G), ptr(M), ptr(V), n, lr, b1, b2, eps, wd, step, None, gs, zero_grad, sp()), "pd_adam_step")
    # the device-side route: t, lr and grad_scale from the step words
    P2, G2, M2, V2 = bufs()
    state = torch.tensor([3, step - 1, 0, 0], dtype=torch.int64, device="cuda")
    check(lib.pd_step_set_hyper(ptr(state), lr, gs, sp()), "pd_step_set_hyper")
    check(lib.pd_step_tick(ptr(state), 0, 1, sp()), "pd_step_tick")
    check(lib.pd_adam_step(ptr(P2), ptr(G2), ptr(M2), ptr(V2), n, 0.5, b1, b2, eps, wd, 0, ptr(state), 3.0, zero_grad, sp()),
          "pd_adam_step")
    torch.cuda.synchronize()
    assert state[:2].tolist() == [3, step]
    r = glue.adam_step(p0, g0, m0, v0, lr, b1, b2, eps, wd, step, gs)
    for name, buf in (("p", P), ("g", G), ("m", M), ("v", V)):
        assert (buf[n:] == SENT).all(), f"{what}: {name} written beyond n"
    err_m, err_v, err_p = (_cpu64(M[:n]) - r["m"]).abs(), (_cpu64(V[:n]) - r["v"]).abs(), (_cpu64(P[:n]) - r["p"]).abs()
    assert (err_m <= 4 * U * r["A_m"]).all(), f"{what}: m off by up to {(err_m / r['A_m'].clamp_min(1e-300)).max().item() / U:.2f} u"
    nv = 4 if wd == 0 else 7                       # module docstring: the weight decay adds two roundings to gr, v squares it
    assert (err_v <= nv * U * r["A_v"]).all(), f"{what}: v off by up to {(err_v / r['A_v'].clamp_min(1e-300)).max().item() / U:.2f} u"
    bound_p = 2 * U * r["p"].abs() + 8 * U * r["A_update"]
    assert (err_p <= bound_p).all(), f"{what}: p beyond 2u|p| + 8u|update| by a factor {(err_p / bound_p).max().item():.2f}"
    if zero_grad:
        assert (G[:n] == 0).all(), what + ": g not cleared"
    else:
        assert torch.equal(G[:n].cpu(), g0), what + ": g changed"
    for a, b, name in ((P, P2, "p"), (G, G2, "g"), (M, M2, "m"), (V, V2, "v")):
        assert torch.equal(a, b), f"{what}: the step_state route differs in {name}"


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_adam_step_small_buffers_every_combination(n):
    g = torch.Generator().manual_seed(n)
    for step, wd, gs, zg in itertools.product((1, 2, 1000), (0.0, 1e-2), (1.0, 0.125), (0, 1)):
        _adam_case(n, step, wd, gs, zg, g)


@pytest.mark.parametrize("step,wd,gs,zg", [(1, 1e-2, 0.125, 1), (2, 0.0, 1.0, 0), (1000, 1e-2, 1.0, 1)])
def test_adam_step_grid_stride_loop_and_tail(step, wd, gs, zg):
    """n = 4096 * 1024 + 7: the grid-stride loop iterates and the last quad is the scalar tail."""
    _adam_case(4096 * 1024 + 7, step, wd, gs, zg, torch.Generator().manual_seed(step))


# ====================================================================================================== small ones
@pytest.mark.parametrize("L", [1, 7, 255, 256, 257, 5120])
def test_softmax_rows(L):
    lib, check, ptr, sp = _L()
    g = torch.Generator().manual_seed(L)
    scale = 0.25
    x = torch.randn(3, L, generator=g) * 8
    x[0] = torch.linspace(-320.0, 320.0, L) if L > 1 else torch.tensor([320.0])      # scale * x spans +-80
    x[0] = x[0][torch.randperm(L, generator=g)]
    x[1] = 3.5                                                                         # a constant row
    xd = torch.full((3 * L + 8,), SENT, dtype=torch.float32, device="cuda")
    xd[:3 * L] = x.flatten().cuda()
    check(lib.pd_softmax_rows_fwd(ptr(xd), 3, L, scale, sp()), "pd_softmax_rows_fwd")
    torch.cuda.synchronize()
    assert (xd[3 * L:] == SENT).all()
    got = _cpu64(xd[:3 * L]).view(3, L)
    ref = glue.softmax_rows(x, scale)
    zmax = (x.double() * scale).abs().max(-1, keepdim=True).values
    bound = U * (2 * zmax + math.ceil(L / 256) + 16) * ref + 2.0 ** -126
    err = (got - ref).abs()
    assert (err <= bound).all(), f"softmax L={L}: worst err/bound {(err / bound).max().item():.2f}"
    assert ((got.sum(-1) - 1).abs() <= (L / 256 + 16) * U).all(), f"softmax L={L}: row sums {got.sum(-1).tolist()}"
    p = ref.to(torch.float32)
    dp = torch.randn(3, L, generator=g)
    rb, Ab = glue.softmax_rows_bwd(p, dp, scale)
    pd_, dd = p.cuda().contiguous(), dp.clone().cuda().contiguous()
    check(lib.pd_softmax_rows_bwd(ptr(pd_), ptr(dd), 3, L, scale, sp()), "pd_softmax_rows_bwd")
    torch.cuda.synchronize()
    _within(dd, rb, Ab, L, f"softmax bwd L={L}", extra=2.0 ** -126)       # p of the +-80 row reaches the subnormal range


@pytest.mark.parametrize("n", [1, 255, 1025])
def test_act_bwd(n):
    lib, check, ptr, sp = _L()
    g = torch.Generator().manual_seed(n)
    dy = torch.randn(n, generator=g)
    for act in (1, 2, 3):
        z = torch.randn(n, generator=g)
        z[::7] = 0.0
        y = {1: torch.relu, 2: torch.nn.functional.elu, 3: torch.sigmoid}[act](z)
        dz = torch.full((n + 4,), SENT, dtype=torch.float32, device="cuda")
        dyd, yd = dy.cuda(), y.cuda()
        check(lib.pd_act_bwd(ptr(dyd), ptr(yd), ptr(dz), n, act, sp()), "pd_act_bwd")
        torch.cuda.synchronize()
        ref = glue.act_bwd(dy, y, act)
        assert (dz[n:] == SENT).all()
        if act == 1:
            _exact(dz[:n], ref, f"act_bwd relu n={n}")
        else:
            _within(dz[:n], ref, ref.abs(), 1, f"act_bwd act={act} n={n}")


@pytest.mark.parametrize("n", [4, 1028])
def test_relu_add(n):
    lib, check, ptr, sp = _L()
    g = torch.Generator().manual_seed(n)
    x, res = _grid(g, (n,)), _grid(g, (n,))
    xd, rd = _dev(x), _dev(res)
    for relu, has_res in itertools.product((0, 1), (0, 1)):
        out = torch.full((n + 4,), SENT, dtype=torch.float32, device="cuda")
        check(lib.pd_relu_add(ptr(xd), ptr(rd) if has_res else None, ptr(out), n, relu, sp()), "pd_relu_add")
        torch.cuda.synchronize()
        _exact(out[:n], glue.relu_add(x, res if has_res else None, relu), f"relu_add n={n} relu={relu} res={has_res}")
        assert (out[n:] == SENT).all()


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_reflect_fold_pad(pad):
    lib, check, ptr, sp = _L()
    g = torch.Generator().manual_seed(pad)
    for (H, W), C in itertools.product(((pad + 1, pad + 1), (5, 9)), (8, 3)):
        dxp = _grid(g, (2, H + 2 * pad, W + 2 * pad, C))
        dd = _dev(dxp)
        dx = torch.full((2 * H * W * C + 4,), SENT, dtype=torch.float32, device="cuda")
        check(lib.pd_reflect_fold_pad(ptr(dd), ptr(dx), 2, H, W, C, pad, sp()), "pd_reflect_fold_pad")
        torch.cuda.synchronize()
        _exact(dx[:2 * H * W * C].view(2, H, W, C), glue.reflect_fold(dxp, pad)[0], f"reflect_fold pad={pad} {H}x{W} C={C}")
        assert (dx[2 * H * W * C:] == SENT).all()


def test_empty_batches_return_ok_and_touch_nothing():
    lib, check, ptr, sp = _L()
    o = torch.full((256,), SENT, dtype=torch.float32, device="cuda")
    i = torch.zeros(256, dtype=torch.float32, device="cuda")
    s = sp()
    assert lib.pd_maxpool3s2_fwd(ptr(i), ptr(o), ptr(o), 0, 4, 4, 4, s) == 0
    assert lib.pd_maxpool3s2_bwd(ptr(i), ptr(i), ptr(o), 0, 4, 4, 4, s) == 0
    assert lib.pd_maxpool3s2_bwd_add(ptr(i), ptr(i), ptr(i), 4, ptr(o), 0, 4, 4, 4, s) == 0
    assert lib.pd_upcat_fwd(ptr(i), ptr(i), 4, ptr(o), 0, 2, 2, 4, 4, s) == 0
    assert lib.pd_up_bwd(ptr(i), 8, ptr(o), 0, 2, 2, 4, s) == 0
    assert lib.pd_up_bwd_elu(ptr(i), 8, ptr(i), ptr(o), 0, 2, 2, 4, s) == 0
    assert lib.pd_up2x_ac_fwd(ptr(i), ptr(o), 0, 2, 2, 4, s) == 0
    assert lib.pd_up2x_ac_bwd(ptr(i), ptr(o), 0, 2, 2, 4, s) == 0
    assert lib.pd_reflect_fold_pad(ptr(i), ptr(o), 0, 3, 3, 4, 1, s) == 0
    assert lib.pd_relu_add(ptr(i), ptr(i), ptr(o), 0, 1, s) == 0
    assert lib.pd_act_bwd(ptr(i), ptr(i), ptr(o), 0, 2, s) == 0
    assert lib.pd_softmax_rows_fwd(ptr(o), 0, 16, 1.0, s) == 0
    assert lib.pd_softmax_rows_bwd(ptr(i), ptr(o), 0, 16, 1.0, s) == 0
    assert lib.pd_adam_step(ptr(o), ptr(o), ptr(o), ptr(o), 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 1.0, 1, s) == 0
    torch.cuda.synchronize()
    assert (o == SENT).all()
