"""PD_CONV_BF16 on the GPU: the single-bf16 forms of the halo-tile forward / data-gradient kernel and of the halo / rolling-row
weight-gradient kernels, per layer class of the network.

Yardsticks (set before measuring):
  * exactness of the scheme: vs an fp64 convolution of the RNE-bf16-rounded operands (bf16 x bf16 products are exact in fp32,
    so only the fp32 accumulation differs), the error is at most 2x the fp32-MFMA kernel's error vs fp64 on the unrounded
    operands at the same shape;
  * the a-priori bound of two operands rounded to 8 significant bits, per element vs fp64 on the unrounded operands:
    |y - y64| <= (2^-8 + K 2^-23) conv(|x|, |w|);
  * no systematic bias: the mean error (vs the rounded-operand reference) is within 4 standard errors of zero;
  * non-finite operands and denormals as documented in include/polardepth.h; determinism, workspace independence, routing."""
import pytest
import torch
import torch.nn.functional as F

from conv_cases import wgrad_raw
from polardepth import ops

pytestmark = pytest.mark.gpu

BF16 = ops.CONV_BF16
# (N, C, H, W, Co, k, mode): 5x5 / 3x3 64 -> 64 at the three encoder / decoder planes, the decoder's reflection-padded
# 128 -> 64 and 96 -> 32 (32-column workgroups, NCB = 1)
CASES = [
    (2, 64, 256, 320, 64, 5, 0),
    (2, 64, 256, 320, 64, 3, 0),
    (8, 64, 128, 160, 64, 3, 0),
    (32, 64, 64, 80, 64, 3, 0),
    (8, 128, 128, 160, 64, 3, 1),
    (2, 96, 256, 320, 32, 3, 1),
]


def _rb(t):
    """RNE to bf16 and back (torch's CPU conversion: round to nearest even, NaN kept, FLT_MAX -> inf)."""
    return t.to(torch.bfloat16).to(torch.float64)


def _fwd64(x, w, p, mode):
    if mode == 1:
        return F.conv2d(F.pad(x, (p, p, p, p), mode="reflect"), w)
    return F.conv2d(x, w, padding=p)


def _dgrad64(dy, w, p):
    return F.conv_transpose2d(dy, w, padding=p)


def _wgrad64(x, dy, w_shape, p, mode):
    xp = F.pad(x, (p, p, p, p), mode="reflect" if mode == 1 else "constant")
    return torch.nn.grad.conv2d_weight(xp, w_shape, dy, padding=0)


def _cl(t):
    return t.float().cuda().contiguous(memory_format=torch.channels_last)


def _run(fn, flags):
    with ops.conv_flags(conv=flags, wgrad=flags):
        out = fn()
    torch.cuda.synchronize()
    return out.cpu().double()


def _check(name, y_bf, y_fp, ref_r, ref_u, bound):
    scale = ref_u.abs().max().item()
    e_bf = (y_bf - ref_r).abs().max().item() / scale           # vs fp64 on the rounded operands: accumulation only
    e_fp = (y_fp - ref_u).abs().max().item() / scale           # the fp32-MFMA kernel vs fp64 on the unrounded operands
    assert e_bf <= 2.0 * e_fp + 1e-9, (name, e_bf, e_fp)
    over = ((y_bf - ref_u).abs() - bound).max().item()
    assert over <= 0.0, (name, over)
    e = (y_bf - ref_r).flatten()
    se = e.std().item() / e.numel() ** 0.5
    assert abs(e.mean().item()) <= 4.0 * se + 1e-30, (name, e.mean().item(), se)
    return e_bf, e_fp


@pytest.mark.parametrize("case", CASES)
def test_bf16_forward_dgrad_wgrad(case):
    N, C, H, W, Co, k, mode = case
    p = k // 2
    q, qw = ops.lib.pd_conv2d_uses_bf16, ops.lib.pd_conv2d_wgrad_uses_bf16
    M = N * H * W
    assert q(M, Co, C, k, k, 1, p, mode, 0, 0, H, W, BF16) == 3
    assert q(M, C, Co, k, k, 1, p, 2, 0, 0, H, W, BF16) == 3
    assert qw(M, Co, C, k, k, 1, p, mode, H, W, H, W, BF16) in (2, 3)
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).float().double()
    x[:, :, : H // 2] *= 37.0
    w = (torch.randn(Co, C, k, k, generator=g, dtype=torch.float64) / (C * k * k) ** 0.5).float().double()
    dy = torch.randn(N, Co, H, W, generator=g, dtype=torch.float64).float().double()
    xd, wd, dyd = _cl(x), _cl(w), _cl(dy)
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    # forward
    ref_u, ref_r = _fwd64(x, w, p, mode), _fwd64(_rb(x), _rb(w), p, mode)
    bound = (2.0 ** -8 + C * k * k * 2.0 ** -23) * _fwd64(x.abs(), w.abs(), p, mode)
    y_bf = _run(lambda: ops.conv2d_fwd(xd, wd, None, 1, p, mode=mode), BF16)
    y_fp = _run(lambda: ops.conv2d_fwd(xd, wd, None, 1, p, mode=mode), ops.CONV_FP32_MFMA)
    _check("fwd", y_bf, y_fp, ref_r, ref_u, bound)
    # data gradient (zero padding on the same grid: also the interior of the reflection-padded layer's)
    ref_u, ref_r = _dgrad64(dy, w, p), _dgrad64(_rb(dy), _rb(w), p)
    bound = (2.0 ** -8 + Co * k * k * 2.0 ** -23) * _dgrad64(dy.abs(), w.abs(), p)
    d_bf = _run(lambda: ops.conv2d_dgrad(dyd, wd, (H, W), 1, p), BF16)
    d_fp = _run(lambda: ops.conv2d_dgrad(dyd, wd, (H, W), 1, p), ops.CONV_FP32_MFMA)
    _check("dgrad", d_bf, d_fp, ref_r, ref_u, bound)
    # weight gradient
    ref_u, ref_r = _wgrad64(x, dy, w.shape, p, mode), _wgrad64(_rb(x), _rb(dy), w.shape, p, mode)
    bound = (2.0 ** -8 + M * 2.0 ** -23) * _wgrad64(x.abs(), dy.abs(), w.shape, p, mode)
    g_bf = _run(lambda: ops.conv2d_wgrad(xd, dyd, w.shape, 1, p, mode=mode), BF16)
    g_fp = _run(lambda: ops.conv2d_wgrad(xd, dyd, w.shape, 1, p, mode=mode), ops.CONV_FP32_MFMA)
    _check("wgrad", g_bf, g_fp, ref_r, ref_u, bound)


@pytest.mark.parametrize("C", [36, 12, 8])
def test_bf16_space_to_depth_stems(C):
    """The three 4x4 / pad 2 stems over the space-to-depth input (row-window form of the halo kernel), forward only: the
    stems read data, and their weight gradient (4x4) keeps its arithmetic."""
    N, H, W, Co = 2, 256, 320, 64
    assert ops.lib.pd_conv2d_uses_bf16(N * H * W, Co, C, 4, 4, 1, 2, 0, 0, 0, H, W, BF16) == 3
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).float().double()
    x[:, :, :, :3] *= 11.0
    w = (torch.randn(Co, C, 4, 4, generator=g, dtype=torch.float64) / (C * 16) ** 0.5).float().double()
    ref_u = F.conv2d(x, w, padding=2)[:, :, :H, :W]
    ref_r = F.conv2d(_rb(x), _rb(w), padding=2)[:, :, :H, :W]
    bound = (2.0 ** -8 + C * 16 * 2.0 ** -23) * F.conv2d(x.abs(), w.abs(), padding=2)[:, :, :H, :W]
    xd, wd = _cl(x), _cl(w)
    y_bf = _run(lambda: ops.conv2d_fwd(xd, wd, None, 1, 2, out_hw=(H, W)), BF16)
    y_fp = _run(lambda: ops.conv2d_fwd(xd, wd, None, 1, 2, out_hw=(H, W)), ops.CONV_FP32_MFMA)
    _check("stem", y_bf, y_fp, ref_r, ref_u, bound)


def test_bf16_epilogue_stays_fp32():
    """Bias, ELU and BatchNorm partial sums on top of the bf16 products: the same fp32 epilogue as the split kernel."""
    N, C, H, W, Co = 2, 64, 256, 320, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / 24.0
    b = torch.randn(Co, generator=g)
    xd, wd = _cl(x), _cl(w)
    with ops.conv_flags(conv=BF16):
        y, st = ops.conv2d_fwd(xd, wd, b.cuda(), 1, 1, mode=1, act=ops.ACT_ELU, want_stats=True)
        z = ops.conv2d_fwd(xd, wd, None, 1, 1, mode=1)
    torch.cuda.synchronize()
    zb = z.cpu().double() + b.double()[None, :, None, None]
    ref = torch.where(zb > 0, zb, torch.expm1(zb))
    assert (y.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    s = st.double().sum(0).cpu()
    M = N * H * W
    assert (s[:, 0] - zb.sum((0, 2, 3))).abs().max().item() / M <= 1e-6 * zb.abs().max().item()


def test_bf16_nonfinite_operands():
    """+-inf, NaN and FLT_MAX (-> +inf in bf16) give what fp64 gives on the rounded operands: the same non-finite pattern,
    the same finite values elsewhere."""
    N, C, H, W, Co = 2, 64, 256, 320, 64
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, C, H, W, generator=g)
    x[0, 3, 10, 10] = float("inf")
    x[0, 5, 100, 200] = float("-inf")
    x[1, 7, 50, 60] = float("nan")
    x[1, 9, 200, 300] = torch.finfo(torch.float32).max
    x[1, 11, 30, 40] = -torch.finfo(torch.float32).max
    w = torch.randn(Co, C, 3, 3, generator=g) / 24.0
    ref = F.conv2d(_rb(x.double()), _rb(w.double()), padding=1)
    y = _run(lambda: ops.conv2d_fwd(_cl(x), _cl(w), None, 1, 1), BF16)
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert torch.equal(torch.isposinf(y), torch.isposinf(ref)) and torch.equal(torch.isneginf(y), torch.isneginf(ref))
    fin = torch.isfinite(ref)
    assert int((~fin).sum()) > 4 * 9
    assert (y[fin] - ref[fin]).abs().max().item() <= 1e-5 * ref[fin].abs().max().item()


# How the bf16 MFMA treats bf16 denormal operands on gfx950, as documented in include/polardepth.h (PD_CONV_BF16)
DENORMALS_FLUSHED = False


def test_bf16_denormal_operands():
    """An input of 2^-130 (an fp32 and bf16 denormal, exact in both) times weights of 2^20: the products are normal numbers, so
    the output shows whether the MFMA kept the denormal operand (2^-110 per tap) or flushed it (0)."""
    N, C, H, W, Co = 2, 64, 256, 320, 64
    x = torch.zeros(N, C, H, W)
    x[0, 0, 100, 100] = 2.0 ** -130
    x[1, 1, 7, 9] = 3.0 * 2.0 ** -131
    x[0, 2, 50, 50] = 1.0                                     # a normal operand next to them
    w = torch.full((Co, C, 3, 3), 2.0 ** 20)
    y = _run(lambda: ops.conv2d_fwd(_cl(x), _cl(w), None, 1, 1), BF16)
    kept = F.conv2d(x.double(), w.double(), padding=1)
    flushed = F.conv2d(torch.where(x.abs() < 2.0 ** -126, torch.zeros_like(x), x).double(), w.double(), padding=1)
    assert kept[0, 0, 100, 100].item() == 2.0 ** -110 and flushed[0, 0, 100, 100].item() == 0.0
    measured = "flushed" if torch.equal(y, flushed) else "kept" if torch.equal(y, kept) else "neither"
    assert measured == ("flushed" if DENORMALS_FLUSHED else "kept"), measured


@pytest.mark.parametrize("case", [CASES[1], CASES[0], CASES[5]])
def test_bf16_determinism_and_workspace_independence(case):
    """The same launch twice: bit-identical (forward, data gradient, weight gradient); the weight gradient also with a
    workspace 8x the size pd_conv2d_wgrad_workspace asks for (the slice count follows the shape and flags only)."""
    N, C, H, W, Co, k, mode = case
    p = k // 2
    g = torch.Generator().manual_seed(11)
    xd = _cl(torch.randn(N, C, H, W, generator=g))
    wd = _cl(torch.randn(Co, C, k, k, generator=g) / 24.0)
    dyd = _cl(torch.randn(N, Co, H, W, generator=g))
    for fn in (lambda: ops.conv2d_fwd(xd, wd, None, 1, p, mode=mode), lambda: ops.conv2d_dgrad(dyd, wd, (H, W), 1, p)):
        assert torch.equal(_run(fn, BF16), _run(fn, BF16))
    need = ops.lib.pd_conv2d_wgrad_workspace(N * H * W, Co, k * k * C, BF16)
    a = wgrad_raw(xd, dyd, (Co, C, k, k), p, mode, need, BF16)
    b = wgrad_raw(xd, dyd, (Co, C, k, k), p, mode, need, BF16)
    c = wgrad_raw(xd, dyd, (Co, C, k, k), p, mode, 8 * need, BF16)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(a, _run(lambda: ops.conv2d_wgrad(xd, dyd, (Co, C, k, k), 1, p, mode=mode), ops.CONV_AUTO).float())


def test_bf16_profiler_labels():
    """ops' profiler labels name the new kernels where they run, and the old ones where the layer keeps its arithmetic."""
    N, C, H, W, Co = 2, 64, 256, 320, 64
    xd = _cl(torch.randn(N, C, H, W))
    wd = _cl(torch.randn(Co, C, 3, 3) / 24.0)
    w1 = _cl(torch.randn(Co, C, 1, 1) / 8.0)
    ops.PROFILE = []
    try:
        with ops.conv_flags(conv=BF16, wgrad=BF16):
            ops.conv2d_fwd(xd, wd, None, 1, 1)
            ops.conv2d_dgrad(xd, wd, (H, W), 1, 1)
            ops.conv2d_wgrad(xd, xd, wd.shape, 1, 1)
            ops.conv2d_fwd(xd, w1, None, 1, 0)
        torch.cuda.synchronize()
        labels = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert labels[:2] == ["conv_halo_bf16_kernel<8x32,64>"] * 2, labels
    assert labels[2] in ("conv_wgrad_roll_bf16_kernel", "conv_wgrad_halo_bf16_kernel"), labels
    assert "bf16" not in labels[3], labels
