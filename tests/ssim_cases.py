"""Shared by tests/test_ssim_cases.py (CPU) and tests/test_ssim_kernels_gpu.py (GPU): named inputs of the SSIM kernels
(csrc/loss.hip, pd_ssim_fwd / pd_ssim_bwd), their fp32 / fp64 references (oracle.losses.ssim and the photometric mix
0.85 mean_c SSIM + 0.15 mean_c |y - x| with autograd), the gate-undecided set, a NumPy fp32 transcription of the kernels'
own order of operations, and the checks as functions of "what the device returned" -- the GPU tests hand them device
results, the CPU test hands them the transcription (which must pass) and mutated transcriptions (which must fail).

Comparison rule (tests/loss_cases.py, imported, nothing fitted to a device result):
  elementwise   |dev - ref64| <= 4 * max|ref32 - ref64| + 1e-6 * max|ref64|
  mean          mean|dev - ref64| <= MEAN_MARGIN * mean|ref32 - ref64| on `training`, `dark` and `steps` at the statistics
                shape (5760 elements), where the max-based rule is loose: the cancellation in E[x^2] - mu^2 against
                C2 = 9e-4 governs the result there, and the worst pixel says little about the typical one.
MEAN_MARGIN = 1.25.  Measured with the transcription below against the oracle (tests/test_ssim_cases.py prints them):
  mean|transcription - ref64| / mean|ref32 - ref64|: forward map / forward mix / gradients (worst of gx, gy, both modes)
    training  0.99 / 0.99 / 0.99      dark  1.00 / 0.99 / 0.97      steps  1.05 / 1.02 / 1.06
The worst ratio measured is 1.06, so 1.25 stands; a precision class below fp32 moves the ratio by orders of magnitude
(window sums in fp16: > 1000 on `training`).

Gradients are compared outside gate_undecided only: where the fp64 unclamped value is within 4 max|ref32 - ref64| of 0 or
1 an fp32 evaluation may sit on the other side of the clamp and its gradient is 0 or not by rounding; dilated by the 5 x 5
footprint of the gather pass.  The excluded share is capped at 5 % (asserted on the CPU for every case with a gradient test).

About the clamp.  With the window averages E[.], sx = E[x^2] - mx^2 >= 0 and |sxy| <= sqrt(sx sy) <= (sx + sy) / 2, and
|2 mx my| <= mx^2 + my^2, so |2 mx my + C1| <= mx^2 + my^2 + C1 and |2 sxy + C2| <= sx + sy + C2: |n| <= d for ANY real images,
signed ones included, and (1 - n / d) / 2 lies in [0, 1] before the clamp.  No input makes the exact value exceed 1 or fall
below 0; only rounding crosses.  `signed` therefore cannot hold what was asked of it (a tenth of the pixels above 1 in
fp64); it is built to bring the exact value within 1e-4 of 1 on half of the image and within 1e-4 of 0 on a quarter, so
that the fp32 value lands on and beyond both clamps by rounding, which is what the gate of the backward pass has to
handle.  test_ssim_cases.py asserts the inequality on every case and these populations on `signed`."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from loss_cases import assert_elem, elem_tol
from oracle import losses as ol

F32, F64 = torch.float32, torch.float64
GEOMS = [(1, 1, 2, 2), (2, 3, 2, 9), (1, 3, 3, 4), (1, 2, 37, 21), (2, 3, 24, 40), (1, 1, 513, 1024)]
STAT = (2, 3, 24, 40)
STRIDE = (1, 1, 513, 1024)
GRID_CAP = 2048 * 256                       # elements one launch covers without a second grid-stride trip
CASES = ["noise", "training", "dark", "flat", "identical", "signed", "steps"]
MEAN_CASES = ("training", "dark", "steps")
GRAD_CASES = ("noise", "training", "dark", "steps")
TRAIN_AMP = 0.01
MEAN_MARGIN = 1.25
MEAN_MIN = 5000
EXCLUDED_CAP = 0.05
NOISE_COND_CAP = 1.0e-5                     # about 2 x the 4.6e-6 measured at the statistics shape


def forward_cases(geom):
    """Every case at the statistics shape, `noise` and `steps` at every shape, `noise` alone at the stride shape."""
    return CASES if geom == STAT else ["noise"] if geom == STRIDE else ["noise", "steps"]


def backward_cases(geom):
    return list(GRAD_CASES) if geom == STAT else ["noise"] if geom == STRIDE else ["noise", "steps"]


# ====================================================================================================== inputs
def _planes(N, C, H, W):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    p = torch.arange(N * C, dtype=F32).view(N, C, 1, 1)
    return yy[None, None], xx[None, None], p


@functools.lru_cache(maxsize=None)
def make(case, geom, seed=0):
    """(x, y) fp32 [N,C,H,W]; x plays the warped neighbour (pred), y the target."""
    N, C, H, W = geom
    g = torch.Generator().manual_seed(1000 * seed + sum(geom) + 17 * CASES.index(case))
    yy, xx, p = _planes(N, C, H, W)
    if case in ("noise", "identical"):
        x = torch.rand(N, C, H, W, generator=g)
        y = (x + 0.15 * torch.randn(N, C, H, W, generator=g)).clamp(0, 1)
        if case == "identical":
            y = x
    elif case in ("training", "dark"):
        x = 0.85 + 0.1 * torch.sin(xx / 9.0 + 0.5 * p) * torch.cos(yy / 7.0 + 0.3 * p)
        y = x + TRAIN_AMP * torch.randn(N, C, H, W, generator=g)
        if case == "dark":
            x, y = 0.05 * x, 0.05 * y
    elif case == "flat":
        x = torch.full((N, C, H, W), 0.7)
        y = torch.full((N, C, H, W), 0.703)
    elif case == "steps":
        # 5 x 5 blocks of constant level, shifted so that the first edges lie behind column 0 and row 1 (a 2 x 2 image is not
        # constant: on constant planes the oracle's fp32 pooling is exact by accident and its deviation says nothing about a
        # nine-term sum); the levels of y differ from those of x by 0.05 .. 0.15
        by, bx = ((yy + 3) // 5).long(), ((xx + 4) // 5).long()
        nb = (H + 6) // 5 + 1, (W + 7) // 5 + 1
        lx = 0.2 + 0.6 * torch.rand(N, C, *nb, generator=g)
        d = (0.05 + 0.1 * torch.rand(N, C, *nb, generator=g)) * (2.0 * torch.randint(0, 2, (N, C, *nb), generator=g) - 1.0)
        idx = (by * nb[1] + bx).expand(N, C, H, W).reshape(N, C, -1)
        x = lx.reshape(N, C, -1).gather(2, idx).view(N, C, H, W)
        y = x + d.reshape(N, C, -1).gather(2, idx).view(N, C, H, W)
    elif case == "signed":
        # left two thirds: opposite offsets +-8 under a common small texture (value -> 1), signs swapped between the upper and
        # the lower half (both images zero-mean overall); right third: y = x + tiny noise around zero (value -> 0)
        u = 0.05 * torch.randn(N, C, H, W, generator=g)
        third = (3 * xx / W).floor().expand(N, C, H, W)
        s = torch.where(third == 2, 0.0, torch.where(yy < H / 2, 8.0, -8.0).expand(N, C, H, W))
        x = s + u
        y = torch.where(third == 2, u + 2e-5 * torch.randn(N, C, H, W, generator=g), -s + u)
    else:
        raise KeyError(case)
    return x.contiguous(), y.contiguous()


@functools.lru_cache(maxsize=None)
def cotangent(geom, mode, seed=0):
    """[N,C,H,W] (mode 0) or [N,1,H,W] (mode 1) normal deviates, zero on the quarter of the pixels with even row and column."""
    N, C, H, W = geom
    g = torch.Generator().manual_seed(77 + seed + sum(geom) + mode)
    w = torch.randn(N, C if mode == 0 else 1, H, W, generator=g)
    yy, xx, _ = _planes(N, C, H, W)
    return (w * ~((yy % 2 == 0) & (xx % 2 == 0))).contiguous()


def cot_zero(geom):
    yy, xx, _ = _planes(*geom)
    return ((yy % 2 == 0) & (xx % 2 == 0)).expand(geom)


# ====================================================================================================== references
def unclamped(x, y, dt):
    """oracle.losses.ssim without its clamp, same operations."""
    x, y = x.to(dt), y.to(dt)
    x = F.pad(x, (1, 1, 1, 1), mode="reflect")
    y = F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sx = F.avg_pool2d(x ** 2, 3, 1) - mu_x ** 2
    sy = F.avg_pool2d(y ** 2, 3, 1) - mu_y ** 2
    sxy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + 0.01 ** 2) * (2 * sxy + 0.03 ** 2)
    d = (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sx + sy + 0.03 ** 2)
    return (1 - n / d) / 2


def ref_ssim(x, y, dt):
    return ol.ssim(x.to(dt), y.to(dt))


def ref_mix(x, y, dt, no_ssim=False):
    """trainer.py:1069-1081: [N,1,H,W]."""
    x, y = x.to(dt), y.to(dt)
    l1 = (y - x).abs().mean(1, True)
    return l1 if no_ssim else 0.85 * ol.ssim(x, y).mean(1, True) + 0.15 * l1


def ref_out(x, y, dt, mode, no_ssim=False):
    return ref_ssim(x, y, dt) if mode == 0 else ref_mix(x, y, dt, no_ssim)


def ref_grads(x, y, cot, dt, mode, no_ssim=False):
    """Autograd of sum(cot * out) for both images."""
    xr, yr = x.to(dt).clone().requires_grad_(True), y.to(dt).clone().requires_grad_(True)
    (ref_out(xr, yr, dt, mode, no_ssim) * cot.to(dt)).sum().backward()
    return xr.grad, yr.grad


def gate_margin(x, y):
    return 4.0 * (ref_ssim(x, y, F32).double() - ref_ssim(x, y, F64)).abs().max().item()


def gate_undecided(x, y, dilate=False):
    """[N,C,H,W] bool: the fp64 unclamped value lies within 4 max|ref32 - ref64| of 0 or 1; dilate: by the 5 x 5 footprint of
    the gather pass (the pixels whose gradient hears of such a window)."""
    u = unclamped(x, y, F64)
    m = gate_margin(x, y)
    und = (u.abs() <= m) | ((u - 1).abs() <= m)
    if dilate:
        und = F.max_pool2d(und.double(), 5, 1, 2) > 0
    return und


def beyond_clamp(x, y):
    """Pixels whose fp64 unclamped value is outside [0, 1] by more than the undecided margin (none, see the module docstring)."""
    u = unclamped(x, y, F64)
    m = gate_margin(x, y)
    return (u < -m) | (u > 1 + m)


def grad_keep(x, y, mode, no_ssim=False):
    """Elements whose gradient is compared: outside the dilated undecided set; mode 1: off the L1 kink x == y, if any."""
    keep = torch.ones_like(x, dtype=torch.bool) if no_ssim else ~gate_undecided(x, y, dilate=True)
    if mode == 1 and (x == y).any():
        keep = keep & (x != y)
    return keep


# ====================================================================================================== the checks
def fig(what, err, tol, ratio=None, excluded=None):
    r = "     -" if ratio is None else f"{ratio:6.3f}"
    e = "     -" if excluded is None else f"{excluded:6.4f}"
    print(f"SSIMFIG | {what:<58} | err {err:.2e} | tol {tol:.2e} | mean ratio {r} | excluded {e}")


def mean_ratio(dev, r32, r64, keep=None):
    dev, r32, r64 = (torch.as_tensor(a).detach().cpu().double() for a in (dev, r32, r64))
    if keep is not None:
        dev, r32, r64 = dev[keep], r32[keep], r64[keep]
    den = (r32 - r64).abs().mean().item()
    return (dev - r64).abs().mean().item() / den if den > 0 else 0.0, dev.numel()


def check_forward(dev, case, geom, mode, no_ssim=False):
    """The rule on a forward result; on MEAN_CASES at the statistics shape the mean condition too.  Returns the mean ratio."""
    x, y = make(case, geom)
    r32, r64 = ref_out(x, y, F32, mode, no_ssim), ref_out(x, y, F64, mode, no_ssim)
    what = f"fwd {case} {geom} mode {mode}" + (" no_ssim" if no_ssim else "")
    err, tol = assert_elem(dev, r32, r64, what)
    ratio = None
    if case in MEAN_CASES and geom == STAT and not no_ssim:
        ratio, n = mean_ratio(dev, r32, r64)
        assert n * (geom[1] if mode == 1 else 1) >= MEAN_MIN
        fig(what, err, tol, ratio)
        assert ratio <= MEAN_MARGIN, f"{what}: mean error {ratio:.3f} x the fp32 oracle's (margin {MEAN_MARGIN})"
    else:
        fig(what, err, tol)
    return ratio


def check_backward(gx, gy, case, geom, mode, no_ssim=False):
    """gx, gy against fp64 autograd outside the exclusion; separately on the pixels whose own cotangent is zero (they hear
    only of their neighbours); the mean condition on MEAN_CASES at the statistics shape.  Returns the worst mean ratio."""
    x, y = make(case, geom)
    cot = cotangent(geom, mode)
    keep = grad_keep(x, y, mode, no_ssim)
    excluded = 1.0 - keep.double().mean().item()
    assert excluded <= EXCLUDED_CAP, f"{case} {geom}: {excluded:.4f} of the gradient excluded"
    g32, g64 = ref_grads(x, y, cot, F32, mode, no_ssim), ref_grads(x, y, cot, F64, mode, no_ssim)
    zero = cot_zero(geom) & keep
    worst = None
    for name, dev, r32, r64 in (("gx", gx, g32[0], g64[0]), ("gy", gy, g32[1], g64[1])):
        what = f"bwd {name} {case} {geom} mode {mode}" + (" no_ssim" if no_ssim else "")
        dev = torch.as_tensor(dev).detach().cpu()
        assert dev.shape == r64.shape and torch.isfinite(dev).all(), what
        # the tolerance comes from the compared elements alone
        err, tol = assert_elem(dev[keep], r32[keep], r64[keep], what)
        if not no_ssim and min(geom[2:]) > 2:
            assert (r64[zero] != 0).double().mean().item() > 0.9          # neighbours reach the pixels without a cotangent
        ez = (dev[zero].double() - r64[zero]).abs().max().item() if zero.any() else 0.0
        assert ez <= tol, f"{what}: zero-cotangent pixels off by {ez:.3e} > {tol:.3e}"
        ratio = None
        if case in MEAN_CASES and geom == STAT and not no_ssim:
            ratio, n = mean_ratio(dev, r32, r64, keep)
            assert n >= MEAN_MIN
            assert ratio <= MEAN_MARGIN, f"{what}: mean error {ratio:.3f} x the fp32 oracle's (margin {MEAN_MARGIN})"
            worst = ratio if worst is None else max(worst, ratio)
        fig(what, err, tol, ratio, excluded)
    return worst


def check_mode1_from_mode0(out1, out0, x, y, what):
    """mode 1 = 0.85 mean_c(mode 0) + 0.15 mean_c |y - x| recomputed in fp64 from the device's own mode-0 map; a division by C,
    two products and a sum: 4 * 2^-24 * max(1, max|.|)."""
    out0, out1 = torch.as_tensor(out0).cpu().double(), torch.as_tensor(out1).cpu().double()
    want = 0.85 * out0.mean(1, True) + 0.15 * (y.double() - x.double()).abs().mean(1, True)
    bound = 4 * 2.0 ** -24 * max(1.0, want.abs().max().item())
    err = (out1 - want).abs().max().item()
    fig(what, err, bound)
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


# ====================================================================================================== transcription
_f = np.float32


def _reflect(i, n, wrong=False):
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= n, (2 * n - 1 - i) if wrong else (2 * n - 2 - i), i))


def _window_sums(x, y, mut):
    """The five 3 x 3 sums in the kernels' tap order (dy outer, dx inner), accumulated in fp32 (mutation: fp16)."""
    H, W = x.shape[-2:]
    acc = np.float16 if mut == "fp16_sums" else _f
    rows, cols = np.arange(H), np.arange(W)
    s = [np.zeros(x.shape, acc) for _ in range(5)]
    for dy in (-1, 0, 1):
        ry = _reflect(rows + dy, H, mut == "reflect")
        for dx in (-1, 0, 1):
            rx = _reflect(cols + dx, W, mut == "reflect")
            a = x[..., ry[:, None], rx[None, :]].astype(acc)
            b = y[..., ry[:, None], rx[None, :]].astype(acc)
            s[0] = s[0] + a; s[1] = s[1] + b; s[2] = s[2] + a * a; s[3] = s[3] + b * b; s[4] = s[4] + a * b
    return [v.astype(_f) for v in s]


def _terms(x, y, mut):
    sx, sy, sxx, syy, sxy = _window_sums(x, y, mut)
    k = _f(1) / _f(8 if mut == "k8" else 9)
    mx, my = sx * k, sy * k
    vx, vy, vxy = sxx * k - mx * mx, syy * k - my * my, sxy * k - mx * my
    a, b = _f(2) * mx * my + _f(1e-4), _f(2) * vxy + _f(9e-4)
    c, e = mx * mx + my * my + _f(1e-4), vx + vy + _f(9e-4)
    return mx, my, a, b, c, e


def emulate_fwd(x, y, mode, no_ssim=False, mut=None):
    """ssim_kernel in NumPy fp32, operation by operation (the library is built without fused multiply-adds)."""
    x, y = x.numpy(), y.numpy()
    C = x.shape[1]
    with np.errstate(all="ignore"):
        _, _, a, b, c, e = _terms(x, y, mut)
        v = (_f(1) - (a * b) / (c * e)) * _f(0.5)
        v = np.where(v != v, v, np.minimum(np.maximum(v, _f(0)), _f(1)))
        if mode == 0:
            return torch.from_numpy(v)
        s_ssim, s_l1 = np.zeros_like(v[:, 0]), np.zeros_like(v[:, 0])
        for ch in range(C):
            s_ssim = s_ssim + v[:, ch]
            s_l1 = s_l1 + np.abs(y[:, ch] - x[:, ch])
        l1 = s_l1 / _f(C)
        out = l1 if no_ssim else _f(0.85) * (s_ssim / _f(C)) + _f(0.15) * l1
    return torch.from_numpy(out[:, None].astype(_f))


def emulate_bwd(x, y, gout, mode, no_ssim=False, mut=None):
    """ssim_bwd_a_kernel and ssim_bwd_b_kernel in NumPy fp32 -> (gx, gy)."""
    x, y, gout = x.numpy(), y.numpy(), gout.numpy()
    N, C, H, W = x.shape
    ax, ay = np.zeros_like(x), np.zeros_like(x)
    with np.errstate(all="ignore"):
        if not no_ssim:
            mx, my, a, b, c, e = _terms(x, y, mut)
            nn, dd = a * b, c * e
            f = (_f(1) - nn / dd) * _f(0.5)
            g = gout if mode == 0 else np.broadcast_to(gout * (_f(0.85) / _f(C)), x.shape)
            g = np.where((f > 0) & (f < 1), g, _f(0)).astype(_f)
            s = _f(-0.5) * g / (dd * dd)
            cf = [s * (_f(2) * my * (b - a) * dd - nn * (_f(2) * mx * (e - c))),
                  s * (_f(2) * mx * (b - a) * dd - nn * (_f(2) * my * (e - c))),
                  s * (-nn * c), s * (-nn * c), s * (_f(2) * a * dd)]
            rows, cols = np.arange(H), np.arange(W)

            def mults(n, idx):      # [5, n]: taps of window idx + o (o = -2 .. 2) that land on idx, 0 where the window is outside
                out = np.zeros((5, n), np.int64)
                for o in range(-2, 3):
                    q = idx + o
                    ok = (q >= 0) & (q < n)
                    for d in (-1, 0, 1):
                        out[o + 2] += ok & (_reflect(q + d, n, mut == "reflect") == idx)
                return out
            My, Mx = mults(H, rows), mults(W, cols)
            for oy in range(-2, 3):
                qy = np.clip(rows + oy, 0, H - 1)
                for ox in range(-2, 3):
                    qx = np.clip(cols + ox, 0, W - 1)
                    m = My[oy + 2][:, None] * Mx[ox + 2][None, :]
                    if mut == "no_mult":
                        m = np.minimum(m, 1)
                    m = m.astype(_f)
                    q = [v[..., qy[:, None], qx[None, :]] for v in cf]
                    ax = ax + m * (q[0] + _f(2) * x * q[2] + y * q[4])
                    ay = ay + m * (q[1] + _f(2) * y * q[3] + x * q[4])
            ax, ay = ax * (_f(1) / _f(9)), ay * (_f(1) / _f(9))
        if mode == 1:
            g1 = gout * (_f(1.0 if no_ssim else 0.15) / _f(C))
            sg = np.where(x > y, _f(1), np.where(x < y, _f(-1), _f(0)))
            ax, ay = ax + g1 * sg, ay - g1 * sg
    return torch.from_numpy(ax.astype(_f)), torch.from_numpy(ay.astype(_f))


MUTATIONS = ("reflect", "k8", "no_mult", "fp16_sums")
