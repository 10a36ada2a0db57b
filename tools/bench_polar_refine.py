"""The polarimetric depth refinement (csrc/polar_refine.hip) at B = 1 and B = 12 at 320x480 and B = 16 at 512x640.

Per shape, in one run and alternating the routes: pd_polar_refine_setup, pd_polar_refine_table, the ``--iters`` Chebyshev steps
on the one-step route (pd_polar_refine_step, a launch per step) and on the fused route (pd_polar_refine_steps with T = 8, 4
and 2 steps per launch), and pd_polar_refine_finish: ms with HIP events, warm, median of ``--reps``; the steps are timed as
the whole chain of launches, so the figure holds the launch gaps a caller pays.  Next to them a device copy that moves the
bytes ONE one-step iteration touches, counted here from the shapes -- per pixel wE, wS, rhs, idiag, zeta and d read (48 bytes),
zeta and d written (16) -- timed the same way, and the same step written with torch ops in fp64 on the same coefficients.
The fused route's result is compared with the one-step route's bit for bit at every size it is timed at.  One JSON line per
measurement, printed and written to ``--out`` (default: profiles/polar_refine.log).  It needs the GPU: there is no CPU
fallback.

``--weighted`` measures the per-pixel weight of the prior instead (default ``--out``: profiles/polar_refine_weighted.log), at
B = 12 at 320x480 and B = 16 at 512x640: pd_polar_refine_setup_w next to pd_polar_refine_setup, pd_polar_refine_weights (both
sources: 28 bytes per pixel) next to a device copy of its bytes, and the whole route -- ``polardepth.refine.solve`` without a
weight, with a weight made from the uncertainty (one more launch), and the two rounds of the robust route -- alternating in one
run."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

SIZES = ((1, 320, 480), (12, 320, 480), (16, 512, 640))
STEP_BYTES = 48 + 16                # per pixel and one-step iteration
LAM, EDGE_MAX, INCIDENCE_MAX_DEG = 0.02, 0.05, 80.0


def _median_ms(call, reps):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (e0, e1) in enumerate(evs):
        e0.record()
        call(i)
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[reps // 2], ts[0], ts[-1]


def make_inputs(N, H, W, seed=0):
    """(depth [N,H,W], K, normal [N,H,W,4], xolp [N,2,H,W]) on the device: a smooth surface with a depth step, noisy normals
    that face the camera, DoLP in 0.05 .. 0.9 with holes."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    depth = torch.stack([1.2 + 0.3 * torch.sin(xx / 61.0 + 0.7 * n) * torch.cos(yy / 47.0 + 0.3 * n) for n in range(N)])
    depth = depth + 0.4 * (xx + 0.5 * yy > 0.7 * W) + 0.002 * torch.randn(depth.shape, device="cuda", generator=g)
    normal = torch.randn((N, H, W, 4), device="cuda", generator=g) * 0.3
    normal[..., 2] -= 1.0
    rho = 0.05 + 0.85 * torch.rand((N, H, W), device="cuda", generator=g)
    rho = torch.where(torch.rand(rho.shape, device="cuda", generator=g) < 0.03, torch.zeros_like(rho), rho)
    xolp = torch.stack([rho, torch.rand(rho.shape, device="cuda", generator=g) * math.pi], 1).contiguous()
    K = torch.eye(4, device="cuda").repeat(N, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.58 * W, 0.8 * H, 0.5 * W - 0.8, 0.5 * H + 0.6
    return depth.contiguous(), K.contiguous(), normal.contiguous(), xolp


def torch_step(coef, alpha, beta, z, d, first):
    """One step with torch ops in fp64 (the same arithmetic; not the same bits where a rounding is reassociated)."""
    import torch
    import torch.nn.functional as F
    wE, wS, rhs, idiag = coef[:, 0], coef[:, 1], coef[:, 2], coef[:, 3]
    wW, wN = F.pad(wE, (1, 0))[..., :-1], F.pad(wS, (0, 0, 1, 0))[..., :-1, :]
    zE, zW = F.pad(z, (0, 1))[..., 1:], F.pad(z, (1, 0))[..., :-1]
    zS, zN = F.pad(z, (0, 0, 0, 1))[..., 1:, :], F.pad(z, (0, 0, 1, 0))[..., :-1, :]
    touched = ((wE + wW) + wS) + wN > 0
    r = torch.where(touched, (rhs + (((wE * zE + wW * zW) + wS * zS) + wN * zN)) * idiag - z, torch.zeros_like(z))
    d = beta * r if first else alpha * d + beta * r
    return z + d, d


def bench(N, H, W, iters, reps, emit):
    import torch
    from polardepth._lib import lib, check, ptr, stream_ptr
    depth, K, normal, xolp = make_inputs(N, H, W)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    zeta0, coef, S, table = f64(N, H, W), f64(N, 4, H, W), f64(N), f64(N, iters, 2)
    zs, ds = [f64(N, H, W) for _ in range(2)], [f64(N, H, W) for _ in range(2)]
    out, touched, residual = torch.empty_like(depth), torch.empty((N, H, W), dtype=torch.uint8, device="cuda"), f64(N)
    ws = torch.empty(int(lib.pd_polar_refine_workspace(N, H, W)), dtype=torch.uint8, device="cuda")
    cos_inc = math.cos(math.radians(INCIDENCE_MAX_DEG))
    st = stream_ptr()
    px = N * H * W

    def setup(_):
        check(lib.pd_polar_refine_setup(ptr(depth), ptr(K), ptr(normal), ptr(xolp), W, None, LAM, EDGE_MAX, cos_inc, ptr(zeta0),
                                        ptr(coef), None, ptr(ws), ws.numel(), N, H, W, st), "setup")

    def tab(_):
        check(lib.pd_polar_refine_table(ptr(ws), ws.numel(), LAM, iters, ptr(S), ptr(table), N, H, W, st), "table")

    def one_step(_):
        src, dst = zeta0, zs[0]
        for k in range(iters):
            check(lib.pd_polar_refine_step(ptr(coef), ptr(table), iters, k, ptr(src), ptr(dst), ptr(ds[0]), N, H, W, st), "step")
            src, dst = dst, (zs[1] if dst is zs[0] else zs[0])
        return src

    def fused(T):
        def run(_):
            src, dst, di, do = zeta0, zs[0], None, ds[0]
            for k in range(0, iters, T):
                check(lib.pd_polar_refine_steps(ptr(coef), ptr(table), iters, k, min(T, iters - k), ptr(src), ptr(dst), ptr(di),
                                                ptr(do), N, H, W, st), "steps")
                src, dst = dst, (zs[1] if dst is zs[0] else zs[0])
                di, do = do, (ds[1] if do is ds[0] else ds[0])
            return src
        return run

    def finish(_):
        check(lib.pd_polar_refine_finish(ptr(depth), ptr(coef), ptr(zs[0]), ptr(out), ptr(touched), ptr(residual), ptr(ws),
                                         ws.numel(), N, H, W, st), "finish")

    setup(0)
    tab(0)
    want = one_step(0).clone()
    equal = {T: bool(torch.equal(fused(T)(0).view(torch.int64), want.view(torch.int64))) for T in (8, 4, 2)}
    finish(0)
    torch.cuda.synchronize()
    base = {"shape": [N, H, W], "iters": iters, "touched_share": float(touched.float().mean()), "residual_max": float(residual.max())}
    emit(dict(base, what="fused_equals_one_step_bits", **{f"T{T}": v for T, v in equal.items()}))

    for name, call in (("setup", setup), ("table", tab), ("finish", finish)):
        call(0)
        ms = _median_ms(call, reps)
        emit(dict(base, what=name, ms=ms[0], ms_min=ms[1], ms_max=ms[2]))
    # the routes alternate rep by rep inside one timed window each: the same minutes of the same machine
    routes = [("one_step", one_step)] + [(f"fused_T{T}", fused(T)) for T in (8, 4, 2)]
    for _, call in routes:
        call(0)
    times = {name: [] for name, _ in routes}
    for _ in range(reps):
        for name, call in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(0)
            e1.record()
            times[name].append((e0, e1))
    torch.cuda.synchronize()
    med = {}
    for name, evs in times.items():
        ts = sorted(a.elapsed_time(b) for a, b in evs)
        med[name] = ts[len(ts) // 2]
        emit(dict(base, what=f"steps_{name}", ms=med[name], ms_min=ts[0], ms_max=ts[-1], us_per_step=1e3 * med[name] / iters,
                  gbps_of_one_step_bytes=px * STEP_BYTES * iters / (med[name] * 1e-3) / 1e9))
    # a device copy of the bytes one one-step iteration touches: half read, half written
    half = px * STEP_BYTES // 2
    a, b = torch.empty(half, dtype=torch.uint8, device="cuda").fill_(1), torch.empty(half, dtype=torch.uint8, device="cuda")
    b.copy_(a)
    ms = _median_ms(lambda _: b.copy_(a), max(reps, 20))
    emit(dict(base, what="copy_of_one_step_bytes", bytes=2 * half, ms=ms[0], us=1e3 * ms[0], gbps=2 * half / (ms[0] * 1e-3) / 1e9,
              one_step_over_copy=(med["one_step"] / iters) / ms[0], fused_T8_over_copy=(med["fused_T8"] / iters) / ms[0]))
    del a, b
    # the same step with torch ops in fp64
    tab_h = table.cpu()
    alphas, betas = tab_h[:, :, 0].cuda(), tab_h[:, :, 1].cuda()
    n_t = min(iters, 10)

    def torch_steps(_):
        z, d = zeta0, None
        for k in range(n_t):
            z, d = torch_step(coef, alphas[:, k, None, None], betas[:, k, None, None], z, d, k == 0)
        return z
    got = torch_steps(0)
    src, dst = zeta0, zs[0]
    for k in range(n_t):
        check(lib.pd_polar_refine_step(ptr(coef), ptr(table), iters, k, ptr(src), ptr(dst), ptr(ds[0]), N, H, W, st), "step")
        src, dst = dst, (zs[1] if dst is zs[0] else zs[0])
    diff = float((got - src).abs().max())
    ms = _median_ms(torch_steps, max(3, reps // 2))
    emit(dict(base, what="steps_torch_fp64", steps=n_t, ms=ms[0], us_per_step=1e3 * ms[0] / n_t, max_abs_diff_to_kernel=diff))


WEIGHT_BYTES = 4 + 4 + 8 + 8 + 4          # per pixel: depth, b, zeta_prev, zeta0 read, the weight written


def _alternate(routes, reps):
    """{name: (median, min, max) ms} of the calls, alternating rep by rep inside one window."""
    import torch
    for call in routes.values():
        call()
    evs = {name: [] for name in routes}
    for _ in range(reps):
        for name, call in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            evs[name].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for name, pairs in evs.items():
        ts = sorted(a.elapsed_time(b) for a, b in pairs)
        out[name] = (ts[len(ts) // 2], ts[0], ts[-1])
    return out


def bench_weighted(N, H, W, iters, reps, emit):
    import torch
    from polardepth import refine
    from polardepth._lib import lib, check, ptr, stream_ptr
    depth, K, normal, xolp = make_inputs(N, H, W)
    g = torch.Generator(device="cuda").manual_seed(1)
    b = (0.002 + 0.02 * torch.rand(depth.shape, device="cuda", generator=g)).contiguous()       # 2 .. 22 mm
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    zeta0, coef = f64(N, H, W), f64(N, 4, H, W)
    ws = torch.empty(int(lib.pd_polar_refine_workspace(N, H, W)), dtype=torch.uint8, device="cuda")
    cos_inc = math.cos(math.radians(INCIDENCE_MAX_DEG))
    st = stream_ptr()
    px = N * H * W
    base = {"shape": [N, H, W], "iters": iters}
    wmap = refine.weights(depth, b)

    def setup():
        check(lib.pd_polar_refine_setup(ptr(depth), ptr(K), ptr(normal), ptr(xolp), W, None, LAM, EDGE_MAX, cos_inc, ptr(zeta0),
                                        ptr(coef), None, ptr(ws), ws.numel(), N, H, W, st), "setup")

    def setup_w():
        check(lib.pd_polar_refine_setup_w(ptr(depth), ptr(K), ptr(normal), ptr(xolp), W, None, LAM, EDGE_MAX, cos_inc, ptr(wmap),
                                          1 / 16, 1.0, ptr(zeta0), ptr(coef), None, ptr(ws), ws.numel(), N, H, W, st), "setup_w")

    ms = _alternate({"setup": setup, "setup_w": setup_w}, max(reps, 20))
    emit(dict(base, what="setup_w_next_to_setup", setup_ms=ms["setup"][0], setup_w_ms=ms["setup_w"][0],
              setup_w_over_setup=ms["setup_w"][0] / ms["setup"][0], setup_minmax=ms["setup"][1:], setup_w_minmax=ms["setup_w"][1:]))

    zprev, wout = zeta0 + 0.004 * torch.randn(zeta0.shape, device="cuda", dtype=torch.float64, generator=g), torch.empty_like(depth)
    half = px * WEIGHT_BYTES // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda").fill_(1), torch.empty(half, dtype=torch.uint8, device="cuda")

    def weights():
        check(lib.pd_polar_refine_weights(ptr(depth), ptr(b), 0.002, ptr(zprev), ptr(zeta0), 0.005, ptr(wout), N, H, W, st), "weights")

    ms = _alternate({"weights": weights, "copy": lambda: dst.copy_(src)}, max(reps, 20))
    emit(dict(base, what="weights_next_to_a_copy_of_its_bytes", bytes=2 * half, weights_us=1e3 * ms["weights"][0],
              copy_us=1e3 * ms["copy"][0], weights_over_copy=ms["weights"][0] / ms["copy"][0],
              weights_gbps=2 * half / (ms["weights"][0] * 1e-3) / 1e9, copy_gbps=2 * half / (ms["copy"][0] * 1e-3) / 1e9))
    del src, dst

    args = (depth, K, normal, xolp, W, None, LAM, iters, EDGE_MAX, INCIDENCE_MAX_DEG)

    def scalar():
        return refine.solve(*args)

    def weighted():
        return refine.solve(*args, weight=refine.weights(depth, b))

    def robust():
        z0 = f64(N, H, W)
        zeta = refine.solve(*args, zeta0_out=z0)[3]
        return refine.solve(*args, weight=refine.weights(depth, None, 0.002, zeta, z0, 0.005))

    ones = refine.solve(*args, weight=torch.ones_like(depth))
    equal = all(bool(torch.equal(x, y)) for x, y in zip(ones, scalar()))
    res = {"scalar": float(scalar()[1].max()), "weighted": float(weighted()[1].max()), "robust": float(robust()[1].max())}
    ms = _alternate({"scalar": scalar, "weighted": weighted, "robust_two_rounds": robust}, reps)
    emit(dict(base, what="route", weight_one_equals_scalar_bits=equal, scalar_ms=ms["scalar"][0], weighted_ms=ms["weighted"][0],
              robust_two_rounds_ms=ms["robust_two_rounds"][0], weighted_over_scalar=ms["weighted"][0] / ms["scalar"][0],
              robust_over_two_scalar=ms["robust_two_rounds"][0] / (2 * ms["scalar"][0]), scalar_minmax=ms["scalar"][1:],
              weighted_minmax=ms["weighted"][1:], residual_max=res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--weighted", action="store_true", help="measure the per-pixel weight of the prior instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "polar_refine_weighted.log" if args.weighted else "polar_refine.log")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_polar_refine.py needs the GPU: there is no CPU fallback")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for N, H, W in SIZES[1:] if args.weighted else SIZES:
            (bench_weighted if args.weighted else bench)(N, H, W, args.iters, args.reps, emit)


if __name__ == "__main__":
    main()
