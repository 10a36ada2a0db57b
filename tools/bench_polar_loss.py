"""The polarimetric normals loss (pd_polar_loss_fwd + pd_polar_loss_bwd, csrc/polar_loss.hip) at the training sizes: B = 12 at
320x480 and B = 16 at 512x640, DoLP-weighted, no ``valid`` map, no per-pixel maps.

ms per forward + backward pair with HIP events, warm: one event pair per pair of calls, median of ``--iters``, every pair on
another of ``--sets`` rotating input sets (sized past the 256 MB Infinity Cache; state, sums, workspace and the gradient are
allocated once).  GB/s from the bytes the algorithm touches, counted here from the shapes -- forward 45 bytes per pixel (depth
4, nine candidate planes 36, DoLP 4, state 1 written), backward 49 (the same reads, state read instead of written, gdepth 4
written; the backward reads only the candidates the state names, the count charges all nine: neighbouring pixels name
different ones and a cache line is fetched whole) -- next to a device copy that moves the SAME number of bytes (half read,
half written, rotating buffers, the same timing).  Then, in the same run and on the same inputs, the same loss written with
torch ops (fp32, Sobel by F.conv2d, the six cosines, max, the azimuth branch, two weighted means) under autograd, forward +
backward, and how far its two values are from the kernel's.  ``--step``: the supervised training step of a Trainer at that
size on synthetic items with and without ``opt.polar_loss``, for the share the term adds.  One JSON line per measurement,
printed and written to ``--out`` (default: profiles/polar_loss.log).  ``--ray_frame``: after the orthographic pair, in the same
run and on the same rotating sets, pd_polar_loss_fwd_ray + pd_polar_loss_bwd_ray with ray_frame = 1 are timed the same way
(``ray_ms`` with its min..max, ``ray_fwd_ms``, ``ray_bwd_ms``, the ratio to the orthographic pair, the two values), and with
``--step`` the training step with ``opt.polar_ray_frame`` too.  It needs the GPU: there is no CPU fallback."""
import argparse
import json
import math
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

SIZES = ((12, 320, 480), (16, 512, 640))
FWD_BYTES = {"depth": 4, "pol_normals": 36, "dolp": 4, "state": 1}
BWD_BYTES = {"depth": 4, "pol_normals": 36, "dolp": 4, "state": 1, "gdepth": 4}
RHO_MIN, RHO_MAX = 0.05, 1.0
TILT2 = math.sin(math.radians(5.0)) ** 2


def bytes_touched(N, H, W):
    """(forward, backward) bytes of one call, from the shapes."""
    return N * H * W * sum(FWD_BYTES.values()), N * H * W * sum(BWD_BYTES.values())


def _median_ms(call, iters):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (e0, e1) in enumerate(evs):
        e0.record()
        call(i)
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[iters // 2], ts[0], ts[-1]


def _copy_ms(moved, sets, iters):
    import torch
    half = moved // 2
    src = [torch.empty(half, dtype=torch.uint8, device="cuda").fill_(s + 1) for s in range(sets)]
    dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    copy = lambda i: dst[i % sets].copy_(src[i % sets])
    for i in range(sets):
        copy(i)
    torch.cuda.synchronize()
    return _median_ms(copy, iters)[0]


def make_set(N, H, W, seed):
    """One input set on the device: a smooth depth surface with 1 % noise, the intrinsics of polardepth.synthetic, a smooth
    DoLP / AoLP field with a few unpolarised pixels and K1's own nine normals for it."""
    import torch
    from polardepth import polar as pdpolar
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = np.stack([1.0 + 0.4 * np.sin(xx / 61.0 + rng.uniform(0, 6)) * np.cos(yy / 47.0 + rng.uniform(0, 6)) for _ in range(N)])
    depth = (depth + 0.01 * rng.random((N, H, W))).astype(np.float32)[:, None]
    K = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = 0.65 * W
    K[:, 0, 2], K[:, 1, 2] = W / 2, H / 2
    rho = np.stack([0.3 + 0.25 * np.sin(xx / 37.0 + rng.uniform(0, 6)) * np.cos(yy / 29.0 + rng.uniform(0, 6))
                    for _ in range(N)]).astype(np.float32)
    rho[rng.random((N, H, W)) < 0.02] = 0.01
    phi = np.stack([1.5 * np.sin(xx / 53.0 + rng.uniform(0, 6)) * np.sin(yy / 41.0 + rng.uniform(0, 6)) for _ in range(N)])
    xolp = torch.from_numpy(np.stack([rho, phi.astype(np.float32)], 1)).cuda()
    return torch.from_numpy(depth).cuda(), torch.from_numpy(K).cuda(), pdpolar.normals_from_xolp(xolp), xolp


def torch_loss(depth, K, pol, xolp, rho_min=RHO_MIN, rho_max=RHO_MAX, tilt2=TILT2):
    """The same two values with torch ops in fp32, differentiable in depth: the decisions are made with comparisons and max,
    whose autograd treats the winner as data."""
    import torch
    import torch.nn.functional as F
    N, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float32),
                            torch.arange(W, device=depth.device, dtype=torch.float32), indexing="ij")
    X = (xs[None] - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None] * depth[:, 0]
    Y = (ys[None] - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None] * depth[:, 0]
    xyz = torch.stack([X, Y, depth[:, 0]], 1).reshape(N * 3, 1, H, W)
    kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device=depth.device) / 8.0
    g = F.conv2d(F.pad(xyz, (1, 1, 1, 1), mode="replicate"), torch.stack([kx, kx.t()])[:, None]).view(N, 3, 2, H, W)
    p = F.normalize(torch.cross(g[:, :, 0], g[:, :, 1], dim=1), dim=1)
    rho = xolp[:, 0]
    C = pol.view(N, 3, 3, H, W)
    cx, cy, cz = C[:, :, 0], C[:, :, 1], C[:, :, 2]
    a2 = (p * p).sum(1)
    b2 = cx * cx + cy * cy + cz * cz
    ok = torch.isfinite(rho) & (rho >= rho_min) & (rho <= rho_max) & (a2 > 0) & torch.isfinite(C).all(2).all(1) & (b2 > 0).any(1)
    p = p * torch.where(p[:, 2:3] < 0, -1.0, 1.0)
    px, py, pz = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    m, q = px * cx + py * cy, pz * cz
    den = (a2.sqrt()[:, None] * b2.sqrt()).clamp(min=1e-30)
    c6 = torch.cat([(m + q) / den, (-m + q) / den], 1)
    c6 = torch.where((b2 > 0).repeat(1, 2, 1, 1), c6, torch.full_like(c6, -2.0))
    l_n = 1.0 - c6.max(1).values.clamp(-1.0, 1.0)
    t2 = (px * px + py * py)[:, 0]
    u2 = (cx * cx + cy * cy)[:, :2]
    ca = ok & ~((t2 <= tilt2 * a2) | ~(u2 > 0).any(1))
    m2 = (px * cx[:, :2] + py * cy[:, :2]) ** 2 / (t2[:, None] * u2).clamp(min=1e-30)
    m2 = torch.where(u2 > 0, m2, torch.full_like(m2, -1.0))
    l_a = (1.0 - m2.max(1).values).clamp(0.0, 1.0)
    wn, wa = rho * ok, rho * ca
    zero = torch.zeros_like(l_n)
    return (wn * torch.where(ok, l_n, zero)).sum() / wn.sum(), (wa * torch.where(ca, l_a, zero)).sum() / wa.sum()


def _step_ms(N, H, W, iters, polar_loss, ray_frame=False):
    """One supervised training step (zero_grad .. Adam) of a Trainer on synthetic items, median of ``iters``."""
    import torch
    from manydepth.options import MonodepthOptions
    from manydepth.trainer import Trainer
    with tempfile.TemporaryDirectory() as tmp:
        opt = MonodepthOptions().parse([
            "--png", "--batch_size", str(N), "--height", str(H), "--width", str(W), "--dataset", "HAMMER", "--split", "HAMMER",
            "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision_only", "True",
            "--depth_supervision", "True", "--augment_xolp", "--augment_normals", "--log_dir", tmp, "--data_path", "synthetic",
            "--data_path_val", "synthetic", "--num_workers", "0", "--weights_init", "scratch"])
        if polar_loss is not None:
            opt.polar_loss = polar_loss
        if ray_frame:
            opt.polar_ray_frame = True
        tr = Trainer(opt)
        tr.set_train()
        ds = tr.train_loader.dataset
        batch = torch.utils.data.default_collate([ds[i % len(ds)] for i in range(N)])
        batch = {k: v.cuda() for k, v in batch.items()}

        def step(_):
            tr.model_optimizer.zero_grad()
            _, losses, _ = tr.process_batch(dict(batch), is_train=True)
            losses["loss"].backward()
            tr.model_optimizer.step()
        for i in range(2):
            step(i)
        torch.cuda.synchronize()
        return _median_ms(step, iters)[0]


def time_loss(N, H, W, iters=24, sets=None, torch_iters=5, with_step=False, ray_frame=False):
    import torch
    from polardepth._lib import lib, check, ptr, stream_ptr
    if not torch.cuda.is_available():
        raise RuntimeError("bench_polar_loss needs the GPU; there is no CPU fallback")
    fwd_b, bwd_b = bytes_touched(N, H, W)
    moved = fwd_b + bwd_b
    sets = sets if sets is not None else max(2, min(12, -(-int(2.5 * 256e6) // moved)))
    data = [make_set(N, H, W, s) for s in range(sets)]
    state = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
    record = torch.empty(96, dtype=torch.uint8, device="cuda")
    values, g = torch.empty(2, device="cuda"), torch.tensor([0.5, 0.5], device="cuda")
    gdepth = torch.empty((N, 1, H, W), device="cuda")
    ws = torch.empty((lib.pd_polar_loss_rows(N, H, W), 11), dtype=torch.float64, device="cuda")

    def fwd(i):
        depth, K, pol, xolp = data[i % sets]
        check(lib.pd_polar_loss_fwd(ptr(depth), ptr(K), ptr(pol), ptr(xolp), W, None, RHO_MIN, RHO_MAX, TILT2, 1, 1, ptr(state),
                                    ptr(record), ptr(values), None, ptr(ws), ws.numel() * 8, N, H, W, stream_ptr()),
              "pd_polar_loss_fwd")

    def bwd(i):
        depth, K, pol, xolp = data[i % sets]
        check(lib.pd_polar_loss_bwd(ptr(depth), ptr(K), ptr(pol), ptr(xolp), W, ptr(state), ptr(g), ptr(record), 1, 1, ptr(gdepth),
                                    N, H, W, stream_ptr()), "pd_polar_loss_bwd")

    def both(i):
        fwd(i)
        bwd(i)

    def fwd_ray(i):
        depth, K, pol, xolp = data[i % sets]
        check(lib.pd_polar_loss_fwd_ray(ptr(depth), ptr(K), ptr(pol), ptr(xolp), W, None, RHO_MIN, RHO_MAX, TILT2, 1, 1, 1,
                                        ptr(state), ptr(record), ptr(values), None, ptr(ws), ws.numel() * 8, N, H, W,
                                        stream_ptr()), "pd_polar_loss_fwd_ray")

    def bwd_ray(i):
        depth, K, pol, xolp = data[i % sets]
        check(lib.pd_polar_loss_bwd_ray(ptr(depth), ptr(K), ptr(pol), ptr(xolp), W, ptr(state), ptr(g), ptr(record), 1, 1, 1,
                                        ptr(gdepth), N, H, W, stream_ptr()), "pd_polar_loss_bwd_ray")

    def both_ray(i):
        fwd_ray(i)
        bwd_ray(i)

    for i in range(sets):
        both(i)
    torch.cuda.synchronize()
    ms, ms_min, ms_max = _median_ms(both, iters)
    fwd_ms = _median_ms(fwd, iters)[0]
    fwd(0)
    bwd_ms = _median_ms(lambda i: bwd(0), iters)[0]          # the state of set 0 throughout
    ray = {}
    if ray_frame:
        for i in range(sets):
            both_ray(i)
        torch.cuda.synchronize()
        r_ms, r_min, r_max = _median_ms(both_ray, iters)
        rf_ms = _median_ms(fwd_ray, iters)[0]
        fwd_ray(0)
        rb_ms = _median_ms(lambda i: bwd_ray(0), iters)[0]
        both_ray(0)
        torch.cuda.synchronize()
        rv = values.cpu().numpy().astype(np.float64)
        ray = {"ray_ms": round(r_ms, 4), "ray_ms_min": round(r_min, 4), "ray_ms_max": round(r_max, 4),
               "ray_fwd_ms": round(rf_ms, 4), "ray_bwd_ms": round(rb_ms, 4), "ray_over_orthographic": round(r_ms / ms, 3),
               "ray_L_n": float(rv[0]), "ray_L_a": float(rv[1])}
    both(0)
    torch.cuda.synchronize()
    vals = values.cpu().numpy().astype(np.float64)
    cnt = record.view(torch.int64)[4:11].cpu().tolist()
    copy_ms = _copy_ms(moved, sets, iters)
    out = {"op": "polar_loss_fwd_bwd", "N": N, "H": H, "W": W, "sets": sets, "fwd_bytes": fwd_b, "bwd_bytes": bwd_b,
           "ms": round(ms, 4), "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4), "fwd_ms": round(fwd_ms, 4),
           "bwd_ms": round(bwd_ms, 4), "GBps": round(moved / (ms * 1e-3) / 1e9, 1),
           "fwd_GBps": round(fwd_b / (fwd_ms * 1e-3) / 1e9, 1), "bwd_GBps": round(bwd_b / (bwd_ms * 1e-3) / 1e9, 1),
           "copy_ms": round(copy_ms, 4), "copy_GBps": round(moved / (copy_ms * 1e-3) / 1e9, 1),
           "time_over_copy": round(ms / copy_ms, 2), "L_n": float(vals[0]), "L_a": float(vals[1]),
           "normal_pixels": cnt[0], "azimuth_pixels": cnt[1]}
    out.update(ray)

    def torch_pair(i):
        depth, K, pol, xolp = data[i % sets]
        d = depth.detach().requires_grad_(True)
        L_n, L_a = torch_loss(d, K, pol, xolp)
        (0.5 * L_n + 0.5 * L_a).backward()
        return L_n.detach(), L_a.detach()

    tn, ta = torch_pair(0)
    torch.cuda.synchronize()
    t_ms, t_min, _ = _median_ms(torch_pair, torch_iters)
    out.update({"torch_ms": round(t_ms, 3), "torch_ms_min": round(t_min, 3), "torch_over_call": round(t_ms / ms, 1),
                "torch_L_n_rel_diff": abs(float(tn) - vals[0]) / max(vals[0], 1e-30),
                "torch_L_a_rel_diff": abs(float(ta) - vals[1]) / max(vals[1], 1e-30)})
    if with_step:
        del data
        torch.cuda.empty_cache()
        step_iters = max(3, iters // 3)
        base, with_term = _step_ms(N, H, W, step_iters, None), _step_ms(N, H, W, step_iters, (0.5, 0.5))
        out.update({"supervised_step_ms": round(base, 3), "step_with_term_ms": round(with_term, 3),
                    "added_share_of_step": round((with_term - base) / base, 4)})
        if ray_frame:
            with_ray = _step_ms(N, H, W, step_iters, (0.5, 0.5), True)
            out.update({"step_with_ray_term_ms": round(with_ray, 3), "ray_added_share_of_step": round((with_ray - base) / base, 4)})
    else:
        out["supervised_step_ms"] = out["step_with_term_ms"] = out["added_share_of_step"] = "not measured"
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--sets", type=int, default=None)
    ap.add_argument("--step", action="store_true", help="also time the supervised training step with and without the term")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_loss.log"), help="the log; '' = print only")
    ap.add_argument("--ray_frame", action="store_true", help="also time the pair in the per-pixel viewing-ray frame")
    args = ap.parse_args()
    log = open(args.out, "w") if args.out else None
    for N, H, W in SIZES:
        line = json.dumps(time_loss(N, H, W, args.iters, args.sets, with_step=args.step, ray_frame=args.ray_frame))
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
    if log:
        log.close()
