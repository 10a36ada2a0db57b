"""The depth-uncertainty kernels at the training sizes, B = 12 at 320x480 and B = 16 at 512x640.

The loss (pd_unc_loss_fwd + pd_unc_loss_bwd + pd_up_gather_bwd, csrc/unc_loss.hip) with the uncertainty map at full resolution
(scale 0, the largest head), no ``valid`` map, no per-pixel maps: ms per forward + backward with HIP events, warm, one event
pair per pair of calls, median of ``--iters``, every pair on another of ``--sets`` rotating input sets (sized past the 256 MB
Infinity Cache).  GB/s from the bytes the algorithm touches, counted here from the shapes -- forward 12 bytes per pixel (depth,
gt, u), backward 20 (the same reads, gdepth and g_up written), the fold 8 (g_up read, the head's gradient written) -- next to a
device copy that moves the SAME number of bytes (half read, half written, rotating buffers, the same timing), and next to the
same loss written with torch ops in fp32 under autograd on the same inputs.

The evaluator (pd_unc_stats, csrc/unc_stats.hip) with the twelve default classes: 16 bytes per pixel read (gt, pred, u, mask),
next to the copy and next to pd_depth_stats (12 bytes per pixel) in the same run and on the same inputs.

``--step``: the supervised training step of a Trainer at that size on synthetic items without ``opt.uncertainty_loss`` (the
step of the commit before the term existed: without the option nothing changes in a bit), with it, and with
``opt.uncertainty_detach`` too.  With the option the decoder carries the uncertainty heads and gives up the ELU mailbox fusion
of its activation gradients, so the difference holds that as well as the term.  One JSON line per measurement, printed and
written to ``--out`` (default: profiles/uncertainty.log).  It needs the GPU: there is no CPU fallback."""
import argparse
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

SIZES = ((12, 320, 480), (16, 512, 640))
LOSS_BYTES = 12 + 20 + 8            # forward, backward, fold: per pixel
STATS_BYTES, DEPTH_STATS_BYTES = 16, 12
B_RANGE = (0.0005, 0.5)
MIN_D, MAX_D = 0.1, 2.0


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
    """(depth, gt, u, mask) on the device: a smooth surface with holes, a prediction whose error follows the stated scale."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    gt = torch.stack([1.0 + 0.4 * torch.sin(xx / 61.0 + 0.7 * n + seed) * torch.cos(yy / 47.0 + 0.3 * n) for n in range(N)])[:, None]
    gt = torch.where(torch.rand(gt.shape, device="cuda", generator=g) < 0.05, torch.zeros_like(gt), gt)
    u = 0.2 + 0.5 * torch.rand(gt.shape, device="cuda", generator=g)
    b = torch.exp(math.log(B_RANGE[0]) + u * math.log(B_RANGE[1] / B_RANGE[0]))
    e = torch.rand(gt.shape, device="cuda", generator=g) - 0.5
    depth = (gt + b * -torch.sign(e) * torch.log1p(-2 * e.abs())).clamp(MIN_D, MAX_D)
    mask = (torch.randint(0, 11, gt.shape, device="cuda", generator=g) * 20).int()
    return depth.contiguous(), gt.contiguous(), u.contiguous(), mask


def torch_loss(depth, gt, u):
    """The same value with torch ops in fp32, differentiable in depth and u."""
    import torch
    m = (gt >= MIN_D) & (gt <= MAX_D)
    logb = math.log(B_RANGE[0]) + u * math.log(B_RANGE[1] / B_RANGE[0])
    term = (gt - depth).abs() * torch.exp(-logb) + logb + math.log(2.0)
    return torch.where(m, term, torch.zeros_like(term)).sum() / m.sum()


def _step_ms(N, H, W, iters, weight, detach=False):
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
        if weight is not None:
            opt.uncertainty_loss = weight
            opt.uncertainty_detach = detach
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


def time_size(N, H, W, iters=24, sets=None, torch_iters=5, with_step=False):
    import torch
    from polardepth import depth_eval, uncertainty_eval
    from polardepth._lib import lib, check, ptr, stream_ptr
    if not torch.cuda.is_available():
        raise RuntimeError("bench_uncertainty needs the GPU; there is no CPU fallback")
    P = N * H * W
    moved = P * LOSS_BYTES
    sets = sets if sets is not None else max(2, min(12, -(-int(2.5 * 256e6) // (P * 16))))
    data = [make_set(N, H, W, s) for s in range(sets)]
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    value, g = torch.empty(1, device="cuda"), torch.ones(1, device="cuda")
    gdepth, gup, gunc = (torch.empty((N, 1, H, W), device="cuda") for _ in range(3))
    ws = torch.empty((lib.pd_unc_loss_rows(N, H, W), 4), dtype=torch.float64, device="cuda")
    common = (MIN_D, MAX_D, B_RANGE[0], B_RANGE[1])

    def fwd(i):
        depth, gt, u, _ = data[i % sets]
        check(lib.pd_unc_loss_fwd(ptr(depth), ptr(gt), W, ptr(u), H, W, None, *common, ptr(sums), ptr(value), None, ptr(ws),
                                  ws.numel() * 8, N, H, W, stream_ptr()), "pd_unc_loss_fwd")

    def bwd(i):
        depth, gt, u, _ = data[i % sets]
        check(lib.pd_unc_loss_bwd(ptr(depth), ptr(gt), W, ptr(u), H, W, None, *common, ptr(g), ptr(sums), ptr(gdepth), ptr(gup),
                                  N, H, W, stream_ptr()), "pd_unc_loss_bwd")
        check(lib.pd_up_gather_bwd(ptr(gup), ptr(gunc), N, H, W, H, W, 0, 0, stream_ptr()), "pd_up_gather_bwd")

    def both(i):
        fwd(i)
        bwd(i)

    for i in range(sets):
        both(i)
    torch.cuda.synchronize()
    ms, ms_min, ms_max = _median_ms(both, iters)
    fwd_ms = _median_ms(fwd, iters)[0]
    fwd(0)
    bwd_ms = _median_ms(lambda i: bwd(0), iters)[0]
    both(0)
    torch.cuda.synchronize()
    dev_value = float(value.item())
    copy_ms = _copy_ms(moved, sets, iters)
    out = {"op": "unc_loss_fwd_bwd", "N": N, "H": H, "W": W, "sets": sets, "bytes": moved, "ms": round(ms, 4),
           "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4), "fwd_ms": round(fwd_ms, 4), "bwd_and_fold_ms": round(bwd_ms, 4),
           "GBps": round(moved / (ms * 1e-3) / 1e9, 1), "fwd_GBps": round(P * 12 / (fwd_ms * 1e-3) / 1e9, 1),
           "copy_ms": round(copy_ms, 4), "copy_GBps": round(moved / (copy_ms * 1e-3) / 1e9, 1),
           "time_over_copy": round(ms / copy_ms, 2), "value": dev_value}

    def torch_pair(i):
        depth, gt, u, _ = data[i % sets]
        d, uu = depth.detach().requires_grad_(True), u.detach().requires_grad_(True)
        L = torch_loss(d, gt, uu)
        L.backward()
        return L.detach()

    tv = torch_pair(0)
    torch.cuda.synchronize()
    t_ms, t_min, _ = _median_ms(torch_pair, torch_iters)
    out.update({"torch_ms": round(t_ms, 3), "torch_ms_min": round(t_min, 3), "torch_over_call": round(t_ms / ms, 1),
                "torch_value_rel_diff": abs(float(tv) - dev_value) / max(abs(dev_value), 1e-30)})

    # ---- the evaluator, next to the copy and to pd_depth_stats
    def ustat(i):
        depth, gt, u, mask = data[i % sets]
        return uncertainty_eval.uncertainty_stats(depth, gt, u, mask=mask, b_range=B_RANGE, min_depth=MIN_D, max_depth=MAX_D)

    def dstat(i):
        depth, gt, _, mask = data[i % sets]
        return depth_eval.depth_stats(depth, gt, mask=mask, min_depth=MIN_D, max_depth=MAX_D)

    for i in range(sets):
        ustat(i), dstat(i)
    torch.cuda.synchronize()
    u_ms, u_min, u_max = _median_ms(ustat, iters)
    d_ms = _median_ms(dstat, iters)[0]
    st = ustat(0)
    m = st.pooled()[0]
    sc_ms = _copy_ms(P * STATS_BYTES, sets, iters)
    out.update({"stats_ms": round(u_ms, 4), "stats_ms_min": round(u_min, 4), "stats_ms_max": round(u_max, 4),
                "stats_GBps": round(P * STATS_BYTES / (u_ms * 1e-3) / 1e9, 1), "stats_copy_ms": round(sc_ms, 4),
                "stats_over_copy": round(u_ms / sc_ms, 2), "depth_stats_ms": round(d_ms, 4),
                "stats_over_depth_stats": round(u_ms / d_ms, 2), "classes": len(st.names),
                "all_mae_mm": float(m[0]), "all_b_mm": float(m[1]), "all_cover50": float(m[3]), "all_cover90": float(m[4]),
                "all_ause_mm": float(m[5]), "all_aurg_mm": float(m[6])})
    if with_step:
        del data
        torch.cuda.empty_cache()
        step_iters = max(3, iters // 3)
        base = _step_ms(N, H, W, step_iters, None)
        with_term = _step_ms(N, H, W, step_iters, 0.1)
        detached = _step_ms(N, H, W, step_iters, 0.1, True)
        out.update({"supervised_step_ms": round(base, 3), "step_with_term_ms": round(with_term, 3),
                    "added_share_of_step": round((with_term - base) / base, 4), "step_detached_ms": round(detached, 3),
                    "detached_added_share_of_step": round((detached - base) / base, 4)})
    else:
        out["supervised_step_ms"] = out["step_with_term_ms"] = out["added_share_of_step"] = "not measured"
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--sets", type=int, default=None)
    ap.add_argument("--step", action="store_true", help="also time the supervised training step with and without the term")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncertainty.log"), help="the log; '' = print only")
    args = ap.parse_args()
    log = open(args.out, "w") if args.out else None
    for N, H, W in SIZES:
        line = json.dumps(time_size(N, H, W, args.iters, args.sets, with_step=args.step))
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
    if log:
        log.close()
