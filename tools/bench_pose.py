"""The pose-network kernels (csrc/pose.hip, pd_view_synth_bwd_pose) at the training sizes: B = 12 at 320x480 and B = 16 at
512x640, everything in one run.  The kernels take 15 - 140 us a call, about what the host needs to enqueue one, so they are
timed as tools/bench_student.py times its kernels: one HIP event pair spans 20 back-to-back calls enqueued behind a spinning
kernel, the span divided by 20, median of ``--iters`` windows; the device copies next to them the same way.  The working
sets stay below the 256 MiB Infinity Cache: warm-cache figures, comparable with each other, not HBM rates.  The torch-op
tail and the training steps are host-bound and are timed per call (one event pair per call, median), as in bench_reproj.py:

  * pd_view_synth_bwd_pose (depth and pose gradient, both launches) next to pd_view_synth_bwd (the depth gradient alone: the
    kernel that was there is the yardstick) and to a device copy that moves the bytes the pass touches, half read, half written
    -- per pixel: gwarped 12, the four taps of three channels counted once 12, coords 8, depth 4, gdepth 4 = 40 bytes (the
    partial rows and the 16 floats of gT are noise next to that);
  * pd_pose_head_fwd and pd_pose_head_bwd on the decoder's 1/32-resolution plane, the number of kernels torch's profiler
    counts for one forward + backward call of them, and the same tail written with torch ops under autograd -- 1x1
    convolution, spatial mean, 0.01, the reference's rot_from_axisangle / get_translation_matrix / matmul for both
    matrices, and the backward of all that -- with its kernel count from the same profiler;
  * with ``--step`` one training step of a Trainer in the pose-network mode next to one in the known-pose mode (synthetic
    items).
One JSON line per size, printed and written to ``--out`` (default: profiles/pose.log).  ``--loss`` times the pose supervision
instead (time_loss: pd_pose_loss_fwd / _bwd at N = 12 and 16, F = 2, next to the same loss with torch ops; default log
profiles/pose_loss.log).  ``--chain`` times the matching-pose chain instead (time_chain: pd_pose_chain at N = 12 and 16, L = 1
and 3, next to the reference's chain with torch ops and its host synchronisations; default log profiles/pose_chain.log)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_reproj import _median_ms                 # noqa: E402  (per call: the host-bound rows)
from bench_student import _queued_ms, _copy_ms      # noqa: E402  (windows of 20 calls: the short kernels and their copies)

SIZES = ((12, 320, 480), (16, 512, 640))
WARP_BYTES_PER_PIXEL = 12 + 12 + 8 + 4 + 4


def _torch_matrix(aa, tr, invert):
    """layers.py:74-149 with tensor ops, as the reference writes it (indexed assignments into zero buffers, matmul)."""
    import torch
    angle = torch.norm(aa, 2, 2, True)
    axis = aa / (angle + 1e-7)
    ca, sa = torch.cos(angle), torch.sin(angle)
    C = 1 - ca
    x, y, z = axis[..., 0].unsqueeze(1), axis[..., 1].unsqueeze(1), axis[..., 2].unsqueeze(1)
    xs, ys, zs, xC, yC, zC = x * sa, y * sa, z * sa, x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    rot = torch.zeros((aa.shape[0], 4, 4), device=aa.device)
    for (i, j), v in (((0, 0), x * xC + ca), ((0, 1), xyC - zs), ((0, 2), zxC + ys), ((1, 0), xyC + zs), ((1, 1), y * yC + ca),
                      ((1, 2), yzC - xs), ((2, 0), zxC - ys), ((2, 1), yzC + xs), ((2, 2), z * zC + ca)):
        rot[:, i, j] = torch.squeeze(v)
    rot[:, 3, 3] = 1
    t = tr.clone()
    if invert:
        rot = rot.transpose(1, 2)
        t = t * -1
    T = torch.zeros(aa.shape[0], 4, 4, device=aa.device)
    for i in range(4):
        T[:, i, i] = 1
    T[:, :3, 3, None] = t.contiguous().view(-1, 3, 1)
    return torch.matmul(rot, T) if invert else torch.matmul(T, rot)


def time_warp(N, H, W, iters):
    import torch
    from polardepth import ops, synthetic
    from polardepth._lib import lib, check, ptr, stream_ptr
    b = synthetic.multiview_plane(N, H, W, frame_ids=(0, 1), seed=0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    depth = 0.5 + torch.rand((N, 1, H, W), generator=gen, device="cuda")
    src, K, iK, T = b[("color", 1, 0)].float().contiguous(), b[("K", 0)], b[("inv_K", 0)], b[("poses", 1)]
    gw = torch.randn((N, 3, H, W), generator=gen, device="cuda")
    with torch.no_grad():
        _, coords = ops.view_synthesis(depth, src, K, iK, T)
    gd = torch.empty_like(depth)
    rows = lib.pd_view_synth_pose_rows(H, W)
    part = torch.empty((N, rows, 12), dtype=torch.float64, device="cuda")
    gT = torch.empty((N, 4, 4), device="cuda")

    def both():
        check(lib.pd_view_synth_bwd_pose(ptr(gw), ptr(src), ptr(coords), ptr(depth), ptr(K), ptr(iK), ptr(T), ptr(gd), ptr(part),
                                         None, ptr(gT), N, 3, H, W, 0, stream_ptr()), "pd_view_synth_bwd_pose")

    def depth_only():
        check(lib.pd_view_synth_bwd(ptr(gw), ptr(src), ptr(coords), ptr(depth), ptr(K), ptr(iK), ptr(T), ptr(gd), N, 3, H, W, 0,
                                    stream_ptr()), "pd_view_synth_bwd")
    out = {}
    for name, call in (("bwd_pose", both), ("bwd_depth", depth_only)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        out[name] = _queued_ms(call, iters)
    moved = N * H * W * WARP_BYTES_PER_PIXEL
    copy_ms = _copy_ms(moved, iters)
    return {"view_synth_bwd_pose_ms": round(out["bwd_pose"][0], 4), "view_synth_bwd_pose_min_max": [round(v, 4) for v in out["bwd_pose"][1:]],
            "view_synth_bwd_ms": round(out["bwd_depth"][0], 4), "pose_rows": rows, "warp_bytes": moved,
            "warp_copy_ms": round(copy_ms, 4), "bwd_pose_ratio_to_bwd": round(out["bwd_pose"][0] / out["bwd_depth"][0], 3),
            "bwd_pose_ratio_to_copy": round(out["bwd_pose"][0] / copy_ms, 3)}


def time_head(N, H, W, iters):
    import torch
    from polardepth import ops
    from polardepth._lib import lib, check, ptr, stream_ptr
    h, w, Cin, Co = H // 32, W // 32, 256, 12
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((N, h, w, Cin), generator=gen, device="cuda")
    wt = 0.1 * torch.randn((Co, Cin), generator=gen, device="cuda")
    bias = 0.1 * torch.randn(Co, generator=gen, device="cuda")
    aa, tr = torch.empty(N, 2, 1, 3, device="cuda"), torch.empty(N, 2, 1, 3, device="cuda")
    T, Ti = torch.empty(N, 4, 4, device="cuda"), torch.empty(N, 4, 4, device="cuda")
    mean = torch.empty(N, Cin, dtype=torch.float64, device="cuda")
    gT, gTi = torch.randn(N, 4, 4, generator=gen, device="cuda"), torch.randn(N, 4, 4, generator=gen, device="cuda")
    gx, gw, gb = torch.empty_like(x), torch.empty_like(wt), torch.empty_like(bias)
    ws = torch.empty(N, Co, dtype=torch.float64, device="cuda")

    def fwd():
        check(lib.pd_pose_head_fwd(ptr(x), ptr(wt), ptr(bias), ptr(aa), ptr(tr), ptr(T), ptr(Ti), ptr(mean), N, h, w, Cin, Co, 1,
                                   stream_ptr()), "pd_pose_head_fwd")

    def bwd():
        check(lib.pd_pose_head_bwd(ptr(gT), ptr(gTi), None, None, ptr(aa), ptr(tr), ptr(wt), ptr(mean), ptr(gx), ptr(gw), ptr(gb),
                                   ptr(ws), N, h, w, Cin, Co, 1, 0, stream_ptr()), "pd_pose_head_bwd")
    xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)
    w4, b4 = wt.reshape(Co, Cin, 1, 1).detach().requires_grad_(True), bias.detach().requires_grad_(True)

    def torch_tail():
        out = torch.nn.functional.conv2d(xt, w4, b4).mean(3).mean(2)
        out = 0.01 * out.view(-1, 2, 1, 6)
        a, t = out[..., :3], out[..., 3:]
        loss = (_torch_matrix(a[:, 0], t[:, 0], True) * gT).sum() + (_torch_matrix(a[:, 0], t[:, 0], False) * gTi).sum()
        loss.backward()
        xt.grad = w4.grad = b4.grad = None
    out = {}
    for name, call, timer in (("fwd", fwd, _queued_ms), ("bwd", bwd, _queued_ms), ("torch", torch_tail, _median_ms)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        out[name] = timer(call, iters)[0]

    return {"head_plane": [h, w], "pose_head_fwd_ms": round(out["fwd"], 4), "pose_head_bwd_ms": round(out["bwd"], 4),
            "pose_head_kernels": _kernels_of(lambda: (fwd(), bwd())), "torch_tail_fwd_bwd_ms": round(out["torch"], 4),
            "torch_tail_kernels": _kernels_of(torch_tail), "torch_ratio": round(out["torch"] / (out["fwd"] + out["bwd"]), 1)}


def _kernels_of(call):
    import torch
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        call()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None
               and "cuda" in str(e.device_type).lower())


def time_loss(N, F, iters):
    """pd_pose_loss_fwd + pd_pose_loss_bwd (csrc/pose_loss.hip) for F frames of N poses next to the same loss written with
    torch ops on the device under autograd (tests/pose_loss_ref.py: torch_rotvec / torch_pose_loss, float32 there), with the
    number of kernels torch's profiler counts for one forward + backward of each.  The two kernels are timed in windows of 20
    queued calls, the host-bound torch chain per call."""
    import ctypes
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pose_loss_ref
    from polardepth import ops
    from polardepth._lib import lib, check, ptr, stream_ptr
    gen = torch.Generator(device="cuda").manual_seed(2)
    mats = lambda: [ops.pose_matrix(1.5 * (torch.rand((N, 3), generator=gen, device="cuda") - 0.5),
                                    0.1 * torch.randn((N, 3), generator=gen, device="cuda"), invert=bool(f & 1))
                    for f in range(F)]
    Tp, Tg = mats(), mats()
    valid = torch.ones((N, F), device="cuda")
    vals = torch.empty(3 + 2 * F, device="cuda")
    gvals = torch.ones(3, device="cuda")
    gT = [torch.empty_like(t) for t in Tp]
    arr = lambda ts: (ctypes.c_void_p * F)(*[t.data_ptr() for t in ts])
    pp, pg, pgT = arr(Tp), arr(Tg), arr(gT)
    w = (ctypes.c_float * F)(*[float(F - f) for f in range(F)])

    def fwd():
        check(lib.pd_pose_loss_fwd(pp, pg, F, w, ptr(valid), None, ptr(vals), N, stream_ptr()), "pd_pose_loss_fwd")

    def bwd():
        check(lib.pd_pose_loss_bwd(ptr(gvals), pp, pg, F, w, ptr(valid), pgT, N, stream_ptr()), "pd_pose_loss_bwd")
    leaves = [t.detach().clone().requires_grad_(True) for t in Tp]

    def op():
        ops.pose_supervision(leaves, Tg, valid=valid)[2].backward()
        for t in leaves:
            t.grad = None

    def torch_chain():
        pose_loss_ref.torch_pose_loss(leaves, Tg)[2].backward()
        for t in leaves:
            t.grad = None
    out = {}
    for name, call, timer in (("fwd", fwd, _queued_ms), ("bwd", bwd, _queued_ms), ("op", op, _median_ms),
                              ("torch", torch_chain, _median_ms)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        out[name] = timer(call, iters)[0]
    return {"op": "pose_loss", "N": N, "F": F, "pose_loss_fwd_ms": round(out["fwd"], 4), "pose_loss_bwd_ms": round(out["bwd"], 4),
            "pose_loss_kernels": _kernels_of(lambda: (fwd(), bwd())), "pose_supervision_fwd_bwd_ms": round(out["op"], 4),
            "pose_supervision_kernels": _kernels_of(op), "torch_loss_fwd_bwd_ms": round(out["torch"], 4),
            "torch_loss_kernels": _kernels_of(torch_chain), "torch_ratio": round(out["torch"] / (out["fwd"] + out["bwd"]), 1)}


def time_chain(N, H, W, L, iters):
    """pd_pose_chain (csrc/pose.hip) for a chain of L past frames of N items next to the reference's chain restated with
    torch ops (trainer.py:713-746): per link both transformation_from_parameters, the matmul with the stored pose, and the
    Python loop over the batch with ``feat.sum() == 0`` per item -- one host synchronisation each, over pictures of the
    training size.  The kernel is timed in windows of 20 queued calls, the host-bound torch chain per call; the kernel counts
    are torch's profiler's for one call of each."""
    import torch
    from polardepth._lib import lib, check, ptr, stream_ptr
    gen = torch.Generator(device="cuda").manual_seed(3)
    aa = 0.3 * (torch.rand((L, N, 3), generator=gen, device="cuda") - 0.5)
    tr = 0.1 * torch.randn((L, N, 3), generator=gen, device="cuda")
    pics = torch.rand((L, N, 3, H, W), generator=gen, device="cuda")
    pics[L - 1, N // 2] = 0                                          # one missing frame
    present = (pics.reshape(L, N, -1).sum(2) != 0).float()
    rel, rel_inv = torch.empty((L, N, 4, 4), device="cuda"), torch.empty((L, N, 4, 4), device="cuda")

    def kernel():
        check(lib.pd_pose_chain(ptr(aa), ptr(tr), ptr(present), None, ptr(rel), ptr(rel_inv), L, N, -1, stream_ptr()),
              "pd_pose_chain")
    state = {}

    def torch_chain():
        prev = None
        for k in range(L):
            pose = _torch_matrix(aa[k][:, None], tr[k][:, None], True)
            state["inv"] = _torch_matrix(aa[k][:, None], tr[k][:, None], False)
            if prev is not None:
                pose = torch.matmul(pose, prev)
            for b, feat in enumerate(pics[k]):
                if feat.sum() == 0:
                    pose[b] *= 0
            prev = pose
        state["rel"] = prev
    out = {}
    for name, call, timer in (("kernel", kernel, _queued_ms), ("torch", torch_chain, _median_ms)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        out[name] = timer(call, iters)
    err = float((state["rel"] - rel[L - 1]).abs().max())
    return {"op": "pose_chain", "N": N, "L": L, "H": H, "W": W, "pose_chain_ms": round(out["kernel"][0], 4),
            "pose_chain_min_max": [round(v, 4) for v in out["kernel"][1:]], "pose_chain_kernels": _kernels_of(kernel),
            "torch_chain_ms": round(out["torch"][0], 4), "torch_chain_kernels": _kernels_of(torch_chain),
            "torch_chain_host_syncs": L * N, "torch_ratio": round(out["torch"][0] / out["kernel"][0], 1),
            "max_abs_diff_last_link": err}


def _step_ms(N, H, W, iters, pose_network):
    import torch
    from manydepth.options import MonodepthOptions
    from manydepth.trainer import Trainer
    with tempfile.TemporaryDirectory() as tmp:
        opt = MonodepthOptions().parse([
            "--png", "--batch_size", str(N), "--height", str(H), "--width", str(W), "--dataset", "HAMMER", "--split", "HAMMER",
            "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", "--depth_supervision", "True",
            "--pose_input", "True", "--augment_xolp", "--augment_normals", "--log_dir", tmp, "--data_path", "synthetic",
            "--data_path_val", "synthetic", "--num_workers", "0", "--weights_init", "scratch"])
        if pose_network:
            opt.pose_input, opt.pose_network = False, True
        tr = Trainer(opt)
        tr.set_train()
        ds = tr.train_loader.dataset
        batch = torch.utils.data.default_collate([ds[i % len(ds)] for i in range(N)])
        batch = {k: v.cuda() for k, v in batch.items()}

        def step():
            tr.model_optimizer.zero_grad()
            _, losses, _ = tr.process_batch(dict(batch), is_train=True)
            losses["loss"].backward()
            tr.model_optimizer.step()
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        return _median_ms(step, iters)[0]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--step", action="store_true", help="also time one step of the pose-network and of the known-pose mode")
    ap.add_argument("--loss", action="store_true", help="time the pose supervision (pd_pose_loss_fwd / _bwd) instead: N = 12 "
                    "and 16, F = 2, next to the same loss with torch ops; the default log is then profiles/pose_loss.log")
    ap.add_argument("--chain", action="store_true", help="time the matching-pose chain (pd_pose_chain) instead: N = 12 and 16, "
                    "L = 1 and 3, next to the reference's chain with torch ops; the default log is then profiles/pose_chain.log")
    ap.add_argument("--out", default=None, help="the log (default profiles/pose.log, with --loss profiles/pose_loss.log, with "
                    "--chain profiles/pose_chain.log); '' = print only")
    args = ap.parse_args()
    if args.loss and args.chain:
        ap.error("--loss and --chain are two runs")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pose_loss.log" if args.loss else "pose_chain.log" if args.chain else "pose.log")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_pose needs the GPU; there is no CPU fallback")
    log = open(args.out, "w") if args.out else None
    for N, H, W in SIZES if args.chain else ():
        for L in (1, 3):
            line = json.dumps(time_chain(N, H, W, L, args.iters))
            print(line, flush=True)
            if log:
                log.write(line + "\n")
                log.flush()
    for N, _, _ in SIZES if args.loss else ():
        line = json.dumps(time_loss(N, 2, args.iters))
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
    for N, H, W in () if args.loss or args.chain else SIZES:
        row = {"op": "pose_network_kernels", "N": N, "H": H, "W": W}
        row.update(time_warp(N, H, W, args.iters))
        row.update(time_head(N, H, W, args.iters))
        if args.step:
            torch.cuda.empty_cache()
            n = max(3, args.iters // 3)
            known, pose = _step_ms(N, H, W, n, False), _step_ms(N, H, W, n, True)
            row.update({"known_pose_step_ms": round(known, 3), "pose_network_step_ms": round(pose, 3),
                        "step_ratio": round(pose / known, 3)})
        else:
            row["known_pose_step_ms"] = row["pose_network_step_ms"] = "not measured"
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
    if log:
        log.close()
