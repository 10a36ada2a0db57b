"""The multi-frame cost volume (csrc/matching.hip; polardepth.ops.cost_volume) at the training sizes of the 1/4-resolution
feature maps: B = 12 at 80 x 120 (320 x 480 input) and B = 16 at 128 x 160 (512 x 640), D = 96 bins, F = 2 lookup frames,
C = 64 channels.

ms per call with HIP events, warm: one event pair per call, median of ``--iters`` calls.  Next to it, in the same run:
  * a device copy that moves the bytes the kernel MUST touch, half read and half written, timed the same way.  The count:
    features in once -- cur 4 C and lookup 4 C F bytes per pixel -- and outputs out once -- cost 4 D, confidence, argmin and
    lowest 4 each -- that is 4 C (1 + F) + 4 D + 12 = 1164 bytes per pixel and item (`missing` is not asked for);
  * the reference's own chain (resnet_encoder.py:430-511, 534-541, 620-630) restated with torch ops on the device: the loop over
    the batch, ``repeat`` of the feature map over the bins, ``grid_sample``, the masks, the fill, the confidence, the argmin.
Also reported: the share of (pixel, bin, frame) entries the edge mask skips (no tap is read for them), the bytes the taps of the
other entries gather (4 taps x 4 C bytes each; they come out of L1 / L2, a lookup map is read from HBM once) and both rates, and
how far the chain's cost is from the kernel's.  The matrix cores are not involved: an L1 distance is no contraction.
One JSON line per size, printed and written to ``--out`` (default: profiles/matching.log)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))

SIZES = ((12, 80, 120), (16, 128, 160))
D, F, C = 96, 2, 64
MIN_BIN, MAX_BIN = 0.1, 2.0
BYTES_PER_PIXEL = 4 * C * (1 + F) + 4 * D + 12


def _median_ms(call, iters):
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in evs:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return ts[iters // 2], ts[0], ts[-1]


def _copy_ms(moved, iters, sets=3):
    import torch
    half = moved // 2
    src = [torch.empty(half, dtype=torch.uint8, device="cuda").fill_(s + 1) for s in range(sets)]
    dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    state = {"i": 0}

    def copy():
        i = state["i"] = (state["i"] + 1) % sets
        dst[i].copy_(src[i])
    for _ in range(sets):
        copy()
    torch.cuda.synchronize()
    return _median_ms(copy, iters)[0]


def inputs(B, h, w, seed=0):
    """Smooth non-negative features, lookup frames shifted by the parallax of a plane at 0.8 m, translations of 6-9 cm."""
    import torch
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    c = torch.arange(C, dtype=torch.float32)[:, None, None]
    K = torch.eye(4).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.62 * w, 1.05 * h, w / 2 - 0.4, h / 2 + 0.3
    poses = torch.eye(4).repeat(B, F, 1, 1)
    sign = torch.tensor([1.0, -1.0])[:F].view(1, F, 1)
    poses[:, :, :3, 3] = sign * torch.tensor([0.075, 0.01, 0.005]) + 0.015 * (torch.rand(B, F, 3, generator=g) - 0.5)

    def pattern(n, sx, sy):
        x, y = xx - sx, yy - sy
        return (0.9 + 0.45 * torch.sin(x / (2.0 + 0.05 * c) + 0.37 * c + n) * torch.cos(y / (3.1 - 0.02 * c) + 0.11 * c)
                + 0.3 * torch.sin((x + 2 * y) / (5.0 + 0.1 * c) + 0.2 * c)).clamp_min(0)
    cur = torch.stack([pattern(n, 0, 0) for n in range(B)])
    lookup = torch.stack([torch.stack([pattern(n, float(K[n, 0, 0] * poses[n, f, 0, 3] / 0.8),
                                               float(K[n, 1, 1] * poses[n, f, 1, 3] / 0.8)) for f in range(F)]) for n in range(B)])
    return cur, lookup, poses, K, torch.linalg.inv(K)


def torch_chain(cur, lookup, poses, K, inv_K, bins):
    """The reference's match_features + compute_confidence_mask + lowest-cost map with torch ops, NCHW as the reference has it.
    Returns (cost * confidence, confidence, lowest, number of entries the edge mask keeps)."""
    import torch
    import torch.nn.functional as TF
    B, _, h, w = cur.shape
    nb = bins.numel()
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=cur.device),
                            torch.arange(w, dtype=torch.float32, device=cur.device), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, device=cur.device)], 0)[None].repeat(nb, 1, 1)
    ones = torch.ones(nb, 1, h * w, device=cur.device)
    warp_depths = bins.view(nb, 1, 1).expand(nb, 1, h * w)
    current_mask = torch.zeros(nb, h, w, device=cur.device)
    current_mask[:, 2:-2, 2:-2] = 1.0
    volumes, masks, kept = [], [], 0
    for b in range(B):
        cost_volume = torch.zeros(nb, h, w, device=cur.device)
        counts = torch.zeros(nb, h, w, device=cur.device)
        world_points = torch.cat([warp_depths * torch.matmul(inv_K[b:b + 1, :3, :3], pix), ones], 1)
        for f in range(lookup.shape[1]):
            lookup_feat = lookup[b:b + 1, f].repeat([nb, 1, 1, 1])
            cam = torch.matmul(torch.matmul(K[b:b + 1], poses[b:b + 1, f])[:, :3, :], world_points)
            pc = (cam[:, :2, :] / (cam[:, 2, :].unsqueeze(1) + 1e-7)).view(nb, 2, h, w).permute(0, 2, 3, 1).clone()
            pc[..., 0] /= w - 1
            pc[..., 1] /= h - 1
            pix_locs = (pc - 0.5) * 2
            warped = TF.grid_sample(lookup_feat, pix_locs, padding_mode="zeros", mode="bilinear", align_corners=True)
            x_vals = (pix_locs[..., 0] / 2 + 0.5) * (w - 1)
            y_vals = (pix_locs[..., 1] / 2 + 0.5) * (h - 1)
            edge_mask = ((x_vals >= 2.0) * (x_vals <= w - 2) * (y_vals >= 2.0) * (y_vals <= h - 2)).float() * current_mask
            kept = kept + edge_mask.sum()
            diffs = torch.abs(warped - cur[b:b + 1]).mean(1) * edge_mask
            cost_volume = cost_volume + diffs
            counts = counts + (diffs > 0).float()
        cost_volume = cost_volume / (counts + 1e-7)
        missing = (cost_volume == 0).float()
        cost_volume = cost_volume * (1 - missing) + cost_volume.max(0)[0].unsqueeze(0) * missing
        volumes.append(cost_volume)
        masks.append(missing)
    cost, missing = torch.stack(volumes, 0), torch.stack(masks, 0)
    confidence = ((cost * (1 - missing) > 0).sum(1) == nb).float()
    viz = cost.clone()
    viz[viz == 0] = 100
    lowest = 1 / bins[torch.min(viz, 1)[1]]
    return cost * confidence.unsqueeze(1), confidence, lowest, kept


def time_size(B, h, w, iters=12):
    import torch
    from polardepth import matching, ops
    if not torch.cuda.is_available():
        raise RuntimeError("bench_matching needs the GPU; there is no CPU fallback")
    cur, lookup, poses, K, inv_K = (t.cuda() for t in inputs(B, h, w))
    bins = matching.depth_bins(MIN_BIN, MAX_BIN, D, "linear").cuda()
    cur_cl = cur.contiguous(memory_format=torch.channels_last)
    lookup_cl = lookup.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    buf = ops.empty_nhwc(B, C + D, h, w, cur.device)

    def kernel():
        return ops.cost_volume(cur_cl, lookup_cl, poses, K, inv_K, bins, out=buf[:, C:], apply_confidence=True)

    def chain():
        with torch.no_grad():
            return torch_chain(cur, lookup, poses, K, inv_K, bins)

    timed = {}
    for name, call in (("kernel", kernel), ("chain", chain)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        timed[name] = _median_ms(call, iters)
    cost, conf, _, low = kernel()
    ccost, cconf, clow, kept = chain()
    entries = B * h * w * D * F
    kept = int(kept.item())
    moved = B * h * w * BYTES_PER_PIXEL
    copy_ms = _copy_ms(moved, iters)
    ms, chain_ms = timed["kernel"][0], timed["chain"][0]
    gathered = kept * 4 * 4 * C
    dcost = (cost - ccost).abs()
    return {"op": "cost_volume", "B": B, "h": h, "w": w, "D": D, "F": F, "C": C, "bytes": moved, "ms": round(ms, 4),
            "ms_min": round(timed["kernel"][1], 4), "ms_max": round(timed["kernel"][2], 4),
            "GBps_of_required_bytes": round(moved / (ms * 1e-3) / 1e9, 1), "copy_ms": round(copy_ms, 4),
            "ratio_to_copy": round(ms / copy_ms, 2), "torch_chain_ms": round(chain_ms, 3),
            "torch_chain_over_kernel": round(chain_ms / ms, 1), "entries": entries,
            "share_skipped_by_edge_mask": round(1 - kept / entries, 4), "tap_bytes": gathered,
            "tap_GBps": round(gathered / (ms * 1e-3) / 1e9, 1), "ns_per_kept_entry": round(ms * 1e6 / max(kept, 1), 4),
            "confident_share": round(conf.mean().item(), 4), "confidence_differs_from_chain": round((conf != cconf).float().mean().item(), 5),
            "cost_differs_from_chain_by_more_than_1e-4": round((dcost > 1e-4).float().mean().item(), 5),
            "cost_median_abs_diff_to_chain": float(dcost.median().item()),
            "lowest_differs_from_chain": round((low != clow).float().mean().item(), 5), "matrix_cores": "not involved"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matching.log"), help="the log; '' = print only")
    args = ap.parse_args()
    log = open(args.out, "w") if args.out else None
    for B, h, w in SIZES:
        line = json.dumps(time_size(B, h, w, args.iters))
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
    if log:
        log.close()
