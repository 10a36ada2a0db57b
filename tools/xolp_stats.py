"""DoLP / AoLP statistics of a data set as the network will see it (polardepth.polar.XolpStats, csrc/xolp_stats.hip): what the
reference's polarisation/xolp_mean_and_std_dev.py printed for 46 HAMMER frames, for any input the loader and K1 accept.

    python tools/xolp_stats.py --data_path /data/HAMMER --split HAMMER --every 10
    python tools/xolp_stats.py --data_path synthetic --batches 2 --json stats.json --hist

Builds HAMMER_Dataset the way the Trainer does and hands every batch to ``polardepth.polar.polar_inputs`` exactly as
Trainer.process_batch does, so the loader switches (PD_POL_NATIVE, PD_DEVICE_RESIZE, PD_POL_DOFP, PD_POL_CDOFP, read by the
data set) and the options manydepth/train.py reads (PD_POL_ANGLES, PD_POL_LAYOUT, PD_POL_DEMOSAIC, PD_POL_BAYER, PD_POL_GAINS,
PD_POL_COLOR_SCALE) apply unchanged; ``--pol_calibration cal.npz`` (or PD_POL_CALIBRATION) applies the sensor's super-pixel
calibration to sensor frames before their demosaic, as ``opt.pol_calibration`` does.  Prints the reference's six lines, the share of pixels whose DoLP lies beyond the diffuse
zenith table and beyond 1 (a wrong layout, wrong angles, a wrong colour scale or a saturating sensor show up here first), the
non-finite count and a ready-to-paste PD_XOLP_NORM.  The statistics accumulate on the device; the one host read is at the end.

``--time`` measures instead: the NumPy statements of the reference's script on one core for its own workload (a 46 x 832 x
1088 stack, synthetic values; no GPU needed), and -- with a GPU -- one pd_xolp_stats call at B = 16, 512 x 640 on K1's output
for synthetic items ("smooth"), on i.i.d. values and on a constant tensor, next to a plain read of the same bytes
(torch.sum of the same tensor) in the same run: HIP events around one call per rotating buffer set, the sets sized past the
256 MB Infinity Cache, median over ``--iters`` rounds.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"))


def options_from_env(env=os.environ):
    """The polarizer options as manydepth/train.py reads them: (angles in radians or None, dofp options, cdofp options)."""
    from polardepth import polar, dofp, cdofp
    layout = env.get("PD_POL_LAYOUT") or None
    return (polar.angles_from_degrees(env.get("PD_POL_ANGLES") or None),
            dofp.options(layout, env.get("PD_POL_DEMOSAIC") or None),
            cdofp.options(layout, env.get("PD_POL_BAYER") or None, env.get("PD_POL_GAINS") or None,
                          env.get("PD_POL_COLOR_SCALE") or None))


def split_files(data_path, split, which="train"):
    from manydepth import datasets
    from manydepth.utils import readlines
    for root in (".", ROOT):
        path = os.path.join(root, "splits", split, f"{which}_files.txt")
        if os.path.exists(path):
            return readlines(path)
    if str(data_path) == datasets.SYNTHETIC:
        return []
    raise FileNotFoundError(f"splits/{split}/{which}_files.txt not found (--data_path {datasets.SYNTHETIC} serves synthetic items)")


def measure(args):
    import torch
    from torch.utils.data import DataLoader, Subset
    from manydepth import datasets
    from polardepth import polar
    if not torch.cuda.is_available():
        raise RuntimeError("tools/xolp_stats.py needs the GPU; there is no CPU fallback")
    device = torch.device("cuda")
    angles, dofp_opts, cdofp_opts = options_from_env()
    from polardepth import calibration as pdcal
    cal = pdcal.parse(args.pol_calibration or os.environ.get("PD_POL_CALIBRATION") or None, device)
    if cal is not None and tuple(cal.layout) != tuple(dofp_opts[0]):
        raise ValueError(f"--pol_calibration was fitted for the layout {tuple(cal.layout)}, PD_POL_LAYOUT is {tuple(dofp_opts[0])}")
    ds = datasets.HAMMER_Dataset(args.data_path, split_files(args.data_path, args.split), args.height, args.width, [0], 4,
                                 is_train=False)
    if args.every > 1:
        ds = Subset(ds, range(0, len(ds), args.every))
    loader = DataLoader(ds, args.batch_size, False, num_workers=args.num_workers, drop_last=False)
    acc = polar.XolpStats(device)
    items = 0
    for i, inputs in enumerate(loader):
        if args.batches and i >= args.batches:
            break
        inputs = {k: v.to(device, non_blocking=True) for k, v in inputs.items()}
        polar.polar_inputs(inputs, (args.height, args.width), ("xolp",), angles, dofp=dofp_opts, cdofp=cdofp_opts,
                           calibration=cal)
        if ("xolp", 0, 0) not in inputs:
            raise KeyError('the loader served neither polarizer planes nor ("xolp", 0, 0)')
        xolp = inputs[("xolp", 0, 0)]
        pol = inputs.get(("pol", 0, 0))
        # planes narrower than the network input are padded by K1 (612 -> 640): the padding is no data
        narrow = pol is not None and pol.shape[2] == args.height and pol.shape[3] < args.width
        acc.add(xolp.float(), width=pol.shape[3] if narrow else None)
        items += xolp.shape[0]
    res = acc.result()
    res["items"] = items
    return res


def report(res, hist=False, out=sys.stdout):
    from polardepth import polar
    from polarisation.xolp_mean_and_std_dev import report as six_lines
    six_lines(res, out)
    print(f"DOLP > {res['thresholds'][0]:.6g} (end of the diffuse table):  {res['frac_over_diffuse']:.6g}", file=out)
    print(f"DOLP > {res['thresholds'][1]:.6g} (end of the specular table): {res['frac_over_one']:.6g}", file=out)
    print(f"NONFINITE:  {res['nonfinite']}   PIXELS: {res['n']}   ITEMS: {res.get('items', '-')}", file=out)
    print(f"DOLP in [{res['dolp_min']:.6g}, {res['dolp_max']:.6g}]   AOLP in [{res['aolp_min']:.6g}, {res['aolp_max']:.6g}]", file=out)
    if res["n"] and np.isfinite(res["xolp_std"]) and res["xolp_std"] > 0:
        print("PD_XOLP_NORM=" + polar.format_xolp_norm((res["xolp_mean"], res["xolp_std"])), file=out)
    else:
        print("PD_XOLP_NORM: no pair (no pixel counted, or a zero standard deviation)", file=out)
    if hist:
        for name, h, lo, hi in (("DOLP", res["hist_dolp"][:256], 0.0, 1.0), ("AOLP", res["hist_aolp"], -np.pi / 2, np.pi / 2)):
            coarse = h.reshape(16, 16).sum(1)
            top = max(int(coarse.max()), 1)
            for k, c in enumerate(coarse):
                a, b = lo + (hi - lo) * k / 16, lo + (hi - lo) * (k + 1) / 16
                print(f"{name} [{a:+.3f}, {b:+.3f})  {int(c):>12d}  " + "#" * int(round(40 * int(c) / top)), file=out)
            if name == "DOLP":
                print(f"DOLP >= 1            {int(res['hist_dolp'][256]):>12d}", file=out)


def to_json(res):
    out = {}
    for k, v in res.items():
        out[k] = v.tolist() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, tuple) else v)
    return out


# ------------------------------------------------------------------------------------------------------- --time
def time_numpy(frames=46, shape=(832, 1088), repeats=3):
    """The eight reductions of xolp_mean_and_std_dev.py:25-30 on fp64 stacks of its size, one core."""
    rng = np.random.default_rng(0)
    dolp = rng.random((frames,) + shape) * 0.6
    aolp = (rng.random((frames,) + shape) - 0.5) * np.pi
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        vals = [dolp.mean(axis=(0, 1, 2)), dolp.std(axis=(0, 1, 2)), aolp.mean(axis=(0, 1, 2)), aolp.std(axis=(0, 1, 2)),
                0.5 * (dolp.mean(axis=(0, 1, 2)) + aolp.mean(axis=(0, 1, 2))),
                0.5 * (dolp.std(axis=(0, 1, 2)) + aolp.std(axis=(0, 1, 2)))]
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"path": "numpy", "frames": frames, "shape": list(shape), "pixels": frames * shape[0] * shape[1],
            "ms": round(ts[len(ts) // 2] * 1e3, 1), "ms_min": round(ts[0] * 1e3, 1),
            "ns_per_pixel": round(ts[len(ts) // 2] * 1e9 / (frames * shape[0] * shape[1]), 3), "xolp_mean": float(vals[4])}


def time_device(kind, B=16, H=512, W=640, iters=20, sets=16):
    import torch
    from polardepth import polar, synthetic
    from polardepth._lib import lib, check, ptr, stream_ptr
    if not torch.cuda.is_available():
        raise RuntimeError("tools/xolp_stats.py --time needs the GPU for the device pass; there is no CPU fallback")
    bufs = []
    for s in range(sets):
        if kind == "smooth":        # K1's output on the planes of synthetic items
            pol = synthetic.make_batch(B, H, W, frame_w=W, device="cuda", seed=s)[("pol", 0, 0)]
            x = polar.polar_forward(pol, want=("xolp",))["xolp"]
        elif kind == "iid":
            g = torch.Generator(device="cuda").manual_seed(s)
            x = torch.rand((B, 2, H, W), generator=g, device="cuda")
            x[:, 1] = (x[:, 1] - 0.5) * np.pi
        else:                       # one bin for every pixel
            x = torch.full((B, 2, H, W), 0.25, device="cuda")
        bufs.append(x.contiguous())
    acc = polar.XolpStats("cuda")
    acc.add(bufs[0])                # sizes the workspace
    nbytes = bufs[0].numel() * 4

    def stats_call(x):
        check(lib.pd_xolp_stats(ptr(x), None, ptr(acc._record), ptr(acc._ws), acc._ws.numel(), B, H, W, W, acc._thr, 0,
                                stream_ptr()), "pd_xolp_stats")

    def run(fn):
        for x in bufs:
            fn(x)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in evs:
            e0.record()
            for x in bufs:
                fn(x)
            e1.record()
        torch.cuda.synchronize()
        ts = sorted(e0.elapsed_time(e1) / len(bufs) for e0, e1 in evs)
        return ts[iters // 2], ts[0]

    read_ms, read_min = run(lambda x: x.sum())
    ms, ms_min = run(stats_call)
    read_ms2, _ = run(lambda x: x.sum())                    # the read again, after: the spread of the comparator
    gbps = lambda t: round(nbytes / (t * 1e-3) / 1e9, 1)
    return {"path": "device", "data": kind, "B": B, "H": H, "W": W, "sets": sets, "bytes": nbytes, "ms": round(ms, 5),
            "ms_min": round(ms_min, 5), "GBps": gbps(ms), "read_ms": round(read_ms, 5), "read_ms_after": round(read_ms2, 5),
            "read_GBps": gbps(read_ms), "fraction_of_read": round(read_ms / ms, 3), "n": acc.result()["n"]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data_path", default=None, help="a HAMMER tree, or 'synthetic'")
    ap.add_argument("--split", default="HAMMER")
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--num_workers", type=int, default=0)
    ap.add_argument("--every", type=int, default=1, help="take every N-th item")
    ap.add_argument("--batches", type=int, default=0, help="stop after this many batches (0: the whole split)")
    ap.add_argument("--pol_calibration", default=None, help="a calibration file of tools/dofp_calibrate.py (or $PD_POL_CALIBRATION)")
    ap.add_argument("--json", default=None, help="write the result to this file")
    ap.add_argument("--hist", action="store_true", help="print coarse histograms")
    ap.add_argument("--time", action="store_true", help="measure instead (see the head of this file)")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args(argv)
    if args.time:
        print(json.dumps(time_numpy()), flush=True)
        for kind in ("smooth", "iid", "constant"):
            print(json.dumps(time_device(kind, iters=args.iters)), flush=True)
        return
    if args.data_path is None:
        ap.error("--data_path is required (a HAMMER tree, or 'synthetic')")
    res = measure(args)
    report(res, args.hist)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(to_json(res), f, indent=1)


if __name__ == "__main__":
    main()
