"""The recorded routing table of the convolutions: one deterministic sweep of layer shapes and flag words, and at every point
what the host queries answer -- pd_conv2d_uses_x3 / _uses_bf16 / pd_conv2d_tile_m and the profiler label of ops._igemm_label
(forward / data gradient), pd_conv2d_wgrad_uses_x3 / _uses_bf16 / pd_conv2d_wgrad_workspace (weight gradient).

tests/golden/conv_routes.npz holds the answers of the commit BEFORE the routing moved behind route_conv / route_wgrad
(its `commit` entry names it); tests/test_conv_routes.py replays the sweep against the built library.  The fixture is never
rewritten from the code under test.  To record the table of another checkout (built: `make -C <package>/csrc`):

    python tests/conv_routes.py --write --package <checkout>/supervised-depth-estimation-from-polarized-images_amd --commit <hash>
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_routes.npz")

PLANES = [(256, 320), (128, 160), (64, 80), (32, 40), (16, 20), (34, 42), (150, 150), (8, 12), (512, 640)]
CHANS = [(64, 64), (128, 128), (256, 512), (512, 512), (96, 32), (32, 96), (64, 32), (36, 64), (12, 64), (8, 64), (16, 16), (48, 64), (100, 64)]
KS = (1, 3, 4, 5, 7)
BATCHES = (1, 2, 16)
STRIDES = (1, 2)
# (act, has_out_scale, grid known): none | ELU | ReLU | folded BatchNorm scale | unknown output grid (Ho = Wo = 0)
EPILOGUES = ((0, 0, True), (2, 0, True), (1, 0, True), (0, 1, True), (0, 0, False))
FLAGS = (0, 1, 2, 4, 8, 16, 32, 128, 128 | 16, 128 | 32, 128 | 1)


def fwd_points():
    """(M, Cout, C, k, stride, pad, mode, act, scale, Ho, Wo, flags): the plane is the OUTPUT grid."""
    for (H, W), (C, Co), k, N, mode, s, (act, scale, grid), fl in itertools.product(PLANES, CHANS, KS, BATCHES, (0, 1, 2), STRIDES,
                                                                                  EPILOGUES, FLAGS):
        yield (N * H * W, Co, C, k, s, k // 2, mode, act, scale, H if grid else 0, W if grid else 0, fl)


def wgrad_points():
    """(M, Cout, C, k, stride, pad, mode, H, W, Ho, Wo, flags): the plane is the output grid, the input grid `stride` times it."""
    for (H, W), (C, Co), k, N, mode, s, fl in itertools.product(PLANES, CHANS, KS, BATCHES, (0, 1), STRIDES, FLAGS):
        yield (N * H * W, Co, C, k, s, k // 2, mode, H * s, W * s, H, W, fl)


def record(lib, ops):
    """The answers of `lib` (and of `ops._igemm_label`, with vec=True) over the sweep, as arrays in sweep order."""
    names, x3, bf16, tile, label = {}, [], [], [], []
    for (M, Co, C, k, s, pad, mode, act, scale, Ho, Wo, fl) in fwd_points():
        x3.append(lib.pd_conv2d_uses_x3(M, Co, C, k, k, s, pad, mode, act, scale, Ho, Wo, fl))
        bf16.append(lib.pd_conv2d_uses_bf16(M, Co, C, k, k, s, pad, mode, act, scale, Ho, Wo, fl))
        tile.append(lib.pd_conv2d_tile_m(M, Co))
        name = ops._igemm_label(M, Co, True, "fwd", C, k, k, s, pad, mode, act, bool(scale), (Ho, Wo), fl)
        label.append(names.setdefault(name, len(names)))
    wx3, wbf16, ws = [], [], []
    for (M, Co, C, k, s, pad, mode, H, W, Ho, Wo, fl) in wgrad_points():
        wx3.append(lib.pd_conv2d_wgrad_uses_x3(M, Co, C, k, k, s, pad, mode, H, W, Ho, Wo, fl))
        wbf16.append(lib.pd_conv2d_wgrad_uses_bf16(M, Co, C, k, k, s, pad, mode, H, W, Ho, Wo, fl))
        ws.append(lib.pd_conv2d_wgrad_workspace(M, Co, k * k * C, fl))
    return {"fwd_x3": np.array(x3, np.int8), "fwd_bf16": np.array(bf16, np.int8), "fwd_tile_m": np.array(tile, np.int16),
            "fwd_label": np.array(label, np.int8), "label_names": np.array(sorted(names, key=names.get)),
            "wgrad_x3": np.array(wx3, np.int8), "wgrad_bf16": np.array(wbf16, np.int8), "wgrad_workspace": np.array(ws, np.int64)}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help="write tests/golden/conv_routes.npz (default: print a summary only)")
    ap.add_argument("--package", default=os.path.join(ROOT, "supervised-depth-estimation-from-polarized-images_amd"),
                    help="directory that holds the built `polardepth` package to record")
    ap.add_argument("--commit", default="", help="the commit of that checkout, stored in the fixture")
    opt = ap.parse_args()
    sys.path.insert(0, opt.package)
    from polardepth import _lib, ops
    assert os.path.dirname(os.path.abspath(_lib.lib.path)) == os.path.join(os.path.abspath(opt.package), "polardepth"), _lib.lib.path
    table = record(_lib.lib, ops)
    for key, v in table.items():
        print(key, len(v), dict(zip(*np.unique(v, return_counts=True))) if key not in ("wgrad_workspace", "label_names") else "")
    if opt.write:
        assert opt.commit, "--write needs --commit"
        np.savez_compressed(FIXTURE, commit=np.array(opt.commit), **table)
        print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
