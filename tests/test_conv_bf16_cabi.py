"""PD_CONV_BF16, the opt-in bf16 training mode of the convolutions: flag validation and the routing queries
pd_conv2d_uses_bf16 / pd_conv2d_wgrad_uses_bf16 (host logic, no GPU)."""
import itertools
import os
import re

from conftest import ROOT

from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
BF16 = 128
AUTO, FP32, X3, REGS, GEN, IM2COL, ROWWG = 0, 1, 2, 4, 8, 16, 32
M16 = 16 * 256 * 320


def _define(name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)u", open(HEADER).read())
    assert m, name
    return int(m.group(1))


def test_flag_is_declared():
    assert _define("PD_CONV_BF16") == BF16 == ops.CONV_BF16
    assert _define("PD_CONV_FLAGS_ALL") & BF16
    assert not _define("PD_CONV_FLAGS_ALL") & 64            # bit 64 stays unassigned
    with ops.conv_flags(conv=ops.CONV_BF16, wgrad=ops.CONV_BF16):
        assert ops.conv_bf16_mode() == (True, True)
    assert ops.conv_bf16_mode() == (False, False)


def test_bf16_excludes_the_other_arithmetics():
    """128 | 1 and 128 | 2: PD_EINVAL with "flags" before anything else is looked at; 128 alone passes the flags check (the
    null tensor is then the complaint)."""
    lib = _lib.lib
    for bad in (BF16 | FP32, BF16 | X3, BF16 | 64):
        rc = lib.pd_conv2d(8, 8, None, None, 8, None, 1, 4, 4, 4, 64, 16, 4, 1, 4, 4, 4, 1, 1, 1, 0, 0, 0, 0, 0.0, 1.0, 4, bad, None)
        assert rc == -22 and b"flags" in lib.pd_last_error(), bad
        rc = lib.pd_conv2d_wgrad(8, 8, 8, None, 8, 1 << 20, 1, 4, 4, 4, 64, 16, 4, 1, 4, 4, 4, 1, 1, 1, 0, 0, 0, 0.0, 1.0, 4, 0, bad, None)
        assert rc == -22 and b"flags" in lib.pd_last_error(), bad
        assert lib.pd_conv2d_uses_bf16(M16, 64, 64, 3, 3, 1, 1, 0, 0, 0, 256, 320, bad) == 0
    for ok in (BF16, BF16 | IM2COL, BF16 | ROWWG, BF16 | GEN, BF16 | REGS):
        rc = lib.pd_conv2d(8, 8, None, None, None, None, 1, 4, 4, 4, 64, 16, 4, 1, 4, 4, 4, 1, 1, 1, 0, 0, 0, 0, 0.0, 1.0, 4, ok, None)
        assert rc == -22 and b"flags" not in lib.pd_last_error() and b"null" in lib.pd_last_error(), ok
        rc = lib.pd_conv2d_wgrad(8, 8, None, None, 8, 1 << 20, 1, 4, 4, 4, 64, 16, 4, 1, 4, 4, 4, 1, 1, 1, 0, 0, 0, 0.0, 1.0, 4, 0, ok, None)
        assert rc == -22 and b"flags" not in lib.pd_last_error() and b"null" in lib.pd_last_error(), ok


def test_the_networks_big_layers_take_the_bf16_kernels():
    """Arguments as pd_conv2d_uses_x3 / pd_conv2d_wgrad_uses_x3: M, Cout, C, KH, KW, stride, pad, mode, act | H, W, scale."""
    lib = _lib.lib
    q, qw = lib.pd_conv2d_uses_bf16, lib.pd_conv2d_wgrad_uses_bf16
    # forward, data gradient and weight gradient of the 5x5 / 3x3 64 -> 64 layers at batch 16
    for k, (H, W) in itertools.product((3, 5), ((256, 320), (128, 160), (64, 80))):
        M = 16 * H * W
        if (k, H) == (5, 64):
            continue                 # (5x5 runs at 256x320 only)
        assert q(M, 64, 64, k, k, 1, k // 2, 0, 0, 0, H, W, BF16) == 3, (k, H)
        assert q(M, 64, 64, k, k, 1, k // 2, 2, 0, 0, H, W, BF16) == 3, (k, H)
        assert qw(M, 64, 64, k, k, 1, k // 2, 0, H, W, H, W, BF16) in (2, 3), (k, H)
    assert qw(M16, 64, 64, 3, 3, 1, 1, 0, 256, 320, 256, 320, BF16) == 3                 # rolling rows
    assert qw(M16, 64, 64, 3, 3, 1, 1, 0, 256, 320, 256, 320, BF16 | ROWWG) == 2         # ... or one filter row per workgroup
    assert qw(M16, 64, 64, 5, 5, 1, 2, 0, 256, 320, 256, 320, BF16) == 2
    # decoder: reflection-padded 3x3 + ELU, 128 -> 64 and 96 -> 32 (32-column workgroups)
    assert q(M16 // 4, 64, 128, 3, 3, 1, 1, 1, 2, 0, 128, 160, BF16) == 3
    assert qw(M16 // 4, 64, 128, 3, 3, 1, 1, 1, 128, 160, 128, 160, BF16) == 3
    assert q(M16, 32, 96, 3, 3, 1, 1, 1, 2, 0, 256, 320, BF16) == 3
    assert qw(M16, 32, 96, 3, 3, 1, 1, 1, 256, 320, 256, 320, BF16) == 2
    # 4x4 space-to-depth stems (C = 4 x 3 | 4 x 9 | 4 x 2)
    for c in (12, 36, 8):
        assert q(M16, 64, c, 4, 4, 1, 2, 0, 0, 0, 256, 320, BF16) == 3, c
    # what keeps its arithmetic: 1x1, stride 2, folded scale, ReLU / sigmoid epilogues, no tile grid, the gather-kernel flag
    assert q(M16, 64, 64, 1, 1, 1, 0, 0, 0, 0, 256, 320, BF16) == 0
    assert q(M16 // 4, 128, 64, 3, 3, 2, 1, 0, 0, 0, 128, 160, BF16) == 0
    assert q(M16, 64, 64, 3, 3, 1, 1, 0, 0, 1, 256, 320, BF16) == 0
    assert q(M16, 64, 64, 3, 3, 1, 1, 0, 1, 0, 256, 320, BF16) == 0
    assert q(M16, 64, 64, 3, 3, 1, 1, 0, 0, 0, 0, 0, BF16) == 0
    assert q(M16, 64, 64, 3, 3, 1, 1, 0, 0, 0, 256, 320, BF16 | IM2COL) == 0
    assert qw(M16, 64, 64, 3, 3, 2, 1, 0, 256, 320, 128, 160, BF16) == 0
    assert qw(M16, 64, 64, 3, 3, 1, 1, 0, 256, 320, 256, 320, BF16 | IM2COL) == 0
    # the same shapes without the flag: 0
    assert q(M16, 64, 64, 3, 3, 1, 1, 0, 0, 0, 256, 320, AUTO) == 0
    assert qw(M16, 64, 64, 3, 3, 1, 1, 0, 256, 320, 256, 320, AUTO) == 0


def _halo_rows(k, C, Co):
    """Partial rows conv_wgrad_halo_bf16_kernel writes before any cap (conv_wgrad_halo.hpp: wgrad_halo_slices)."""
    co32 = Co % 64 != 0
    per = k * ((C + 63) // 64) * (Co // 32 if co32 else Co // 64)
    return max(1, (768 if k == 3 else 512) // max(per, 1)) * (2 if co32 else 1)


def test_bf16_routing_queries_over_a_shape_sweep():
    """Over the sweep of test_cabi.py's routing test: documented codes only; 0 for every shape without the flag; with it,
    exactly the shapes the split queries send to the halo-tile / rolling-row kernels (per-layer fallback otherwise), and a
    workspace of pd_conv2d_wgrad_workspace(flags) bytes holds every slice those kernels plan -- their slice count never
    depends on a larger caller workspace."""
    lib = _lib.lib
    planes = [(256, 320), (128, 160), (64, 80), (32, 40), (16, 20), (34, 42), (150, 150), (8, 12), (512, 640)]
    chans = [(64, 64), (128, 128), (256, 512), (512, 512), (96, 32), (32, 96), (64, 32), (36, 64), (12, 64), (8, 64), (16, 16), (48, 64), (100, 64)]
    seen = set()
    for (H, W), (C, Co), k, N, mode, extra in itertools.product(planes, chans, (1, 3, 4, 5), (1, 16), (0, 1, 2), (0, 4, 8, 16, 32)):
        if mode == 1 and k != 3:
            continue
        M, pad = N * H * W, k // 2
        assert lib.pd_conv2d_uses_bf16(M, Co, C, k, k, 1, pad, mode, 0, 0, H, W, extra) == 0
        a = lib.pd_conv2d_uses_bf16(M, Co, C, k, k, 1, pad, mode, 0, 0, H, W, BF16 | extra)
        assert a in (0, 3)
        assert a == (3 if lib.pd_conv2d_uses_x3(M, Co, C, k, k, 1, pad, mode, 0, 0, H, W, extra) == 3 else 0)
        if mode == 2:
            continue
        assert lib.pd_conv2d_wgrad_uses_bf16(M, Co, C, k, k, 1, pad, mode, H, W, H, W, extra) == 0
        b = lib.pd_conv2d_wgrad_uses_bf16(M, Co, C, k, k, 1, pad, mode, H, W, H, W, BF16 | extra)
        assert b in (0, 2, 3)
        x3 = lib.pd_conv2d_wgrad_uses_x3(M, Co, C, k, k, 1, pad, mode, H, W, H, W, extra)
        assert b == (x3 if x3 in (2, 3) else 0), (H, W, C, Co, k, N, mode, extra, b, x3)
        ws = lib.pd_conv2d_wgrad_workspace(M, Co, k * k * C, BF16 | extra)
        per = 4 * (Co * k * k * C + Co)
        if b == 2:
            # (the workspace query bounds the partial rows by one per 64 pixels: the kernel then plans that many)
            assert ws // per >= min(_halo_rows(k, C, Co), (M + 63) // 64), (H, W, C, Co, k, N)
        if b == 3:
            assert ws // per >= 512 // ((C // 64) * (Co // 64)) and (ws // per) * (C // 64) * (Co // 64) >= 384
        seen.add((a, b))
    assert (3, 3) in seen and (3, 2) in seen and (0, 0) in seen
