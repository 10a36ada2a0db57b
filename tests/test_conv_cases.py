"""The case table of tests/conv_cases.py against the built library's host queries (no GPU): every row's call launches the
instantiation the row names, the rows cover every instantiation the launch functions can reach, and the exactness conditions
that make tests/test_conv_exact_gpu.py a bit-for-bit comparison hold on every row's generated data."""
import collections

import pytest
import torch

import conv_cases as cc
from polardepth import _lib

lib = _lib.lib
torch.set_num_threads(min(16, torch.get_num_threads()))


def test_flag_words_are_the_library_binding_s():
    from polardepth import ops
    assert (cc.FP32, cc.BF16X3, cc.SPLIT_REGS, cc.GENERAL, cc.IM2COL, cc.ROW_WG, cc.BF16) == (
        ops.CONV_FP32_MFMA, ops.CONV_BF16X3, ops.CONV_WGRAD_SPLIT_IN_REGS, ops.CONV_GENERAL_KERNELS, ops.CONV_X3_IM2COL,
        ops.CONV_WGRAD_ROW_WORKGROUPS, ops.CONV_BF16)
    assert (cc.ZERO, cc.REFLECT, cc.TRANSPOSED) == (ops.MODE_ZERO, ops.MODE_REFLECT, ops.MODE_TRANSPOSED)
    assert (cc.ACT_NONE, cc.ACT_RELU, cc.ACT_ELU) == (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_ELU)


def test_row_ids_are_unique():
    dup = [k for k, n in collections.Counter(r.id for r in cc.ROWS).items() if n > 1]
    assert not dup, dup


@pytest.mark.parametrize("row", cc.ROWS, ids=lambda r: r.id)
def test_row_launches_what_it_names(row):
    assert cc.instantiation(row, lib) == row.want


# the issue's table: (N, H, W, C, Cout, k), mode, flags -> (family, BN, BM) of pd_conv2d_route / code of pd_conv2d_wgrad_uses_x3
ROUTES = [
    ((1, 128, 128, 16, 512, 3), 0, 0, (3, 64, 256)), ((16, 64, 16, 16, 512, 5), 0, 0, (3, 64, 256)), ((64, 32, 8, 16, 512, 3), 1, 0, (3, 64, 256)),
    ((13, 32, 40, 16, 512, 5), 2, 0, (3, 64, 256)), ((1, 64, 128, 16, 512, 3), 0, 0, (3, 32, 256)), ((8, 64, 16, 16, 512, 3), 0, 0, (3, 32, 256)),
    ((32, 32, 8, 16, 512, 5), 0, 0, (3, 32, 256)), ((8, 128, 128, 16, 32, 3), 0, 0, (3, 32, 256)), ((3, 128, 128, 16, 96, 3), 0, 0, (3, 32, 256)),
    ((1, 128, 128, 4, 512, 4), 0, 0, (3, 64, 256)), ((1, 128, 128, 8, 512, 4), 0, 0, (3, 64, 256)), ((1, 128, 128, 36, 512, 4), 0, 0, (3, 64, 256)),
    ((1, 128, 128, 16, 512, 3), 0, cc.BF16, (4, 64, 256)), ((1, 128, 128, 8, 512, 3), 0, 0, (2, 64, 256)), ((1, 128, 128, 16, 512, 3), 0, cc.IM2COL, (2, 64, 256)),
    ((1, 8, 16, 64, 64, 3), 0, cc.BF16X3, (2, 64, 128)), ((1, 8, 16, 8, 64, 3), 0, cc.BF16X3, (2, 64, 128)), ((2, 8, 8, 64, 64, 5), 2, cc.BF16X3, (2, 64, 128)),
    ((1, 8, 16, 64, 64, 3), 1, cc.BF16X3, (2, 64, 128)), ((2, 16, 20, 64, 64, 3), 0, cc.GENERAL, (0, 64, 64)),
    ((1, 8, 8, 32, 64, 3), 0, cc.FP32, (1, 64, 64)), ((1, 16, 16, 32, 32, 3), 0, cc.FP32, (1, 32, 128)), ((1, 16, 16, 32, 16, 3), 0, cc.FP32, (0, 16, 128)),
    ((4, 128, 128, 32, 64, 3), 0, cc.FP32, (1, 64, 128)),
]
WROUTES = [
    ((1, 8, 32, 64, 64, 3), 0, 0, 2), ((1, 8, 16, 64, 64, 5), 0, 0, 2), ((1, 8, 8, 64, 64, 3), 0, 0, 2), ((1, 8, 4, 64, 64, 3), 0, 0, 2),
    ((1, 8, 32, 32, 32, 3), 1, 0, 2), ((1, 96, 32, 512, 512, 3), 0, 0, 3), ((1, 384, 32, 256, 256, 3), 0, 0, 3), ((2, 96, 16, 512, 512, 3), 0, 0, 3),
    ((1, 96, 32, 512, 512, 3), 0, cc.ROW_WG, 2), ((1, 6, 18, 64, 64, 3), 0, 0, 1), ((1, 8, 16, 64, 64, 3), 0, cc.IM2COL, 1), ((1, 6, 18, 64, 64, 3), 1, 0, 1),
    ((1, 8, 16, 64, 64, 1), 0, 0, 1), ((1, 6, 18, 64, 64, 3), 0, cc.FP32, 0), ((1, 6, 18, 64, 64, 3), 0, cc.SPLIT_REGS, 0), ((1, 6, 18, 64, 64, 3), 0, cc.GENERAL, 0),
    ((1, 6, 18, 64, 32, 3), 0, 0, 0),
]


@pytest.mark.parametrize("shape,mode,flags,want", ROUTES)
def test_route_words_as_tabulated(shape, mode, flags, want):
    N, H, W, C, Co, k = shape
    r = cc.Row("fwd", N, H, W, C, Co, k, "", mode=mode, flags=flags, out_hw=(H, W))
    assert cc.route_word(r, lib) == want
    assert lib.pd_conv2d_uses_bf16(r.M, Co, C, k, k, 1, k // 2, mode, 0, 0, H, W, flags) == (3 if want[0] == 4 else 0)


@pytest.mark.parametrize("shape,mode,flags,want", WROUTES)
def test_wgrad_codes_as_tabulated(shape, mode, flags, want):
    N, H, W, C, Co, k = shape
    assert lib.pd_conv2d_wgrad_uses_x3(N * H * W, Co, C, k, k, 1, k // 2, mode, H, W, H, W, flags) == want


def test_s2_phase_launches_run_the_uniform_tap_kernel():
    """The four parity-class launches of the stride-2 data gradient: 1x1, 1x2, 2x1, 2x2 transposed sub-filters."""
    r = next(r for r in cc.ROWS if r.call == "s2 phases")
    for ph, pw in ((0, 0), (0, 1), (1, 0), (1, 1)):
        q = cc.Row("rect", r.N, r.H, r.W, r.C, r.Co, 1 + ph, "", kw=1 + pw, pad=ph, pad_w=pw, mode=cc.TRANSPOSED, out_hw=(r.H, r.W))
        assert cc.route_word(q, lib)[0] in (1, 2)      # (a shape the bf16-split gather kernel takes at the network's sizes)


def test_rows_cover_every_reachable_instantiation():
    named = set(cc.INSTANTIATIONS)
    assert len(named) == len(cc.INSTANTIATIONS)
    # the counts the launch functions spell out: 24 general + 18 uniform-tap + 6 gather x3 + 2 x 28 halo; 12 + 10 + 6 slices,
    # 2 x (14 + 2) wgrad halo, 2 x 4 rolling rows
    count = collections.Counter(k.split("<")[0] for k in named)
    assert (count["igemm"], count["uni"], count["x3"], count["halo"]) == (24, 18, 6, 56)
    assert (count["wgen"], count["wuni"], count["x3c"], count["whalo"], count["wroll"]) == (12, 10, 6, 32, 8)
    assert set(cc.UNREACHABLE) <= named
    covered = {r.want for r in cc.ROWS}
    assert covered <= named, covered - named
    assert not (covered & set(cc.UNREACHABLE)), "a row reaches an instantiation listed as unreachable"
    missing = named - covered - set(cc.UNREACHABLE)
    assert not missing, sorted(missing)


def test_rows_cover_both_statistics_heights():
    got = {cc.stats_height(r, lib) for r in cc.ROWS if r.stats}
    assert got >= cc.STATS_HEIGHTS, cc.STATS_HEIGHTS - got


def test_rows_cover_the_named_edge_cases():
    rows = cc.ROWS
    fwd = [r for r in rows if r.call in ("fwd", "dgrad", "dgrad+addend", "rect")]
    assert any(r.stride == 2 and r.call == "fwd" for r in fwd) and any(r.stride == 2 and r.transposed for r in fwd)
    assert any(r.call == "rect" and r.ph != r.pw for r in rows)
    assert any(r.nchw and r.affine for r in fwd) and any(r.C % 4 for r in fwd)
    assert {1, 16, 24} <= {r.Co for r in fwd}
    assert any(r.N > 1 and (r.grid[0] * r.grid[1]) % 64 for r in fwd)                   # a tile spans two images
    assert any(r.transposed and r.M % 128 and r.want.startswith("x3<") for r in fwd)
    assert any(r.accumulate for r in rows if r.call == "wgrad")
    assert {(r.N, r.C if r.c16_mode == 0 else r.Co, r.H, r.W) for r in rows if r.call == "conv16"} == {(1, 16, 2, 2), (2, 16, 9, 35), (1, 32, 13, 7)}
    assert {r.c16_mode for r in rows if r.call == "conv16"} == {0, 1, 2}
    assert {r.addend for r in fwd} >= {"own", "view"}
    assert {r.act for r in fwd} >= {cc.ACT_RELU, cc.ACT_ELU} and any(r.scale for r in fwd)
    # class S: one case per kernel family (and mode, for the forward families)
    s = {r.want.split(",t")[0].split("<")[0] + ("/" + cc.MODE_NAMES[r.mode] if r.call != "wgrad" else "") for r in rows if r.s}
    assert s >= {"halo/zero", "halo/reflect", "halo/transposed", "x3/zero", "x3/reflect", "x3/transposed", "uni/zero", "x3c", "wuni", "whalo", "wroll"}, s
    assert any(r.s and r.flags & cc.BF16 for r in rows if r.call == "wgrad") and any(r.s and r.flags & cc.BF16 for r in fwd)


@pytest.mark.parametrize("v", cc.variants(), ids=cc.vid)
def test_exactness_conditions_hold(v):
    row, cls, role = v
    cc.check_conditions(row, cls, role)
    if cls == "E8":
        assert cc.check_fp32_cpu(row), "fp32 on the CPU does not reproduce the fp64 reference: the case is not exactly summable"
