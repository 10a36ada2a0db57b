"""Shared by tests/test_conv_cases.py (CPU) and tests/test_conv_exact_gpu.py (GPU): the case table of the K2 convolutions
(csrc/conv.hip, conv_x3_halo.hpp, conv_wgrad_halo.hpp, conv_wgrad_roll.hpp, conv16.hip), the input generators, the fp64
references, the exactness conditions as code, and the list of every kernel instantiation the launch functions can reach.

No tolerance is chosen anywhere.  The operands are built so that every product and every partial sum, in any order, is an
fp32 number; every kernel family -- fp32 MFMA, three-way bf16 split, single bf16 -- must then return the bits of the fp64
convolution, and the assertion is torch.equal.

  class E8   x, w, dy, bias, addend: small integers (|v| <= 3, or <= 1 where BatchNorm sums of squares need it).  bf16
             conversion is exact (hi = v, mid = lo = 0).  Condition: K * max|a| * max|b| + max|bias| < 2^24 with K the
             contraction length -- an upper bound of conv(|x|, |w|).max() + |bias|.max() computed from the case's data; for
             the statistics sum|y| and sum y^2 < 2^24 per column.
  class S    one operand "wide": m * 2^-18, |m| < 2^18, three quarters of them built with a 9-bit odd remainder under the
             leading 8 bits, so the third split term v - bf16(v) - bf16(v - bf16(v)) is non-zero; the other "narrow and
             sparse": {0, +-0.5, +-1, +-2} with few non-zeros along each contraction.  Condition: sum|a||b| <= 16 along every
             contraction, evaluated as the fp64 convolution of the absolute values.  Every product is a multiple of 2^-19 below
             2^5: 24 bits.  Each S row runs twice, roles swapped ("xw": wide activations, "wx": wide weights / dy).  Under
             PD_CONV_BF16 the reference is the fp64 convolution of the operands rounded RNE to bf16.
             The bias gradient of a wide dy sums thousands of 18-bit values and is not exactly summable: it is not compared
             in role "wx".

Class-S measurement on the MI355X (the bf16 MFMA aligns its addends by truncation; whether 24 bits below the largest
addend survive was not known beforehand): bit-exact at the first dynamic range, m * 2^-18 with up to 8 non-zeros per
contraction, for every split family and for the single-bf16 forms (against the RNE-rounded operands) -- all 82 class-S runs.
The fallback foreseen for a failure (m * 2^-16, |v| < 0.5, 4 non-zeros) was therefore not needed and is not built (S_OUTCOME).

A row's `want` names the instantiation that must run; `instantiation(row, lib)` derives it from the library's host queries
(pd_conv2d_route; pd_conv2d_wgrad_uses_x3 / _uses_bf16) and from the rules the headers state next to the launch functions
(halo tile width, ring depth, lean walker, scalar-pixel eligibility -- the queries answer code 0 for all three of UNI, UNI_X3 and
GENERAL, so those are told apart here by the predicate of route_wgrad).
"""
import dataclasses
import functools
import itertools
import zlib

import torch
import torch.nn.functional as F

FP32, BF16X3, SPLIT_REGS, GENERAL, IM2COL, ROW_WG, BF16 = 1, 2, 4, 8, 16, 32, 128
ZERO, REFLECT, TRANSPOSED = 0, 1, 2
MODE_NAMES = ("zero", "reflect", "transposed")
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2
ELU_TOL = 3e-5          # this suite's ELU tolerance (tests/test_conv_gpu.py), for z < 0 only
S_OUTCOME = (
    "bit-exact at the first dynamic range.  "
    "All 82 class-S runs (41 rows, roles swapped) -- halo-tile and gather kernels in their three modes, the row-window form, "
    "the in-register split, x3c, halo-tile and rolling-row weight gradients, and the single-bf16 forms against the RNE-rounded "
    "operands -- return the fp64 bits with m * 2^-18 and up to 8 non-zeros per contraction; the halved range (m * 2^-16, "
    "4 non-zeros) was not needed and is not built.")

F64 = torch.float64


# ====================================================================================================== the rows
@dataclasses.dataclass(frozen=True)
class Row:
    """call: fwd | dgrad | dgrad+addend | rect | wgrad | conv16 | conv16_wgrad | s2 phases | reflect bwd.
    (N, H, W, C) is the grid and channel count of the tensor the kernel READS (x; for data gradients dy), Co the columns it
    writes, k the filter.  pad < 0: k // 2.  out_hw None: the same-size grid (stride 1), H * stride for a data gradient of
    stride 2, the full forward grid otherwise."""
    call: str
    N: int
    H: int
    W: int
    C: int
    Co: int
    k: int
    want: str
    kw: int = 0                 # filter columns when they differ from k (rect)
    stride: int = 1
    pad: int = -1
    pad_w: int = -1
    mode: int = ZERO
    flags: int = 0
    act: int = ACT_NONE
    bias: bool = False
    scale: bool = False
    affine: tuple = None
    addend: str = None          # "own" | "view"
    stats: bool = False
    amp: int = 3
    out_hw: tuple = None
    accumulate: bool = False
    nchw: bool = False
    s: bool = False             # also run in class S
    c16_mode: int = 0

    @property
    def KH(self):
        return self.k

    @property
    def KW(self):
        return self.kw or self.k

    @property
    def ph(self):
        return self.k // 2 if self.pad < 0 else self.pad

    @property
    def pw(self):
        return self.ph if self.pad_w < 0 else self.pad_w

    @property
    def transposed(self):
        return self.mode == TRANSPOSED

    @property
    def grid(self):
        """Output grid of forward-like calls; dy grid of weight gradients."""
        if self.out_hw is not None:
            return self.out_hw
        if self.transposed:
            if self.stride == 1:
                return (self.H - 1 - 2 * self.ph + self.KH, self.W - 1 - 2 * self.pw + self.KW)
            return (self.H * self.stride, self.W * self.stride)
        return ((self.H + 2 * self.ph - self.KH) // self.stride + 1, (self.W + 2 * self.pw - self.KW) // self.stride + 1)

    @property
    def M(self):
        return self.N * self.grid[0] * self.grid[1]

    @property
    def K(self):
        return self.KH * self.KW * self.C

    @property
    def vec(self):
        return self.C % 4 == 0 and not self.nchw and self.affine is None

    @property
    def id(self):
        f = "".join(n for b, n in ((FP32, "F"), (BF16X3, "X"), (SPLIT_REGS, "R"), (GENERAL, "G"), (IM2COL, "I"), (ROW_WG, "W"), (BF16, "B"))
                    if self.flags & b)
        e = "".join(n for c, n in ((self.bias, "b"), (self.scale, "s"), (self.affine, "a"), (self.addend, "+"), (self.stats, "n"),
                                   (self.act == ACT_RELU, "r"), (self.act == ACT_ELU, "e"), (self.accumulate, "A"), (self.nchw, "p")) if c)
        kk = f"{self.KH}x{self.KW}" + (f"s{self.stride}" if self.stride > 1 else "") + (f"p{self.ph}{self.pw}" if self.pad >= 0 else "")
        return f"{self.call.replace(' ', '_')}-{self.N}x{self.H}x{self.W}x{self.C}-{self.Co}-{kk}-{MODE_NAMES[self.mode]}-{f or '0'}-{e or '0'}"

    @property
    def data_key(self):
        """Everything the data and the reference depend on: rows that differ in `flags` and `want` only share both."""
        return dataclasses.replace(self, want="", flags=0, s=False)


def _fwd(N, H, W, C, Co, k, want, mode=ZERO, **kw):
    return Row("dgrad" if mode == TRANSPOSED and "call" not in kw else kw.pop("call", "fwd"), N, H, W, C, Co, k, want, mode=mode, **kw)


def _rows():
    rows = []
    # ---- halo-tile kernel: (k, tw, ncb) x mode x terms.  Cout = 512 over C = 16: the smallest launches with 512 workgroups
    halo = [(3, 32, 2, (1, 128, 128)), (3, 16, 2, (16, 64, 16)), (3, 8, 2, (64, 32, 8)),
            (5, 32, 2, (1, 128, 128)), (5, 16, 2, (16, 64, 16)), (5, 8, 2, (13, 32, 40)),
            (3, 32, 1, (1, 64, 128)), (3, 16, 1, (8, 64, 16)), (5, 8, 1, (32, 32, 8))]
    for (k, tw, ncb, (N, H, W)), mode in itertools.product(halo, (ZERO, REFLECT, TRANSPOSED)):
        if mode == REFLECT and k == 5:
            continue        # x3_common_ok: reflection on the bf16-split kernels is ReflectionPad2d(1) + 3x3 only
        epi = ({"bias": True, "stats": True, "amp": 1} if mode == ZERO else {"bias": True, "act": ACT_ELU} if mode == REFLECT else
               {"call": "dgrad+addend", "addend": "view" if tw == 16 else "own"} if tw != 32 else {})
        for terms in (3, 1):
            rows.append(_fwd(N, H, W, 16, 512, k, f"halo<{k}x{k},tw{tw},ncb{ncb},{MODE_NAMES[mode]},t{terms}>", mode=mode,
                             flags=BF16 if terms == 1 else 0, s=(k, tw, ncb) in ((3, 32, 2), (5, 8, 1), (3, 16, 1)), **epi))
    for terms in (3, 1):
        fl = BF16 if terms == 1 else 0
        # 32-column workgroups through Cout = 32 (128-row statistics: Cout <= 32) and Cout = 96
        rows.append(_fwd(8, 128, 128, 16, 32, 3, f"halo<3x3,tw32,ncb1,zero,t{terms}>", flags=fl, stats=True, amp=1))
        rows.append(_fwd(3, 128, 128, 16, 96, 3, f"halo<3x3,tw32,ncb1,reflect,t{terms}>", mode=REFLECT, flags=fl))
        # row-window stems: a 4x4 filter over the space-to-depth input, the leading 128 x 128 outputs of the 129 x 129 grid
        for C in (4, 8, 36):
            rows.append(_fwd(1, 128, 128, C, 512, 4, f"halo<rowwin,t{terms}>", flags=fl, out_hw=(128, 128), bias=True, stats=C == 8,
                             amp=1 if C == 8 else 3, s=C == 4))
    # ---- bf16-split gather kernel
    for mode in (ZERO, REFLECT, TRANSPOSED):
        rows.append(_fwd(1, 128, 128, 8, 512, 3, f"x3<{MODE_NAMES[mode]},2>", mode=mode, s=True, stats=mode == ZERO, amp=1 if mode == ZERO else 3,
                         bias=mode != TRANSPOSED))
    rows.append(_fwd(1, 128, 128, 16, 512, 3, "x3<zero,2>", flags=IM2COL, act=ACT_ELU, bias=True))
    rows.append(_fwd(4, 128, 128, 16, 64, 3, "x3<zero,1>", flags=IM2COL, stats=True, amp=1))          # 128-row statistics
    rows.append(_fwd(1, 8, 16, 64, 64, 3, "x3<zero,1>", flags=BF16X3, s=True, stats=True, bias=True))
    rows.append(_fwd(1, 8, 16, 8, 64, 3, "x3<zero,1>", flags=BF16X3))
    rows.append(_fwd(2, 8, 8, 64, 64, 5, "x3<transposed,1>", mode=TRANSPOSED, flags=BF16X3, s=True))
    rows.append(_fwd(1, 8, 16, 64, 64, 3, "x3<reflect,1>", mode=REFLECT, flags=BF16X3, act=ACT_ELU, bias=True, s=True))
    rows.append(_fwd(1, 10, 16, 64, 64, 3, "x3<transposed,1>", mode=TRANSPOSED, flags=BF16X3))         # last 128-row tile partial
    rows.append(_fwd(1, 10, 16, 64, 64, 3, "x3<transposed,1>", mode=TRANSPOSED, flags=BF16X3, call="dgrad+addend", addend="view"))
    # ---- uniform-tap fp32 kernel: three tiles x three modes (ring depth by the rule of route_conv)
    for mode in (ZERO, REFLECT, TRANSPOSED):
        ns = 2 if mode == REFLECT else 3
        rows.append(_fwd(1, 8, 8, 32, 64, 3, f"uni<64,64,{MODE_NAMES[mode]},{ns}>", mode=mode, flags=FP32, s=mode == ZERO,
                         stats=mode != TRANSPOSED, bias=mode == REFLECT, act=ACT_RELU if mode == REFLECT else ACT_NONE))
        rows.append(_fwd(1, 16, 16, 32, 32, 3, f"uni<128,32,{MODE_NAMES[mode]},2>", mode=mode, flags=FP32, stats=mode == ZERO,
                         scale=mode == REFLECT, bias=mode == REFLECT))
        rows.append(_fwd(4, 128, 128, 32, 64, 3, f"uni<128,64,{MODE_NAMES[mode]},2>", mode=mode, flags=FP32, stats=mode == ZERO,
                         amp=1 if mode == ZERO else 3))
    rows.append(_fwd(3, 5, 7, 32, 64, 3, "uni<64,64,zero,3>", flags=FP32, stats=True, bias=True))      # tiles span images, M tail
    rows.append(_fwd(3, 5, 7, 32, 64, 3, "uni<64,64,transposed,3>", mode=TRANSPOSED, flags=FP32, call="dgrad+addend", addend="own"))
    rows.append(_fwd(2, 16, 20, 64, 128, 3, "uni<64,64,zero,3>", stride=2, flags=FP32, stats=True))     # stride 2 forward
    # ---- general kernel: four tiles x vec / scalar x three modes
    gen = [(128, 64, (4, 128, 128), 16, 3, 64), (64, 64, (2, 16, 20), 64, 6, 64), (128, 32, (1, 16, 16), 32, 5, 24), (128, 16, (1, 16, 16), 48, 5, 16)]
    for (bm, bn, (N, H, W), cv, cs, Co), mode in itertools.product(gen, (ZERO, REFLECT, TRANSPOSED)):
        epi = {"bias": True, "stats": True, "act": ACT_RELU, "amp": 1 if bm == 128 and bn == 64 else 3} if mode == ZERO else \
              {"bias": True, "act": ACT_ELU, "scale": True} if mode == REFLECT else {}
        rows.append(_fwd(N, H, W, cv, Co, 3, f"igemm<{bm},{bn},vec,{MODE_NAMES[mode]}>", mode=mode, flags=FP32 | GENERAL, **epi))
        rows.append(_fwd(N, H, W, cs, Co, 3, f"igemm<{bm},{bn},scalar,{MODE_NAMES[mode]}>", mode=mode, **epi))
    rows.append(_fwd(2, 9, 11, 5, 1, 3, "igemm<128,16,scalar,reflect>", mode=REFLECT, bias=True))        # Cout = 1
    rows.append(_fwd(2, 32, 40, 2, 64, 7, "igemm<64,64,scalar,zero>", stride=2, nchw=True, affine=(2.0, 0.5), bias=True, stats=True, amp=1))
    rows.append(_fwd(1, 32, 40, 9, 64, 7, "igemm<64,64,scalar,zero>", stride=2, nchw=True, affine=(-1.0, 4.0)))
    rows.append(_fwd(2, 8, 10, 64, 32, 3, "igemm<128,32,vec,transposed>", mode=TRANSPOSED, stride=2))   # masked transposed gather
    rows.append(_fwd(2, 8, 10, 64, 64, 3, "igemm<64,64,vec,transposed>", mode=TRANSPOSED, stride=2, call="dgrad+addend", addend="own"))
    # ---- pd_conv2d_rect: unequal paddings (the sub-filters of the stride-2 data gradient and their forward counterparts)
    rows.append(Row("rect", 2, 8, 10, 32, 64, 2, "uni<64,64,zero,3>", kw=1, pad=1, pad_w=0, out_hw=(8, 10), flags=FP32))
    rows.append(Row("rect", 2, 8, 10, 32, 64, 1, "uni<64,64,transposed,3>", kw=2, pad=0, pad_w=1, mode=TRANSPOSED, out_hw=(8, 10), flags=FP32))
    rows.append(Row("rect", 2, 8, 10, 32, 64, 2, "uni<64,64,transposed,3>", kw=2, pad=1, pad_w=0, mode=TRANSPOSED, out_hw=(8, 11)))
    # ---- stride-2 data gradient by output parity (pd_dgrad_s2_filters, four pd_conv2d_rect, pd_interleave4) through ops
    rows.append(Row("s2 phases", 2, 8, 10, 64, 32, 3, "s2 phases", stride=2, mode=TRANSPOSED))
    # ---- ReflectionPad2d(1) + conv3x3 backward: pd_reflect_dgrad_border | pd_reflect_fold (functional.reflect_conv_act, act none)
    rows.append(Row("reflect bwd", 2, 9, 11, 32, 64, 3, "reflect bwd", mode=REFLECT, bias=True))

    # ---- weight gradients
    def wg(N, H, W, C, Co, k, want, **kw):
        return Row("wgrad", N, H, W, C, Co, k, want, **kw)
    whalo = [(3, 32, (1, 8, 32)), (3, 16, (1, 8, 16)), (3, 8, (1, 8, 8)), (3, 4, (1, 8, 4)), (5, 32, (1, 8, 32)), (5, 16, (1, 8, 16)), (5, 8, (1, 8, 8))]
    for (k, tw, (N, H, W)), bias, terms in itertools.product(whalo, (True, False), (3, 1)):
        rows.append(wg(N, H, W, 64, 64, k, f"whalo<{k},tw{tw},bias{int(bias)},co64,t{terms}>", bias=bias, flags=BF16 if terms == 1 else 0,
                       mode=REFLECT if (k == 3 and tw in (16, 4)) else ZERO, s=bias and (k, tw) in ((3, 32), (5, 16)), accumulate=(k, tw, bias) == (3, 8, True)))
    for bias, terms in itertools.product((True, False), (3, 1)):
        fl = BF16 if terms == 1 else 0
        rows.append(wg(1, 8, 32, 32, 32, 3, f"whalo<3,tw32,bias{int(bias)},co32,t{terms}>", mode=REFLECT, bias=bias, flags=fl, s=bias))
        rows.append(wg(1, 96, 32, 512, 512, 3, f"wroll<tw32,bias{int(bias)},t{terms}>", bias=bias, flags=fl, s=bias))
        rows.append(wg(2, 96, 16, 512, 512, 3, f"wroll<tw16,bias{int(bias)},t{terms}>", bias=bias, flags=fl, mode=REFLECT))
    rows.append(wg(1, 96, 32, 512, 512, 3, "whalo<3,tw32,bias1,co64,t3>", bias=True, flags=ROW_WG))
    for bias in (True, False):
        rows.append(wg(1, 6, 18, 64, 64, 3, f"x3c<bias{int(bias)},general>", bias=bias, s=bias, accumulate=bias))
        rows.append(wg(1, 8, 16, 64, 64, 3, f"x3c<bias{int(bias)},lean>", bias=bias, flags=IM2COL, s=bias))
        rows.append(wg(1, 6, 18, 64, 64, 3, f"x3c<bias{int(bias)},reflect>", bias=bias, mode=REFLECT, s=bias))
        for refl in (False, True):
            md = REFLECT if refl else ZERO
            rows.append(wg(1, 6, 18, 64, 64, 3, f"wuni<refl{int(refl)},bias{int(bias)},64,fp32>", bias=bias, mode=md, flags=FP32))
            rows.append(wg(1, 6, 18, 64, 64, 3, f"wuni<refl{int(refl)},bias{int(bias)},64,x3>", bias=bias, mode=md, flags=SPLIT_REGS, s=bias))
    rows.append(wg(1, 8, 16, 64, 64, 1, "x3c<bias0,lean>"))                                            # 1x1
    rows.append(wg(1, 16, 32, 64, 64, 3, "x3c<bias1,lean>", stride=2, bias=True))                      # stride 2
    for refl in (False, True):
        rows.append(wg(1, 6, 18, 64, 32, 3, f"wuni<refl{int(refl)},bias1,32>", bias=refl, mode=REFLECT if refl else ZERO))
        for (Co, tco), (C, v) in itertools.product(((64, 64), (24, 32), (16, 16)), ((64, 1), (6, 0))):
            rows.append(wg(1, 6, 18, C, Co, 3, f"wgen<{tco},vec{v},refl{int(refl)}>", bias=bool(v), mode=REFLECT if refl else ZERO, flags=GENERAL,
                           accumulate=(Co, C, refl) == (64, 6, False)))
    rows.append(wg(2, 32, 40, 2, 64, 7, "wgen<64,vec0,refl0>", stride=2, nchw=True, affine=(2.0, 0.5), bias=True))   # NCHW stem

    # ---- 16-channel decoder tail (pd_conv16 modes 0 | 1 | 2, pd_conv16_wgrad): (N, C, H, W) = (1,16,2,2), (2,16,9,35), (1,32,13,7)
    for N, C, H, W in ((1, 16, 2, 2), (2, 16, 9, 35), (1, 32, 13, 7)):
        rows.append(Row("conv16", N, H, W, C, 16, 3, "conv16<0>", mode=REFLECT, bias=True, act=ACT_ELU if W == 35 else ACT_NONE, s=W == 35))
        rows.append(Row("conv16", N, H, W, 16, C, 3, "conv16<1>", mode=TRANSPOSED, pad=0, c16_mode=1))
        rows.append(Row("conv16", N, H, W, 16, C, 3, "conv16<2>", mode=TRANSPOSED, pad=1, c16_mode=2, s=W == 35))
        rows.append(Row("conv16_wgrad", N, H, W, C, 16, 3, "conv16_wgrad", mode=REFLECT, bias=True, accumulate=W == 7, s=W == 35))
    return rows


ROWS = _rows()


# ====================================================================================================== coverage
def _prod(fmt, *axes):
    return [fmt.format(*p) for p in itertools.product(*axes)]


_MODES3 = MODE_NAMES
# every instantiation the launch functions name, family by family
INSTANTIATIONS = (
    # launch_conv -> launch_conv_fp32: general kernel, four tiles x vec | scalar x three modes
    _prod("igemm<{0},{1},{2}>", ("128,64", "64,64", "128,32", "128,16"), ("vec", "scalar"), _MODES3)
    # ... uniform-tap kernel, three tiles x three modes x ring depth
    + _prod("uni<{0},{1},{2}>", ("128,64", "64,64", "128,32"), _MODES3, (2, 3))
    # launch_conv: conv_igemm_x3_kernel<MODE, 1 | 2>
    + _prod("x3<{0},{1}>", _MODES3, (1, 2))
    # launch_conv_x3_halo: 27 PD_HALO combinations and the row-window form, each with TERMS 3 and 1
    + _prod("halo<{0},tw{1},ncb2,{2},t{3}>", ("3x3", "5x5"), (32, 16, 8), _MODES3, (3, 1))
    + _prod("halo<3x3,tw{0},ncb1,{1},t{2}>", (32, 16), _MODES3, (3, 1))
    + _prod("halo<5x5,tw8,ncb1,{0},t{1}>", _MODES3, (3, 1))
    + _prod("halo<rowwin,t{0}>", (3, 1))
    # launch_wgrad_slices: general 64 | 32 | 16 x vec x reflect; conv_wgrad_uni_kernel in 10 forms; conv_wgrad_x3c_kernel in 6
    + _prod("wgen<{0},vec{1},refl{2}>", (64, 32, 16), (1, 0), (0, 1))
    + _prod("wuni<refl{0},bias{1},64,{2}>", (0, 1), (0, 1), ("fp32", "x3"))
    + _prod("wuni<refl{0},bias1,32>", (0, 1))
    + _prod("x3c<bias{0},{1}>", (0, 1), ("lean", "general", "reflect"))
    # launch_wgrad_halo: KS x TW x bias x CO32, each also under PD_CONV_BF16
    + _prod("whalo<3,tw{0},bias{1},co64,t{2}>", (32, 16, 8, 4), (0, 1), (3, 1))
    + _prod("whalo<5,tw{0},bias{1},co64,t{2}>", (32, 16, 8), (0, 1), (3, 1))
    + _prod("whalo<3,tw32,bias{0},co32,t{1}>", (0, 1), (3, 1))
    # launch_wgrad_roll: TW 32 | 16 x bias, each also under PD_CONV_BF16
    + _prod("wroll<tw{0},bias{1},t{2}>", (32, 16), (0, 1), (3, 1))
    # conv16.hip
    + ["conv16<0>", "conv16<1>", "conv16<2>", "conv16_wgrad", "s2 phases", "reflect bwd"]
)

# named by a launch function, reached by no legal call
UNREACHABLE = {
    **{k: "route_conv: ring depth 2 on every 128-row tile and under reflection, 3 on the 64x64 tile otherwise; "
          "launch_conv_fp32 does not instantiate <REFLECT, 3>"
       for k in _prod("uni<{0},{1},3>", ("128,64", "128,32"), _MODES3) + ["uni<64,64,reflect,3>", "uni<64,64,zero,2>", "uni<64,64,transposed,2>"]},
    **{k: "x3_common_ok admits reflection for ReflectionPad2d(1) + 3x3 only: no 5x5 reflection reaches launch_conv_x3_halo"
       for k in _prod("halo<5x5,tw{0},ncb2,reflect,t{1}>", (32, 16, 8), (3, 1)) + _prod("halo<5x5,tw8,ncb1,reflect,t{0}>", (3, 1))},
}

# both statistics tile heights (pd_conv2d_stats_rows: one row per 64 | 128 output pixels) of the halo and the gather kernels
STATS_HEIGHTS = {("halo", 64), ("halo", 128), ("x3", 64), ("x3", 128), ("uni", 64), ("uni", 128), ("igemm", 64), ("igemm", 128)}


def halo_tw(Ho, Wo):
    """conv_x3_halo.hpp: the widest of 32 | 16 | 8 whose 256-pixel tile divides the output grid."""
    return 32 if (Wo % 32 == 0 and Ho % 8 == 0) else 16 if (Wo % 16 == 0 and Ho % 16 == 0) else 8 if (Wo % 8 == 0 and Ho % 32 == 0) else 0


def wgrad_halo_tw(Ho, Wo):
    """conv_wgrad_halo.hpp: the widest of 32 | 16 | 8 | 4 whose 32-pixel tile divides the output grid."""
    return 32 if Wo % 32 == 0 else 16 if (Wo % 16 == 0 and Ho % 2 == 0) else 8 if (Wo % 8 == 0 and Ho % 4 == 0) else 4 if (Wo % 4 == 0 and Ho % 8 == 0) else 0


def route_word(r, lib):
    """pd_conv2d_route for a forward-like row: (family, BN, BM).  An input the 16-byte path cannot read is documented by the
    flags ops._igemm_label uses for it (the query assumes a dense NHWC tensor).  The query knows one padding: a pd_conv2d_rect row
    asks with the smaller of its two (route_conv wants pad < KH and pad_w < KW, which then hold together or not at all here)."""
    Ho, Wo = r.grid
    flags = r.flags if r.vec else FP32 | GENERAL
    w = lib.pd_conv2d_route(r.M, r.Co, r.C, r.KH, r.KW, r.stride, min(r.ph, r.pw), r.mode, r.act, int(r.scale), Ho, Wo, flags)
    return w & 15, (w >> 4) & 255, w >> 12


def instantiation(r, lib):
    """The kernel instantiation a row's call launches, as the host queries and the headers' rules answer."""
    Ho, Wo = r.grid
    md = MODE_NAMES[r.mode]
    if r.call in ("s2 phases", "reflect bwd", "conv16_wgrad"):
        return r.call
    if r.call == "conv16":
        return f"conv16<{r.c16_mode}>"
    if r.call == "wgrad":
        args = (r.M, r.Co, r.C, r.KH, r.KW, r.stride, r.ph, r.mode, r.H, r.W, Ho, Wo)
        code = lib.pd_conv2d_wgrad_uses_x3(*args, r.flags) if r.vec else 0
        one = lib.pd_conv2d_wgrad_uses_bf16(*args, r.flags) if r.vec else 0
        assert one in (0, code)
        t, b, refl = (1 if one else 3), int(r.bias), int(r.mode == REFLECT)
        if code == 3:
            return f"wroll<tw{32 if Wo % 32 == 0 else 16},bias{b},t{t}>"
        if code == 2:
            return f"whalo<{r.k},tw{wgrad_halo_tw(Ho, Wo)},bias{b},co{32 if r.Co % 64 else 64},t{t}>"
        if code == 1:
            return f"x3c<bias{b},{'reflect' if refl else 'lean' if (Wo % 8 == 0 and r.M % 8 == 0) else 'general'}>"
        # code 0: general | scalar-pixel fp32 | scalar-pixel split in registers, by the predicate of route_wgrad
        tco = 64 if r.Co > 32 else 32 if r.Co > 16 else 16
        nb = (r.ph + r.stride - 1) // r.stride
        nbw = (nb + 1) // 2
        refl_ok = r.mode == REFLECT and r.ph == 1 and r.k == 3 and r.stride == 1 and (Ho, Wo) == (r.H, r.W) and r.H >= 3
        uni = ((r.mode == ZERO or refl_ok) and not (r.flags & GENERAL) and tco in (64, 32) and r.vec and r.Co % 4 == 0 and Wo % 2 == 0 and
               Ho >= 2 * nb and Wo >= 4 * nbw and Wo >= 14 and (2 * nb + 1) * (2 * nbw + 1) <= 31 and r.M % 4 == 0 and r.K >= 4)
        if not uni:
            return f"wgen<{tco},vec{int(r.vec)},refl{refl}>"
        if tco == 32:
            return f"wuni<refl{refl},bias1,32>"
        assert r.flags & (FP32 | SPLIT_REGS), "a 64-wide scalar-pixel launch without either flag is the x3c kernel (code 1)"
        return f"wuni<refl{refl},bias{b},64,{'x3' if (r.flags & SPLIT_REGS) and not (r.flags & FP32) else 'fp32'}>"
    fam, bn, bm = route_word(r, lib)
    if fam == 0:
        return f"igemm<{bm},{bn},{'vec' if r.vec else 'scalar'},{md}>"
    if fam == 1:
        return f"uni<{bm},{bn},{md},{3 if (bm == 64 and r.mode != REFLECT) else 2}>"
    if fam == 2:
        return f"x3<{md},{bm // 128}>"
    t = 1 if fam == 4 else 3
    if r.k == 4:
        return f"halo<rowwin,t{t}>"
    return f"halo<{r.k}x{r.k},tw{halo_tw(Ho, Wo)},ncb{bn // 32},{md},t{t}>"


def stats_height(r, lib):
    """(kernel family, output pixels per row of the BatchNorm partials) of a forward row that asks for them."""
    return instantiation(r, lib).split("<")[0], lib.pd_conv2d_tile_m(r.M, r.Co)


# ====================================================================================================== data
def _gen(row, salt):
    return torch.Generator().manual_seed(zlib.crc32(repr((row.data_key, salt)).encode()))


def _ints(g, shape, amp):
    return torch.randint(-amp, amp + 1, tuple(shape), generator=g).to(F64)


def _signs(g, shape):
    return torch.randint(0, 2, tuple(shape), generator=g).to(F64) * 2 - 1


def _e8_image(g, shape, amp):
    """Integers in [-amp, amp]; the first and last two rows and columns carry +-amp (a wrong border tap cannot hide)."""
    t = _ints(g, shape, amp)
    edge = _signs(g, shape) * amp
    m = torch.zeros(shape[-2:], dtype=torch.bool)
    m[:2] = m[-2:] = True
    m[:, :2] = m[:, -2:] = True
    return torch.where(m, edge, t)


def _wide(g, shape):
    """m * 2^-18, |m| < 2^18: three quarters as (8 leading bits) * 2^10 + (odd 9-bit remainder), so that the third bf16 term
    is non-zero; the rest uniform."""
    h = torch.randint(128, 256, tuple(shape), generator=g)
    r = torch.randint(128, 256, tuple(shape), generator=g) * 2 + 1
    r = r * (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1)
    m = (h * 1024 + r) * (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1)
    u = torch.randint(-(2 ** 18) + 1, 2 ** 18, tuple(shape), generator=g)
    m = torch.where(torch.rand(tuple(shape), generator=g) < 0.75, m, u)
    return m.to(F64) * 2.0 ** -18


def _narrow(g, n):
    return (2.0 ** torch.randint(-1, 2, (n,), generator=g).to(F64)) * _signs(g, (n,))


def _sparse_rows(g, rows, cols, nnz, first=()):
    """[rows, cols] with `nnz` non-zeros of {+-0.5, +-1, +-2} per row at independent positions; `first`: columns every row uses."""
    t = torch.zeros(rows, cols, dtype=F64)
    for i in range(rows):
        pos = torch.randperm(cols, generator=g)[:nnz]
        pos[:len(first)] = torch.tensor(first, dtype=torch.long)[:nnz]
        t[i, pos] = _narrow(g, len(pos))
    return t


def _sparse_image(g, N, C, H, W, k):
    """One non-zero channel at the pixels of a lattice of pitch k (any k x k window holds one lattice pixel; a reflected
    border window sees it at most four times: 4 * 2 * 1 <= 16), origin on the border for the first image."""
    t = torch.zeros(N, C, H, W, dtype=F64)
    for n in range(N):
        oy, ox = (0, 0) if n == 0 else (int(torch.randint(0, k, (1,), generator=g)), int(torch.randint(0, k, (1,), generator=g)))
        ys, xs = torch.arange(oy, H, k), torch.arange(ox, W, k)
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        cc = torch.randint(0, C, yy.shape, generator=g)
        t[n, cc, yy, xx] = _narrow(g, yy.numel()).view(yy.shape)
    return t


def third_term_fraction(v):
    v = v.float()
    hi = v.bfloat16().float()
    r = v - hi
    return ((r - r.bfloat16().float()) != 0).double().mean().item()


def rb(t):
    """RNE to bf16 and back (as _rb of tests/test_conv_bf16_gpu.py)."""
    return t.to(torch.bfloat16).to(F64)


def _affine(x, affine):
    return x if affine is None else (x - affine[0]) / affine[1]


# ---------------------------------------------------------------------------------------------------- fp64 references
def ref_forward(x, w, r, dtype=F64):
    """Pre-activation z = conv(x, w) on the row's grid, before scale / bias."""
    x, w = _affine(x, r.affine).to(dtype), w.to(dtype)
    Ho, Wo = r.grid
    if r.transposed:
        s, kh, kw = r.stride, r.KH, r.KW
        Hf, Wf = (Ho + 2 * r.ph - kh) // s + 1, (Wo + 2 * r.pw - kw) // s + 1        # the forward output grid dy is the leading part of
        assert r.H <= Hf and r.W <= Wf, "dy exceeds the forward output grid"
        x = F.pad(x, (0, Wf - r.W, 0, Hf - r.H))
        op = (Ho - ((Hf - 1) * s - 2 * r.ph + kh), Wo - ((Wf - 1) * s - 2 * r.pw + kw))
        return F.conv_transpose2d(x, w.permute(1, 0, 2, 3), stride=s, padding=(r.ph, r.pw), output_padding=op)
    if r.mode == REFLECT:
        z = F.conv2d(F.pad(x, (r.pw, r.pw, r.ph, r.ph), mode="reflect"), w, stride=r.stride)
    else:
        z = F.conv2d(x, w, stride=r.stride, padding=(r.ph, r.pw))
    return z[:, :, :Ho, :Wo]


def ref_wgrad(x, dy, r, dtype=F64):
    """dW [Co, C, kh, kw] = sum over pixels of dy * the (padded, affine) input taps: one GEMM over the unfolded input."""
    x, dy = _affine(x, r.affine).to(dtype), dy.to(dtype)
    xp = F.pad(x, (r.pw, r.pw, r.ph, r.ph), mode="reflect" if r.mode == REFLECT else "constant")
    cols = F.unfold(xp, (r.KH, r.KW), stride=r.stride)                  # [N, C*kh*kw, L]
    Ho, Wo = r.grid
    assert cols.shape[2] == Ho * Wo
    dw = torch.einsum("nol,nkl->ok", dy.reshape(r.N, r.Co, -1), cols)
    return dw.view(r.Co, r.C, r.KH, r.KW)


@functools.lru_cache(maxsize=2)
def _case(key, cls, role, bf16):
    r = key
    g = _gen(r, (cls, role))
    Ho, Wo = r.grid
    d = {"bias": None, "scale": None, "addend": None, "act": ACT_NONE, "stats": False, "bound": None}
    wgrad = r.call in ("wgrad", "conv16_wgrad")
    wshape = (r.Co, r.C, r.KH, r.KW)
    if cls == "E8":
        x = _e8_image(g, (r.N, r.C, r.H, r.W), r.amp)
        if wgrad:
            w = _e8_image(g, (r.N, r.Co, Ho, Wo), r.amp)                # dy
        else:
            w = _ints(g, wshape, r.amp)
            w[:, :, 0, 0] = torch.where(w[:, :, 0, 0] == 0, torch.ones(()).to(F64), w[:, :, 0, 0])
        if r.bias and not wgrad:
            d["bias"] = _ints(g, (r.Co,), 3)
        if r.scale:
            d["scale"] = _signs(g, (r.Co,)) * 2.0 ** torch.randint(-2, 3, (r.Co,), generator=g).to(F64)
        if r.addend:
            d["addend"] = _ints(g, (r.N, r.Co, Ho, Wo), 3)
        d["act"], d["stats"] = r.act, r.stats
        ax = _affine(x, r.affine).abs().max().item()
        contraction = r.M if wgrad else r.K
        d["bound"] = contraction * ax * w.abs().max().item() * (4.0 if r.scale else 1.0) + 3.0 + 3.0
    else:
        assert r.stride == 1 and r.affine is None
        if wgrad:
            if role == "xw":        # wide x, sparse dy: 8 non-zero pixels per dy channel, two of them on the border of the grid
                x = _wide(g, (r.N, r.C, r.H, r.W))
                w = _sparse_rows(g, r.Co, r.N * Ho * Wo, 8, first=(0, r.N * Ho * Wo - 1)).view(r.Co, r.N, Ho, Wo).permute(1, 0, 2, 3).contiguous()
            else:                   # wide dy, sparse x: 2 non-zero pixels per x channel (a reflected border pixel counts up to 4 times)
                w = _wide(g, (r.N, r.Co, Ho, Wo))
                x = _sparse_rows(g, r.C, r.N * r.H * r.W, 2, first=(0,)).view(r.C, r.N, r.H, r.W).permute(1, 0, 2, 3).contiguous()
        elif role == "xw":          # wide activations, 8 non-zero weights along (tap, ci) of each output column
            x = _wide(g, (r.N, r.C, r.H, r.W))
            w = _sparse_rows(g, r.Co, r.K, 8).view(r.Co, r.KH, r.KW, r.C).permute(0, 3, 1, 2).contiguous()
        else:
            x = _sparse_image(g, r.N, r.C, r.H, r.W, max(r.KH, r.KW))
            w = _wide(g, wshape)
    if bf16:
        xr, wr = rb(x), rb(w)
    else:
        xr, wr = x, w
    d["x"], d["w"] = x, w
    if wgrad:
        d["dw"] = ref_wgrad(xr, wr, r)
        d["db"] = wr.sum((0, 2, 3))
        d["abs"] = (lambda: ref_wgrad(xr.abs(), wr.abs(), r)) if cls == "S" else None
    else:
        z = ref_forward(xr, wr, r)
        if d["scale"] is not None:
            z = z * d["scale"].view(1, -1, 1, 1)
        if d["bias"] is not None:
            z = z + d["bias"].view(1, -1, 1, 1)
        d["z"] = z
        y = z.clamp_min(0) if d["act"] == ACT_RELU else z
        d["y"] = y if d["addend"] is None else y + d["addend"]         # ELU: z >= 0 compared exactly, z < 0 against expm1(z)
        d["abs"] = (lambda: ref_forward(xr.abs(), wr.abs(), r)) if cls == "S" else None
    return d


def case(row, cls="E8", role="xw"):
    """Operands (fp64 holding fp32-exact values) and references of a row: x, w (dy for weight gradients), bias, scale, addend,
    z / y or dw / db."""
    return _case(row.data_key, cls, role, cls == "S" and bool(row.flags & BF16))


def variants(rows=None):
    """(row, class, role) of every run: each row in E8, the S rows twice more with the roles swapped."""
    out = []
    for r in (ROWS if rows is None else rows):
        out.append((r, "E8", "xw"))
        if r.s:
            out += [(r, "S", "xw"), (r, "S", "wx")]
    return out


def vid(v):
    r, cls, role = v
    return r.id + ("" if cls == "E8" else f"-S{role}")


# ---------------------------------------------------------------------------------------------------- conditions
def check_conditions(row, cls, role):
    """The exactness conditions of one run, asserted on its generated data (CPU)."""
    d = case(row, cls, role)
    wgrad = "dw" in d
    out = d["dw"] if wgrad else d["y"]
    assert torch.equal(out.float().double(), out), "reference not an fp32 number"
    if cls == "E8":
        for t in (d["x"], d["w"], d["bias"], d["addend"]):
            if t is not None:
                assert torch.equal(t, t.round()) and t.abs().max() <= 3 and torch.equal(rb(t), t)
        assert d["bound"] < 2 ** 24, d["bound"]
        x = d["x"]
        edge = torch.cat([x[..., :2, :].flatten(), x[..., -2:, :].flatten(), x[..., :, :2].flatten(), x[..., :, -2:].flatten()])
        assert (edge.abs() == row.amp).all()
        assert (x.abs().amax((2, 3)) > 0).all()
        if not wgrad:
            w = d["w"]
            assert (w.abs().amax((0, 1)) > 0).all() and (w.abs().amax((0, 2, 3)) > 0).all(), "a tap or a channel without a non-zero weight"
            if row.KH * row.KW > 1:
                assert not any(torch.equal(w, w.flip(dims)) for dims in ((2,), (3,), (2, 3)) if all(w.shape[i] > 1 for i in dims))
        if d["stats"]:
            z = d["z"]
            assert z.abs().sum((0, 2, 3)).max() < 2 ** 24 and (z * z).sum((0, 2, 3)).max() < 2 ** 24
    else:
        wide, narrow = (d["x"], d["w"]) if role == "xw" else (d["w"], d["x"])
        m = wide * 2.0 ** 18
        assert torch.equal(m, m.round()) and m.abs().max() < 2 ** 18
        assert third_term_fraction(wide) >= 0.5
        assert set(narrow.abs().unique().tolist()) <= {0.0, 0.5, 1.0, 2.0}
        assert d["abs"]().max() <= 16.0
        if wgrad and role == "xw":
            assert d["w"].abs().sum((0, 2, 3)).max() <= 16.0


def check_fp32_cpu(row):
    """The class itself: the same reference evaluated in fp32 on the CPU returns the fp64 bits on E8 data."""
    d = case(row, "E8", "xw")
    if "dw" in d:
        return torch.equal(ref_wgrad(d["x"], d["w"], row, torch.float32), d["dw"].float())
    z = ref_forward(d["x"], d["w"], row, torch.float32)
    if d["scale"] is not None:
        z = z * d["scale"].float().view(1, -1, 1, 1)
    if d["bias"] is not None:
        z = z + d["bias"].float().view(1, -1, 1, 1)
    return torch.equal(z, d["z"].float())


# ====================================================================================================== raw C ABI
def wgrad_raw(xd, dyd, w_shape, p, mode, ws_bytes, flags, dbias=None):
    """pd_conv2d_wgrad through the C ABI with a workspace of exactly `ws_bytes` bytes (ops.conv2d_wgrad passes a cached buffer
    of whatever size it has grown to): channels_last device tensors x and dy on the same grid, stride 1; dbias, where given, is
    overwritten like dW.  Returns dW on the CPU."""
    from polardepth._lib import lib, stream_ptr
    N, C, H, W = xd.shape
    Co, k = w_shape[0], w_shape[2]
    dw = torch.empty(tuple(w_shape), device="cuda", memory_format=torch.channels_last)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    sN, sC, sH, sW = xd.stride()
    rc = lib.pd_conv2d_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), None if dbias is None else dbias.data_ptr(),
                             ws.data_ptr(), ws_bytes, N, H, W, C, sN, sH, sW, sC, H, W, Co, k, k, 1, p, mode, 0, 0.0, 1.0,
                             dyd.stride(3), 0, flags, stream_ptr())
    assert rc == 0, lib.pd_last_error()
    torch.cuda.synchronize()
    return dw.cpu()
