"""Shared by tests/test_disphead_cases.py (CPU) and tests/test_disphead_gpu.py (GPU): the case table of the disparity-head kernels
(csrc/disphead.hip), the input generators, the NumPy fp64 reference, the exactness conditions as code and a restatement of the
launch arithmetic.

The five kernels -- disphead_fwd_kernel<4|8> (tile form), disphead_fwd_direct_kernel<16|32>, disphead_bwd_data_kernel<L>,
disphead_bwd_weight_kernel<L>, disphead_bwd_kernel<L> (L = C / 4 lanes per pixel, C in 16 | 32 | 64 | 128) -- and
disphead_reduce_kernel are reached through the four entry points pd_disphead_fwd / _bwd_data / _bwd_weight / _bwd.

Reference (`ref_forward`, `ref_backward`), written from the definition and not from the kernels' formulation:
    z  = b + conv3x3(np.pad(x, 1, mode="reflect"), w),  y = 1 / (1 + exp(-z))
    dz = dy * y * (1 - y)          from the y that is PASSED IN (y is an argument of every backward entry point)
    dx = the gradient scattered onto the padded grid, then folded with np.add.at over the reflect index map
    dw[t] = sum_p dz[p] * x[refl(p + t - 1)],  db = sum_p dz[p]
    with add / elu:  dx = (dx + add) * (1 if x > 0 else x + 1)
next to every output the sum of the absolute values of its terms, and for dx the number of terms.
Arrays are NHWC as the kernels read them: x [N, H, W, C], w [3, 3, C], y / dy [N, H, W].

Exactly summable class ("exact"): x from multiples of 1/4 in [-3/4, 1] (negatives in (-1, 0], so that ELU's factor x + 1 is exact),
w, bias, add and dy non-zero integers of magnitude <= 3, y from {1/4, 1/2, 3/4}: dz = dy y (1 - y) is a multiple of 1/16.  Condition,
per output element: sum|terms| / lsb < 2^24 with lsb = 2^-4 (dx, db), 2^-6 (dw; dx after the ELU factor), 2^-2 (z).  Every product and
every partial sum, in any order, with or without FMA, is then an fp32 number and the kernels must return the bits of the fp64
reference.  The forward uses its own weights `wf` (four channels per tap non-zero, magnitude <= 2): |z| <= 36 * 2 + 3 = 75 keeps
exp(-z) and y normal fp32 numbers, so that the sigmoid's rounding is the only error of y.

Random class ("random"): randn with two scales in one tensor (the upper half of every image times 37), y the fp32 rounding of the
fp64 sigmoid of these inputs.
"""
import dataclasses
import functools
import zlib

import numpy as np

TR, TW = 8, 64                       # output tile of the tile forms
CAP_TILE_FWD, CAP_WGRAD, CAP_WAVE = 4096, 1024, 16384
WIDTHS = (16, 32, 64, 128)
ENTRIES = ("pd_disphead_fwd", "pd_disphead_bwd_data", "pd_disphead_bwd_weight", "pd_disphead_bwd")
FWD, BWD_DATA, BWD_WEIGHT, BWD = ENTRIES
BORDER_HW = ((2, 2), (2, 3), (3, 2), (3, 3), (4, 5))
TILE_EDGE_HW = ((8, 64), (9, 65), (17, 129))
REDUCE_S = (1, 15, 16, 17, 31, 32, 33, 49, 1024)
U = 2.0 ** -24
EXPF_ULP = 2        # the HIP math documentation (its table of ulp errors) is not part of the ROCm install: the fallback E = 2


# ====================================================================================================== launch arithmetic
def ppw(C):
    """Pixels per wave of the wave forms: C / 4 lanes share a pixel."""
    return 64 // (C // 4)


def grid_for(npix, C):
    return min(-(-npix // (4 * ppw(C))), CAP_WAVE)


def ntiles(N, H, W):
    return N * (-(-H // TR)) * (-(-W // TW))


@dataclasses.dataclass(frozen=True)
class Launch:
    kernel: str         # the instantiation
    blocks: int         # workgroups
    iters: int          # the largest number of iterations of the grid-stride loop in one workgroup
    ragged: bool        # tile forms: a tile overhangs the image; wave forms: the last running wave has lanes with p >= npix
    S: int              # slices handed to disphead_reduce_kernel (0: none)


def launch(entry, N, C, H, W):
    """What an entry point launches for a shape, restated from its host code."""
    L, npix = C // 4, N * H * W
    if entry == BWD or (entry == FWD and C < 64):
        nt = ntiles(N, H, W)
        blocks = min(nt, CAP_WGRAD if entry == BWD else CAP_TILE_FWD)
        name = f"disphead_bwd_kernel<{L}>" if entry == BWD else f"disphead_fwd_kernel<{L}>"
        return Launch(name, blocks, -(-nt // blocks), H % TR != 0 or W % TW != 0, blocks if entry == BWD else 0)
    blocks = grid_for(npix, C)
    if entry == BWD_WEIGHT:
        blocks = min(blocks, CAP_WGRAD)
    name = {FWD: "disphead_fwd_direct_kernel", BWD_DATA: "disphead_bwd_data_kernel", BWD_WEIGHT: "disphead_bwd_weight_kernel"}[entry]
    steps = -(-npix // ppw(C))          # wave-sized steps; wave 0 of workgroup 0 runs the most
    return Launch(f"{name}<{L}>", blocks, -(-steps // (4 * blocks)), npix % ppw(C) != 0, blocks if entry == BWD_WEIGHT else 0)


# ====================================================================================================== the rows
WANT = {
    (FWD, 16): "disphead_fwd_kernel<4>", (FWD, 32): "disphead_fwd_kernel<8>",
    (FWD, 64): "disphead_fwd_direct_kernel<16>", (FWD, 128): "disphead_fwd_direct_kernel<32>",
    **{(BWD_DATA, C): f"disphead_bwd_data_kernel<{C // 4}>" for C in WIDTHS},
    **{(BWD_WEIGHT, C): f"disphead_bwd_weight_kernel<{C // 4}>" for C in WIDTHS},
    **{(BWD, C): f"disphead_bwd_kernel<{C // 4}>" for C in WIDTHS},
}
OPTIONS = {
    FWD: ("bias", "bias=NULL"),
    BWD_DATA: (),
    BWD_WEIGHT: ("accumulate=0", "accumulate=1", "dbias=NULL"),
    BWD: ("accumulate=0", "add", "add+elu", "elu", "dx=NULL", "dbias=NULL", "accumulate=1"),
}


@dataclasses.dataclass(frozen=True)
class Row:
    entry: str
    N: int
    C: int
    H: int
    W: int
    options: tuple
    want: str
    regime: str          # border | tile edge | ragged | second pass | reduce
    big: bool = False    # a 64 MiB tensor: one test, the reference through torch fp64

    @property
    def shape(self):
        return (self.N, self.C, self.H, self.W)

    @property
    def id(self):
        return f"{self.entry[12:]}-{self.N}x{self.H}x{self.W}x{self.C}"


def _rows():
    rows = []

    def add(entries, N, C, H, W, regime, big=False):
        for e in entries:
            rows.append(Row(e, N, C, H, W, () if big else OPTIONS[e], WANT[(e, C)], regime, big))

    for C in WIDTHS:
        # borders: at 3 both borders fold onto the same row, at 2 onto each other's row
        for H, W in BORDER_HW:
            add(ENTRIES, 2, C, H, W, "border")
        # tile edges (tile forward at 16 | 32, fused backward at all widths): full tiles, one pixel of overhang in both axes, tiles of
        # two images interleaved in the workgroup order; the wave forms run the same shapes for the equality of the two routes
        for H, W in TILE_EDGE_HW:
            add(ENTRIES, 2, C, H, W, "tile edge")
        # ragged pixel count of the wave forms: 105 pixels = 9 mod 16, 1 mod 8 | 4 | 2
        add(ENTRIES, 3, C, 5, 7, "ragged")
        # second pass of the tile forward (cap 4096, C = 16 | 32) and of the fused backward (cap 1024): one tile per image
        add(ENTRIES, 4097 if C < 64 else 1025, C, 2, 2, "second pass")
        # second pass of the weight gradient: just over 1024 * 4 * PPW pixels (65 600 at C = 16 ... 8 200 at C = 128)
        add(ENTRIES, 1, C, 3200 // C, 328, "second pass")
        # second pass of the data gradient (all widths) and of the direct forward (64 | 128): just over 16384 * 4 * PPW pixels
        add((BWD_DATA,) + ((FWD,) if C >= 64 else ()), 1, C, 16384 // C, 1025, "second pass", big=True)
    # slice counts of the reduce kernel: with H <= 8 and W <= 64 the fused backward has S = N (1024 comes from the rows above)
    for S in REDUCE_S[:-1]:
        add((BWD, BWD_WEIGHT), S, 16, 2, 2, "reduce")
    return rows


ROWS = _rows()


def shapes(entries, big=False, regimes=None):
    """The distinct (N, C, H, W) with a row of one of `entries`, in table order."""
    out = []
    for r in ROWS:
        if r.entry in entries and r.big == big and (regimes is None or r.regime in regimes) and r.shape not in out:
            out.append(r.shape)
    return out


def rows_of(shape, big=False):
    return {r.entry: r for r in ROWS if r.shape == tuple(shape) and r.big == big}


def sid(shape):
    return "x".join(str(v) for v in shape)


# ====================================================================================================== fp64 reference
def refl_map(n):
    """Index map of ReflectionPad(1): position i of the padded line reads element refl_map(n)[i]."""
    return np.pad(np.arange(n), 1, mode="reflect")


def ref_forward(x, w, b):
    """x [N, H, W, C], w [3, 3, C], b scalar (0 for no bias), fp64.  Returns z, y and sum|terms| of z (|b| included)."""
    N, H, W, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="reflect")
    z = np.full((N, H, W), float(b))
    za = np.full((N, H, W), abs(float(b)))
    for kh in range(3):
        for kw in range(3):
            win = xp[:, kh:kh + H, kw:kw + W, :]
            z += win @ w[kh, kw]
            za += np.abs(win) @ np.abs(w[kh, kw])
    with np.errstate(over="ignore"):
        y = 1.0 / (1.0 + np.exp(-z))
    return {"z": z, "y": y, "z_abs": za}


def ref_backward(x, w, y, dy, add=None, elu=False):
    """Gradients of sum(dy * y) for y = sigmoid(b + conv3x3(reflect-pad(x), w)), with the y passed in.  fp64 NHWC arrays.
    dx_abs / dw_abs / db_abs: sum of the absolute terms per element (dx_abs: of dz * w, and |add| where given, times the ELU factor);
    dx_terms [H, W]: the number of (padded position, tap) pairs behind a dx pixel."""
    N, H, W, C = x.shape
    dz = dy * y * (1.0 - y)
    gp = np.zeros((N, H + 2, W + 2, C))
    ga = np.zeros((N, H + 2, W + 2, C))
    cnt = np.zeros((H + 2, W + 2))
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="reflect")
    dw, dwa = np.zeros((3, 3, C)), np.zeros((3, 3, C))
    for kh in range(3):
        for kw in range(3):
            # output pixel p read the padded position p + (kh, kw) with weight w[kh, kw]
            gp[:, kh:kh + H, kw:kw + W, :] += dz[..., None] * w[kh, kw]
            ga[:, kh:kh + H, kw:kw + W, :] += np.abs(dz)[..., None] * np.abs(w[kh, kw])
            cnt[kh:kh + H, kw:kw + W] += 1
            win = xp[:, kh:kh + H, kw:kw + W, :]
            dw[kh, kw] = np.einsum("nhw,nhwc->c", dz, win)
            dwa[kh, kw] = np.einsum("nhw,nhwc->c", np.abs(dz), np.abs(win))
    ih, iw = refl_map(H)[:, None], refl_map(W)[None, :]
    dx, dxa, terms = np.zeros((N, H, W, C)), np.zeros((N, H, W, C)), np.zeros((H, W))
    np.add.at(dx, (slice(None), ih, iw), gp)
    np.add.at(dxa, (slice(None), ih, iw), ga)
    np.add.at(terms, (ih, iw), cnt)
    if add is not None:
        dx, dxa = dx + add, dxa + np.abs(add)
    if elu:
        f = np.where(x > 0, 1.0, x + 1.0)
        dx, dxa = dx * f, dxa * np.abs(f)
    return {"dz": dz, "dx": dx, "dx_abs": dxa, "dx_terms": terms, "dw": dw, "dw_abs": dwa, "db": dz.sum(), "db_abs": np.abs(dz).sum()}


def window_pixels(H, W, h0, w0):
    """Pixels of the reflected 3x3 window of (h0, w0): what the forward reads for y[h0, w0], and the dx pixels dz[h0, w0] reaches."""
    ih, iw = refl_map(H), refl_map(W)
    return {(int(ih[h0 + a]), int(iw[w0 + b])) for a in range(3) for b in range(3)}


# ====================================================================================================== data
def _rng(shape, salt):
    return np.random.default_rng(zlib.crc32(repr((tuple(shape), salt)).encode()))


def _nonzero_ints(g, shape, amp):
    return g.integers(1, amp + 1, shape).astype(np.float64) * (g.integers(0, 2, shape) * 2 - 1)


def exact_inputs(shape, need_x=True):
    """Operands of the exactly summable class (fp64 arrays holding fp32 numbers) for (N, C, H, W)."""
    N, C, H, W = shape
    g = _rng(shape, "exact")
    d = {"w": _nonzero_ints(g, (3, 3, C), 3), "b": float(_nonzero_ints(g, (), 3)),
         "dy": _nonzero_ints(g, (N, H, W), 3), "y": g.integers(1, 4, (N, H, W)) * 0.25}
    wf = np.zeros((3, 3, C))
    for t in range(9):                  # four channels per tap, anywhere in the lane group
        ch = g.permutation(C)[:4]
        wf[t // 3, t % 3, ch] = _nonzero_ints(g, (4,), 2)
    d["wf"] = wf
    if need_x:
        d["x"] = g.integers(-3, 5, (N, H, W, C)) * 0.25
        d["add"] = _nonzero_ints(g, (N, H, W, C), 3)
    return d


def random_inputs(shape, need_x=True):
    """randn with two scales in one tensor (fp64 arrays holding fp32 numbers); y = fp32(sigmoid) of these inputs."""
    N, C, H, W = shape
    g = _rng(shape, "random")
    f32 = lambda a: a.astype(np.float32).astype(np.float64)         # noqa: E731
    d = {"w": f32(g.standard_normal((3, 3, C)) / (9 * C) ** 0.5), "b": float(f32(g.standard_normal(()) * 0.1)),
         "dy": f32(g.standard_normal((N, H, W)))}
    d["dy"][:, : H // 2] *= 37.0
    if need_x:
        x = g.standard_normal((N, H, W, C), dtype=np.float32).astype(np.float64)
        x[:, : H // 2] *= 37.0
        d["x"] = x
    return d


@functools.lru_cache(maxsize=128)
def case(shape, cls="exact"):
    """Operands and references of a small shape, computed once and shared (do not modify).  exact: fwd (weights wf, with and without
    bias) and the backward references plain | add | add+elu | elu.  random: fwd (weights w), y32 = fp32(y), the plain backward of y32."""
    d = exact_inputs(shape) if cls == "exact" else random_inputs(shape)
    if cls == "exact":
        d["fwd"] = ref_forward(d["x"], d["wf"], d["b"])
        d["fwd0"] = ref_forward(d["x"], d["wf"], 0.0)
        d["bwd"] = ref_backward(d["x"], d["w"], d["y"], d["dy"])
        d["bwd+add"] = ref_backward(d["x"], d["w"], d["y"], d["dy"], add=d["add"])
        d["bwd+add+elu"] = ref_backward(d["x"], d["w"], d["y"], d["dy"], add=d["add"], elu=True)
        d["bwd+elu"] = ref_backward(d["x"], d["w"], d["y"], d["dy"], elu=True)
    else:
        d["fwd"] = ref_forward(d["x"], d["w"], d["b"])
        d["y"] = d["fwd"]["y"].astype(np.float32).astype(np.float64)
        d["bwd"] = ref_backward(d["x"], d["w"], d["y"], d["dy"])
    return d


# ---------------------------------------------------------------------------------------------------- the 64 MiB rows
def big_forward(x, w, b):
    """z, y and sum|terms| of a [N, H, W, C] fp64 array through torch.nn.functional.conv2d in fp64 (one output channel)."""
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w)).permute(2, 0, 1)[None].contiguous()
    z = F.conv2d(F.pad(xt, (1, 1, 1, 1), mode="reflect"), wt)[:, 0] + b
    za = F.conv2d(F.pad(xt.abs(), (1, 1, 1, 1), mode="reflect"), wt.abs())[:, 0] + abs(b)
    return {"z": z.numpy(), "y": torch.sigmoid(z).numpy(), "z_abs": za.numpy()}


def big_dx(w, y, dy, with_abs=False):
    """dx [N, H, W, C] of the data gradient: the padded-grid gradient through conv_transpose2d in fp64, folded with index_add_ over
    the reflect index map (the fold of ref_backward, one call per axis).  with_abs: also sum|dz * w| and the number of terms."""
    import torch
    import torch.nn.functional as F
    N, H, W = y.shape
    dz = torch.from_numpy(dy * y * (1.0 - y))[:, None]
    wt = torch.from_numpy(np.ascontiguousarray(w)).permute(2, 0, 1)[None].contiguous()
    ih, iw = torch.from_numpy(refl_map(H)), torch.from_numpy(refl_map(W))

    def fold(gp):
        rows = torch.zeros(gp.shape[0], gp.shape[1], H, W + 2, dtype=gp.dtype).index_add_(2, ih, gp)
        return torch.zeros(gp.shape[0], gp.shape[1], H, W, dtype=gp.dtype).index_add_(3, iw, rows)

    out = {"dx": fold(F.conv_transpose2d(dz, wt)).permute(0, 2, 3, 1)}
    if with_abs:
        out["dx_abs"] = fold(F.conv_transpose2d(dz.abs(), wt.abs())).permute(0, 2, 3, 1)
        out["dx_terms"] = fold(F.conv_transpose2d(torch.ones(1, 1, H, W, dtype=dz.dtype), torch.ones(1, 1, 3, 3, dtype=dz.dtype)))[0, 0]
    return out


# ====================================================================================================== conditions
def _fp32(a):
    return np.array_equal(np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64), a)


def check_conditions(shape):
    """The exactness conditions of a small shape's exact class, asserted on its generated data: for each output element
    sum|terms| / lsb < 2^24, the weight gradient's sum over all pixels included."""
    d = case(tuple(shape), "exact")
    for k, step, amp in (("x", 0.25, 1.0), ("w", 1.0, 3.0), ("wf", 1.0, 2.0), ("add", 1.0, 3.0), ("dy", 1.0, 3.0), ("y", 0.25, 0.75)):
        v = d[k] / step
        assert np.array_equal(v, np.round(v)) and np.abs(d[k]).max() <= amp, k
    assert d["x"].min() > -1.0 and (d["x"] > 0).any() and (d["x"] <= 0).any()
    assert set(np.unique(d["y"])) <= {0.25, 0.5, 0.75} and (d["dy"] != 0).all() and (d["w"] != 0).all()
    assert ((d["wf"] != 0).sum(2) == 4).all()
    dz16 = d["bwd"]["dz"] * 16
    assert np.array_equal(dz16, np.round(dz16))
    for k in ("bwd", "bwd+add"):
        assert d[k]["dx_abs"].max() * 2 ** 4 < 2 ** 24, k
    for k in ("bwd+elu", "bwd+add+elu"):
        # the sum before the factor is a multiple of 2^-4, the product with x + 1 (a multiple of 1/4) one of 2^-6
        assert d[k]["dx_abs"].max() * 2 ** 6 < 2 ** 24 and d["bwd+add"]["dx_abs"].max() * 2 * 2 ** 6 < 2 ** 24, k
    assert d["bwd"]["dw_abs"].max() * 2 ** 6 < 2 ** 24 and d["bwd"]["db_abs"] * 2 ** 4 < 2 ** 24
    # accumulate = 1 adds to integers of magnitude <= 8
    assert (d["bwd"]["dw_abs"].max() + 8) * 2 ** 6 < 2 ** 24 and (d["bwd"]["db_abs"] + 8) * 2 ** 4 < 2 ** 24
    for k in ("fwd", "fwd0"):
        assert d[k]["z_abs"].max() * 2 ** 2 < 2 ** 24 and np.abs(d[k]["z"]).max() <= 75.0, k
    for k in ("bwd", "bwd+add", "bwd+add+elu", "bwd+elu"):
        assert _fp32(d[k]["dx"]) and _fp32(d[k]["dw"]) and _fp32(np.float64(d[k]["db"])), k
    assert _fp32(d["fwd"]["z"]) and _fp32(d["fwd0"]["z"])


def check_conditions_big(row):
    """The same conditions for a 64 MiB row from the value ranges alone (no tensor is built): a dx element has at most 36 terms
    |dz * w| <= 3/4 * 3, a z element 36 non-zero terms |x * wf| <= 2 and the bias."""
    assert row.big and row.entry in (FWD, BWD_DATA)
    assert 36 * 0.75 * 3 * 2 ** 4 < 2 ** 24 and (36 * 2 + 3) * 2 ** 2 < 2 ** 24 and 36 * 2 + 3 <= 75
