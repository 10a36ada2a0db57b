"""The definition of pd_dofp_demosaic (include/polardepth.h) in NumPy, fp64 -- written differently from the kernel: the
frame is padded once with ``np.pad(mode="reflect")`` (index -1 reads 1, index n reads n-2), the three neighbour means are
whole-frame sums of shifted slices, and parity masks pick one of the four per plane; the kernel decides per pixel.
tests/test_dofp_ref.py pins it against a naive per-pixel loop.

Shared by the DoFP tests: layouts, shapes, the deterministic test frames and ``mosaic_of``."""
import functools
import itertools

import numpy as np

IMX250MZR = (2, 1, 3, 0)
LAYOUTS = list(itertools.permutations(range(4)))            # all 24
SMALL_SHAPES = [(2, 2), (2, 4), (4, 2), (6, 10)]            # 2x2: every neighbour is a mirrored one
DTYPES = ["uint8", "uint16", "float32"]
FLT_MAX = np.finfo(np.float32).max


def site_of(layout, p):
    """(r_p, c_p): the row / column parity of the site that feeds plane p."""
    s = list(layout).index(p)
    return s >> 1, s & 1


def mosaic_of(planes, layout):
    """What a sensor with this layout records of four full-resolution planes [..., 4, H2, W2]: the frame [..., H2, W2] whose
    site (r, c) shows plane layout[2 r + c]."""
    planes = np.asarray(planes)
    out = np.empty(planes.shape[:-3] + planes.shape[-2:], planes.dtype)
    for r in (0, 1):
        for c in (0, 1):
            out[..., r::2, c::2] = planes[..., layout[2 * r + c], r::2, c::2]
    return out


def superpixel(mosaic, layout):
    """[..., H2, W2] -> [..., 4, H2/2, W2/2] of the same dtype: planes[p][y][x] = mosaic[2y + r_p][2x + c_p]."""
    mosaic = np.asarray(mosaic)
    sl = [site_of(layout, p) for p in range(4)]
    return np.stack([mosaic[..., r::2, c::2] for r, c in sl], axis=-3)


def bilinear(mosaic, layout):
    """[..., H2, W2] -> float32 [..., 4, H2, W2]: fp64 in the header's order, rounded once."""
    m = np.asarray(mosaic).astype(np.float64)
    H2, W2 = m.shape[-2:]
    pad = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)], mode="reflect")
    at = lambda dy, dx: pad[..., 1 + dy:1 + dy + H2, 1 + dx:1 + dx + W2]
    with np.errstate(all="ignore"):
        cand = [at(0, 0),
                (at(0, -1) + at(0, 1)) * 0.5,
                (at(-1, 0) + at(1, 0)) * 0.5,
                ((at(-1, -1) + at(-1, 1)) + (at(1, -1) + at(1, 1))) * 0.25]
        yy, xx = np.mgrid[0:H2, 0:W2]
        out = np.empty(m.shape[:-2] + (4, H2, W2), np.float32)
        for p in range(4):
            r, c = site_of(layout, p)
            k = 2 * ((yy - r) & 1) + ((xx - c) & 1)
            out[..., p, :, :] = np.choose(k, cand).astype(np.float32)
    return out


def demosaic(mosaic, layout, mode):
    return superpixel(mosaic, layout) if mode == "superpixel" else bilinear(mosaic, layout)


def bits(a):
    """the array as unsigned integers of its element width: comparisons as bytes (NaN payloads, signed zeros)"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def frame(shape, dtype, seed=0, B=1):
    """A deterministic random frame [B,H2,W2]: full-range integers, or floats with fractional parts and both signs."""
    rng = np.random.default_rng([seed, shape[0], shape[1], DTYPES.index(dtype)])
    if dtype == "uint8":
        a = rng.integers(0, 256, (B,) + shape).astype(np.uint8)
    elif dtype == "uint16":
        a = rng.integers(0, 65536, (B,) + shape).astype(np.uint16)
    else:
        a = (rng.standard_normal((B,) + shape) * 1000.0).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def wide_range_frame(shape, seed=5, B=1):
    """float32 values spread over 2^40 in magnitude, both signs, full mantissas: the fp64 sums of the definition round (two
    24-bit mantissas up to 40 binades apart do not fit 53 bits), so the order of the additions and the single rounding to
    fp32 matter, and an fp32 accumulation gives other bits."""
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    a = (rng.uniform(1.0, 2.0, (B,) + shape) * np.exp2(rng.integers(-20, 21, (B,) + shape)) *
         rng.choice([-1.0, 1.0], (B,) + shape)).astype(np.float32)
    a.setflags(write=False)
    return a


def affine_field(shape):
    """the unpolarised ramp 3x + 5y + 7 as a uint16 frame (every site sees the same scene intensity)"""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (3 * xx + 5 * yy + 7).astype(np.uint16)
