"""The definition of pd_cdofp_demosaic (include/polardepth.h) in NumPy, fp64, in the stated operation order -- written
differently from the kernel: each of the 16 sub-lattices is a strided slice of the frame, interpolated to the whole grid at
once by gathering its four neighbours with clamped index vectors; the kernel walks the frame in 4-column chunks with
compile-time column weights.  tests/test_cdofp_ref.py pins it against a per-pixel loop and checks the definition's properties.

Shared by the colour-DoFP tests: layouts, Bayer orders, the deterministic test frames and ``mosaic_of``."""
import functools

import numpy as np

IMX250MYR_POL = (2, 1, 3, 0)
OTHER_LAYOUT = (1, 3, 0, 2)
RGGB, BGGR, GRBG, GBRG = (0, 1, 1, 2), (2, 1, 1, 0), (1, 0, 2, 1), (1, 2, 0, 1)
BAYERS = [RGGB, BGGR, GRBG, GBRG]
DTYPES = ["uint8", "uint16", "float32"]
SHAPES = [(4, 4), (4, 8), (8, 4), (12, 20), (36, 52), (72, 136)]
SCALE_12BIT = 255.0 / 4095.0
FLT_MAX = np.finfo(np.float32).max


def site_of(layout, p):
    """(r_p, c_p): the row / column parity of the polarizer site that feeds plane p."""
    s = list(layout).index(p)
    return s >> 1, s & 1


def cells_of(bayer, k):
    """The Bayer cells (by, bx) of colour k in reading order: one for R and B, two for G (the upper row's first)."""
    return [(c >> 1, c & 1) for c in range(4) if bayer[c] == k]


def interp_lattice(m, ry, rx):
    """The sub-lattice (ry, rx) of m [..., H4, W4] (fp64) interpolated to the full grid: v of the definition."""
    H4, W4 = m.shape[-2:]
    L = m[..., ry::4, rx::4]
    ny, nx = L.shape[-2:]
    y, x = np.arange(H4), np.arange(W4)
    i0, ty = (y - ry) // 4, ((y - ry) % 4).astype(np.float64)[:, None]
    j0, tx = (x - rx) // 4, ((x - rx) % 4).astype(np.float64)[None, :]
    it, ib = np.clip(i0, 0, ny - 1), np.clip(i0 + 1, 0, ny - 1)
    jl, jr = np.clip(j0, 0, nx - 1), np.clip(j0 + 1, 0, nx - 1)
    top, bot = np.take(L, it, axis=-2), np.take(L, ib, axis=-2)
    a, b = np.take(top, jl, axis=-1), np.take(top, jr, axis=-1)
    c, d = np.take(bot, jl, axis=-1), np.take(bot, jr, axis=-1)
    return ((4.0 - ty) * ((4.0 - tx) * a + tx * b) + ty * ((4.0 - tx) * c + tx * d)) * 0.0625


def channels(mosaic, layout=IMX250MYR_POL, bayer=RGGB, gains=None):
    """ch of the definition, fp64 [..., 4, 3, H4, W4]."""
    m = np.asarray(mosaic).astype(np.float64)
    g = (1.0, 1.0, 1.0) if gains is None else tuple(float(x) for x in gains)
    ch = np.empty(m.shape[:-2] + (4, 3) + m.shape[-2:], np.float64)
    with np.errstate(all="ignore"):
        for p in range(4):
            py, px = site_of(layout, p)
            for k in range(3):
                vs = [interp_lattice(m, 2 * by + py, 2 * bx + px) for by, bx in cells_of(bayer, k)]
                v = vs[0] if len(vs) == 1 else (vs[0] + vs[1]) * 0.5
                ch[..., p, k, :, :] = v * g[k]
    return ch


def demosaic(mosaic, layout=IMX250MYR_POL, bayer=RGGB, gains=None, color_scale=1.0):
    """[..., H4, W4] -> (planes float32 [..., 4, H4, W4], color_u8 uint8 [..., 3, H4, W4], rgb_planes float32
    [..., 4, 3, H4, W4])."""
    ch = channels(mosaic, layout, bayer, gains)
    with np.errstate(all="ignore"):
        R, G, B = ch[..., 0, :, :], ch[..., 1, :, :], ch[..., 2, :, :]
        planes = (((19595.0 * R + 38470.0 * G) + 7471.0 * B) * (1.0 / 65536.0)).astype(np.float32)
        c = ((ch[..., 0, :, :, :] + ch[..., 1, :, :, :]) + (ch[..., 2, :, :, :] + ch[..., 3, :, :, :])) * 0.25 * float(color_scale)
        r = np.floor(c + 0.5)
        r = np.where(np.isnan(r), 0.0, r)
        color = np.clip(r, 0.0, 255.0).astype(np.uint8)
        rgb = ch.astype(np.float32)
    return planes, color, rgb


def mosaic_of(rgb_planes, layout=IMX250MYR_POL, bayer=RGGB):
    """What the sensor records of twelve full-resolution images [..., 4, 3, H4, W4]: the frame [..., H4, W4] whose site
    (y, x) shows plane layout[2 (y & 1) + (x & 1)] in colour bayer[2 ((y >> 1) & 1) + ((x >> 1) & 1)]."""
    a = np.asarray(rgb_planes)
    out = np.empty(a.shape[:-4] + a.shape[-2:], a.dtype)
    for ry in range(4):
        for rx in range(4):
            p, k = layout[2 * (ry & 1) + (rx & 1)], bayer[2 * (ry >> 1) + (rx >> 1)]
            out[..., ry::4, rx::4] = a[..., p, k, ry::4, rx::4]
    return out


def strided_planes(mosaic, layout=IMX250MYR_POL, bayer=RGGB):
    """Sampling instead of interpolating: one value per 4x4 super-pixel, fp64 [..., 4, H4/4, W4/4] (L of the sampled colours)."""
    m = np.asarray(mosaic).astype(np.float64)
    out = []
    for p in range(4):
        py, px = site_of(layout, p)
        col = []
        for k in range(3):
            vs = [m[..., 2 * by + py::4, 2 * bx + px::4] for by, bx in cells_of(bayer, k)]
            col.append(vs[0] if len(vs) == 1 else (vs[0] + vs[1]) * 0.5)
        out.append(((19595.0 * col[0] + 38470.0 * col[1]) + 7471.0 * col[2]) * (1.0 / 65536.0))
    return np.stack(out, axis=-3)


def dolp(planes):
    """DoLP of four planes [..., 4, H, W] at 0/45/90/135 degrees (fp64)."""
    p = np.asarray(planes, dtype=np.float64)
    i0, i45, i90, i135 = p[..., 0, :, :], p[..., 1, :, :], p[..., 2, :, :], p[..., 3, :, :]
    s0 = (i0 + i45 + i90 + i135) * 0.5
    return np.sqrt((i0 - i90) ** 2 + (i45 - i135) ** 2) / s0


def ramp_frame(shape=(36, 52), layout=IMX250MYR_POL, bayer=RGGB, dtype=np.uint8):
    """An unpolarised scene of three colour ramps R = 10 + 2x + y, G = 20 + x + 2y, B = 5 + x + y, and the ramps [3, H4, W4]."""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    ramps = np.stack([10 + 2 * xx + yy, 20 + xx + 2 * yy, 5 + xx + yy])
    twelve = np.broadcast_to(ramps[None], (4,) + ramps.shape)
    return mosaic_of(twelve, layout, bayer).astype(dtype), ramps


def bits(a):
    """the array as unsigned integers of its element width"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, ref):
    """fp32 compared as bits with the NaN positions equal (payloads are free), integers exactly"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, ref))
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(ref)[~nan]))


@functools.lru_cache(maxsize=None)
def frame(shape, dtype, seed=0, B=1):
    """A deterministic random frame [B,H4,W4]: full-range uint8, 12-bit uint16, or floats with fractions and both signs."""
    rng = np.random.default_rng([seed, shape[0], shape[1], DTYPES.index(dtype)])
    if dtype == "uint8":
        a = rng.integers(0, 256, (B,) + shape).astype(np.uint8)
    elif dtype == "uint16":
        a = rng.integers(0, 4096, (B,) + shape).astype(np.uint16)
    else:
        a = (rng.standard_normal((B,) + shape) * 1000.0).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def special_frame(shape=(36, 52), seed=7):
    """One float32 frame [1,H4,W4] holding NaN, +inf, FLT_MAX and a block of denormals among ordinary values."""
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    a = (rng.standard_normal((1,) + shape) * 100.0).astype(np.float32)
    den = rng.integers(1, 1 << 23, (8, 12)).astype(np.uint32) | (rng.integers(0, 2, (8, 12)).astype(np.uint32) << 31)
    a[0, 20:28, 8:20] = den.view(np.float32)
    a[0, 5, 7] = np.nan
    a[0, 13, 40] = np.inf
    a[0, 30, 30] = FLT_MAX
    a[0, 30, 34] = FLT_MAX        # the same sub-lattice, one cell on: their mean stays finite only in fp64
    a[0, 0, 0] = -np.inf          # a corner: every clamped index of its sub-lattice
    a.setflags(write=False)
    return a


def polarised_scene(shape, layout=IMX250MYR_POL, bayer=RGGB):
    """A smooth polarised colour scene and the frame the sensor records of it: (mosaic fp64 [H4,W4], true DoLP [H4,W4])."""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    rho = 0.1 + 0.3 * (0.5 + 0.5 * np.sin(xx / 31.0 + yy / 43.0)) ** 2
    phi = (np.pi / 2) * np.sin(xx / 53.0 - yy / 47.0)
    base = [900.0 * (0.5 + 0.3 * np.sin(xx / 37.0) * np.cos(yy / 29.0)),
            1100.0 * (0.5 + 0.3 * np.cos(xx / 41.0 + yy / 33.0)),
            700.0 * (0.5 + 0.3 * np.sin(yy / 27.0 - xx / 45.0))]
    twelve = np.stack([np.stack([c * (1 + rho * np.cos(2 * a - 2 * phi)) for c in base])
                       for a in (0, np.pi / 4, np.pi / 2, 3 * np.pi / 4)])
    return mosaic_of(twelve, layout, bayer), rho
