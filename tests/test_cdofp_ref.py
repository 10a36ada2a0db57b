"""Properties of the definition of pd_cdofp_demosaic as tests/cdofp_ref.py states it (CPU only): the reference is pinned
against a per-pixel loop that follows the header word for word, and then shown to do what the definition is for."""
import numpy as np
import pytest

import cdofp_ref as C

LAYOUT = C.IMX250MYR_POL


def _loop(m, layout, bayer, gains, scale):
    """the header, one output at a time"""
    H4, W4 = m.shape
    ny, nx = H4 // 4, W4 // 4
    g = (1.0, 1.0, 1.0) if gains is None else gains
    ch = np.empty((4, 3, H4, W4))
    md = m.astype(np.float64)

    def v_of(ry, rx, y, x):
        i0, ty, j0, tx = (y - ry) // 4, float((y - ry) % 4), (x - rx) // 4, float((x - rx) % 4)
        cl = lambda i, n: min(max(i, 0), n - 1)
        L = lambda i, j: md[4 * cl(i, ny) + ry, 4 * cl(j, nx) + rx]
        a, b, c, d = L(i0, j0), L(i0, j0 + 1), L(i0 + 1, j0), L(i0 + 1, j0 + 1)
        return ((4.0 - ty) * ((4.0 - tx) * a + tx * b) + ty * ((4.0 - tx) * c + tx * d)) * 0.0625

    with np.errstate(all="ignore"):
        for y in range(H4):
            for x in range(W4):
                for p in range(4):
                    s = list(layout).index(p)
                    py, px = s >> 1, s & 1
                    for k in range(3):
                        cells = [c for c in range(4) if bayer[c] == k]
                        vs = [v_of(2 * (c >> 1) + py, 2 * (c & 1) + px, y, x) for c in cells]
                        v = vs[0] if k != 1 else (vs[0] + vs[1]) * 0.5
                        ch[p, k, y, x] = v * g[k]
        planes = (((19595.0 * ch[:, 0] + 38470.0 * ch[:, 1]) + 7471.0 * ch[:, 2]) * (1.0 / 65536.0)).astype(np.float32)
        c = ((ch[0] + ch[1]) + (ch[2] + ch[3])) * 0.25 * scale
        r = np.floor(c + 0.5)
        color = np.clip(np.where(np.isnan(r), 0.0, r), 0.0, 255.0).astype(np.uint8)
    return planes, color, ch.astype(np.float32)


@pytest.mark.parametrize("bayer", C.BAYERS)
@pytest.mark.parametrize("layout", [LAYOUT, C.OTHER_LAYOUT])
def test_reference_equals_the_per_pixel_loop(layout, bayer):
    gains = (1.7, 0.9, 2.3)
    for dtype, shape, scale in (("uint8", (8, 12), 1.0), ("uint16", (12, 8), C.SCALE_12BIT), ("float32", (12, 12), 0.01)):
        m = C.frame(shape, dtype)[0]
        if dtype == "float32":
            m = m.copy()
            m[5, 6], m[2, 9] = np.nan, np.inf
        got, ref = C.demosaic(m, layout, bayer, gains, scale), _loop(m, layout, bayer, gains, scale)
        for g, r in zip(got, ref):
            assert C.same_bits(g, r), (dtype, layout, bayer)


def test_ramps_come_back_exactly_and_unpolarised():
    """36x52 RGGB, layout (2,1,3,0), R = 10+2x+y, G = 20+x+2y, B = 5+x+y: off the clamped border every per-colour polarizer
    image IS its ramp, the four planes agree (DoLP exactly 0) and the picture is the ramps."""
    m, ramps = C.ramp_frame((36, 52), LAYOUT, C.RGGB)
    planes, color, rgb = C.demosaic(m, LAYOUT, C.RGGB)
    inner = (slice(3, 36 - 3), slice(3, 52 - 3))
    for p in range(4):
        for k in range(3):
            assert np.array_equal(rgb[p, k][inner], ramps[k][inner].astype(np.float32)), (p, k)
        assert np.array_equal(C.bits(planes[p][inner]), C.bits(planes[0][inner]))
    assert (C.dolp(planes)[inner] == 0).all()
    assert np.array_equal(color[(slice(None),) + inner], ramps[(slice(None),) + inner].astype(np.uint8))
    # sampling the super-pixels instead reads the gradients as polarisation, everywhere
    d = C.dolp(C.strided_planes(m, LAYOUT, C.RGGB))
    assert (d > 0).all(), (d.min(), d.max())


@pytest.mark.parametrize("bayer", C.BAYERS)
def test_a_single_super_pixel_returns_its_samples(bayer):
    """4x4: every lattice index is clamped, so each sub-lattice is its one sample; G is the mean of its two."""
    m = C.frame((4, 4), "uint16")[0]
    planes, color, rgb = C.demosaic(m, LAYOUT, bayer, None, C.SCALE_12BIT)
    for p in range(4):
        py, px = C.site_of(LAYOUT, p)
        for k in range(3):
            vals = [float(m[2 * by + py, 2 * bx + px]) for by, bx in C.cells_of(bayer, k)]
            want = vals[0] if k != 1 else (vals[0] + vals[1]) * 0.5
            assert (rgb[p, k] == np.float32(want)).all(), (p, k)


@pytest.mark.parametrize("bayer", C.BAYERS)
@pytest.mark.parametrize("layout", [LAYOUT, C.OTHER_LAYOUT])
def test_red_and_blue_reproduce_the_mosaic_at_their_own_sites(layout, bayer):
    m = C.frame((36, 52), "uint16")[0]
    rgb = C.demosaic(m, layout, bayer, None, C.SCALE_12BIT)[2]
    for ry in range(4):
        for rx in range(4):
            p, k = layout[2 * (ry & 1) + (rx & 1)], bayer[2 * (ry >> 1) + (rx >> 1)]
            if k != 1:
                assert np.array_equal(rgb[p, k, ry::4, rx::4], m[ry::4, rx::4].astype(np.float32)), (ry, rx)


def test_unit_gains_are_no_gains():
    for dtype in C.DTYPES:
        m = C.frame((12, 20), dtype, B=2)
        for a, b in zip(C.demosaic(m, LAYOUT, C.GRBG, None, 0.5), C.demosaic(m, LAYOUT, C.GRBG, (1, 1, 1), 0.5)):
            assert C.same_bits(a, b)
    g = C.demosaic(C.frame((12, 20), "uint8"), LAYOUT, C.RGGB, (2.0, 1.0, 0.5))[2]
    u = C.demosaic(C.frame((12, 20), "uint8"), LAYOUT, C.RGGB)[2]
    assert np.array_equal(g[:, :, 0], u[:, :, 0] * 2) and np.array_equal(g[:, :, 2], u[:, :, 2] * 0.5)


def test_non_finite_samples_reach_their_lattice_cells_only():
    m = C.special_frame()
    planes, color, rgb = C.demosaic(m, LAYOUT, C.RGGB, None, 1.0)
    assert np.isnan(planes).any() and np.isinf(planes).any()
    # the NaN at (5, 7) sits in sub-lattice (1, 3), lattice cell (1, 1): it reaches rows 1..8 and columns 3..10 of its green
    # image -- zero weights included -- and nothing else of that neighbourhood
    p = LAYOUT[2 * (5 & 1) + (7 & 1)]
    bad = ~np.isfinite(rgb[0, p, C.RGGB[2 * (5 >> 1 & 1) + (7 >> 1 & 1)]])
    assert bad[1:9, 3:11].all() and not bad[9:13, :].any() and not bad[1:9, 11:30].any()
    # two FLT_MAX neighbours of one sub-lattice: their interpolation stays FLT_MAX (fp64), it does not overflow
    k = C.RGGB[2 * (30 >> 1 & 1) + (30 >> 1 & 1)]
    assert (rgb[0, LAYOUT[0], k, 30, 30:35] == C.FLT_MAX).all()
    assert color.dtype == np.uint8


def test_interpolation_beats_sampling_on_a_polarised_scene():
    """Mean DoLP error against the truth: the definition's is smaller than strided sampling's (the ordering only)."""
    m, rho = C.polarised_scene((96, 128))
    planes = C.demosaic(m, LAYOUT, C.RGGB)[0].astype(np.float64)
    inner = (slice(4, -4), slice(4, -4))
    err_interp = np.abs(C.dolp(planes) - rho)[inner].mean()
    err_sample = np.abs(C.dolp(C.strided_planes(m, LAYOUT, C.RGGB)) - rho[2::4, 2::4])[1:-1, 1:-1].mean()
    assert err_interp < err_sample, (err_interp, err_sample)
