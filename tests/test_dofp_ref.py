"""tests/dofp_ref.py, the NumPy statement of pd_dofp_demosaic, against a naive per-pixel loop that follows the table in
include/polardepth.h literally, and the properties the definition is meant to have.  No GPU."""
import numpy as np
import pytest

import dofp_ref as D


def _mirror(i, n):
    return 1 if i == -1 else (n - 2 if i == n else i)


def _naive_bilinear(m, layout):
    H2, W2 = m.shape
    out = np.empty((4, H2, W2), np.float32)
    g = lambda y, x: np.float64(m[_mirror(y, H2), _mirror(x, W2)])
    for p in range(4):
        r, c = D.site_of(layout, p)
        for y in range(H2):
            for x in range(W2):
                dy, dx = (y - r) & 1, (x - c) & 1
                if (dy, dx) == (0, 0):
                    v = g(y, x)
                elif (dy, dx) == (0, 1):
                    v = (g(y, x - 1) + g(y, x + 1)) * 0.5
                elif (dy, dx) == (1, 0):
                    v = (g(y - 1, x) + g(y + 1, x)) * 0.5
                else:
                    v = ((g(y - 1, x - 1) + g(y - 1, x + 1)) + (g(y + 1, x - 1) + g(y + 1, x + 1))) * 0.25
                out[p, y, x] = np.float32(v)
    return out


def _naive_superpixel(m, layout):
    H2, W2 = m.shape
    out = np.empty((4, H2 // 2, W2 // 2), m.dtype)
    for p in range(4):
        r, c = D.site_of(layout, p)
        for y in range(H2 // 2):
            for x in range(W2 // 2):
                out[p, y, x] = m[2 * y + r, 2 * x + c]
    return out


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("shape", D.SMALL_SHAPES)
def test_statement_equals_the_per_pixel_loop(shape, dtype):
    m = D.wide_range_frame(shape)[0] if dtype == "float32" else D.frame(shape, dtype)[0]
    for layout in D.LAYOUTS:
        assert np.array_equal(D.bits(D.bilinear(m, layout)), D.bits(_naive_bilinear(m, layout))), layout
        sp = D.superpixel(m, layout)
        assert sp.dtype == m.dtype and np.array_equal(D.bits(sp), D.bits(_naive_superpixel(m, layout))), layout


@pytest.mark.parametrize("dtype", D.DTYPES)
def test_both_modes_return_the_samples_at_their_own_sites(dtype):
    m = D.frame((6, 10), dtype)[0]
    for layout in D.LAYOUTS:
        bl, sp = D.bilinear(m, layout), D.superpixel(m, layout)
        for p in range(4):
            r, c = D.site_of(layout, p)
            assert layout[2 * r + c] == p
            assert np.array_equal(bl[p, r::2, c::2], m[r::2, c::2].astype(np.float32))
            assert np.array_equal(sp[p], m[r::2, c::2])
        # and a frame recorded from four planes gives those planes back where they were sampled
        planes = np.stack([D.frame((6, 10), dtype, seed=10 + p)[0] for p in range(4)])
        again = D.superpixel(D.mosaic_of(planes, layout), layout)
        for p in range(4):
            r, c = D.site_of(layout, p)
            assert np.array_equal(again[p], planes[p, r::2, c::2])


def test_unpolarised_ramp_gives_identical_interior_planes_only_when_interpolated():
    """3x + 5y + 7 seen through any layout: bilinear reconstructs the ramp itself in the interior of all four planes (no false
    polarisation); the sampled planes differ by up to 3 + 5 = 8 counts."""
    m = D.affine_field((12, 16))
    for layout in (D.IMX250MZR, (0, 1, 2, 3), (3, 0, 1, 2)):
        bl = D.bilinear(m, layout)
        for p in range(4):
            assert np.array_equal(bl[p, 1:-1, 1:-1], m[1:-1, 1:-1].astype(np.float32))
        sp = D.superpixel(m, layout).astype(np.int64)
        assert (sp.max(axis=0) - sp.min(axis=0)).max() == 8


def test_extreme_frames_come_back_unchanged():
    for layout in (D.IMX250MZR, (1, 3, 0, 2)):
        big = np.full((6, 10), D.FLT_MAX, np.float32)
        out = D.bilinear(big, layout)
        assert np.isfinite(out).all() and np.array_equal(D.bits(out), D.bits(np.full((4, 6, 10), D.FLT_MAX, np.float32)))
        assert np.array_equal(D.bilinear(np.full((6, 10), 65535, np.uint16), layout), np.full((4, 6, 10), 65535.0, np.float32))
        assert np.array_equal(D.superpixel(np.full((6, 10), 65535, np.uint16), layout), np.full((4, 3, 5), 65535, np.uint16))


def test_the_wide_range_frame_tells_fp64_from_fp32_accumulation():
    """On the 2^40-range frame an fp32 accumulation of the diagonal mean differs from the definition on a good share of the
    diagonal sites: a kernel that takes that shortcut cannot pass the bit comparison."""
    m = D.wide_range_frame((34, 70))[0]
    ref = D.bilinear(m, D.IMX250MZR)
    pad = np.pad(m, 1, mode="reflect")
    at = lambda dy, dx: pad[1 + dy:35 + dy, 1 + dx:71 + dx]
    short = ((at(-1, -1) + at(-1, 1)) + (at(1, -1) + at(1, 1))) * np.float32(0.25)      # float32 throughout
    r, c = D.site_of(D.IMX250MZR, 0)
    diag = ref[0, 1 - r::2, 1 - c::2]
    differ = (D.bits(diag) != D.bits(short[1 - r::2, 1 - c::2])).mean()
    assert 0.05 < differ < 0.5, differ
