"""General polar kernel, host side (no GPU): pd_polar_fit_matrix, the argument checks of pd_polar_general_fwd, the
canonical arithmetic (fp64 restatement) against the reference's lstsq-based Iun_and_xolp on the fixture
tests/golden/g10_polar_general.npz, and the argument handling of the polarisation.xolp façade."""
import ctypes

import numpy as np
import pytest

import polar_general_ref as G
from polardepth import _lib
from polardepth import polar as pdpolar

_dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _A(angles):
    return np.stack([np.ones(4), np.cos(2 * angles), np.sin(2 * angles)], axis=1)


def test_fit_matrix_of_the_standard_set_is_exact():
    P = pdpolar.fit_matrix(np.array([0, 45, 90, 135]) * np.pi / 180)
    assert P.dtype == np.float64 and P.shape == (3, 4)
    assert np.array_equal(P, np.array([[.25, .25, .25, .25], [.5, 0, -.5, 0], [0, .5, 0, -.5]]))
    assert not np.signbit(P[P == 0]).any()      # the snapped zeros are +0


@pytest.mark.parametrize("slug", [s for s in G.SETS if s != "std"])
def test_fit_matrix_agrees_with_pinv(slug):
    angles = G.fixture()[f"{slug}__angles"]
    P = pdpolar.fit_matrix(angles)
    ref = np.linalg.pinv(_A(angles))
    assert np.abs(P - ref).max() <= 1e-13 * np.abs(P).max()


def test_fit_matrix_refuses_rank_deficient_and_non_finite_angles():
    L = _lib.lib
    out = np.full(12, 7.0)
    for deg in ([0, 90, 180, 270], [10, 100, 190, 280], [30, 30, 30, 30], [0, 45, 0, 45]):
        a = np.array(deg, dtype=np.float64) * np.pi / 180
        assert L.pd_polar_fit_matrix(_dp(a), _dp(out)) == -22 and b"rank < 3" in L.pd_last_error(), deg
        with pytest.raises(ValueError, match="rank < 3"):
            pdpolar.fit_matrix(a)
    for bad in (np.nan, np.inf, -np.inf):
        a = np.array([0.0, bad, 1.0, 2.0])
        assert L.pd_polar_fit_matrix(_dp(a), _dp(out)) == -22 and b"not finite" in L.pd_last_error()
    assert L.pd_polar_fit_matrix(None, _dp(out)) == -22
    with pytest.raises(ValueError, match="four"):
        pdpolar.fit_matrix([0.0, 1.0, 2.0])


def test_argument_validation_of_the_general_kernel_needs_no_gpu():
    """Every refusal of pd_polar_general_fwd is decided before anything touches the device: PD_EINVAL (-22) with a
    message; an empty batch returns 0."""
    L = _lib.lib
    err = L.pd_last_error
    p = ctypes.c_void_p(16)      # a non-null, 16-byte aligned dummy: never dereferenced on these paths
    odd = ctypes.c_void_p(24)
    coef = np.ascontiguousarray(pdpolar.fit_matrix(pdpolar.STD_ANGLES).reshape(-1))
    c = _dp(coef)
    nbytes = L.pd_polar_tables_bytes(1000, 600, 400)

    def call(pol=p, dtype=0, coef=c, iun=None, xolp=p, std=None, normals=None, tables=None, tb=0, B=1, H=8, W=8, Wout=0, flags=0):
        return L.pd_polar_general_fwd(pol, dtype, coef, iun, xolp, std, normals, tables, tb, B, H, W, Wout, flags, None)

    assert call(B=0, pol=None, coef=None, xolp=None) == 0                                   # empty batch
    assert call(B=-1) == -22 and b"bad shape" in err()
    assert call(H=0) == -22 and b"bad shape" in err()
    assert call(dtype=3) == -22 and b"unknown dtype" in err()
    assert call(dtype=-1) == -22 and b"unknown dtype" in err()
    for flags in (2, 4, 8, 3, 16):                                                          # IEEE_RHO, NT_LOADS, PLAIN_LOADS, ...
        assert call(flags=flags) == -22 and b"PD_POLAR_PRECISE_NORMALS only" in err()
    assert call(pol=None) == -22 and b"must not be null" in err()
    assert call(coef=None) == -22 and b"must not be null" in err()
    assert call(xolp=None) == -22 and b"no output" in err()
    assert call(normals=p) == -22 and b"tables" in err()                                    # normals without the blob
    assert call(normals=p, tables=p, tb=1000) == -22 and b"unexpected size" in err()
    assert call(H=5, W=5) == -22 and b"multiples of 4" in err()                             # H*W % 4
    assert call(H=5, W=6, Wout=8) == -22 and b"multiples of 4" in err()                     # pitched: W % 4
    assert call(H=5, W=8, Wout=10) == -22 and b"multiples of 4" in err()                    # pitched: Wout % 4
    assert call(W=8, Wout=4) == -22 and b"pitch" in err()
    for kw in ({"pol": odd}, {"xolp": odd}, {"iun": odd}, {"std": odd}, {"normals": odd, "tables": p, "tb": nbytes},
               {"normals": p, "tables": odd, "tb": nbytes}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    assert call(H=16384, W=8192) == -22 and b"too large" in err()                           # 9 * H * W >= 2^30
    bad = coef.copy()
    bad[5] = np.nan
    assert call(coef=_dp(bad)) == -22 and b"coefficient 5" in err()


@pytest.mark.parametrize("slug,dtype", G.CASES)
def test_canonical_form_matches_the_reference(slug, dtype):
    """The restatement (x = P I in fp64, then xolp.py:22-30 literally, rounded once to fp32) against the reference's
    lstsq solve.  AoLP is compared where it is defined: where the polarised part vanishes (r = 0) the reference's lstsq
    noise decides phi and its +-pi/2 branch.  Measured with NumPy on these inputs: excluded <= 0.26 % (uint8 only), and on
    the kept pixels phi equal mod pi and rho within 2e-16 before rounding."""
    images, angles, (iun, rho, phi) = G.case(slug, dtype)
    got = G.restate(images, pdpolar.fit_matrix(angles))
    d_rho = np.abs(got["rho"].astype(np.float64) - rho)
    assert (d_rho <= 1.2e-7 * np.maximum(1.0, np.abs(rho))).all(), d_rho.max()
    d_iun = np.abs(got["iun"].astype(np.float64) - iun)
    ulp = np.spacing(np.abs(iun).astype(np.float32)).astype(np.float64)
    assert (d_iun <= ulp).all(), (d_iun / ulp).max()
    keep = got["r"] > 1e-9 * np.abs(images.astype(np.float64)).max()
    excluded = 1.0 - keep.mean()
    d = np.abs(got["phi"].astype(np.float64) - phi) % np.pi
    d_phi = np.minimum(d, np.pi - d)[keep]
    print(f"{slug}/{dtype}: rho {d_rho.max():.3g}  iun {(d_iun / ulp).max():.3g} ulp  phi {d_phi.max():.3g}  excluded {excluded:.4%}")
    assert excluded <= 0.01
    assert (d_phi <= 2.4e-7).all(), d_phi.max()


def test_facade_refuses_what_the_kernel_cannot_represent():
    """polarisation.xolp.Iun_and_xolp checks its arguments on the host: intensities that do not survive a round trip through
    fp32 and angle sets of rank < 3 are ValueErrors (and say which value / why), before any device work."""
    from polarisation.xolp import Iun_and_xolp
    std = np.array([0, 45, 90, 135]) * np.pi / 180
    img = np.full((4, 4, 4), 0.5)
    img[2, 1, 3] = 0.1                              # not an fp32 number
    with pytest.raises(ValueError, match=r"images\[2, 1, 3\] = 0\.1 "):
        Iun_and_xolp(img, std)
    big = np.full((4, 4, 4), 100.0)
    big[0, 3, 0] = 2.0 ** 24 + 1                    # an integer beyond uint16 that fp32 cannot hold
    with pytest.raises(ValueError, match=r"images\[0, 3, 0\]"):
        Iun_and_xolp(big, std)
    with pytest.raises(ValueError, match="rank < 3"):
        Iun_and_xolp(np.full((4, 4, 4), 3.0), np.array([0, 90, 180, 270]) * np.pi / 180)
    with pytest.raises(ValueError, match="H,W,4"):
        Iun_and_xolp(np.zeros((4, 4, 3)), std)
