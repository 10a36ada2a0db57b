"""Shared by tests/test_polar_general_cabi.py and tests/test_polar_general_gpu.py: the fixture of the general polar kernel
(tests/golden/g10_polar_general.npz, written by tests/golden/make_golden_general.py from the reference's Iun_and_xolp) and
the fp64 NumPy restatement of the canonical arithmetic ("general angles")."""
import functools
import os

import numpy as np

from conftest import GOLDEN

SETS = ("std", "std_rot", "calib", "sixty", "perm")
DTYPES = ("uint8", "uint16", "float32")
CASES = [(s, d) for s in SETS for d in DTYPES]


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(os.path.join(GOLDEN, "g10_polar_general.npz"))
    assert tuple(z["sets"]) == SETS and tuple(z["dtypes"]) == DTYPES
    return {k: z[k] for k in z.files}


def case(slug, dtype):
    """-> images [32,48,4] (own dtype), angles [4] radians, reference (iun, rho, phi) fp64 [32,48]"""
    z = fixture()
    k = f"{slug}__{dtype}__"
    return z[k + "images"], z[f"{slug}__angles"], (z[k + "iun"], z[k + "rho"], z[k + "phi"])


def restate(images, P):
    """The canonical arithmetic on [..., 4] intensities (last axis = polarizer) with the 3x4 coefficients P of
    pd_polar_fit_matrix: fp64, left-to-right sums, no fused multiply-add (NumPy evaluates one ufunc per operation),
    each result rounded once to fp32.  -> dict iun, rho, phi (fp32) and r (fp64)."""
    I = np.asarray(images).astype(np.float64)
    i0, i1, i2, i3 = (I[..., j] for j in range(4))
    with np.errstate(all="ignore"):
        x0, x1, x2 = (((P[k, 0] * i0 + P[k, 1] * i1) + P[k, 2] * i2) + P[k, 3] * i3 for k in range(3))
        r = np.sqrt(x1 * x1 + x2 * x2)
        imax = x0 + r
        imin = x0 - r
        s = imax + imin
        rho = (imax - imin) / s
        rho[np.isinf(rho) | np.isnan(rho)] = 0.0
        phi = 0.5 * np.arctan2(x2, x1)
        return {"iun": (s / 2.0).astype(np.float32), "rho": rho.astype(np.float32), "phi": phi.astype(np.float32), "r": r}


def standardise(x):
    """pre_encoders.py:78-79 on fp32 (IEEE subtraction and division)."""
    x = np.asarray(x, dtype=np.float32)
    mean, std = np.float32(0.08693199701957657), np.float32(0.44430732785457433)
    return (x - mean) / std


def planes(images):
    """[H,W,4] -> contiguous [4,H,W] of the same dtype"""
    return np.ascontiguousarray(np.moveaxis(np.asarray(images), -1, 0))
