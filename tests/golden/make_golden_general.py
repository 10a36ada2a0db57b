#!/usr/bin/env python3
"""Generate tests/golden/g10_polar_general.npz by RUNNING THE REFERENCE's polarisation.xolp.Iun_and_xolp.

Like make_golden.py this runs only where the reference checkout is available ($PD_REFERENCE); the output is data only
(inputs, angles and the reference's fp64 Iun / rho / phi), no reference source text is stored.  Re-run with:

    PD_REFERENCE=<reference checkout> python tests/golden/make_golden_general.py

Cases: five polarizer angle sets x {uint8, uint16 (12-bit), float32 in [0, 1.3]} on 32x48 frames.  The field is the one
HAMMER_Dataset._synthetic_item uses (manydepth/datasets/__init__.py), evaluated at the given angles, with Gaussian noise
of sigma 1.5 / 6 / 0.004 in the units of the three formats.

Key layout of the .npz: "sets" (slugs), "dtypes", "<set>__angles_deg", "<set>__angles" (radians, as handed to the
reference), "<set>__<dtype>__images" [32,48,4] in the case's own dtype, "<set>__<dtype>__iun" / "__rho" / "__phi" [32,48] fp64.
"""
import os
import sys

import numpy as np

REF = os.environ.get("PD_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))

SETS = {                                   # slug -> degrees, in the order of the planes
    "std": [0.0, 45.0, 90.0, 135.0],
    "std_rot": [3.7, 48.7, 93.7, 138.7],   # the standard set, rotated by 3.7 degrees
    "calib": [0.8, 44.1, 91.3, 134.6],     # a calibrated filter set: never exactly nominal
    "sixty": [0.0, 60.0, 120.0, 30.0],
    "perm": [90.0, 0.0, 135.0, 45.0],      # the standard set, planes in another order
}
#            scale of the 8-bit field, noise sigma, clip, storage dtype
FORMATS = {
    "uint8": (1.0, 1.5, 255.0, np.uint8),
    "uint16": (16.0, 6.0, 4095.0, np.uint16),
    "float32": (1.0 / 180.0, 0.004, 1.3, np.float32),
}
H, W = 32, 48


def field(angles, scale):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    iun = 120 + 60 * np.sin(xx / 41.0) * np.cos(yy / 37.0)
    rho = 0.02 + 0.25 * (0.5 + 0.5 * np.sin(xx / 29.0 + yy / 53.0)) ** 2
    phi = (np.pi / 2) * np.sin(xx / 61.0 - yy / 43.0)
    return np.stack([scale * iun * (1 + rho * np.cos(2 * a - 2 * phi)) for a in angles], axis=-1).astype(np.float64)


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set PD_REFERENCE to the reference checkout")
    sys.path.insert(0, REF)
    from polarisation.xolp import Iun_and_xolp
    rng = np.random.default_rng(10)
    data = {"sets": np.array(list(SETS)), "dtypes": np.array(list(FORMATS))}
    for slug, deg in SETS.items():
        angles = np.array(deg) * np.pi / 180
        data[f"{slug}__angles_deg"] = np.array(deg)
        data[f"{slug}__angles"] = angles
        for name, (scale, sigma, top, dt) in FORMATS.items():
            img = field(angles, scale) + rng.normal(0, sigma, (H, W, 4))
            if np.issubdtype(dt, np.integer):
                img = np.rint(img)
            img = np.clip(img, 0, top).astype(dt)
            iun, rho, phi = Iun_and_xolp(img.astype(np.float64), angles)
            data[f"{slug}__{name}__images"] = img
            for k, v in (("iun", iun), ("rho", rho), ("phi", phi)):
                assert v.dtype == np.float64 and v.shape == (H, W)
                data[f"{slug}__{name}__{k}"] = v
    path = os.path.join(OUT, "g10_polar_general.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
