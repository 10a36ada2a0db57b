"""The definition of pd_frame_moments, pd_dofp_cal_solve and pd_dofp_calibrate (include/polardepth.h) in NumPy, fp64, in the
header's operation order -- whole-frame array expressions where the kernels work per lane -- and the host recipe of
``polardepth.calibration.fit`` restated with the identical NumPy calls, so that device results can be compared bit for bit.
tests/test_dofp_cal_ref.py pins it (nominal sensor, the synthetic sensor below, dead sites).

Shared by the calibration tests: the synthetic sensor of the issue's experiment, its flat-field series and scenes."""
import functools

import numpy as np

IMX250MZR = (2, 1, 3, 0)
NOMINAL_DEG = (0.0, 45.0, 90.0, 135.0)
SHAPES = [(2, 2), (6, 10), (8, 8), (10, 18)]            # 6x10, 10x18: W2 % 4 == 2 (one cell per lane, 8-byte stores)
DTYPES = ["uint8", "uint16", "float32"]
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ the three calls
def moments(frames, weights, dark=None, out=None):
    """frames [N,H2,W2], weights fp64 [N,Q] -> fp64 [Q,H2,W2]; ``out``: the array to accumulate onto (not modified)."""
    frames, weights = np.asarray(frames), np.asarray(weights, np.float64)
    N, Q = weights.shape
    acc = np.zeros((Q,) + frames.shape[1:], np.float64) if out is None else np.array(out, np.float64)
    with np.errstate(all="ignore"):
        for n in range(N):
            e = frames[n].astype(np.float64)
            if dark is not None:
                e = e - np.asarray(dark, np.float32).astype(np.float64)
            for q in range(Q):
                t = weights[n, q] * e
                acc[q] = acc[q] + t
    return acc


def _cells(a):
    """[..., H2, W2] -> [..., 4 sites, H2/2, W2/2]"""
    return np.stack([a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]], axis=-3)


def solve(M, rinv, a_nom, qmin):
    """M fp64 [3,H2,W2] -> (gain float32 [H2/2,W2/2,4,4], quality float32 [H2/2,W2/2])."""
    rinv, a_nom = np.asarray(rinv, np.float64).reshape(3, 3), np.asarray(a_nom, np.float64).reshape(4, 3)
    m = _cells(np.asarray(M, np.float64))                       # m[k][s] : [3,4,h,w]
    with np.errstate(all="ignore"):
        A = [[(m[0][s] * rinv[0][l] + m[1][s] * rinv[1][l]) + m[2][s] * rinv[2][l] for l in range(3)] for s in range(4)]
        N = [[None] * 3 for _ in range(3)]
        for k in range(3):
            for l in range(k, 3):
                N[k][l] = N[l][k] = ((A[0][k] * A[0][l] + A[1][k] * A[1][l]) + A[2][k] * A[2][l]) + A[3][k] * A[3][l]
        C = [[None] * 3 for _ in range(3)]
        C[0][0] = N[1][1] * N[2][2] - N[1][2] * N[1][2]
        C[0][1] = N[0][2] * N[1][2] - N[0][1] * N[2][2]
        C[0][2] = N[0][1] * N[1][2] - N[0][2] * N[1][1]
        C[1][1] = N[0][0] * N[2][2] - N[0][2] * N[0][2]
        C[1][2] = N[0][1] * N[0][2] - N[0][0] * N[1][2]
        C[2][2] = N[0][0] * N[1][1] - N[0][1] * N[0][1]
        C[1][0], C[2][0], C[2][1] = C[0][1], C[0][2], C[1][2]
        det = (N[0][0] * C[0][0] + N[0][1] * C[0][1]) + N[0][2] * C[0][2]
        V = [[C[k][l] / det for l in range(3)] for k in range(3)]
        P = [[(V[k][0] * A[s][0] + V[k][1] * A[s][1]) + V[k][2] * A[s][2] for s in range(4)] for k in range(3)]
        q = det / ((N[0][0] * N[1][1]) * N[2][2])
        good = q >= qmin                                        # False for NaN
        gain = np.empty(det.shape + (4, 4), np.float32)
        for t in range(4):
            for s in range(4):
                g = (a_nom[t][0] * P[0][s] + a_nom[t][1] * P[1][s]) + a_nom[t][2] * P[2][s]
                gain[..., t, s] = np.where(good, g.astype(np.float32), np.float32(1.0 if s == t else 0.0))
        quality = np.where(good, q.astype(np.float32), np.float32(0.0)).astype(np.float32)
    return gain, quality


def calibrate(mosaic, dark, gain):
    """mosaic [B,H2,W2] -> float32 [B,H2,W2]; gain [H2/2,W2/2,4,4] (CELL) or [H2,W2] (PIXEL); dark float32 [H2,W2] or None."""
    mosaic, gain = np.asarray(mosaic), np.asarray(gain, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e = mosaic.astype(np.float64)
        if dark is not None:
            e = e - np.asarray(dark, np.float32).astype(np.float64)
        if gain.ndim == 2:
            return (gain * e).astype(np.float32)
        es = _cells(e)                                          # [B,4,h,w]
        out = np.empty(mosaic.shape, np.float32)
        for t in range(4):
            G = gain[..., t, :]
            v = ((G[..., 0] * es[:, 0] + G[..., 1] * es[:, 1]) + G[..., 2] * es[:, 2]) + G[..., 3] * es[:, 3]
            out[:, (t >> 1)::2, (t & 1)::2] = v.astype(np.float32)
    return out


# ------------------------------------------------------------------------------ the host recipe of calibration.fit
def fit_weights(polarizer_deg, dolp=1.0, intensity=None):
    a = np.deg2rad(np.asarray(polarizer_deg, np.float64))
    iota = np.ones_like(a) if intensity is None else np.asarray(intensity, np.float64)
    return np.stack([iota, iota * (dolp * np.cos(2.0 * a)), iota * (dolp * np.sin(2.0 * a))], axis=1)


def nominal_matrix(layout=IMX250MZR, pol_angles=None):
    deg = NOMINAL_DEG if pol_angles is None else pol_angles
    th = np.deg2rad(np.asarray([deg[layout[s]] for s in range(4)], np.float64))
    return 0.5 * np.stack([np.ones_like(th), np.cos(2.0 * th), np.sin(2.0 * th)], axis=1)


def fit(frames, polarizer_deg, dark=None, layout=IMX250MZR, pol_angles=None, dolp=1.0, intensity=None, qmin=1e-3, chunks=None):
    """-> (gain, quality); ``chunks``: split points along N, the accumulate path of pd_frame_moments."""
    w = fit_weights(polarizer_deg, dolp, intensity)
    M = None
    edges = [0] + list(chunks or []) + [len(w)]
    for a, b in zip(edges[:-1], edges[1:]):
        M = moments(frames[a:b], w[a:b], dark, out=M)
    R1 = (w[:, :, None] * w[:, None, :]).sum(axis=0)
    kappa = 1.0 if intensity is not None else 2.0 * np.mean(M[0]) / len(w)
    rinv = np.linalg.inv(R1) / kappa
    return solve(M, rinv, nominal_matrix(layout, pol_angles), qmin)


def flat_field_gain(flat_mean, dark=None):
    """The PIXEL kind: (mean of the pixel's site class) / (pixel) of flat_mean - dark, fp64, stored as float32."""
    e = np.asarray(flat_mean, np.float64) - (0.0 if dark is None else np.asarray(dark, np.float32).astype(np.float64))
    g = np.empty(e.shape, np.float64)
    with np.errstate(all="ignore"):
        for r in (0, 1):
            for c in (0, 1):
                g[r::2, c::2] = np.mean(e[r::2, c::2]) / e[r::2, c::2]
    return g.astype(np.float32)


# ---------------------------------------------------------------------------------------------- synthetic sensor
class Sensor:
    """Per pixel: gain U(0.85, 1.15), analyzer angle error U(-3, 3) degrees, diattenuation U(0.90, 0.99), dark U(0.01, 0.03)
    of full scale.  ``dead``: {(i, j): [sites]} -- pixels that read their dark level whatever the light."""

    def __init__(self, shape, seed, layout=IMX250MZR, full=4095.0, ideal=False, dead=None):
        rng = np.random.default_rng([seed, shape[0], shape[1]])
        self.shape, self.layout, self.full = shape, layout, full
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        site = 2 * (yy & 1) + (xx & 1)
        nominal = np.asarray(NOMINAL_DEG)[np.asarray(layout)[site]]
        g, dth = rng.uniform(0.85, 1.15, shape), rng.uniform(-3.0, 3.0, shape)
        D, dk = rng.uniform(0.90, 0.99, shape), rng.uniform(0.01, 0.03, shape) * full
        if ideal:
            g, dth, D, dk = np.ones(shape), np.zeros(shape), np.ones(shape), np.zeros(shape)
        for (i, j), sites in (dead or {}).items():
            for s in sites:
                g[2 * i + (s >> 1), 2 * j + (s & 1)] = 0.0
        th = np.deg2rad(nominal + dth)
        self.a = 0.5 * g * np.stack([np.ones(shape), D * np.cos(2 * th), D * np.sin(2 * th)])      # [3,H2,W2]
        self.dark = dk.astype(np.float32)
        thn = np.deg2rad(nominal)
        self.a_ideal = 0.5 * np.stack([np.ones(shape), np.cos(2 * thn), np.sin(2 * thn)])

    def _up(self, S):
        """Stokes [..., 3, h, w] per cell -> [..., 3, H2, W2]"""
        return np.repeat(np.repeat(S, 2, axis=-2), 2, axis=-1)

    def measure(self, S, dtype="float32"):
        """What the sensor records of the per-cell Stokes vectors S [..., 3, h, w]: [..., H2, W2]."""
        v = (self.a * self._up(S)).sum(axis=-3) + self.dark.astype(np.float64)
        return v.astype(np.float32) if dtype == "float32" else np.clip(np.rint(v), 0, np.iinfo(dtype).max).astype(dtype)

    def flat_series(self, polarizer_deg, level=0.4, dtype="float32"):
        h, w = self.shape[0] // 2, self.shape[1] // 2
        a = np.deg2rad(np.asarray(polarizer_deg, np.float64))
        S = level * self.full * np.stack([np.ones_like(a), np.cos(2 * a), np.sin(2 * a)], axis=1)
        return self.measure(np.broadcast_to(S[:, :, None, None], (len(a), 3, h, w)), dtype)

    def scene(self, seed, B=1):
        """Per-cell Stokes vectors [B,3,h,w] with DoLP U(0, 0.6), and their (DoLP, AoLP)."""
        rng = np.random.default_rng([seed, 77])
        h, w = self.shape[0] // 2, self.shape[1] // 2
        I = rng.uniform(0.2, 0.6, (B, h, w)) * self.full
        rho, phi = rng.uniform(0.0, 0.6, (B, h, w)), rng.uniform(-np.pi / 2, np.pi / 2, (B, h, w))
        return np.stack([I, I * rho * np.cos(2 * phi), I * rho * np.sin(2 * phi)], axis=1), rho, phi


def cell_stokes(frame, layout=IMX250MZR):
    """Least-squares Stokes vector of every cell of a frame [..., H2, W2] under the nominal angles: [..., 3, h, w] fp64."""
    pinv = np.linalg.pinv(nominal_matrix(layout))               # [3,4]
    return np.einsum("ks,...shw->...khw", pinv, _cells(np.asarray(frame, np.float64)))


def dolp_aolp(S):
    return np.sqrt(S[..., 1, :, :] ** 2 + S[..., 2, :, :] ** 2) / S[..., 0, :, :], 0.5 * np.arctan2(S[..., 2, :, :], S[..., 1, :, :])


# the two cases of the issue: (mosaic shape, number of polarizer angles, seed)
CASES = [((8, 12), 12, 1), ((6, 10), 7, 2)]


def polarizer_angles(n):
    return [180.0 * k / n for k in range(n)]


@functools.lru_cache(maxsize=None)
def case(shape, n_angles, seed):
    """(sensor, angles, flat-field series float32 [N,H2,W2]) of one of CASES, read-only."""
    sensor = Sensor(shape, seed)
    deg = polarizer_angles(n_angles)
    flats = sensor.flat_series(deg)
    flats.setflags(write=False)
    return sensor, deg, flats


@functools.lru_cache(maxsize=None)
def frame(shape, dtype, seed=0, B=1):
    """A deterministic random stack [B,H2,W2]: full-range integers, or floats with fractional parts and both signs."""
    rng = np.random.default_rng([seed, shape[0], shape[1], DTYPES.index(dtype)])
    if dtype == "float32":
        a = (rng.standard_normal((B,) + shape) * 1000.0).astype(np.float32)
    else:
        a = rng.integers(0, np.iinfo(dtype).max + 1, (B,) + shape).astype(dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_dark(shape, seed=11):
    a = np.random.default_rng([seed, shape[0], shape[1]]).uniform(0.0, 40.0, shape).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_gain(shape, kind, seed=12):
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    a = (rng.standard_normal((shape[0] // 2, shape[1] // 2, 4, 4)) if kind == "cell" else rng.uniform(0.5, 1.5, shape)).astype(np.float32)
    a.setflags(write=False)
    return a
