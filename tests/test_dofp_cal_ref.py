"""tests/dofp_cal_ref.py, the NumPy statement of the DoFP calibration (include/polardepth.h), pinned on the host: the nominal
sensor, the property the feature rests on (a sensor with per-pixel gain, angle, extinction and dark errors measures the
scene's DoLP after calibration and not before), dead sites, the per-pixel kind and chunked accumulation."""
import numpy as np
import pytest

import dofp_cal_ref as C


def test_nominal_sensor_gives_the_projector_and_keeps_the_stokes_vector():
    """An ideal sensor, dark 0: every G is A_nom pinv(A_nom) -- 3/4 on the diagonal, +-1/4 elsewhere for 0/45/90/135 -- to a few
    ulp of fp32, the quality is 1 to rounding, and the least-squares Stokes vector of a calibrated frame is the raw frame's."""
    shape, deg = (8, 12), C.polarizer_angles(12)
    sensor = C.Sensor(shape, 3, ideal=True)
    gain, quality = C.fit(sensor.flat_series(deg), deg)
    a = C.nominal_matrix()
    want = a @ np.linalg.pinv(a)
    assert np.allclose(np.abs(want), np.where(np.eye(4, dtype=bool), 0.75, 0.25), atol=1e-15)
    assert np.abs(gain - want.astype(np.float32)).max() <= 4 * np.finfo(np.float32).eps
    assert np.abs(quality - 1.0).max() <= 4 * np.finfo(np.float32).eps
    S, _, _ = sensor.scene(5, B=2)
    raw = sensor.measure(S)
    cal = C.calibrate(raw, None, gain)
    s_raw, s_cal = C.cell_stokes(raw), C.cell_stokes(cal)
    assert np.abs(s_cal - s_raw).max() <= 2e-6 * np.abs(s_raw).max()      # fp32 storage of G and of the calibrated samples


@pytest.mark.parametrize("shape,n_angles,seed", C.CASES)
def test_calibration_recovers_the_dolp_the_raw_frame_loses(shape, n_angles, seed):
    """Gain U(0.85, 1.15), angle error U(-3, 3) degrees, diattenuation U(0.90, 0.99), dark 1..3 % of full scale; float32 frames,
    noise-free; a scene with DoLP U(0, 0.6).  Measured max DoLP error with this generator -- 8x12, 12 angles: uncalibrated 0.205,
    calibrated 1.05e-7; 6x10, 7 angles: uncalibrated 0.138, calibrated 8.0e-8 (AoLP at rho > 0.05, calibrated: 3.0e-7 and
    1.8e-7 rad).  What is left is the fp32 storage of frames, matrices and calibrated samples (2^-24 relative each); the AoLP
    bound is the DoLP bound over 2 rho_min = 0.1."""
    sensor, deg, flats = C.case(shape, n_angles, seed)
    gain, quality = C.fit(flats, deg, dark=sensor.dark)
    assert (quality > 0.5).all()
    S, rho, phi = sensor.scene(seed, B=2)
    raw = sensor.measure(S)
    d_raw, a_raw = C.dolp_aolp(C.cell_stokes(raw))
    d_cal, a_cal = C.dolp_aolp(C.cell_stokes(C.calibrate(raw, sensor.dark, gain)))
    wrap = lambda x: np.abs((x + np.pi / 2) % np.pi - np.pi / 2)
    strong = rho > 0.05
    print(shape, "DoLP error raw %.3g cal %.3g; AoLP error raw %.3g cal %.3g" % (
        np.abs(d_raw - rho).max(), np.abs(d_cal - rho).max(), wrap(a_raw - phi)[strong].max(), wrap(a_cal - phi)[strong].max()))
    assert np.abs(d_raw - rho).max() > 0.1
    assert np.abs(d_cal - rho).max() < 1e-6
    assert wrap(a_cal - phi)[strong].max() < 1e-5
    # the mean level of raw - dark survives (kappa)
    lvl_raw = (raw.astype(np.float64) - sensor.dark).mean()
    assert abs(C.calibrate(raw, sensor.dark, gain).mean() / lvl_raw - 1) < 0.05


def test_one_dead_site_is_rebuilt_and_two_give_the_identity():
    shape, deg = (8, 12), C.polarizer_angles(12)
    sensor = C.Sensor(shape, 4, dead={(1, 2): [3], (2, 4): [0, 1], (3, 0): [0]})
    gain, quality = C.fit(sensor.flat_series(deg), deg, dark=sensor.dark)
    assert np.isfinite(gain).all()
    for (i, j), s in (((1, 2), 3), ((3, 0), 0)):
        assert quality[i, j] > 1e-3 and (gain[i, j][:, s] == 0).all() and np.abs(gain[i, j]).max() > 0.5
    assert quality[2, 4] == 0 and np.array_equal(gain[2, 4], np.eye(4, dtype=np.float32))
    assert (quality == 0).sum() == 1
    # the dead sample is rebuilt from the other three: the cell's DoLP is the scene's
    S, rho, _ = sensor.scene(9)
    d_cal, _ = C.dolp_aolp(C.cell_stokes(C.calibrate(sensor.measure(S), sensor.dark, gain)))
    assert abs(d_cal[0, 1, 2] - rho[0, 1, 2]) < 1e-6 and abs(d_cal[0, 3, 0] - rho[0, 3, 0]) < 1e-6
    # moments that are NaN give the identity too
    w = C.fit_weights(deg)
    M = C.moments(sensor.flat_series(deg), w, sensor.dark)
    M[1, 0, 0] = np.nan
    g2, q2 = C.solve(M, np.linalg.inv((w[:, :, None] * w[:, None, :]).sum(axis=0)), C.nominal_matrix(), 1e-3)
    assert q2[0, 0] == 0 and np.array_equal(g2[0, 0], np.eye(4, dtype=np.float32)) and q2[0, 1] > 0


def test_pixel_kind_and_flat_field_gain():
    """The classical flat field: under unpolarised light every pixel of a site class is brought to the class mean."""
    sensor = C.Sensor((8, 12), 6)
    S = np.zeros((1, 3, 4, 6))
    S[:, 0] = 0.5 * sensor.full
    flat = sensor.measure(S)[0]
    g = C.flat_field_gain(flat, sensor.dark)
    assert g.dtype == np.float32 and g.shape == (8, 12)
    out = C.calibrate(flat[None], sensor.dark, g)[0]
    e = flat.astype(np.float64) - sensor.dark
    for r in (0, 1):
        for c in (0, 1):
            assert np.abs(out[r::2, c::2] / e[r::2, c::2].mean() - 1).max() < 1e-6
    # the definition, element by element
    m = C.frame((6, 10), "uint16", B=2)
    dark, gain = C.random_dark((6, 10)), C.random_gain((6, 10), "pixel")
    want = (gain.astype(np.float64) * (m.astype(np.float64) - dark.astype(np.float64))).astype(np.float32)
    assert np.array_equal(C.bits(C.calibrate(m, dark, gain)), C.bits(want))


def test_cell_kind_against_a_per_pixel_loop():
    shape = (6, 10)
    m, dark, gain = C.frame(shape, "float32", B=2), C.random_dark(shape), C.random_gain(shape, "cell")
    got = C.calibrate(m, dark, gain)
    for b in range(2):
        for y in range(shape[0]):
            for x in range(shape[1]):
                i, j, t = y // 2, x // 2, 2 * (y & 1) + (x & 1)
                e = [np.float64(m[b, 2 * i + (s >> 1), 2 * j + (s & 1)]) - np.float64(dark[2 * i + (s >> 1), 2 * j + (s & 1)])
                     for s in range(4)]
                G = gain[i, j, t].astype(np.float64)
                v = np.float32(((G[0] * e[0] + G[1] * e[1]) + G[2] * e[2]) + G[3] * e[3])
                assert C.bits(got[b, y, x]) == C.bits(v), (b, y, x)
    assert (got < 0).any()                                      # nothing is clamped


def test_chunked_accumulation_is_one_pass_bit_for_bit():
    sensor, deg, flats = C.case(*C.CASES[0])
    w = C.fit_weights(deg)
    one = C.moments(flats, w, sensor.dark)
    acc = None
    for a, b in ((0, 5), (5, 6), (6, 12)):
        acc = C.moments(flats[a:b], w[a:b], sensor.dark, out=acc)
    assert np.array_equal(C.bits(one), C.bits(acc))
    g1, q1 = C.fit(flats, deg, dark=sensor.dark)
    g2, q2 = C.fit(flats, deg, dark=sensor.dark, chunks=[5, 6])
    assert np.array_equal(C.bits(g1), C.bits(g2)) and np.array_equal(C.bits(q1), C.bits(q2))
    # Q = 1, w = 1 / N, no dark: the mean frame
    mean = C.moments(flats, np.full((12, 1), 1.0 / 12))[0]
    assert np.allclose(mean, flats.astype(np.float64).mean(axis=0), rtol=1e-14)
