"""pd_frame_moments, pd_dofp_cal_solve and pd_dofp_calibrate on the device against tests/dofp_cal_ref.py (the fp64 NumPy
statement, pinned by tests/test_dofp_cal_ref.py), bit for bit, and the calibration through fit, polar_inputs, a captured
graph and the Trainer.

Shapes are the smallest at which each path of csrc/dofp_cal.hip runs: 2x2 (one cell, one 4-pixel group), 6x10 and 10x18
(W2 % 4 == 2: one cell per lane, 8-byte stores), 8x8 (two cells per lane, 16-byte stores), and one uint8 frame with more work
items than the capped grid has threads (the grid-stride loop)."""
import warnings
import weakref

import numpy as np
import pytest
import torch

import dofp_cal_ref as C

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: cached arrays are read-only


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _equal(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    bad = C.bits(got) != C.bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _weights(N, Q, seed=3):
    return np.random.default_rng([seed, N, Q]).uniform(-1.5, 1.5, (N, Q))


# -------------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("with_dark", [False, True])
def test_moments_bit_for_bit(dtype, with_dark):
    from polardepth import calibration as cal
    for shape in C.SHAPES:
        dark = C.random_dark(shape) if with_dark else None
        for N in (1, 7):
            frames = C.frame(shape, dtype, seed=N, B=N)
            for Q in (1, 3):
                w = _weights(N, Q)
                got = _host(cal.frame_moments(_dev(frames), w, _dev(dark)))
                _equal(got, C.moments(frames, w, dark), (shape, N, Q))


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_two_accumulated_chunks_are_one_call(dtype):
    from polardepth import calibration as cal
    for shape in C.SHAPES:
        frames, dark, w = C.frame(shape, dtype, seed=7, B=7), C.random_dark(shape), _weights(7, 3)
        one = _host(cal.frame_moments(_dev(frames), w, _dev(dark)))
        acc = cal.frame_moments(_dev(frames[:3]), w[:3], _dev(dark))
        two = cal.frame_moments(_dev(frames[3:]), w[3:], _dev(dark), out=acc)
        assert two is acc
        _equal(_host(two), one, shape)
        _equal(one, C.moments(frames[3:], w[3:], dark, out=C.moments(frames[:3], w[:3], dark)), shape)
    # mean_frame: Q = 1, w = 1 / N, no dark, over chunks
    frames = C.frame((6, 10), dtype, seed=7, B=7)
    got = _host(cal.mean_frame([_dev(frames[:2]), _dev(frames[2:, None])]))
    _equal(got, C.moments(frames, np.full((7, 1), 1.0 / 7))[0].astype(np.float32))


def test_fit_and_mean_frame_take_a_generator_one_chunk_at_a_time():
    """An iterable of chunks is consumed lazily: when the generator is asked for the next chunk, nothing refers to the one
    before any more (it loads chunks that together need not fit in memory), and the result is the one-pass result bit for bit."""
    from polardepth import calibration as cal
    shape, n_angles, seed = C.CASES[1]
    sensor, deg, flats = C.case(shape, n_angles, seed)
    live = []

    def chunks(parts):
        for a in parts:
            assert all(r() is None for r in live), "an earlier chunk is still referenced when the next one is asked for"
            t = _dev(a)
            live.append(weakref.ref(t))
            yield t
            del t

    parts = [flats[:2], flats[2:3, None], flats[3:]]
    one = cal.fit(_dev(flats), deg, dark=_dev(sensor.dark))
    lazy = cal.fit(chunks(parts), deg, dark=_dev(sensor.dark))
    assert len(live) == 3 and all(r() is None for r in live)
    _equal(_host(lazy.gain), _host(one.gain))
    _equal(_host(lazy.quality), _host(one.quality))
    del live[:]
    _equal(_host(cal.mean_frame(chunks(parts), count=len(flats))), _host(cal.mean_frame(_dev(flats))))
    assert len(live) == 3 and all(r() is None for r in live)
    del live[:]
    with pytest.raises(ValueError, match="count=N"):
        cal.mean_frame(chunks(parts))
    for call, message in ((lambda: cal.mean_frame(chunks(parts), count=len(flats) + 1), f"{len(flats)} frames, but count = {len(flats) + 1}"),
                          (lambda: cal.fit(chunks(parts), deg[:-1]), f"{len(flats)} frames but {len(flats) - 1} polarizer angles"),
                          (lambda: cal.fit(chunks(parts[:2]), deg), f"3 frames but {len(flats)} polarizer angles")):
        del live[:]                                            # (a refused call's traceback may hold its chunk)
        with pytest.raises(ValueError, match=message):
            call()


# ---------------------------------------------------------------------------------------------------------- solve
def _flat_moments(shape, seed=4):
    """the moments of a flat-field series of the synthetic sensor, with one-dead, two-dead and NaN cells where they fit"""
    h, w = shape[0] // 2, shape[1] // 2
    dead = {(h - 1, w - 1): [3], (1, 2): [0, 1], (2, 0): [0]} if h >= 3 and w >= 3 else {}
    sensor = C.Sensor(shape, seed, dead=dead)
    deg = C.polarizer_angles(7)
    wts = C.fit_weights(deg)
    M = C.moments(sensor.flat_series(deg), wts, sensor.dark)
    if h >= 3:
        M[2, 1, 3] = np.nan
    R1 = (wts[:, :, None] * wts[:, None, :]).sum(axis=0)
    return M, np.linalg.inv(R1) / (2.0 * np.nanmean(M[0]) / len(wts)), dead


@pytest.mark.parametrize("layout,angles", [(C.IMX250MZR, None), ((1, 3, 0, 2), [0.8, 44.1, 91.3, 134.6])])
def test_solve_bit_for_bit(layout, angles):
    from polardepth import calibration as cal
    for shape in C.SHAPES:
        M, rinv, dead = _flat_moments(shape)
        a_nom = C.nominal_matrix(layout, angles)
        g_ref, q_ref = C.solve(M, rinv, a_nom, 1e-3)
        gain, quality = cal.solve(_dev(M), rinv, a_nom, 1e-3)
        _equal(_host(gain), g_ref, shape)
        _equal(_host(quality), q_ref, shape)
        only, none = cal.solve(_dev(M), rinv, a_nom, 1e-3, want_quality=False)
        assert none is None
        _equal(_host(only), g_ref, shape)
        if dead:
            h, w = shape[0] // 2, shape[1] // 2
            g, q = _host(gain), _host(quality)
            assert q[h - 1, w - 1] > 1e-3 and (g[h - 1, w - 1][:, 3] == 0).all() and np.isfinite(g[h - 1, w - 1]).all()
            for cell in ((1, 2), (0, 1)):                     # two dead sites; a NaN moment
                assert q[cell] == 0 and np.array_equal(g[cell], np.eye(4, dtype=np.float32)), cell
            assert int((q == 0).sum()) == 2


# ---------------------------------------------------------------------------------------------------------- apply
def _apply(mosaic, dark, gain):
    from polardepth import calibration as cal
    c = cal.Calibration(_dev(gain), _dev(dark))
    return _host(cal.apply(_dev(mosaic), c))


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("kind", ["cell", "pixel"])
def test_apply_bit_for_bit(kind, dtype):
    for shape in C.SHAPES:
        gain = C.random_gain(shape, kind)
        for B in (1, 3):
            m = C.frame(shape, dtype, seed=B, B=B)
            for dark in (C.random_dark(shape), None):
                _equal(_apply(m, dark, gain), C.calibrate(m, dark, gain), (shape, B, dark is None))
    m = C.frame((6, 10), dtype, B=2)
    got = _apply(m[:, None], None, C.random_gain((6, 10), kind))          # [B,1,H2,W2] keeps its shape
    assert got.shape == (2, 1, 6, 10)


@pytest.mark.parametrize("kind", ["cell", "pixel"])
def test_more_work_than_the_grid_has_threads(kind):
    """2048 workgroups x 256 threads = 524288 lanes: a 2048 x 2056 frame has 526336 pairs of cells (and twice as many 4-pixel
    groups), so the grid-stride loop takes a second pass."""
    shape = (2048, 2056)
    m = C.frame(shape, "uint8")
    rng = np.random.default_rng(8)
    dark = rng.uniform(0, 8, shape).astype(np.float32)
    gain = (rng.standard_normal((1024, 1028, 4, 4)) if kind == "cell" else rng.uniform(0.5, 1.5, shape)).astype(np.float32)
    _equal(_apply(m, dark, gain), C.calibrate(m, dark, gain))


def test_non_finite_samples_reach_exactly_their_cells():
    """A NaN, an infinity or FLT_MAX spreads to the four outputs of its own cell (a zero matrix entry still multiplies) and to
    nothing else; the rest of the frame keeps the reference's bits."""
    for shape in ((6, 10), (8, 8)):
        base, gain, dark = C.frame(shape, "float32")[0], C.random_gain(shape, "cell").copy(), C.random_dark(shape)
        gain[1, 1] = np.eye(4, dtype=np.float32)              # the identity: zeros multiply the non-finite sample
        for (y, x), v in (((2, 3), np.nan), ((3, 2), np.inf), ((0, 5), -np.inf), ((5, 0), C.FLT_MAX)):
            m = base.copy()
            m[y, x] = v
            got, ref = _apply(m[None], dark, gain)[0], C.calibrate(m[None], dark, gain)[0]
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
            ok = ~np.isnan(ref)
            assert np.array_equal(C.bits(got)[ok], C.bits(ref)[ok])
            if not np.isfinite(v):
                hit = ~np.isfinite(got)
                i, j = y // 2, x // 2
                assert hit.sum() == 4 and hit[2 * i:2 * i + 2, 2 * j:2 * j + 2].all(), (shape, y, x)
        # the per-pixel kind touches its own pixel only
        m = base.copy()
        m[2, 3], m[3, 2] = np.nan, np.inf
        g = C.random_gain(shape, "pixel")
        got, ref = _apply(m[None], dark, g)[0], C.calibrate(m[None], dark, g)[0]
        assert (~np.isfinite(got)).sum() == 2 and np.isnan(got[2, 3]) and np.isinf(got[3, 2])
        ok = ~np.isnan(ref)
        assert np.array_equal(C.bits(got)[ok], C.bits(ref)[ok])


def test_python_layer_on_the_device():
    from polardepth import calibration as cal
    c = cal.Calibration(_dev(C.random_gain((6, 10), "cell")))
    with pytest.raises(ValueError, match="8x8.*6x10"):
        cal.apply(torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda"), c)
    with pytest.raises(ValueError, match="torch.int32"):
        cal.apply(torch.zeros((1, 6, 10), dtype=torch.int32, device="cuda"), c)
    with pytest.raises(ValueError, match="cpu"):
        cal.apply(torch.zeros((1, 6, 10), dtype=torch.uint8, device="cuda"), c.to("cpu"))
    assert cal.apply(torch.zeros((0, 6, 10), dtype=torch.uint8, device="cuda"), c).shape == (0, 6, 10)
    assert c.to("cpu").to("cuda").gain.is_cuda


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("shape,n_angles,seed", C.CASES)
def test_fit_is_the_statement_and_polar_inputs_measures_the_scene(shape, n_angles, seed):
    """The synthetic sensor of tests/test_dofp_cal_ref.py: ``fit`` on the device gives the statement's matrices bit for bit
    (one pass and chunked), and K1 behind ``polar_inputs(calibration=)`` reports the scene's DoLP within that test's bound of
    1e-6, against more than 0.1 without the calibration.  8x12: a scene that varies from cell to cell, sampled planes (4x6);
    6x10 (planes of 3x5 are no multiple of K1's four pixels): three uniform scenes at the ends of the scene's ranges,
    interpolated planes.  Measured on the MI355X: 8x12 raw 0.205, calibrated 9.8e-8; 6x10 raw 0.227, calibrated 8.3e-8."""
    from polardepth import calibration as cal
    from polardepth import polar as pdpolar
    sensor, deg, flats = C.case(shape, n_angles, seed)
    g_ref, q_ref = C.fit(flats, deg, dark=sensor.dark)
    c = cal.fit(_dev(flats), deg, dark=_dev(sensor.dark))
    _equal(_host(c.gain), g_ref)
    _equal(_host(c.quality), q_ref)
    assert c.bad_cells == 0 and c.shape == shape and c.kind == "cell" and torch.equal(c.dark.cpu(), torch.from_numpy(sensor.dark))
    chunked = cal.fit([_dev(flats[:2]), _dev(flats[2:, None])], deg, dark=_dev(sensor.dark))
    _equal(_host(chunked.gain), g_ref)
    if shape[1] % 4 == 0:
        S, rho, _ = sensor.scene(seed, B=2)
        mode, size = "superpixel", (shape[0] // 2, shape[1] // 2)
    else:
        S, rho, mode, size = _uniform_scenes(sensor) + ("bilinear", shape)
    raw = sensor.measure(S)
    errs = []
    for calibration in (None, c):
        inputs = {("pol_dofp", 0, 0): _dev(raw[:, None])}
        pdpolar.polar_inputs(inputs, size, ("xolp",), dofp=(C.IMX250MZR, mode), calibration=calibration)
        dolp = _host(inputs[("xolp", 0, 0)])[:, 0].astype(np.float64)
        errs.append(np.abs(dolp - (rho if mode == "superpixel" else rho[:, None, None])).max())
    print(shape, "max DoLP error: raw %.3g, calibrated %.3g" % tuple(errs))
    assert errs[0] > 0.1
    assert errs[1] < 1e-6


def _uniform_scenes(sensor):
    """three spatially uniform scenes, DoLP 0 / 0.3 / 0.6 at intensities 0.6 / 0.4 / 0.2 of full scale: [3,3,h,w] and rho [3]"""
    h, w = sensor.shape[0] // 2, sensor.shape[1] // 2
    rho, phi, I = np.array([0.0, 0.3, 0.6]), np.array([0.3, -1.0, 1.2]), np.array([0.6, 0.4, 0.2]) * sensor.full
    S = np.stack([I, I * rho * np.cos(2 * phi), I * rho * np.sin(2 * phi)], axis=1)[:, :, None, None] * np.ones((1, 1, h, w))
    return S, rho


def test_colour_sensor_frames_are_calibrated_before_their_demosaic():
    """("pol_cdofp", 0, 0): every 2x2 polarizer cell lies under one Bayer colour, so the same matrices serve.  Uniform grey
    scenes (the demosaic interpolates between cells): DoLP within 1e-6 with the calibration, off by more than 0.1 without;
    expand_batch, which may run first, makes the same call.  Measured on the MI355X: raw 0.138, calibrated 7.1e-8."""
    from polardepth import calibration as cal
    from polardepth import polar as pdpolar
    from polardepth import color as pdcolor
    shape, n_angles, seed = C.CASES[0]
    sensor, deg, flats = C.case(shape, n_angles, seed)
    c = cal.fit(_dev(flats), deg, dark=_dev(sensor.dark))
    S, rho = _uniform_scenes(sensor)
    raw = sensor.measure(S)
    errs = []
    for calibration in (None, c):
        inputs = {("pol_cdofp", 0, 0): _dev(raw[:, None])}
        pdpolar.polar_inputs(inputs, shape, ("xolp",), cdofp=((2, 1, 3, 0), (0, 1, 1, 2), None, 255.0 / 4095.0),
                             calibration=calibration)
        assert inputs[("color_raw", 0, 0)].dtype == torch.uint8
        errs.append(np.abs(_host(inputs[("xolp", 0, 0)])[:, 0].astype(np.float64) - rho[:, None, None]).max())
    print("colour sensor, max DoLP error: raw %.3g, calibrated %.3g" % tuple(errs))
    assert errs[0] > 0.1
    assert errs[1] < 1e-6
    first = {("pol_cdofp", 0, 0): _dev(raw[:, None])}
    pdcolor.expand_batch(first, shape, 1, cdofp=((2, 1, 3, 0), (0, 1, 1, 2), None, 255.0 / 4095.0), calibration=c)
    assert torch.equal(first[("pol", 0, 0)], inputs[("pol", 0, 0)])
    # a uint8 frame keeps its default colour scale of 1 although the calibrated frame is float32
    u8 = {("pol_cdofp", 0, 0): _dev(np.clip(raw[:, None] / 16.0, 0, 255).astype(np.uint8))}
    pdpolar.polar_inputs(u8, shape, ("xolp",), calibration=c)
    assert u8[("color_raw", 0, 0)].dtype == torch.uint8 and u8[("pol", 0, 0)].dtype == torch.float32


def test_apply_captured_in_a_graph_replays_the_eager_result():
    from polardepth import calibration as cal
    shape = (8, 8)
    c = cal.Calibration(_dev(C.random_gain(shape, "cell")), _dev(C.random_dark(shape)))
    static = _dev(C.frame(shape, "uint16", seed=1, B=3))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cal.apply(static, c)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cal.apply(static, c)
    for seed in (2, 3):
        m = C.frame(shape, "uint16", seed=seed, B=3)
        static.copy_(_dev(m))
        graph.replay()
        _equal(_host(out), C.calibrate(m, C.random_dark(shape), C.random_gain(shape, "cell")), seed)
        assert torch.equal(out, cal.apply(static, c))


# -------------------------------------------------------------------------------------------------------- Trainer
NET_HW = (64, 96)
TREE_HW = (192, 256)         # the sensor frames of test_dofp_cabi._tree


@pytest.fixture(scope="module")
def dofp_tree(tmp_path_factory):
    """a small HAMMER tree whose polarizer data are uint8 pol_dofp mosaics of 192 x 256 (two frames of one scene)"""
    from PIL import Image
    from test_dofp_cabi import _tree, _mosaic
    root = tmp_path_factory.mktemp("dofp_tree")
    _tree(root, ("pol_dofp",), lambda path, idx: Image.fromarray(_mosaic(idx, np.uint8)).save(path))
    return root


def _fitted(shape):
    from polardepth import calibration as cal
    sensor = C.Sensor(shape, 5, full=255.0)
    deg = C.polarizer_angles(7)
    return cal.fit(_dev(sensor.flat_series(deg)), deg, dark=_dev(sensor.dark))


@pytest.fixture(scope="module")
def tree_calibration():
    return _fitted(TREE_HW)


def _tree_trainer(tmp_path, tree, spec):
    """a Trainer whose loaders read the tree's sensor frames (PD_POL_DOFP=1 is set by the caller)"""
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    torch.manual_seed(0)
    opts = _opts(tmp_path, ["--dropout_rate", "0.0", "--overfit", "True", "--overfit_scene", "scene1_traj1_1",
                            "--data_path", str(tree)])
    if spec is not None:
        opts.pol_calibration = spec
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        tr = Trainer(opts)
    assert not [w for w in seen if "pol_calibration" in str(w.message)]          # the loaders do serve sensor frames
    tr.set_train()
    return tr


def _eager_step(tr, batch):
    tr.model_optimizer.zero_grad()
    inputs = dict(batch)
    _, loss, _ = tr.process_batch(inputs, is_train=True)
    loss["loss"].backward()
    tr.model_optimizer.step()
    return loss["loss"].detach().clone(), inputs


def test_trainer_steps_on_a_sensor_tree_with_the_calibration_eager_and_captured(tmp_path, monkeypatch, dofp_tree, tree_calibration):
    """Training steps on the batch a Trainer's own loader reads from a ``pol_dofp`` tree: with ``opt.pol_calibration`` (given as
    the path of a saved calibration of the tree's frame size, accepted at construction) K1 sees the calibrated frame and the loss
    differs from the step without it; the captured step (``GraphedTrainStep``, what PD_STEP_GRAPH=1 builds) holds the
    calibration pass and replays the eager steps bit for bit."""
    from polardepth import polar as pdpolar
    from polardepth import calibration as cal
    from polardepth import functional as PF
    from polardepth.graph import GraphedTrainStep
    monkeypatch.setenv("PD_POL_DOFP", "1")
    path = tmp_path / "cal.npz"
    tree_calibration.save(str(path))
    tr_plain = _tree_trainer(tmp_path / "plain", dofp_tree, None)
    assert tr_plain.pol_calibration is None
    batch = {k: v.cuda() for k, v in next(iter(tr_plain.train_loader)).items()}
    mosaic = batch[("pol_dofp", 0, 0)]
    assert mosaic.shape == (2, 1) + TREE_HW and mosaic.dtype == torch.uint8 and ("pol", 0, 0) not in batch
    PF.DropoutState.manual_seed(3)
    loss_plain, in_plain = _eager_step(tr_plain, batch)
    PF.DropoutState.manual_seed(3)
    tr_cal = _tree_trainer(tmp_path / "cal", dofp_tree, str(path))
    assert tr_cal.pol_calibration.shape == TREE_HW and tr_cal.pol_calibration.gain.is_cuda
    losses_e = []
    for _ in range(2):
        loss, in_cal = _eager_step(tr_cal, batch)
        losses_e.append(loss)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss_plain)) and all(bool(torch.isfinite(x)) for x in losses_e)
    assert not torch.equal(loss_plain, losses_e[0]) and not torch.equal(in_plain[("xolp", 0, 0)], in_cal[("xolp", 0, 0)])
    want = {("pol_dofp", 0, 0): cal.apply(mosaic, tree_calibration)}           # what K1 saw is the calibrated frame
    pdpolar.polar_inputs(want, NET_HW, ("xolp",))
    assert torch.equal(want[("xolp", 0, 0)], in_cal[("xolp", 0, 0)])
    PF.DropoutState.manual_seed(3)
    tr_g = _tree_trainer(tmp_path / "graph", dofp_tree, tree_calibration)
    gs = GraphedTrainStep(tr_g, batch, warmup=1, restore_state=True)
    losses_g = [gs.step(batch).detach().clone() for _ in range(2)]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(losses_e, losses_g)):
        assert torch.equal(a, b), f"loss of step {i}: eager {a.item()!r} graph {b.item()!r}"
    assert torch.equal(tr_cal.store.flat, tr_g.store.flat)


def test_trainer_refuses_a_calibration_of_another_layout_or_shape(tmp_path, monkeypatch, dofp_tree):
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    from manydepth.evaluation import Evaluation
    c = _fitted(NET_HW)
    bad = _opts(tmp_path / "layout", ["--dropout_rate", "0.0"])
    bad.pol_calibration, bad.pol_layout = c, [1, 3, 0, 2]
    with pytest.raises(ValueError, match=r"\(2, 1, 3, 0\).*\(1, 3, 0, 2\)"):
        Trainer(bad)
    with pytest.raises(ValueError, match=r"\(2, 1, 3, 0\).*\(1, 3, 0, 2\)"):
        Evaluation(data_path="synthetic", height=NET_HW[0], width=NET_HW[1], batch_size=2, pol_layout=(1, 3, 0, 2), pol_calibration=c)
    # loaders that serve no sensor frames: the option is idle, one warning
    idle = _opts(tmp_path / "idle", ["--dropout_rate", "0.0"])
    idle.pol_calibration = c
    with pytest.warns(UserWarning, match="pol_calibration"):
        assert Trainer(idle).pol_calibration.shape == NET_HW
    # the tree's sensor frames are 192 x 256: the 64 x 96 calibration does not serve them
    monkeypatch.setenv("PD_POL_DOFP", "1")
    opts = _opts(tmp_path / "shape", ["--dropout_rate", "0.0", "--overfit", "True", "--overfit_scene", "scene1_traj1_1",
                                      "--data_path", str(dofp_tree)])
    opts.pol_calibration = c
    with pytest.raises(ValueError, match="64x96.*training loader.*192x256"):
        Trainer(opts)
