"""pd_dofp_demosaic on the device against tests/dofp_ref.py (the fp64 NumPy statement, pinned by tests/test_dofp_ref.py),
bit for bit, and the new input path through polar_inputs, the Trainer and Evaluation.

Shapes are the smallest at which each path of csrc/dofp.hip runs: 2x2 (every neighbour mirrored) .. 6x10 for all 24
layouts; 34x70 and 70x134 with B = 3 (several waves in both directions, rows 16-byte aligned for no dtype, odd plane widths:
the element-wide super-pixel kernel and the 8-byte bilinear stores); widths that give the super-pixel kernel each of its
access widths and the bilinear kernel its 16-byte path, across more than one workgroup; and one frame per mode with more
work items than the capped grid has threads (the grid-stride loop)."""
import ctypes

import numpy as np
import pytest
import torch

import dofp_ref as D

pytestmark = pytest.mark.gpu

MODES = ["superpixel", "bilinear"]
OTHER = (1, 3, 0, 2)
NET_HW = (64, 96)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cached frames are read-only


def _run(mosaic, layout, mode):
    from polardepth import dofp
    out = dofp.demosaic(_dev(mosaic), layout, mode)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(mosaic, layout, mode):
    got = _run(mosaic, layout, mode)
    ref = D.demosaic(mosaic.reshape((mosaic.shape[0],) + mosaic.shape[-2:]), layout, mode)      # [B,1,H2,W2] or [B,H2,W2]
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.dtype, ref.shape)
    bad = D.bits(got) != D.bits(ref)
    assert not bad.any(), (mosaic.shape, mosaic.dtype, layout, mode, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_all_layouts_at_the_smallest_shapes(mode, dtype):
    for shape in D.SMALL_SHAPES:
        m = D.frame(shape, dtype, B=2)
        for layout in D.LAYOUTS:
            _check(m, layout, mode)


@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(34, 70), (70, 134)])
def test_unaligned_rows_over_several_waves(shape, mode, dtype):
    m = D.frame(shape, dtype, B=3)
    for layout in (D.IMX250MZR, OTHER):
        _check(m, layout, mode)
    _check(m[:, None], D.IMX250MZR, mode)       # [B,1,H2,W2] is taken too


# plane widths 128, 24, 12, 10 (and 35, 67 above): 16 / 8 / 4 / 2 (/ 1) elements per super-pixel access for uint8, capped at 16
# bytes for the wider types; mosaic widths that are multiples of 4 take the 16-byte bilinear path, 20 does with two workgroups
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(40, 256), (6, 48), (6, 24), (22, 20)])
def test_every_access_width(shape, mode, dtype):
    m = D.frame(shape, dtype, B=3)
    for layout in (D.IMX250MZR, OTHER):
        _check(m, layout, mode)


@pytest.mark.parametrize("mode,shape", [("bilinear", (1030, 2048)), ("superpixel", (1452, 1454))])
def test_more_work_than_the_grid_has_threads(mode, shape):
    """2048 workgroups x 256 threads = 524288: 1030 x 512 bilinear chunks and 726 x 727 element-wide super-pixels exceed it."""
    _check(D.frame(shape, "uint8"), D.IMX250MZR, mode)


# ---------------------------------------------------------------------------------------------------- value cases
@pytest.mark.parametrize("layout", [D.IMX250MZR, OTHER])
def test_extreme_frames_come_back_unchanged(layout):
    for shape in ((6, 10), (34, 70), (8, 16)):
        got = _run(np.full((1,) + shape, 65535, np.uint16), layout, "bilinear")
        assert np.array_equal(got, np.full((1, 4) + shape, 65535.0, np.float32))
        got = _run(np.full((1,) + shape, 65535, np.uint16), layout, "superpixel")
        assert got.dtype == np.uint16 and (got == 65535).all()
        for v in (D.FLT_MAX, -D.FLT_MAX):
            got = _run(np.full((1,) + shape, v, np.float32), layout, "bilinear")
            assert np.isfinite(got).all() and (got == np.float32(v)).all()


@pytest.mark.parametrize("shape", [(34, 70), (36, 72)])
def test_wide_dynamic_range_needs_the_fp64_order(shape):
    """Values over 2^40: an fp32 accumulation differs from the definition on about 14 % of the diagonal sites at 34x70
    (tests/test_dofp_ref.py asserts it), so only fp64 sums in the header's order, rounded once, pass."""
    m = D.wide_range_frame(shape, B=2)
    for layout in (D.IMX250MZR, OTHER):
        _check(m, layout, "bilinear")
        _check(m, layout, "superpixel")


def test_denormals_are_kept():
    rng = np.random.default_rng(9)
    for shape in ((6, 10), (8, 16)):
        bitsv = rng.integers(1, 1 << 23, (2,) + shape).astype(np.uint32) | (rng.integers(0, 2, (2,) + shape).astype(np.uint32) << 31)
        m = bitsv.view(np.float32)
        assert (np.abs(m) < np.finfo(np.float32).tiny).all() and (m != 0).all()
        ref = D.bilinear(m, D.IMX250MZR)
        assert (ref != 0).mean() > 0.9
        _check(m, D.IMX250MZR, "bilinear")
        _check(m, D.IMX250MZR, "superpixel")


@pytest.mark.parametrize("shape", [(10, 14), (12, 16)])
def test_non_finite_samples_reach_exactly_their_stencils(shape):
    """A NaN or an infinity spreads to the outputs whose stencil holds it -- nine in the plane its site feeds, none elsewhere --
    and the rest of the frame keeps the reference's bits."""
    base = D.frame(shape, "float32")[0]
    for layout in (D.IMX250MZR, OTHER):
        for (y, x), v in (((4, 6), np.nan), ((7, 3), np.inf), ((5, 9), -np.inf)):
            m = base.copy()
            m[y, x] = v
            got, ref = _run(m[None], layout, "bilinear")[0], D.bilinear(m, layout)
            hit = ~np.isfinite(got)
            assert np.array_equal(hit, ~np.isfinite(ref)) and np.array_equal(np.isnan(got), np.isnan(ref))
            p = layout[2 * (y & 1) + (x & 1)]
            assert hit.sum() == 9 and hit[p, y - 1:y + 2, x - 1:x + 2].all()
            assert np.array_equal(D.bits(got)[~np.isnan(ref)], D.bits(ref)[~np.isnan(ref)])
            sp = _run(m[None], layout, "superpixel")[0]
            assert np.array_equal(D.bits(sp), D.bits(D.superpixel(m, layout)))
        # +inf and -inf under one stencil give NaN there, like the definition
        m = base.copy()
        m[4, 4], m[4, 6] = np.inf, -np.inf
        got, ref = _run(m[None], layout, "bilinear")[0], D.bilinear(m, layout)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got).sum() >= 1
        assert np.array_equal(D.bits(got)[~np.isnan(ref)], D.bits(ref)[~np.isnan(ref)])


# ---------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("dtype", D.DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_nothing_is_written_outside_the_planes(mode, dtype):
    """Input and output sit inside larger sentinel-filled buffers at 16-byte aligned offsets; afterwards the output region
    holds the reference and every other byte of both buffers is what it was."""
    from polardepth._lib import lib, check
    from polardepth.dofp import MODES as CODES
    for shape, B in (((2, 2), 1), ((6, 10), 2), ((34, 70), 2), ((8, 48), 2)):
        m = D.frame(shape, dtype, seed=3, B=B)
        ref = D.demosaic(m, D.IMX250MZR, mode)
        in_off, out_off, tail = 48, 64, 4096
        src = np.full(in_off + m.nbytes + tail, 0xA5, np.uint8)
        src[in_off:in_off + m.nbytes] = m.view(np.uint8).reshape(-1)
        d_src = _dev(src)
        d_dst = torch.full((out_off + ref.nbytes + tail,), 0x5A, dtype=torch.uint8, device="cuda")
        layout = (ctypes.c_int * 4)(*D.IMX250MZR)
        check(lib.pd_dofp_demosaic(ctypes.c_void_p(d_src.data_ptr() + in_off), D.DTYPES.index(dtype),
                                   ctypes.c_void_p(d_dst.data_ptr() + out_off), CODES[mode], layout, B, shape[0], shape[1],
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pd_dofp_demosaic")
        torch.cuda.synchronize()
        dst = d_dst.cpu().numpy()
        assert np.array_equal(d_src.cpu().numpy(), src)
        assert (dst[:out_off] == 0x5A).all() and (dst[out_off + ref.nbytes:] == 0x5A).all(), (shape, mode, dtype)
        assert np.array_equal(dst[out_off:out_off + ref.nbytes], ref.view(np.uint8).reshape(-1)), (shape, mode, dtype)


# ------------------------------------------------------------------------------------------- through the pipeline
def _mosaic_for(dtype, shape, B=2, seed=21):
    """a frame with structure (a smooth polarised scene seen through the IMX250MZR's filters) plus noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    hi = 255.0 if dtype == "uint8" else 4095.0
    iun = hi * (0.45 + 0.25 * np.sin(xx / 17.0) * np.cos(yy / 13.0))
    rho = 0.05 + 0.3 * (0.5 + 0.5 * np.sin(xx / 11.0 + yy / 19.0)) ** 2
    phi = (np.pi / 2) * np.sin(xx / 23.0 - yy / 29.0)
    planes = np.stack([iun * (1 + rho * np.cos(2 * a - 2 * phi)) for a in (0, np.pi / 4, np.pi / 2, 3 * np.pi / 4)])
    planes = np.clip(planes[None] + rng.normal(0, hi / 100.0, (B,) + planes.shape), 0, hi)
    m = D.mosaic_of(planes, D.IMX250MZR)
    return m.astype(np.float32) if dtype == "float32" else np.rint(m).astype(dtype)


PIPELINE = [  # dtype, mode, mosaic size, layout, calibrated angles
    ("uint8", "superpixel", (128, 192), D.IMX250MZR, None),           # planes 64x96 uint8: K1's look-up-table kernel
    ("uint16", "superpixel", (128, 192), D.IMX250MZR, None),          # general kernel
    ("uint16", "bilinear", (64, 96), D.IMX250MZR, None),              # float planes at network size: general kernel
    ("uint16", "superpixel", (128, 192), OTHER, [0.8, 44.1, 91.3, 134.6]),
    ("uint16", "bilinear", (208, 272), D.IMX250MZR, None),            # float planes 208x272: the device LANCZOS resize first
    ("uint8", "superpixel", (416, 544), OTHER, None),                 # uint8 planes 208x272: the 8-bit resize, then K1
]


@pytest.mark.parametrize("dtype,mode,shape,layout,angles_deg", PIPELINE)
def test_polar_inputs_demosaics_first(dtype, mode, shape, layout, angles_deg):
    """A batch that carries only ("pol_dofp", 0, 0) gives the ("xolp", 0, 0) and normals of the batch that carries the planes
    tests/dofp_ref.py computes from it on the host."""
    from polardepth import polar as pdpolar
    m = _mosaic_for(dtype, shape)
    angles = pdpolar.angles_from_degrees(angles_deg)
    dev = {("pol_dofp", 0, 0): _dev(m[:, None])}
    host = {("pol", 0, 0): _dev(D.demosaic(m, layout, mode))}
    n_dev = pdpolar.polar_inputs(dev, NET_HW, ("xolp", "normals"), angles, dofp=(layout, mode))
    n_host = pdpolar.polar_inputs(host, NET_HW, ("xolp", "normals"), angles)
    torch.cuda.synchronize()
    assert dev[("pol", 0, 0)].dtype == host[("pol", 0, 0)].dtype and dev[("pol", 0, 0)].shape == host[("pol", 0, 0)].shape
    assert dev[("xolp", 0, 0)].shape == (2, 2) + NET_HW and n_dev.shape == (2, 9) + NET_HW
    assert _same(dev[("xolp", 0, 0)], host[("xolp", 0, 0)]) and _same(n_dev, n_host)
    assert bool((dev[("xolp", 0, 0)][:, 0] > 0).any())


def test_polar_inputs_defaults_and_precedence():
    from polardepth import polar as pdpolar
    m = _mosaic_for("uint16", NET_HW)
    dflt = {("pol_dofp", 0, 0): _dev(m)}                                # [B,H2,W2]; dofp=None: IMX250MZR, bilinear
    pdpolar.polar_inputs(dflt, NET_HW, ("xolp",))
    host = {("pol", 0, 0): _dev(D.bilinear(m, D.IMX250MZR))}
    pdpolar.polar_inputs(host, NET_HW, ("xolp",))
    assert _same(dflt[("xolp", 0, 0)], host[("xolp", 0, 0)])
    # planes that are already there win: the mosaic is not looked at
    both = {("pol_dofp", 0, 0): _dev(m), ("pol", 0, 0): host[("pol", 0, 0)].clone()}
    pdpolar.polar_inputs(both, NET_HW, ("xolp",), dofp=(OTHER, "superpixel"))
    assert _same(both[("xolp", 0, 0)], host[("xolp", 0, 0)])
    for bad, match in ((((0, 1, 2, 2), "bilinear"), "permutation"), ((D.IMX250MZR, "cubic"), "'cubic'")):
        with pytest.raises(ValueError, match=match):
            pdpolar.polar_inputs({("pol_dofp", 0, 0): _dev(m)}, NET_HW, ("xolp",), dofp=bad)
    from polardepth import dofp
    with pytest.raises(ValueError, match="even sides"):
        dofp.demosaic(torch.zeros((1, 5, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="torch.int32"):
        dofp.demosaic(torch.zeros((1, 4, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match=r"\(1, 2, 4, 8\)"):
        dofp.demosaic(torch.zeros((1, 2, 4, 8), dtype=torch.uint8, device="cuda"))
    assert dofp.demosaic(torch.zeros((0, 4, 8), dtype=torch.uint8, device="cuda")).shape == (0, 4, 4, 8)


def test_unpolarised_ramp_has_no_dolp_only_when_interpolated():
    """The physics: 3x + 5y + 7 is unpolarised.  Bilinear planes agree in the interior, so DoLP is exactly 0 there; the sampled
    planes differ by up to 8 counts and report polarisation that is not in the scene."""
    from polardepth import dofp
    from polardepth import polar as pdpolar
    m = _dev(D.affine_field((64, 96))[None])
    bl = pdpolar.polar_forward(dofp.demosaic(m, D.IMX250MZR, "bilinear"), want=("xolp",))["xolp"]
    sp = pdpolar.polar_forward(dofp.demosaic(m, D.IMX250MZR, "superpixel"), want=("xolp",))["xolp"]
    torch.cuda.synchronize()
    assert bool((bl[0, 0, 1:-1, 1:-1] == 0).all())
    assert bool((sp[0, 0] > 0).any())


def test_evaluation_takes_the_sensor_frame():
    """Evaluation.predict: a synthetic batch whose planes were re-packed into the sensor's mosaic and sampled in super-pixel
    mode gives, bit for bit, the depth of the batch that carries the corresponding half-size planes."""
    from manydepth.evaluation import Evaluation
    from polardepth import synthetic
    torch.manual_seed(0)
    ev = Evaluation(data_path="synthetic", height=NET_HW[0], width=NET_HW[1], batch_size=2, pol_layout=OTHER,
                    pol_demosaic="superpixel")
    base = synthetic.make_batch(2, NET_HW[0], NET_HW[1], frame_w=NET_HW[1], device="cuda", seed=3)
    planes = base[("pol", 0, 0)].cpu().numpy()
    half = np.stack([planes[:, p, r::2, c::2] for p, (r, c) in ((p, D.site_of(OTHER, p)) for p in range(4))], axis=1)
    outs = []
    for key, value in ((("pol", 0, 0), half), (("pol_dofp", 0, 0), D.mosaic_of(planes, OTHER)[:, None])):
        inputs = {k: v for k, v in base.items() if k not in (("pol", 0, 0), ("xolp", 0, 0))}
        inputs[key] = _dev(value)
        depth = ev.predict(inputs)
        torch.cuda.synchronize()
        assert depth.shape == (2, 1) + NET_HW and bool(torch.isfinite(depth).all())
        outs.append((depth, inputs[("xolp", 0, 0)]))
    assert _same(outs[0][1], outs[1][1]) and _same(outs[0][0], outs[1][0])
    with pytest.raises(ValueError, match="permutation"):
        Evaluation(data_path="synthetic", height=NET_HW[0], width=NET_HW[1], batch_size=2, pol_layout="0,1,2,2")


def test_trainer_reads_layout_and_mode_from_its_options(tmp_path):
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    from polardepth import dofp
    torch.manual_seed(0)
    opts = _opts(tmp_path / "dofp", ["--dropout_rate", "0.0"])
    opts.pol_layout, opts.pol_demosaic = list(OTHER), "superpixel"
    tr = Trainer(opts)
    assert tr.pol_dofp == (OTHER, "superpixel")
    m = _mosaic_for("uint16", (128, 192))
    dev = {("pol_dofp", 0, 0): _dev(m[:, None])}
    host = {("pol", 0, 0): _dev(D.superpixel(m, OTHER))}
    n_dev, n_host = tr._polar_inputs(dev), tr._polar_inputs(host)
    torch.cuda.synchronize()
    assert _same(dev[("xolp", 0, 0)], host[("xolp", 0, 0)]) and _same(n_dev, n_host)
    assert Trainer(_opts(tmp_path / "default", ["--dropout_rate", "0.0"])).pol_dofp == (dofp.IMX250MZR, "bilinear")
    bad = _opts(tmp_path / "bad", ["--dropout_rate", "0.0"])
    bad.pol_demosaic = "nearest"
    with pytest.raises(ValueError, match="'nearest'"):
        Trainer(bad)
