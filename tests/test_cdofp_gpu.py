"""pd_cdofp_demosaic on the device against tests/cdofp_ref.py (the fp64 NumPy statement, pinned by tests/test_cdofp_ref.py),
bit for bit -- fp32 as bits with the NaN positions equal, uint8 exactly -- and the new input path through polar_inputs,
expand_batch and the Trainer.

Shapes: 4x4, 4x8 and 8x4 (every lattice index clamped, in one or both directions), 12x20 (colour rows that are only 4-byte
aligned), 36x52 and 72x136 (several chunks per row, rows spread over more than one workgroup, interior and all four borders),
and one frame with more chunks than the capped grid has threads (the grid-stride loop)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cdofp_ref as C

pytestmark = pytest.mark.gpu

GAINS = (1.7, 0.9, 2.3)
LAYOUTS = [C.IMX250MYR_POL, C.OTHER_LAYOUT, (0, 1, 2, 3), (3, 0, 1, 2)]      # the three ways planes 0/1 and 2/3 can pair up on sites
NET_HW = (64, 96)
KEYS = ("planes", "color", "rgb_planes")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cached frames are read-only


def _scale(dtype):
    return 1.0 if str(dtype) == "uint8" else C.SCALE_12BIT


@functools.lru_cache(maxsize=None)
def _ref(shape, dtype, B, layout, bayer, gains, scale):
    return dict(zip(KEYS, C.demosaic(C.frame(shape, dtype, B=B), layout, bayer, gains, scale)))


def _run(mosaic, layout, bayer, gains, scale, want=KEYS):
    from polardepth import cdofp
    out = cdofp.demosaic(_dev(mosaic), layout, bayer, gains, scale, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, what):
    for k, g in got.items():
        r = ref[k]
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, g.shape, r.dtype, r.shape)
        if not C.same_bits(g, r):
            bad = (C.bits(g) != C.bits(r)) & ~(np.isnan(g) & np.isnan(r)) if g.dtype.kind == "f" else g != r
            raise AssertionError((what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist()))


# ------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_bit_equal_to_the_definition(shape, dtype):
    """B = 1 and 3, the four Bayer orders each with another polarizer layout, white-balance gains, all three outputs."""
    for B in (1, 3):
        for layout, bayer in zip(LAYOUTS, C.BAYERS):
            got = _run(C.frame(shape, dtype, B=B), layout, bayer, GAINS, _scale(dtype))
            _compare(got, _ref(shape, dtype, B, layout, bayer, GAINS, _scale(dtype)), (shape, dtype, B, layout, bayer))


@pytest.mark.parametrize("layout", [C.IMX250MYR_POL, C.OTHER_LAYOUT])
@pytest.mark.parametrize("bayer", C.BAYERS)
def test_every_bayer_order_with_both_layouts(bayer, layout):
    got = _run(C.frame((36, 52), "uint16", B=1), layout, bayer, None, C.SCALE_12BIT)
    _compare(got, _ref((36, 52), "uint16", 1, layout, bayer, None, C.SCALE_12BIT), (layout, bayer))
    got = _run(C.frame((36, 52), "uint16", B=1)[:, None], layout, bayer, (1, 1, 1), C.SCALE_12BIT)      # [B,1,H4,W4] too
    _compare(got, _ref((36, 52), "uint16", 1, layout, bayer, None, C.SCALE_12BIT), (layout, bayer, "unit gains"))


@pytest.mark.parametrize("mask", range(1, 8))
def test_each_output_alone_and_together(mask):
    """The NULL paths: any subset of the three outputs gives the bits of the full call."""
    want = tuple(k for i, k in enumerate(KEYS) if mask >> i & 1)
    for dtype, shape in (("uint8", (12, 20)), ("float32", (36, 52))):
        scale = 1.0 if dtype == "uint8" else 0.01
        got = _run(C.frame(shape, dtype, B=3), C.IMX250MYR_POL, C.GRBG, GAINS, scale, want)
        assert set(got) == set(want)
        _compare(got, _ref(shape, dtype, 3, C.IMX250MYR_POL, C.GRBG, GAINS, scale), (mask, dtype))


@pytest.mark.parametrize("bayer", C.BAYERS)
def test_nan_inf_flt_max_and_denormals(bayer):
    m = C.special_frame()
    ref = dict(zip(KEYS, C.demosaic(m, C.IMX250MYR_POL, bayer, (1.3, 1.0, 0.7), 1.0)))
    assert np.isnan(ref["planes"]).any() and np.isinf(ref["rgb_planes"]).any()
    den = np.abs(ref["rgb_planes"][0, :, :, 21:26, 9:18])
    assert ((den > 0) & (den < np.finfo(np.float32).tiny)).any()            # denormal outputs exist and must be kept
    _compare(_run(m, C.IMX250MYR_POL, bayer, (1.3, 1.0, 0.7), 1.0), ref, bayer)


def test_more_work_than_the_grid_has_threads():
    """2048 workgroups x 256 threads = 524288 lanes; 1028 rows x 513 chunks exceed them."""
    shape = (1028, 2052)
    got = _run(C.frame(shape, "uint8"), C.IMX250MYR_POL, C.RGGB, None, 1.0, ("planes", "color"))
    _compare(got, _ref(shape, "uint8", 1, C.IMX250MYR_POL, C.RGGB, None, 1.0), shape)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_nothing_is_written_outside_the_outputs(dtype):
    """Input and outputs sit inside larger sentinel-filled buffers at 16-byte aligned offsets; afterwards each output region
    holds the reference and every other byte is what it was."""
    from polardepth._lib import lib, check
    scale = 1.0 if dtype == "uint8" else 0.01
    for shape, B in (((4, 4), 1), ((12, 20), 2), ((36, 52), 2)):
        m = C.frame(shape, dtype, seed=3, B=B)
        ref = C.demosaic(m, C.IMX250MYR_POL, C.RGGB, GAINS, scale)
        off, tail = 48, 4096
        src = np.full(off + m.nbytes + tail, 0xA5, np.uint8)
        src[off:off + m.nbytes] = m.view(np.uint8).reshape(-1)
        d_src = _dev(src)
        d_out = [torch.full((off + r.nbytes + tail,), 0x5A, dtype=torch.uint8, device="cuda") for r in ref]
        at = lambda t: ctypes.c_void_p(t.data_ptr() + off)
        check(lib.pd_cdofp_demosaic(at(d_src), C.DTYPES.index(dtype), (ctypes.c_int * 4)(*C.IMX250MYR_POL),
                                    (ctypes.c_int * 4)(*C.RGGB), (ctypes.c_double * 3)(*GAINS), scale, at(d_out[0]), at(d_out[1]),
                                    at(d_out[2]), B, shape[0], shape[1],
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pd_cdofp_demosaic")
        torch.cuda.synchronize()
        assert np.array_equal(d_src.cpu().numpy(), src)
        for d, r in zip(d_out, ref):
            dst = d.cpu().numpy()
            assert (dst[:off] == 0x5A).all() and (dst[off + r.nbytes:] == 0x5A).all(), (shape, dtype)
            assert np.array_equal(dst[off:off + r.nbytes], r.view(np.uint8).reshape(-1)), (shape, dtype)


def test_empty_batch_and_graph_replay():
    """B = 0 gives empty outputs.  Captured into a graph, the call replays on new frame contents and gives the new result:
    layout, Bayer order, gains and scale travel as kernel arguments, nothing is allocated or copied inside the call."""
    from polardepth import cdofp
    out = cdofp.demosaic(torch.zeros((0, 8, 12), dtype=torch.uint8, device="cuda"), want=KEYS)
    assert out["planes"].shape == (0, 4, 8, 12) and out["color"].shape == (0, 3, 8, 12) and out["rgb_planes"].shape == (0, 4, 3, 8, 12)
    shape = (36, 52)
    frames = [C.frame(shape, "uint16", seed=s, B=2) for s in (0, 1)]
    static = _dev(frames[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires
        cdofp.demosaic(static, C.OTHER_LAYOUT, C.GBRG, GAINS, C.SCALE_12BIT, want=KEYS)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cdofp.demosaic(static, C.OTHER_LAYOUT, C.GBRG, GAINS, C.SCALE_12BIT, want=KEYS)
    refs = [dict(zip(KEYS, C.demosaic(f, C.OTHER_LAYOUT, C.GBRG, GAINS, C.SCALE_12BIT))) for f in frames]
    assert not np.array_equal(refs[0]["color"], refs[1]["color"])
    for s in (1, 0):
        static.view(torch.int16).copy_(_dev(frames[s]).view(torch.int16))      # (torch's uint16 has few kernels of its own)
        graph.replay()
        torch.cuda.synchronize()
        _compare({k: v.cpu().numpy() for k, v in out.items()}, refs[s], ("replay", s))


# ------------------------------------------------------------------------------------------- through the pipeline
def test_unpolarised_colour_ramps_have_no_dolp():
    """The physics on the device: three unpolarised colour ramps give four equal planes off the clamped border, so the DoLP
    K1 computes from them is exactly 0 there."""
    from polardepth import cdofp
    from polardepth import polar as pdpolar
    m, ramps = C.ramp_frame((36, 52))
    out = cdofp.demosaic(_dev(m[None]), want=KEYS)
    xolp = pdpolar.polar_forward(out["planes"], want=("xolp",))["xolp"]
    torch.cuda.synchronize()
    inner = (slice(3, 36 - 3), slice(3, 52 - 3))
    assert bool((xolp[0, 0][inner] == 0).all())
    rgb = out["rgb_planes"].cpu().numpy()[0]
    for p in range(4):
        for k in range(3):
            assert np.array_equal(rgb[p, k][inner], ramps[k][inner].astype(np.float32)), (p, k)
    assert np.array_equal(out["color"].cpu().numpy()[0][(slice(None),) + inner], ramps[(slice(None),) + inner].astype(np.uint8))


def _scene_frames(dtype, shape=(128, 192), B=2):
    """the polarised colour scene of cdofp_ref at the sensor's depth, with a different offset per item"""
    m, _ = C.polarised_scene(shape)
    hi = 255.0 if dtype == "uint8" else 4095.0
    frames = np.stack([np.clip(m * (hi / 2048.0) + 3 * b, 0, hi) for b in range(B)])
    return np.rint(frames).astype(dtype)


class _Counting:
    """polardepth._lib.lib with pd_cdofp_demosaic counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def pd_cdofp_demosaic(self, *args):
        self.calls += 1
        return self._lib.pd_cdofp_demosaic(*args)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("order", ["polar_first", "color_first"])
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_hand_over_is_one_launch_whichever_runs_first(dtype, order, monkeypatch):
    """A batch with only ("pol_cdofp", 0, 0) through polar_inputs and expand_batch, in either order: xolp, normals and the eight
    pyramid tensors are those of the batch that carries ("pol", 0, 0) and ("color_raw", 0, 0) from a separate demosaic call,
    and the library is entered once."""
    from polardepth import cdofp
    from polardepth import color as pdcolor
    from polardepth import polar as pdpolar
    opts = cdofp.options(C.OTHER_LAYOUT, "GRBG", (1.2, 1.0, 1.4), None if dtype == "uint8" else C.SCALE_12BIT)
    frames = _dev(_scene_frames(dtype)[:, None])
    jitter = torch.zeros((2, 8), dtype=torch.float64)
    jitter[1] = torch.tensor([1, 1.1, 3, 0.9, 2, 1.15, 4, 0.05], dtype=torch.float64)
    sep = cdofp.demosaic(frames, *opts)
    host = {("pol", 0, 0): sep["planes"], ("color_raw", 0, 0): sep["color"], "color_jitter": jitter.cuda()}
    pdcolor.expand_batch(host, NET_HW, 4)
    n_host = pdpolar.polar_inputs(host, NET_HW, ("xolp", "normals"))
    counting = _Counting(cdofp.lib)
    monkeypatch.setattr(cdofp, "lib", counting)
    dev = {("pol_cdofp", 0, 0): frames, "color_jitter": jitter.cuda()}
    if order == "polar_first":
        n_dev = pdpolar.polar_inputs(dev, NET_HW, ("xolp", "normals"), cdofp=opts)
        pdcolor.expand_batch(dev, NET_HW, 4, cdofp=opts)
    else:
        pdcolor.expand_batch(dev, NET_HW, 4, cdofp=opts)
        n_dev = pdpolar.polar_inputs(dev, NET_HW, ("xolp", "normals"), cdofp=opts)
    cdofp.expand(dev, opts)                                  # idempotent
    torch.cuda.synchronize()
    assert counting.calls == 1
    assert dev[("pol", 0, 0)].dtype == torch.float32 and dev[("pol", 0, 0)].shape == (2, 4, 128, 192)
    assert dev[("color_raw", 0, 0)].dtype == torch.uint8 and dev[("color_raw", 0, 0)].shape == (2, 3, 128, 192)
    assert _same(dev[("xolp", 0, 0)], host[("xolp", 0, 0)]) and _same(n_dev, n_host) and n_dev.shape == (2, 9) + NET_HW
    for s in range(4):
        for key in (("color", 0, s), ("color_aug", 0, s)):
            assert _same(dev[key], host[key]), key
    assert not torch.equal(dev[("color_aug", 0, 0)][1], dev[("color", 0, 0)][1])
    assert bool((dev[("xolp", 0, 0)][:, 0] > 0).any())


def test_trainer_takes_a_colour_sensor_batch(tmp_path, monkeypatch):
    """One Trainer.process_batch on a batch of two 128x192 colour sensor frames (network 64x96, the smallest the tests use):
    the options come from the opt attributes, the library is entered once, and the losses are finite."""
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    from polardepth import cdofp, synthetic
    torch.manual_seed(0)
    opts = _opts(tmp_path / "cdofp", ["--dropout_rate", "0.0"])
    opts.pol_layout, opts.pol_bayer, opts.pol_gains, opts.pol_color_scale = list(C.OTHER_LAYOUT), "BGGR", "1.2,1,1.4", C.SCALE_12BIT
    tr = Trainer(opts)
    assert tr.pol_cdofp == (C.OTHER_LAYOUT, C.BGGR, (1.2, 1.0, 1.4), C.SCALE_12BIT)
    base = synthetic.make_batch(2, NET_HW[0], NET_HW[1], frame_w=NET_HW[1], device="cuda", seed=3)
    drop = {("pol", 0, 0), ("xolp", 0, 0)} | {(k, 0, s) for k in ("color", "color_aug") for s in range(4)}
    batch = {k: v for k, v in base.items() if k not in drop}
    batch[("pol_cdofp", 0, 0)] = _dev(_scene_frames("uint16")[:, None])
    batch["color_jitter"] = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    counting = _Counting(cdofp.lib)
    monkeypatch.setattr(cdofp, "lib", counting)
    tr.set_train()
    tr.model_optimizer.zero_grad()
    outputs, losses, _ = tr.process_batch(batch, is_train=True)
    losses["loss"].backward()
    torch.cuda.synchronize()
    assert counting.calls == 1
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in losses.values())
    sep = cdofp.demosaic(batch[("pol_cdofp", 0, 0)], *tr.pol_cdofp)
    assert _same(batch[("pol", 0, 0)], sep["planes"]) and torch.equal(batch[("color_raw", 0, 0)], sep["color"])
    assert batch[("color", 0, 0)].shape == (2, 3) + NET_HW and batch[("xolp", 0, 0)].shape == (2, 2) + NET_HW
    assert Trainer(_opts(tmp_path / "default", ["--dropout_rate", "0.0"])).pol_cdofp == (C.IMX250MYR_POL, C.RGGB, None, None)
    bad = _opts(tmp_path / "bad", ["--dropout_rate", "0.0"])
    bad.pol_bayer = "RGBG"
    with pytest.raises(ValueError, match="'RGBG'"):
        Trainer(bad)
