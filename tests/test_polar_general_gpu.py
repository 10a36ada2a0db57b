"""General polar kernel (pd_polar_general_fwd: any four polarizer angles, uint8 / uint16 / float32 planes) on the GPU:
against the fp64 restatement of the canonical arithmetic (tests/polar_general_ref.py, itself pinned to the reference by
tests/test_polar_general_cabi.py), against K1's look-up-table path where both apply, and through the façade and the Trainer.

Shapes: the 32x48 fixture frames (B = 2), their 32x44 crop written at pitch 64 (B = 3: pad columns, more than one block of
the 256-thread kernel) and a 5x12 crop (odd height, a single row of quads)."""
import numpy as np
import pytest
import torch

import polar_general_ref as G

pytestmark = pytest.mark.gpu

HALF_PI32 = np.float32(0.5 * np.arctan2(0.0, -1.0))


def _batches(images):
    """[H,W,4] -> the test shapes: (name, planes [B,4,h,w], out_width)"""
    p = G.planes(images)                                              # [4,H,W]
    flips = [p, p[:, ::-1], p[:, :, ::-1]]
    return [("32x48", np.ascontiguousarray(np.stack(flips[:2])), None),
            ("32x44->64", np.ascontiguousarray(np.stack([f[:, :, :44] for f in flips])), 64),
            ("5x12", np.ascontiguousarray(np.stack([f[:, :5, :12] for f in flips[:2]])), None)]


def _run(pol, angles, want, out_width=None, precise=False):
    from polardepth import polar as pdpolar
    out = pdpolar.polar_forward(torch.from_numpy(pol).cuda(), want=want, angles=angles, out_width=out_width, precise=precise)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _within_one_ulp(a, b):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return ((np.abs(a64 - b64) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("slug,dtype", G.CASES)
def test_kernel_matches_the_restatement(slug, dtype):
    """Iun and rho bit for bit (IEEE fp64 sqrt and division, one rounding), phi within one fp32 ulp and bit-equal on at least
    99.9 % of the pixels (the device's fp64 atan2 is not correctly rounded), xolp_std = standardise(own xolp), zero padding."""
    from polardepth import polar as pdpolar
    images, angles, _ = G.case(slug, dtype)
    P = pdpolar.fit_matrix(angles)
    same = total = 0
    for name, pol, ow in _batches(images):
        got = _run(pol, angles, ("iun", "xolp", "xolp_std"), out_width=ow)
        W = pol.shape[3]
        ref = G.restate(np.moveaxis(pol, 1, -1), P)                   # [B,h,w]
        assert got["iun"].shape == (pol.shape[0], 1, pol.shape[2], ow or W) and got["xolp"].shape[1] == 2
        assert _same_bits(got["iun"][:, 0, :, :W], ref["iun"]), name
        assert _same_bits(got["xolp"][:, 0, :, :W], ref["rho"]), name
        phi = got["xolp"][:, 1, :, :W]
        assert _within_one_ulp(phi, ref["phi"]), name
        same += int((_bits(phi) == _bits(ref["phi"])).sum())
        total += phi.size
        assert _same_bits(got["xolp_std"][..., :W], G.standardise(got["xolp"][..., :W])), name
        for k in ("iun", "xolp", "xolp_std"):
            assert not got[k][..., W:].any(), (name, k)
    print(f"{slug}/{dtype}: phi bit-equal on {same}/{total} = {same / total:.5f}")
    assert same >= 0.999 * total


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("slug,dtype", [("std", "uint8"), ("calib", "uint16"), ("sixty", "float32")])
def test_normals_equal_normals_from_xolp(slug, dtype, precise):
    """The fused normals are the ones pd_polar_normals_from_xolp computes from the kernel's own fp32 DoLP / AoLP, bit for
    bit, on both trigonometry paths; the pad columns of a pitched output are zero."""
    from polardepth import polar as pdpolar
    images, angles, _ = G.case(slug, dtype)
    for name, pol, ow in _batches(images):
        W = pol.shape[3]
        out = pdpolar.polar_forward(torch.from_numpy(pol).cuda(), want=("xolp", "normals"), angles=angles, out_width=ow,
                                    precise=precise)
        ref = pdpolar.normals_from_xolp(out["xolp"][..., :W].contiguous(), precise=precise)
        torch.cuda.synchronize()
        assert out["normals"].shape == (pol.shape[0], 9, pol.shape[2], ow or W)
        assert _same_bits(out["normals"][..., :W].cpu().numpy(), ref.cpu().numpy()), name
        assert not out["normals"][..., W:].any() and not out["xolp"][..., W:].any(), name
        # and the xolp written next to the normals is the xolp written alone
        alone = _run(pol, angles, ("xolp",), out_width=ow)
        assert _same_bits(out["xolp"].cpu().numpy(), alone["xolp"]), name


def test_uint8_standard_angles_agree_with_the_lut_kernel():
    """Where both kernels apply they compute the same thing: rho bit-equal, phi within one ulp (K1's table holds the correctly
    rounded value), and the two conventions of the degenerate pixels: x1 = x2 = 0 gives rho = phi = 0; x2 = 0, x1 < 0
    gives phi = +pi/2.  Frames: the fixture's uint8 frames and 256x256 frames holding all 65 536 (I0, I90) pairs against a
    few fixed (I45, I135)."""
    from polardepth import polar as pdpolar
    frames = [G.planes(G.case(s, "uint8")[0]) for s in G.SETS]
    i0, i90 = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    pairs = [(0, 0), (255, 0), (17, 200), (128, 128), (100, 101)]
    full = np.stack([np.stack([i0, np.full_like(i0, a), i90, np.full_like(i0, b)]) for a, b in pairs])
    for pol in (np.stack(frames), full):
        t = torch.from_numpy(np.ascontiguousarray(pol)).cuda()
        k1 = pdpolar.polar_forward(t, want=("xolp",))["xolp"].cpu().numpy()
        gen = pdpolar.polar_forward(t, want=("xolp",), angles=pdpolar.STD_ANGLES)["xolp"].cpu().numpy()
        assert _same_bits(gen[:, 0], k1[:, 0])
        assert _within_one_ulp(gen[:, 1], k1[:, 1])
        d1 = pol[:, 0].astype(np.int32) - pol[:, 2]
        d2 = pol[:, 1].astype(np.int32) - pol[:, 3]
        zero = (d1 == 0) & (d2 == 0)
        for x in (gen, k1):
            assert not _bits(x[:, 0][zero]).any() and not _bits(x[:, 1][zero]).any()
            assert (x[:, 1][(d2 == 0) & (d1 < 0)] == HALF_PI32).all()
    assert zero.sum() >= 2 * 256 and ((d2 == 0) & (d1 < 0)).sum() > 60000          # (the pair frames exercise both)


def test_the_three_dtypes_give_identical_bits():
    from polardepth import polar as pdpolar
    images, _, _ = G.case("std_rot", "uint8")
    angles = G.fixture()["calib__angles"]
    outs = []
    for dt in (np.uint8, np.uint16, np.float32):
        name, pol, ow = _batches(images.astype(dt))[1]
        outs.append(_run(pol, angles, ("iun", "xolp", "xolp_std", "normals"), out_width=ow))
    for other in outs[1:]:
        for k in outs[0]:
            assert _same_bits(outs[0][k], other[k]), k
    # uint8 planes WITH angles take the general kernel, without them K1: "iun" exists only in the former
    with pytest.raises(ValueError, match="iun"):
        pdpolar.polar_forward(torch.from_numpy(_batches(images)[0][1]).cuda(), want=("iun",))


def test_general_kernel_refuses_the_lut_only_options():
    from polardepth import polar as pdpolar
    pol = torch.zeros((1, 4, 4, 4), dtype=torch.uint16, device="cuda")
    for kw in ({"mode": pdpolar.MODE_STOKES}, {"mask": torch.ones((1, 4, 4), dtype=torch.uint8, device="cuda")},
               {"want": ("xolp", "ints")}, {"ieee_rho": True}, {"nt_loads": True}, {"nt_loads": False}):
        with pytest.raises(ValueError, match="general kernel"):
            pdpolar.polar_forward(pol, **kw)
    with pytest.raises(ValueError, match="uint8, uint16 or float32"):
        pdpolar.polar_forward(pol.to(torch.int32), angles=pdpolar.STD_ANGLES)
    with pytest.raises(ValueError, match="rank < 3"):
        pdpolar.polar_forward(pol, angles=np.array([0, 90, 180, 270]) * np.pi / 180)


def test_a_nan_pixel_stays_local():
    """xolp.py:26-30 on a NaN intensity: rho = 0 (nan_to_num), phi = NaN, Iun = NaN -- for that pixel only."""
    images, angles, _ = G.case("calib", "float32")
    pol = _batches(images)[0][1]
    bad = pol.copy()
    bad[1, 2, 7, 13] = np.nan
    a = _run(pol, angles, ("iun", "xolp"))
    b = _run(bad, angles, ("iun", "xolp"))
    assert b["xolp"][1, 0, 7, 13] == 0.0 and np.isnan(b["xolp"][1, 1, 7, 13]) and np.isnan(b["iun"][1, 0, 7, 13])
    for k in a:
        hit = np.zeros(a[k].shape, dtype=bool)
        hit[1, :, 7, 13] = True
        assert np.array_equal(_bits(a[k])[~hit], _bits(b[k])[~hit]), k
        assert np.isfinite(b[k][~hit]).all()


@pytest.mark.parametrize("slug,dtype", [("calib", "uint16"), ("sixty", "float32")])
def test_facade_serves_any_angles(slug, dtype):
    """polarisation.xolp.Iun_and_xolp(images, angles) against the reference's values, at the tolerances of the host-side
    comparison of the canonical form (tests/test_polar_general_cabi.py)."""
    from polarisation.xolp import Iun_and_xolp
    from polardepth import polar as pdpolar
    images, angles, (iun, rho, phi) = G.case(slug, dtype)
    g_iun, g_rho, g_phi = Iun_and_xolp(images.astype(np.float64), angles)
    assert g_iun.dtype == g_rho.dtype == g_phi.dtype == np.float64 and g_iun.shape == g_rho.shape == g_phi.shape == (32, 48)
    assert (np.abs(g_rho - rho) <= 1.2e-7 * np.maximum(1.0, np.abs(rho))).all()
    assert (np.abs(g_iun - iun) <= np.spacing(np.abs(iun).astype(np.float32)).astype(np.float64)).all()
    keep = G.restate(images, pdpolar.fit_matrix(angles))["r"] > 1e-9 * np.abs(images.astype(np.float64)).max()
    assert 1.0 - keep.mean() <= 0.01
    d = np.abs(g_phi - phi) % np.pi
    assert (np.minimum(d, np.pi - d)[keep] <= 2.4e-7).all()
    # a frame whose pixel count is no multiple of 4 (the façade pads the flattened planes)
    o_iun, o_rho, o_phi = Iun_and_xolp(images[:5, :3].astype(np.float64), angles)
    assert np.array_equal(o_iun, g_iun[:5, :3]) and np.array_equal(o_rho, g_rho[:5, :3]) and np.array_equal(o_phi, g_phi[:5, :3])


CALIB_DEG = [0.8, 44.1, 91.3, 134.6]


def _u16_batch(seed):
    """synthetic batch whose planes are 12-bit: the uint8 planes scaled by 16 plus a 4-bit pattern"""
    from polardepth import synthetic
    b = synthetic.make_batch(2, 64, 96, frame_w=92, device="cuda", seed=seed)
    p8 = b[("pol", 0, 0)].cpu().numpy()
    low = (np.arange(p8.size, dtype=np.uint32).reshape(p8.shape) * 7) % 16
    b16 = dict(b)
    b16[("pol", 0, 0)] = torch.from_numpy((p8.astype(np.uint32) * 16 + low).astype(np.uint16)).cuda()
    return b, b16


def _trainer(tmp_path, tag, pol_angles):
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    torch.manual_seed(0)
    opts = _opts(tmp_path / tag, ["--dropout_rate", "0.0"])
    opts.pol_angles = pol_angles
    return Trainer(opts)


def test_trainer_takes_uint16_planes_and_calibrated_angles(tmp_path):
    from polardepth import polar as pdpolar
    b8, b16 = _u16_batch(4)
    rad = np.array(CALIB_DEG) * np.pi / 180
    tr = _trainer(tmp_path, "calib", CALIB_DEG)
    tr.set_train()
    inputs = dict(b16)
    _, losses, _ = tr.process_batch(inputs, is_train=True)
    direct = pdpolar.polar_forward(b16[("pol", 0, 0)], want=("xolp",), angles=rad)["xolp"]
    torch.cuda.synchronize()
    assert torch.equal(inputs[("xolp", 0, 0)].view(torch.int32), direct.view(torch.int32))
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in losses.values())
    # a 16-bit frame of another height cannot take the uint8-only device resize
    short = dict(b16)
    short[("pol", 0, 0)] = b16[("pol", 0, 0)][:, :, :32].contiguous()
    with pytest.raises(ValueError, match="uint8"):
        tr.process_batch(short, is_train=True)
    # default options, uint8 planes: the call that was there before
    tr0 = _trainer(tmp_path, "default", None)
    tr0.set_train()
    assert tr0.pol_angles is None
    inputs = dict(b8)
    tr0.process_batch(inputs, is_train=True)
    k1 = pdpolar.polar_forward(b8[("pol", 0, 0)], want=("xolp",))["xolp"]
    torch.cuda.synchronize()
    assert torch.equal(inputs[("xolp", 0, 0)].view(torch.int32), k1.view(torch.int32))
    with pytest.raises(ValueError, match="rank < 3"):
        _trainer(tmp_path, "bad", [0, 90, 180, 270])


def test_graphed_step_replays_the_general_kernel(tmp_path):
    """One eager step and one replay of the captured step on the same uint16 batch give the same loss: the 12 fit
    coefficients travel as kernel arguments, nothing is allocated or copied inside the call."""
    from polardepth import functional as PF
    from polardepth.graph import GraphedTrainStep
    _, b16 = _u16_batch(5)
    PF.DropoutState.manual_seed(3)
    tr_e = _trainer(tmp_path, "eager", CALIB_DEG)
    tr_e.set_train()
    tr_e.model_optimizer.zero_grad()
    _, L, _ = tr_e.process_batch(dict(b16), is_train=True)
    L["loss"].backward()
    tr_e.model_optimizer.step()
    loss_e = L["loss"].detach().clone()
    PF.DropoutState.manual_seed(3)
    tr_g = _trainer(tmp_path, "graph", CALIB_DEG)
    tr_g.set_train()
    gs = GraphedTrainStep(tr_g, b16, warmup=1, restore_state=True)
    loss_g = gs.step(b16).detach().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(loss_e) and torch.equal(loss_e, loss_g), (loss_e.item(), loss_g.item())
    assert torch.equal(tr_e.store.flat, tr_g.store.flat)
