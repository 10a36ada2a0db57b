"""Device LANCZOS resize of uint16 / float32 planes (pd_resize_wide_pass) against PIL's ``Image.resize(..., Image.LANCZOS)``
in mode I;16 / F, bit for bit, on the cases of tests/resize_wide_ref.py (tests/test_resize_wide.py pins the NumPy
restatement on the same PIL results); then the chain raw planes -> device resize -> K1 against PIL resize -> K1, from a
uint16 mosaic too, and through Trainer._polar_inputs and Evaluation.predict.

Shapes: the planes are [2,4,Hs,Ws] (8 planes: plane strides), odd widths, down- and upscaling, each pass skipped once; the
full-range cases overshoot 65535 and undershoot 0 (asserted in tests/test_resize_wide.py), so the bytewise store is under
test.  The chain runs 208x272 -> 64x96: more than one block of the 256-thread kernels in both passes."""
import numpy as np
import pytest
import torch

import resize_wide_ref as R

pytestmark = pytest.mark.gpu

RAW_HW, NET_HW = (208, 272), (64, 96)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("case", R.CASES)
def test_resize_matches_pillow_bit_exactly(case, dtype):
    from polardepth import resize as pdresize
    p = R.planes(case, dtype)
    got = pdresize.resize_lanczos(torch.from_numpy(p.copy()).cuda(), case[2:4])
    torch.cuda.synchronize()
    assert got.dtype == getattr(torch, dtype) and got.shape == (2, 4) + case[2:4]
    got = got.cpu().numpy()
    ref = R.pil_planes(case, dtype)
    for b in range(2):
        for c in range(4):
            np.testing.assert_array_equal(R.bits(got[b, c]), R.bits(ref[b, c]), err_msg=f"plane {b},{c}")


def test_uint8_takes_the_8_bit_kernels_and_other_dtypes_are_refused():
    from polardepth import resize as pdresize
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.integers(0, 256, (2, 4, 37, 53), dtype=np.uint8)).cuda()
    assert torch.equal(pdresize.resize_lanczos(x, (16, 20)), pdresize.resize_lanczos_u8(x, (16, 20)))
    for dt in (torch.int16, torch.int32, torch.float16, torch.float64):
        with pytest.raises(ValueError, match="uint8, uint16 and float32"):
            pdresize.resize_lanczos(torch.zeros((4, 8, 8), dtype=dt, device="cuda"), (4, 4))
    # same size: no pass runs, the planes come back as they are
    y = torch.from_numpy(R.planes(R.CASES[0], "uint16").copy()).cuda()
    assert torch.equal(pdresize.resize_lanczos(y, y.shape[-2:]).view(torch.int16), y.view(torch.int16))


def _raw(dtype, B=1, seed=11):
    """raw frames [B,4,208,272]: 12-bit counts, or floats with fractional parts in the same range"""
    rng = np.random.default_rng(seed)
    if dtype == "uint16":
        return rng.integers(0, 4096, (B, 4) + RAW_HW).astype(np.uint16)
    return rng.uniform(0.0, 4095.0, (B, 4) + RAW_HW).astype(np.float32)


def _pil(raw):
    return np.stack([np.stack([R.pil_resize(pl, NET_HW) for pl in item]) for item in raw])


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("angles_deg", [None, [0.8, 44.1, 91.3, 134.6]])
def test_resize_then_k1_equals_host_resize_then_k1(angles_deg):
    """The loader's two hand-overs agree: raw uint16 planes -> device resize -> K1 equals PIL I;16 resize -> K1; the raw
    planes may also arrive as one uint16 mosaic (split_mosaic on the device)."""
    from polardepth import polar as pdpolar
    from polardepth import resize as pdresize
    raw = _raw("uint16")
    kw = {} if angles_deg is None else {"angles": pdpolar.angles_from_degrees(angles_deg)}
    b = pdpolar.polar_forward(torch.from_numpy(_pil(raw)).cuda(), want=("xolp", "normals"), **kw)
    dev = pdresize.resize_lanczos(torch.from_numpy(raw).cuda(), NET_HW)
    a = pdpolar.polar_forward(dev, want=("xolp", "normals"), **kw)
    assert torch.equal(a["xolp"], b["xolp"]) and torch.equal(a["normals"], b["normals"])
    h, w = RAW_HW
    mosaic = np.zeros((1, 2 * h, 2 * w), np.uint16)
    mosaic[:, :h, :w], mosaic[:, :h, w:], mosaic[:, h:, :w], mosaic[:, h:, w:] = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3]
    planes = pdpolar.split_mosaic(torch.from_numpy(mosaic).cuda())
    assert planes.dtype == torch.uint16 and planes.is_contiguous()
    np.testing.assert_array_equal(planes.cpu().numpy(), raw)
    c = pdpolar.polar_forward(pdresize.resize_lanczos(planes, NET_HW), want=("xolp", "normals"), **kw)
    assert torch.equal(c["xolp"], b["xolp"]) and torch.equal(c["normals"], b["normals"])


def test_trainer_resizes_uint16_and_float32_planes_on_the_device(tmp_path):
    """Trainer._polar_inputs with raw 208x272 planes and opt.height, width = 64, 96 gives the ("xolp", 0, 0) and normals it
    gives with the PIL-resized planes; a uint16 mosaic is split first."""
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    torch.manual_seed(0)
    tr = Trainer(_opts(tmp_path, ["--dropout_rate", "0.0"]))
    assert (tr.opt.height, tr.opt.width) == NET_HW
    for dtype in R.DTYPES:
        raw = _raw(dtype, B=2)
        host = {("pol", 0, 0): torch.from_numpy(_pil(raw)).cuda()}
        dev = {("pol", 0, 0): torch.from_numpy(raw).cuda()}
        n_host, n_dev = tr._polar_inputs(host), tr._polar_inputs(dev)
        torch.cuda.synchronize()
        assert dev[("xolp", 0, 0)].shape == (2, 2) + NET_HW and n_dev.shape == (2, 9) + NET_HW
        assert _same(dev[("xolp", 0, 0)], host[("xolp", 0, 0)]) and _same(n_dev, n_host), dtype
    h, w = RAW_HW
    raw = _raw("uint16", B=2)
    mosaic = np.concatenate([np.concatenate([raw[:, 0], raw[:, 1]], axis=2), np.concatenate([raw[:, 2], raw[:, 3]], axis=2)], axis=1)
    mos = {("pol_mosaic", 0, 0): torch.from_numpy(mosaic).cuda()}
    host = {("pol", 0, 0): torch.from_numpy(_pil(raw)).cuda()}
    n_host, n_mos = tr._polar_inputs(host), tr._polar_inputs(mos)
    assert mos[("pol", 0, 0)].shape == (2, 4, h, w)
    assert _same(mos[("xolp", 0, 0)], host[("xolp", 0, 0)]) and _same(n_mos, n_host)
    with pytest.raises(ValueError, match="uint8, uint16 or float32"):
        tr._polar_inputs({("pol", 0, 0): torch.zeros((2, 4) + RAW_HW, dtype=torch.int32, device="cuda")})
    # 16-bit / float planes shorter than the network input are a loader / options mismatch, not something to enlarge
    for dt in (torch.uint16, torch.float32):
        with pytest.raises(ValueError, match="fewer rows"):
            tr._polar_inputs({("pol", 0, 0): torch.zeros((2, 4, 32, 96), dtype=dt, device="cuda")})


def test_evaluation_takes_the_trainers_hand_over():
    """Evaluation.predict on one batch: raw uint16 planes (and a uint16 mosaic) give the depth the PIL-resized planes give."""
    from manydepth.evaluation import Evaluation
    from polardepth import synthetic
    torch.manual_seed(0)
    ev = Evaluation(data_path="synthetic", height=NET_HW[0], width=NET_HW[1], batch_size=2)
    base = synthetic.make_batch(2, NET_HW[0], NET_HW[1], frame_w=NET_HW[1], device="cuda", seed=3)
    raw = _raw("uint16", B=2)
    mosaic = np.concatenate([np.concatenate([raw[:, 0], raw[:, 1]], axis=2), np.concatenate([raw[:, 2], raw[:, 3]], axis=2)], axis=1)
    outs = []
    for key, planes in ((("pol", 0, 0), _pil(raw)), (("pol", 0, 0), raw), (("pol_mosaic", 0, 0), mosaic)):
        inputs = {k: v for k, v in base.items() if k not in (("pol", 0, 0), ("xolp", 0, 0))}
        inputs[key] = torch.from_numpy(planes).cuda()
        depth = ev.predict(inputs)
        torch.cuda.synchronize()
        assert depth.shape == (2, 1) + NET_HW and bool(torch.isfinite(depth).all())
        outs.append((depth, inputs[("xolp", 0, 0)]))
    for depth, xolp in outs[1:]:
        assert _same(xolp, outs[0][1]) and _same(depth, outs[0][0])
