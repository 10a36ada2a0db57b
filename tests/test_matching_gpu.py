"""pd_cost_volume (csrc/matching.hip) on the device: bit for bit against tests/matching_ref.py -- the order of every sum is
stated in include/polardepth.h, so nothing is excluded -- and against the reference's float64 run (g13_matching.npz) under the
exclusions and the bound of tests/test_matching_ref.py; determinism, graph capture, and the Python layer's shapes."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import matching_ref as MR
from polardepth import matching, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("cost", "missing", "confidence", "argmin", "lowest")


@pytest.fixture(scope="module")
def g13():
    return dict(np.load(os.path.join(GOLDEN, "g13_matching.npz")))


def make_case(seed, B, F, C, h, w, D, lo=0.3, hi=2.0, binning="linear", shift=0.08):
    """Random non-negative features, a K per item, small poses whose parallax sends some bins past the borders."""
    rng = np.random.default_rng(seed)
    K = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    for n in range(B):
        K[n, 0, 0], K[n, 1, 1] = (0.62 + 0.05 * n) * w, (1.05 - 0.07 * n) * h
        K[n, 0, 2], K[n, 1, 2] = w / 2 - 0.4 + 0.3 * n, h / 2 + 0.3 - 0.2 * n
    T = np.tile(np.eye(4, dtype=np.float32), (B, max(F, 1), 1, 1))[:, :F]
    if F:
        T[:, :, :3, 3] = rng.uniform(-shift, shift, (B, F, 3))
        T[:, :, 0, 1] = rng.uniform(-0.02, 0.02, (B, F))
    return {"cur": rng.random((B, C, h, w), dtype=np.float32), "lookup": rng.random((B, F, C, h, w), dtype=np.float32),
            "poses": T, "K": K, "inv_K": np.linalg.pinv(K).astype(np.float32),
            "bins": matching.depth_bins(lo, hi, D, binning).numpy()}


def device_run(c, valid=None, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cur = t(c["cur"]).contiguous(memory_format=torch.channels_last)
    out = ops.cost_volume(cur, t(c["lookup"]), t(c["poses"]), t(c["K"]), t(c["inv_K"]), t(c["bins"]),
                          valid=None if valid is None else t(np.asarray(valid, np.float32)), want_missing=True, **kw)
    torch.cuda.synchronize()
    cost, conf, arg, low, miss = out
    assert cost.shape == (c["cur"].shape[0], len(c["bins"]), *c["cur"].shape[2:]) and cost.stride(1) == 1
    assert conf.dtype == torch.float32 and arg.dtype == torch.int32 and low.dtype == torch.float32 and miss.dtype == torch.uint8
    return {"cost": cost.cpu().numpy(), "missing": miss.cpu().numpy(), "confidence": conf.cpu().numpy(),
            "argmin": arg.cpu().numpy(), "lowest": low.cpu().numpy()}


def ref_run(c, valid=None, apply_confidence=False):
    return MR.cost_volume(c["cur"], c["lookup"], c["poses"], c["K"], c["inv_K"], c["bins"], MR.frame_valid(c["poses"], valid),
                          apply_confidence=apply_confidence)


def assert_bit_equal(got, want, where=None):
    for k in KEYS:
        g, w_ = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w_.shape and g.dtype == w_.dtype, (k, g.shape, w_.shape, g.dtype, w_.dtype)
        if where is not None:
            g, w_ = g[where], w_[where]
        # the same bits; a NaN matches a NaN (its sign and payload are the adder's business)
        same = (g == w_) | ((g != g) & (w_ != w_))
        if g.dtype == np.float32:
            same &= (g.view(np.uint32) == w_.view(np.uint32)) | (g != g)
        assert same.all(), (k, int((~same).sum()), np.argwhere(~same)[:5])


def fixture_case(g13, binning):
    return {"cur": g13["cur"], "lookup": g13["lookup"], "poses": g13["poses"], "K": g13["K"], "inv_K": g13["inv_K"],
            "bins": g13[f"bins_{binning}"]}


@pytest.mark.parametrize("binning", ("linear", "inverse"))
def test_fixture_inputs_bit_equal_and_against_the_reference(g13, binning):
    c = fixture_case(g13, binning)
    got, want = device_run(c), ref_run(c)
    assert_bit_equal(got, want)
    assert 0.2 < want["confidence"][:, 2:-2, 2:-2].mean() < 0.9 and want["missing"].any() and not want["missing"].all()
    # the reference's own float64 run, under tests/test_matching_ref.py's exclusions and bound
    near = g13["near"]
    keep = ~(near | g13[f"tie_{binning}"])
    n4 = np.broadcast_to(~near[:, None], got["cost"].shape)
    assert np.array_equal(got["missing"][n4], g13[f"missing_{binning}"][n4])
    assert np.array_equal(got["confidence"][~near], g13[f"confidence_{binning}"][~near].astype(np.float32))
    assert np.array_equal(got["argmin"][keep], g13[f"argmin_{binning}"][keep])
    dev = np.abs(got["cost"].astype(np.float64) - g13[f"cost_{binning}"])[n4].max()
    print("cost deviation", dev, "bound", 2 * float(g13["dev_cost_max"]))
    assert dev <= 2 * float(g13["dev_cost_max"])
    assert np.allclose(got["lowest"][keep], g13[f"lowest_{binning}"][keep], rtol=1e-6, atol=0)


@pytest.mark.parametrize("B,F,C,h,w,D", [(2, 1, 16, 19, 37, 7),       # odd sizes, a quarter of a row's lanes, D % 4 != 0
                                         (2, 2, 8, 5, 7, 5),          # the interior is 1 x 3
                                         (2, 2, 64, 12, 20, 1),       # one bin
                                         (2, 2, 64, 12, 20, 96),      # the production bin count
                                         (1, 3, 132, 9, 11, 128),     # three channel chunks, the last one partial; most bins
                                         (3, 8, 4, 6, 9, 33)])        # most frames, fewest channels
def test_shapes_bit_equal(B, F, C, h, w, D):
    c = make_case(B * 1000 + D, B, F, C, h, w, D)
    want = ref_run(c)
    assert_bit_equal(device_run(c), want)
    if h * w > 100 and D > 1:
        assert want["missing"].any() and (want["nframes"] > 0).any() and (want["argmin"] > 0).any()


def test_empty_interior_no_frames_and_all_invalid():
    c = make_case(1, 2, 2, 16, 4, 4, 6)                                # 4 x 4: no interior pixel
    got = device_run(c)
    assert_bit_equal(got, ref_run(c))
    assert not got["cost"].any() and got["missing"].all() and not got["confidence"].any() and not got["argmin"].any()
    c = make_case(2, 2, 0, 16, 8, 9, 6)                                # F = 0
    got = device_run(c)
    assert_bit_equal(got, ref_run(c))
    assert not got["cost"].any() and np.array_equal(got["lowest"], np.full((2, 8, 9), np.float32(1) / c["bins"][0]))
    c = make_case(3, 2, 2, 16, 8, 9, 6)                                # every frame invalid: by the flag, by a zero pose
    got = device_run(c, valid=np.zeros((2, 2)))
    assert_bit_equal(got, ref_run(c, np.zeros((2, 2))))
    assert not got["cost"].any() and got["missing"].all() and not got["argmin"].any()
    c["poses"][:] = 0
    assert_bit_equal(device_run(c), got)


def test_valid_mixed_per_item():
    c = make_case(4, 3, 3, 16, 10, 13, 9)
    valid = np.array([[1, 0, 1], [0, 0, 0], [0, 1, 1]], np.float32)
    c["poses"][2, 2] = 0                                               # the missing-frame rule on top of the flags
    got, want = device_run(c, valid), ref_run(c, valid)
    assert_bit_equal(got, want)
    assert want["nframes"][0].max() == 2 and want["nframes"][1].max() == 0 and want["nframes"][2].max() == 1
    assert not np.array_equal(got["cost"], device_run(c)["cost"])


@pytest.mark.parametrize("apply_confidence", (False, True))
def test_wider_buffer_and_apply_confidence(g13, apply_confidence):
    c = fixture_case(g13, "linear")
    B, C, h, w = c["cur"].shape
    D = len(c["bins"])
    rng = np.random.default_rng(5)
    buf = torch.from_numpy(rng.random((B, h, w, C + D + 3), dtype=np.float32)).to(DEV).permute(0, 3, 1, 2)   # NHWC storage
    before = buf.clone()
    got = device_run(c, out=buf[:, C:C + D], apply_confidence=apply_confidence)
    want = ref_run(c, apply_confidence=apply_confidence)
    assert_bit_equal(got, want)
    assert torch.equal(buf[:, :C], before[:, :C]) and torch.equal(buf[:, C + D:], before[:, C + D:])
    assert np.array_equal(buf[:, C:C + D].cpu().numpy(), want["cost"])
    plain = ref_run(c)
    conf = want["confidence"][:, None] > 0
    if apply_confidence:
        assert not want["cost"][np.broadcast_to(~conf, want["cost"].shape)].any() and (plain["cost"] * conf == want["cost"]).all()
    else:
        assert want["cost"][np.broadcast_to(~conf, want["cost"].shape)].any()


def test_nan_pose_and_nan_feature_stay_in_their_item():
    c = make_case(6, 2, 2, 16, 10, 13, 9)
    clean = device_run(c)
    d = {k: v.copy() for k, v in c.items()}
    d["poses"][0, 0, 0, 3] = np.nan                                    # every coordinate of frame 0 is NaN: masked
    d["lookup"][0, 1, 3, 5, 6] = np.nan                                # one NaN feature in frame 1
    d["cur"][0, 2, 4, 4] = np.nan
    got, want = device_run(d), ref_run(d)
    assert_bit_equal(got, want)
    assert np.isnan(want["cost"][0]).any() and not np.isnan(want["cost"][0]).all()
    for k in KEYS:
        assert np.array_equal(got[k][1], clean[k][1]), k


def test_static_camera_identical_frames():
    c = make_case(7, 2, 2, 16, 10, 13, 9)
    c["lookup"][:] = c["cur"][:, None]
    c["poses"][:] = np.eye(4, dtype=np.float32)
    got, want = device_run(c), ref_run(c)
    assert_bit_equal(got, want)
    # the warp is the identity up to the 1e-7 of the division and the rounding of the coordinates: costs of almost nothing
    assert want["cost"].max() < 1e-4


def test_deterministic_and_capturable(g13):
    c = fixture_case(g13, "linear")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cur, look = t(c["cur"]).contiguous(memory_format=torch.channels_last), t(c["lookup"])
    poses, K, iK, bins = t(c["poses"]), t(c["K"]), t(c["inv_K"]), t(c["bins"])
    a = ops.cost_volume(cur, look, poses, K, iK, bins, want_missing=True)
    b = ops.cost_volume(cur, look, poses, K, iK, bins, want_missing=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.cost_volume(cur, look, poses, K, iK, bins, want_missing=True)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.cost_volume(cur, look, poses, K, iK, bins, want_missing=True)
    bins.copy_(t(g13["bins_inverse"]))                                             # new bins, in place, after the capture
    graph.replay()
    torch.cuda.synchronize()
    want = ref_run(fixture_case(g13, "inverse"))
    got = {"cost": out[0], "confidence": out[1], "argmin": out[2], "lowest": out[3], "missing": out[4]}
    assert_bit_equal({k: v.cpu().numpy() for k, v in got.items()}, want)
    assert not np.array_equal(want["cost"], a[0].cpu().numpy())


def test_match_features_and_confidence_mask_shapes(g13):
    c = fixture_case(g13, "linear")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    bins = t(c["bins"])
    cost, missing = matching.match_features(t(c["cur"]), t(c["lookup"]), t(c["poses"]), t(c["K"]), t(c["inv_K"]), bins)
    assert cost.shape == missing.shape == (2, 16, 24, 40) and cost.dtype == missing.dtype == torch.float32
    want = ref_run(c)
    assert np.array_equal(cost.cpu().numpy(), want["cost"]) and np.array_equal(missing.cpu().numpy(), want["missing"])
    conf = matching.compute_confidence_mask(cost * (1 - missing))                  # resnet_encoder.py:620-621
    assert conf.shape == (2, 24, 40) and conf.dtype == torch.float32
    assert np.array_equal(conf.cpu().numpy(), want["confidence"])
    disp = matching.indices_to_disparity(t(want["argmin"]), bins)
    assert disp.shape == (2, 24, 40) and np.array_equal(disp.cpu().numpy(), want["lowest"])
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.cost_volume(t(c["cur"])[:, :6], t(c["lookup"])[:, :, :6], t(c["poses"]), t(c["K"]), t(c["inv_K"]), bins)
    with pytest.raises(ValueError, match="channel s"):
        ops.cost_volume(t(c["cur"]), t(c["lookup"]), t(c["poses"]), t(c["K"]), t(c["inv_K"]), bins,
                        out=torch.empty(2, 16, 24, 40, device=DEV))


# ------------------------------------------------------------------ ResnetEncoderMatching
FWD_TOL, GRAD_TOL = 2e-5, 5e-4          # tests/test_modules_gpu.py's, for the existing encoders
WANTED = ("reduce_conv.0.weight", "reduce_conv.0.bias", "layer0.0.weight")
# features[-1].sum() passes 17 ReLUs, the last ones over 2 x 3 pixels, with batch statistics of 12 samples behind them: one
# unit within rounding distance of its kink moves these gradients by 0.06 % to 12 % in ANY float32 evaluation -- PyTorch's own
# float32 CPU run of the restatement below does so for four of the image seeds 13..21.  The images are drawn from a seed for
# which that run stays within GRAD_TOL / 16 of the float64 run (which run crosses a kink depends on the arithmetic of the
# machine, so this is a choice of the case, not an assertion of the test).
ENCODER_SEED = 16


def _close(a, b, tol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).double()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _restate(sd, img, lookups, poses, K, invK, bins, training):
    """ResnetEncoderMatching.forward (resnet_encoder.py:562-707) with the module's own weights in fp64 on the CPU: F.conv2d,
    F.batch_norm, F.max_pool2d and matching_ref for the plane sweep.  ``sd``: fp64 tensors, the weights requiring grad."""
    import torch.nn.functional as F

    def bn(x, p):
        return F.batch_norm(x, None if training else sd[p + ".running_mean"], None if training else sd[p + ".running_var"],
                            sd[p + ".weight"], sd[p + ".bias"], training, 0.1, 1e-5)

    def block(x, p, stride):
        y = F.relu(bn(F.conv2d(x, sd[p + ".conv1.weight"], None, stride, 1), p + ".bn1"))
        y = bn(F.conv2d(y, sd[p + ".conv2.weight"], None, 1, 1), p + ".bn2")
        if p + ".downsample.0.weight" in sd:
            x = bn(F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride), p + ".downsample.1")
        return F.relu(y + x)

    def extract(image):
        f0 = F.relu(bn(F.conv2d((image - 0.45) / 0.225, sd["layer0.0.weight"], None, 2, 3), "layer0.1"))
        x = F.max_pool2d(f0, 3, 2, 1)
        return f0, block(block(x, "layer1.1.0", 1), "layer1.1.1", 1)

    f0, f1 = extract(img)
    with torch.no_grad():
        B, Fr = lookups.shape[:2]
        lf = extract(lookups.reshape(B * Fr, *lookups.shape[2:]))[1]
        lf = lf.reshape(B, Fr, *lf.shape[1:])
        r = MR.cost_volume(f1.detach().numpy(), lf.numpy(), poses, K, invK, bins, MR.frame_valid(poses), apply_confidence=True,
                           dtype=np.float64)
    x = torch.cat([f1, torch.from_numpy(r["cost"]).to(f1.dtype)], 1)
    x = F.relu(F.conv2d(x, sd["reduce_conv.0.weight"], sd["reduce_conv.0.bias"], 1, 1))
    feats = [f0, f1]
    for i in (2, 3, 4):
        x = block(block(x, f"layer{i}.0", 2), f"layer{i}.1", 1)
        feats.append(x)
    return feats, r


def _encoder_case(seed=ENCODER_SEED):
    import sys
    sys.path.insert(0, GOLDEN)
    from synth_weights import fill_state_dict
    from manydepth import networks
    B, Fr, H, W, D = 2, 2, 64, 96, 16
    mod = networks.ResnetEncoderMatching(18, False, H, W, 0.3, 2.0, D)
    fill_state_dict(mod, 0, prefix="matching_encoder.")
    g = torch.Generator().manual_seed(seed)
    img, lookups = torch.rand(B, 3, H, W, generator=g), torch.rand(B, Fr, 3, H, W, generator=g)
    geo = make_case(13, B, Fr, 4, H // 4, W // 4, D)
    geo["poses"][1, 1] = 0                                             # a missing frame
    return mod, img, lookups, geo


@pytest.mark.parametrize("mode", ("eval", "train"))
def test_resnet_encoder_matching_against_fp64_restatement(mode):
    mod, img, lookups, geo = _encoder_case()
    assert mod.matching_height == 16 and mod.matching_width == 24 and mod.num_ch_enc.tolist() == [64, 64, 128, 256, 512]
    sd = {k: v.detach().double().clone() for k, v in mod.state_dict().items()}
    wanted = WANTED
    for k in wanted:
        sd[k].requires_grad_(True)
    training = mode == "train"
    bins = mod.depth_bins.numpy().copy()
    want, r = _restate(sd, img.double(), lookups.double(), geo["poses"], geo["K"], geo["inv_K"], bins, training)
    mod.cuda()
    getattr(mod, mode)()
    t = lambda a: torch.from_numpy(a).to(DEV)
    look_dev, poses_dev = lookups.to(DEV).requires_grad_(training), t(geo["poses"]).requires_grad_(training)
    got, lowest, conf = mod(img.to(DEV), look_dev, poses_dev, t(geo["K"]), t(geo["inv_K"]))
    assert len(got) == 5 and lowest.shape == conf.shape == (2, 16, 24) and lowest.dtype == conf.dtype == torch.float32
    for i in range(5):
        assert got[i].shape == want[i].shape
        _close(got[i], want[i].detach(), FWD_TOL, f"features[{i}] {mode}")
    # the discrete maps, where the fp64 cost is not within 1e-5 of a tie or of 0
    c = np.moveaxis(r["c"], 1, -1)
    filled = np.where(c == 0, c.max(-1, keepdims=True), c)
    two = np.sort(np.where(filled == 0, 100.0, filled), -1)[..., :2]
    unsure = ((two[..., 1] - two[..., 0]) < 1e-5) | ((c > 0) & (c < 1e-5)).any(-1)
    inner = np.zeros(unsure.shape, bool)
    inner[:, 2:-2, 2:-2] = True
    assert (~unsure & inner).mean() > 0.5 * inner.mean() and 0 < r["confidence"].mean() < 1
    assert np.array_equal(conf.cpu().numpy()[~unsure], r["confidence"][~unsure].astype(np.float32))
    assert np.array_equal(lowest.cpu().numpy()[~unsure], r["lowest"][~unsure].astype(np.float32))
    border = ~inner
    assert not conf.cpu().numpy()[border].any() and (lowest.cpu().numpy()[border] == np.float32(1) / bins[0]).all()
    if not training:
        return
    want[-1].sum().backward()
    mod.zero_grad()
    got[-1].sum().backward()
    torch.cuda.synchronize()
    named = dict(mod.named_parameters())
    for k in wanted:
        _close(named[k].grad, sd[k].grad, GRAD_TOL, "grad " + k)
    # the cost-volume channels carry no gradient back: nothing reaches the lookup frames or the poses
    assert look_dev.grad is None and poses_dev.grad is None
    assert named["prematching_conv.0.weight"].grad is None                       # constructed, never run


def test_resnet_encoder_matching_state_dict_and_adaptive_bins():
    mod, img, lookups, geo = _encoder_case()
    keys = list(mod.state_dict().keys())
    for k in ("layer0.0.weight", "layer0.1.running_var", "layer1.1.0.conv1.weight", "layer1.1.1.bn2.num_batches_tracked",
              "layer2.0.downsample.0.weight", "layer3.0.downsample.1.bias", "layer4.1.conv2.weight",
              "prematching_conv.0.bias", "reduce_conv.0.weight", "reduce_conv.0.bias"):
        assert k in keys, k
    assert len(keys) == 124 and not any(k.startswith(("depth_bins", "backprojector", "projector")) for k in keys)
    assert tuple(mod.state_dict()["reduce_conv.0.weight"].shape) == (64, 80, 3, 3)
    # a torchvision-named resnet18 state_dict goes in and comes back out
    tv = {}
    for k, v in mod.state_dict().items():
        if k.startswith("layer0.0."):
            tv["conv1." + k[9:]] = torch.full_like(v, 0.25)
        elif k.startswith("layer0.1."):
            tv["bn1." + k[9:]] = torch.full_like(v, 2)
        elif k.startswith("layer1.1."):
            tv["layer1." + k[9:]] = torch.full_like(v, 3)
        elif k.startswith(("layer2.", "layer3.", "layer4.")):
            tv[k] = torch.full_like(v, 4)
    tv["fc.weight"], tv["fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)
    mod.load_torchvision_state_dict(tv)
    sd = mod.state_dict()
    assert (sd["layer0.0.weight"] == 0.25).all() and (sd["layer0.1.running_mean"] == 2).all()
    assert (sd["layer1.1.1.conv2.weight"] == 3).all() and (sd["layer4.0.downsample.0.weight"] == 4).all()
    # a checkpoint of the reference also holds the index grids of its backprojector: dropped on loading
    ck = dict(sd)
    ck["backprojector.pix_coords"] = torch.zeros(16, 3, 384)
    other, _, _, _ = _encoder_case()
    other.load_state_dict(ck)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))
    # adaptive bins: recomputed on every call, in place
    from manydepth import networks
    ad = networks.ResnetEncoderMatching(18, False, 64, 96, 0.3, 2.0, 16, adaptive_bins=True, depth_binning="inverse").cuda().eval()
    ptr0 = ad.depth_bins.data_ptr()
    t = lambda a: torch.from_numpy(a).to(DEV)
    with torch.no_grad():
        _, low, _ = ad(img.to(DEV), lookups.to(DEV), t(geo["poses"]), t(geo["K"]), t(geo["inv_K"]), 0.5, 3.0)
    assert ad.depth_bins.data_ptr() == ptr0
    assert torch.equal(ad.depth_bins.cpu(), matching.depth_bins(0.5, 3.0, 16, "inverse"))
    assert (low[:, 0, 0].cpu() == 1 / matching.depth_bins(0.5, 3.0, 16, "inverse")[0]).all()
