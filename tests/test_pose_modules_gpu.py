"""networks.ResnetEncoder (two stacked input images) and networks.PoseDecoder: forward, and backward to every parameter that
runs, against a float64 CPU restatement built from F.conv2d / F.batch_norm with the modules' own weights; the state-dict
names; the ``pretrained`` halving of conv1.  Tolerances: those tests/test_matching_gpu.py uses for ResnetEncoderMatching."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

import pose_ref as P

FWD_TOL, GRAD_TOL = 2e-5, 5e-4          # tests/test_matching_gpu.py's
# The loss passes 17 ReLUs of the encoder and three of the decoder, the last ones over 2 x 3 pixels with batch statistics of 12
# samples behind them: a unit within rounding distance of its kink moves these gradients in ANY float32 evaluation.  As in
# tests/test_matching_gpu.py the images are drawn from a seed for which PyTorch's own float32 CPU run of the restatement below
# stays within GRAD_TOL / 16 of the float64 run (a choice of the case, not an assertion of the test).
POSE_SEED = 13
B, H, W = 2, 64, 96


def _close(a, b, tol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).double()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def restate(esd, dsd, img, training, invert):
    """ResnetEncoder.forward (resnet_encoder.py:769-781) and PoseDecoder.forward (pose_decoder.py:33-52) with the matrices of
    trainer.py:694-707, in the dtype of the weights.  esd / dsd: the two state dicts."""
    def bn(x, p):
        return F.batch_norm(x, None if training else esd[p + ".running_mean"], None if training else esd[p + ".running_var"],
                            esd[p + ".weight"], esd[p + ".bias"], training, 0.1, 1e-5)

    def block(x, p, stride):
        y = F.relu(bn(F.conv2d(x, esd[p + ".conv1.weight"], None, stride, 1), p + ".bn1"))
        y = bn(F.conv2d(y, esd[p + ".conv2.weight"], None, 1, 1), p + ".bn2")
        if p + ".downsample.0.weight" in esd:
            x = bn(F.conv2d(x, esd[p + ".downsample.0.weight"], None, stride), p + ".downsample.1")
        return F.relu(y + x)

    feats = [F.relu(bn(F.conv2d((img - 0.45) / 0.225, esd["encoder.conv1.weight"], None, 2, 3), "encoder.bn1"))]
    x = F.max_pool2d(feats[0], 3, 2, 1)
    for i in (1, 2, 3, 4):
        x = block(block(x, f"encoder.layer{i}.0", 1 if i == 1 else 2), f"encoder.layer{i}.1", 1)
        feats.append(x)
    out = F.relu(F.conv2d(feats[-1], dsd["net.0.weight"], dsd["net.0.bias"]))
    for i in (1, 2):
        out = F.relu(F.conv2d(out, dsd[f"net.{i}.weight"], dsd[f"net.{i}.bias"], 1, 1))
    out = F.conv2d(out, dsd["net.3.weight"], dsd["net.3.bias"])
    out = 0.01 * out.mean(3).mean(2).view(-1, 2, 1, 6)
    aa, tr = out[..., :3], out[..., 3:]
    return feats, aa, tr, P.torch_matrix(aa[:, 0], tr[:, 0], invert), P.torch_matrix(aa[:, 0], tr[:, 0], not invert)


def build(seed=POSE_SEED):
    sys.path.insert(0, GOLDEN)
    from synth_weights import fill_state_dict
    from manydepth import networks
    enc = networks.ResnetEncoder(18, False, num_input_images=2)
    dec = networks.PoseDecoder(enc.num_ch_enc, 1, 2)
    fill_state_dict(enc, 0, prefix="pose_encoder.")
    fill_state_dict(dec, 0, prefix="pose.")
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 6, H, W, generator=g)
    cot = [torch.randn(s, generator=g) for s in ((B, 2, 1, 3), (B, 2, 1, 3), (B, 4, 4), (B, 4, 4))]
    return enc, dec, img, cot


def loss_of(outs, cot):
    return sum((o * c.to(o.dtype).to(o.device)).sum() for o, c in zip(outs, cot))


def _ran(name):
    return not name.startswith("encoder.fc.")                          # constructed, never run (as in the reference)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("eval", "train"))
def test_pose_network_against_fp64_restatement(mode):
    enc, dec, img, cot = build()
    training = mode == "train"
    esd = {k: v.detach().double().clone() for k, v in enc.state_dict().items()}
    dsd = {k: v.detach().double().clone() for k, v in dec.state_dict().items()}
    enames = [k for k, _ in enc.named_parameters() if _ran(k)]
    dnames = [k for k, _ in dec.named_parameters()]
    for k in enames:
        esd[k].requires_grad_(True)
    for k in dnames:
        dsd[k].requires_grad_(True)
    wf, waa, wtr, wT, wTi = restate(esd, dsd, img.double(), training, True)
    enc.cuda()
    dec.cuda()
    getattr(enc, mode)()
    getattr(dec, mode)()
    with torch.set_grad_enabled(training):
        feats = enc(img.cuda())
        aa, tr, T, Ti = dec.forward_with_matrices([feats], invert=True)
    assert len(feats) == 5 and [f.shape[1] for f in feats] == [64, 64, 128, 256, 512] and tuple(feats[-1].shape[2:]) == (2, 3)
    for i in range(5):
        _close(feats[i], wf[i].detach(), FWD_TOL, f"features[{i}] {mode}")
    assert tuple(aa.shape) == tuple(tr.shape) == (B, 2, 1, 3) and tuple(T.shape) == tuple(Ti.shape) == (B, 4, 4)
    for got, want, name in ((aa, waa, "axisangle"), (tr, wtr, "translation"), (T, wT, "cam_T_cam"), (Ti, wTi, "cam_T_cam_inv")):
        _close(got, want.detach(), FWD_TOL, f"{name} {mode}")
    # forward() is the reference's: (axisangle, translation), the same bits
    with torch.no_grad():
        aa2, tr2 = dec([[f.detach() for f in feats]])
    if not training:
        assert torch.equal(aa2, aa) and torch.equal(tr2, tr)
        return
    loss_of((waa, wtr, wT, wTi), cot).backward()
    enc.zero_grad()
    dec.zero_grad()
    loss_of((aa, tr, T, Ti), cot).backward()
    torch.cuda.synchronize()
    for names, mod, sd, tag in ((enames, enc, esd, "pose_encoder"), (dnames, dec, dsd, "pose")):
        named = dict(mod.named_parameters())
        for k in names:
            assert named[k].grad is not None, k
            _close(named[k].grad, sd[k].grad, GRAD_TOL, f"grad {tag}.{k}")
    assert dict(enc.named_parameters())["encoder.fc.weight"].grad is None


def test_state_dict_names_are_torchvisions_and_the_references():
    from manydepth import networks
    from oracle import nets as onets
    enc = networks.ResnetEncoder(18, False, num_input_images=2)
    tv = onets.ShallowResnetEncoder(18, False).encoder.state_dict()           # torchvision key names
    sd = enc.state_dict()
    assert list(sd.keys()) == ["encoder." + k for k in tv.keys()]
    for k, v in tv.items():
        want = (64, 6, 7, 7) if k == "conv1.weight" else tuple(v.shape)
        assert tuple(sd["encoder." + k].shape) == want, k
    assert tuple(networks.ResnetEncoder(18, False).state_dict()["encoder.conv1.weight"].shape) == (64, 3, 7, 7)
    assert enc.num_ch_enc.tolist() == [64, 64, 128, 256, 512]
    dec = networks.PoseDecoder(enc.num_ch_enc, 1, 2)
    shapes = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    assert shapes == {"net.0.weight": (256, 512, 1, 1), "net.0.bias": (256,), "net.1.weight": (256, 256, 3, 3),
                      "net.1.bias": (256,), "net.2.weight": (256, 256, 3, 3), "net.2.bias": (256,),
                      "net.3.weight": (12, 256, 1, 1), "net.3.bias": (12,)}
    assert networks.PoseDecoder(enc.num_ch_enc, 2).state_dict()["net.1.weight"].shape[1] == 512     # two feature stacks
    assert networks.PoseDecoder(enc.num_ch_enc, 2).num_frames_to_predict_for == 1
    with pytest.raises(ValueError):
        networks.ResnetEncoder(50, False)
    with pytest.raises(NotImplementedError):
        networks.PoseCNN(2)


def test_pretrained_halves_conv1_for_two_images(tmp_path, monkeypatch):
    from manydepth import networks
    from manydepth.networks.resnet_encoder import ResNet18
    torch.manual_seed(3)
    tv = ResNet18().state_dict()
    path = str(tmp_path / "resnet18.pth")
    torch.save(tv, path)
    monkeypatch.setenv("PD_RESNET18_WEIGHTS", path)
    two = networks.ResnetEncoder(18, True, num_input_images=2).state_dict()
    assert torch.equal(two["encoder.conv1.weight"], torch.cat([tv["conv1.weight"]] * 2, 1) / 2)
    assert torch.equal(two["encoder.layer3.1.conv2.weight"], tv["layer3.1.conv2.weight"])
    one = networks.ResnetEncoder(18, True, num_input_images=1).state_dict()
    assert torch.equal(one["encoder.conv1.weight"], tv["conv1.weight"])
    monkeypatch.delenv("PD_RESNET18_WEIGHTS")
    with pytest.warns(UserWarning, match="from scratch"):
        networks.ResnetEncoder(18, True, num_input_images=2)
