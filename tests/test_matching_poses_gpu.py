"""polardepth.matching.matching_poses with the real pose modules (64 x 96, B = 2, the size of the ResnetEncoderMatching test):
which frames are paired and in which order, the result against ops.pose_chain of the modules' own outputs, an absent frame,
no tape, untouched buffers in eval mode -- and the plane sweep of ResnetEncoderMatching fed from these poses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, H, W, D = 2, 64, 96, 16
# (matching ids, {frame id: absent items})
CASES = {"past": ([0, -1, -2], {-1: [1]}), "both": ([0, 1, -1], {1: [1], -1: [1]})}


class _Recording(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, x):
        self.seen.append(x.detach().clone())
        return self.inner(x)


@pytest.fixture(scope="module")
def modules():
    from manydepth import networks
    torch.manual_seed(11)
    enc = networks.ResnetEncoder(18, False, num_input_images=2).cuda().eval()
    dec = networks.PoseDecoder(enc.num_ch_enc, num_input_features=1, num_frames_to_predict_for=2).cuda().eval()
    with torch.no_grad():                                     # poses of a size a cost volume can see: the fresh head gives ~1e-4
        dec.convs[("pose", 2)].weight.mul_(30.0)
        dec.convs[("pose", 2)].bias.copy_(torch.tensor([.3, -.2, .1, .5, -.4, .2] * 2, device="cuda"))
    return enc, dec


def _batch(ids, absent):
    g = torch.Generator().manual_seed(21)
    frames, present = {}, {}
    for f in sorted(set(ids) | {0}):
        frames[f] = torch.rand(B, 3, H, W, generator=g).cuda()
        present[f] = torch.ones(B).cuda()
        for n in absent.get(f, ()):                           # what the loaders serve for a frame that does not exist
            frames[f][n] = 0
            present[f][n] = 0
    return frames, present


@pytest.mark.parametrize("case", list(CASES))
def test_matching_poses_and_the_sweep_from_them(modules, case):
    from manydepth import networks
    from polardepth import matching, ops
    enc, dec = modules
    ids, absent = CASES[case]
    frames, present = _batch(ids, absent)
    rec = _Recording(enc)
    before = {k: v.clone() for m in (enc, dec) for k, v in m.named_buffers()}
    rel, rel_inv = matching.matching_poses(rec, dec, frames, ids, present)
    # one pass per id, in the order of the ids, the pair stacked in temporal order
    assert list(rel) == list(rel_inv) == ids[1:] and len(rec.seen) == len(ids) - 1
    for fi, x in zip(ids[1:], rec.seen):
        a, b = (fi, fi + 1) if fi < 0 else (fi - 1, fi)
        assert torch.equal(x, torch.cat([frames[a], frames[b]], 1)), fi
    # ... equal to ops.pose_chain of the modules' own slot-0 outputs
    with torch.no_grad():
        own = {fi: dec([enc(x)]) for fi, x in zip(ids[1:], rec.seen)}
    for s in (-1, 1):
        chain = sorted([f for f in ids if f * s > 0], key=abs)
        if not chain:
            continue
        r, ri = ops.pose_chain(torch.stack([own[f][0][:, 0] for f in chain]), torch.stack([own[f][1][:, 0] for f in chain]),
                               torch.stack([present[f] for f in chain]), None, s)
        for k, f in enumerate(chain):
            assert torch.equal(rel[f], r[k]) and torch.equal(rel_inv[f], ri[k]), f
    for f in ids[1:]:
        assert tuple(rel[f].shape) == tuple(rel_inv[f].shape) == (B, 4, 4)
        assert torch.isfinite(rel[f]).all() and torch.isfinite(rel_inv[f]).all()
        assert not rel[f].requires_grad and not rel_inv[f].requires_grad and rel[f].grad_fn is None
        assert rel[f][0].any() and rel_inv[f].reshape(B, 16).any(1).all()          # item 0 has every frame
    # an absent frame: zeros there and from there on down its chain; the other direction does not see it
    if case == "past":
        assert not rel[-1][1].any() and not rel[-2][1].any()
    else:
        assert not rel[1][1].any() and not rel[-1][1].any()
    # eval mode: no buffer moved
    after = {k: v for m in (enc, dec) for k, v in m.named_buffers()}
    assert before and all(torch.equal(before[k], after[k]) for k in before)
    # the poses are of a size the sweep can see
    assert float((rel[ids[1]][0, :3, 3]).abs().max()) > 1e-3

    # the plane sweep from these poses
    torch.manual_seed(12)
    sweep = networks.ResnetEncoderMatching(18, False, H, W, 0.3, 2.0, D).cuda().eval()
    K = torch.eye(4).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.58 * (W // 4), 0.9 * (H // 4), 0.5 * (W // 4), 0.5 * (H // 4)
    inv_K = torch.linalg.inv(K)
    lookups = torch.stack([frames[f] for f in ids[1:]], 1)
    poses = torch.stack([rel[f] for f in ids[1:]], 1)
    with torch.no_grad():
        feats, lowest, conf = sweep(frames[0], lookups, poses, K.cuda(), inv_K.cuda())
    assert len(feats) == 5 and all(torch.isfinite(f).all() for f in feats) and torch.isfinite(lowest).all()
    assert tuple(conf.shape) == (B, H // 4, W // 4)
    assert not conf[1].any()                                  # item 1: every lookup frame absent -> all-zero poses
    assert conf[0].any()


def test_matching_poses_refuses_ids_with_gaps(modules):
    from polardepth import matching
    enc, dec = modules
    frames, present = _batch([0, -1, -2], {})
    for bad in ([0, -2], [0, -1, -3], [0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="matching_ids"):
            matching.matching_poses(enc, dec, frames, bad, present)
