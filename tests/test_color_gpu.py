"""The colour pyramid and ColorJitter on the device against Pillow as installed (manydepth.datasets.apply_color_jitter,
Image.resize(..., LANCZOS), the loader's to_t): every comparison is exact.  The arithmetic is csrc/color_math.hpp; the
kernels take four pixels per lane when H*W is a multiple of 4 (4096x4096, 8x12, 4x4, 16x16) and one otherwise (37x53,
1x1, 3x87), and the contrast mean comes from one workgroup (the small images) up to 256 (every colour)."""
import itertools
import random

import numpy as np
import pytest
import torch

from color_cases import make_hammer_tree, dataset, pil_jitter, pil_pyramid

pytestmark = pytest.mark.gpu

OPS = ("brightness", "contrast", "saturation", "hue")
_R = random.Random(7)
_SEEDED = [_R.uniform(0.8, 1.2), _R.uniform(0.8, 1.2)]


def _rows(param_lists):
    from polardepth import color as pdcolor
    return torch.from_numpy(np.stack([pdcolor.pack_jitter(p) for p in param_lists]))


def _jitter(x, param_lists, want=("u8",)):
    from polardepth import color as pdcolor
    out = pdcolor.color_jitter_u8(torch.as_tensor(x).cuda(), None if param_lists is None else _rows(param_lists), want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _workspace_is_clean():
    """sum_ws contract: the sum (2 words) and the ticket of every sample are zero again after a call."""
    from polardepth import color as pdcolor
    ws = pdcolor._WS[torch.cuda.current_device()].view(torch.int32).view(-1, 4).cpu()
    return not ws[:, :3].any()


# ---------------------------------------------------------------------------------------------- 1. every colour
@pytest.fixture(scope="module")
def every_colour():
    g = np.arange(256, dtype=np.uint8)
    hwc = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(4096, 4096, 3)
    chw = np.ascontiguousarray(hwc.transpose(2, 0, 1))
    return chw, torch.from_numpy(chw)[None].cuda()


_EVERY = [("hue", v) for v in (-0.1, -0.037, 0, 0.05, 0.1)] + \
         [(n, v) for n in ("saturation", "brightness") for v in (0.8, 1.0, 1.2, *_SEEDED)] + \
         [("contrast", 0.8), ("contrast", 1.2)]


@pytest.mark.parametrize("op,value", _EVERY, ids=[f"{n}{v:+.4f}" for n, v in _EVERY])
def test_every_colour(every_colour, op, value):
    from polardepth import color as pdcolor
    chw, dev = every_colour
    got = pdcolor.color_jitter_u8(dev, _rows([[(op, value)]]), want=("u8",))["u8"][0].cpu().numpy()
    ref = pil_jitter(chw, [(op, value)])
    bad = int((got != ref).any(0).sum())
    print(f"{op} {value!r}: {bad} of 2^24 colours differ")
    np.testing.assert_array_equal(got, ref)
    assert _workspace_is_clean()


# ---------------------------------------------------------------------------------------------- 2. contrast rounding
def test_contrast_mean_rounds_half_up_and_small_images():
    grey = np.array([10] * 8 + [11] * 8, np.uint8).reshape(4, 4)
    x = np.stack([grey, grey, grey])[None]                     # L of a grey pixel is the grey: mean 10.5 -> degenerate 11
    for f in (0.0, 0.8, 1.2):
        got = _jitter(x, [[("contrast", f)]])["u8"][0]
        np.testing.assert_array_equal(got, pil_jitter(x[0], [("contrast", f)]))
        if f == 0.0:
            assert (got == 11).all()                           # factor 0 is the degenerate itself
    rng = np.random.default_rng(2)
    one = rng.integers(1, 256, (1, 3, 1, 1), dtype=np.uint8)   # 1x1: the pixel is its own mean
    zero = np.zeros((1, 3, 5, 7), np.uint8)                    # blank frames stay blank (indoor_dataset.py:222-225)
    random.seed(11)
    from manydepth import datasets
    for x in (one, zero):
        for p in ([("contrast", 0.8)], [("contrast", 1.2)], datasets.color_jitter_params(), datasets.color_jitter_params()):
            np.testing.assert_array_equal(_jitter(x, [p])["u8"][0], pil_jitter(x[0], p))
    assert not _jitter(zero, [datasets.color_jitter_params()])["u8"].any()
    assert _workspace_is_clean()


# ---------------------------------------------------------------------------------------------- 3. chains
@pytest.mark.parametrize("H,W", [(37, 53), (8, 12)])
def test_chains_of_all_24_orders(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    r = random.Random(H + W)
    x = rng.integers(0, 256, (24, 3, H, W), dtype=np.uint8)
    params = []
    for b, perm in enumerate(itertools.permutations(OPS)):
        f = {"brightness": r.uniform(0.8, 1.2), "contrast": r.uniform(0.8, 1.2), "saturation": r.uniform(0.8, 1.2),
             "hue": r.uniform(-0.1, 0.1)}
        params.append(None if b in (5, 17) else [(n, f[n]) for n in perm])
    got = _jitter(x, params, want=("u8", "f32"))
    for b in range(24):
        ref = x[b] if params[b] is None else pil_jitter(x[b], params[b])
        np.testing.assert_array_equal(got["u8"][b], ref, err_msg=f"sample {b}: {params[b]}")
    np.testing.assert_array_equal(got["f32"], got["u8"].astype(np.float32) / 255.0)
    assert _workspace_is_clean()


def test_unknown_codes_and_a_repeated_contrast_behave_as_none():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (3, 3, 6, 10), dtype=np.uint8)
    rows = torch.tensor([[7, 1.1, 2.5, 0.9, -1, 1.2, 0, 0.5],            # nothing the device knows: a copy
                         [2, 1.2, 2, 0.8, 0, 0, 0, 0],                   # the second contrast is dropped
                         [1, 0.9, 9, 0.3, 4, 0.05, 0, 0]], dtype=torch.float64)
    from polardepth import color as pdcolor
    got = pdcolor.color_jitter_u8(torch.from_numpy(x).cuda(), rows, want=("u8",))["u8"].cpu().numpy()
    np.testing.assert_array_equal(got[0], x[0])
    np.testing.assert_array_equal(got[1], pil_jitter(x[1], [("contrast", 1.2)]))
    np.testing.assert_array_equal(got[2], pil_jitter(x[2], [("brightness", 0.9), ("hue", 0.05)]))


# ---------------------------------------------------------------------------------------------- 4. conversion
@pytest.mark.parametrize("shape", [(1, 3, 16, 16), (2, 3, 3, 87)])
def test_conversion_is_the_correctly_rounded_quotient(shape):
    n = int(np.prod(shape))
    x = (np.arange(n) % 256).astype(np.uint8).reshape(shape)             # every plane holds all 256 values
    assert all(len(np.unique(x[b, c])) == 256 for b in range(shape[0]) for c in range(3))
    plain = _jitter(x, None, want=("u8", "f32"))
    want = np.float32(x) / 255.0
    assert want.dtype == np.float32
    np.testing.assert_array_equal(plain["f32"].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(plain["u8"], x)
    zeros = _jitter(x, [None] * shape[0], want=("u8", "f32"))            # params == NULL is a batch of zero rows
    np.testing.assert_array_equal(zeros["f32"].view(np.uint32), plain["f32"].view(np.uint32))
    np.testing.assert_array_equal(zeros["u8"], x)


# ---------------------------------------------------------------------------------------------- 5. pyramid
def test_pyramid_matches_the_host_loader():
    from manydepth import datasets
    from polardepth import color as pdcolor
    rng = np.random.default_rng(12)
    raw = rng.integers(0, 256, (2, 3, 96, 128), dtype=np.uint8)
    random.seed(3)
    params = [datasets.color_jitter_params(), None]                      # sample 0 augmented, sample 1 not
    got = pdcolor.color_pyramid(torch.from_numpy(raw).cuda(), _rows(params).cuda(), (64, 96), 4)
    assert len(got) == 8
    for b in range(2):
        ref = pil_pyramid(raw[b], params[b], (64, 96), 4)
        for k, v in ref.items():
            assert got[k].dtype == torch.float32 and got[k].shape == (2, 3, 64 >> k[2], 96 >> k[2]), k
            np.testing.assert_array_equal(got[k][b].cpu().numpy(), v, err_msg=f"{k} sample {b}")
    assert not torch.equal(got[("color_aug", 0, 0)][0], got[("color", 0, 0)][0])
    plain = pdcolor.color_pyramid(torch.from_numpy(raw).cuda(), None, (64, 96), 4)
    for s in range(4):
        assert plain[("color_aug", 0, s)] is plain[("color", 0, s)]
        assert torch.equal(plain[("color", 0, s)], got[("color", 0, s)])


# ---------------------------------------------------------------------------------------------- 6. end to end
@pytest.fixture(scope="module")
def hammer_tree(tmp_path_factory):
    return make_hammer_tree(tmp_path_factory.mktemp("hammer"))


def _batch_seed(want_gates):
    """A seed after which two consecutive training items pass the augmentation gate as in want_gates."""
    from manydepth import datasets
    for k in range(256):
        random.seed(k)
        gates = []
        for _ in want_gates:
            gates.append(random.random() > 0.5)
            if gates[-1]:
                datasets.color_jitter_params()
        if tuple(gates) == tuple(want_gates):
            return k
    raise AssertionError(want_gates)


def _batch(ds, seed):
    random.seed(seed)
    return torch.utils.data.default_collate([ds[0], ds[1]])


def _trainer(tmp_path, tag):
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    torch.manual_seed(0)
    return Trainer(_opts(tmp_path / tag, ["--dropout_rate", "0.0"]))


def test_raw_colour_batch_gives_the_bits_of_the_host_batch(hammer_tree, tmp_path):
    seed = _batch_seed((True, False))
    host = _batch(dataset(hammer_tree, is_train=True), seed)
    raw = _batch(dataset(hammer_tree, is_train=True, raw_color=True), seed)
    assert raw["color_jitter"][0].any() and not raw["color_jitter"][1].any()
    tr = _trainer(tmp_path, "e2e")
    tr.set_eval()
    with torch.no_grad():
        o1, l1, _ = tr.process_batch(raw)
        o2, l2, _ = tr.process_batch(host)
    for s in range(4):
        assert torch.equal(raw[("color", 0, s)], host[("color", 0, s)]), s
        assert torch.equal(raw[("color_aug", 0, s)], host[("color_aug", 0, s)]), s
    assert not torch.equal(host[("color_aug", 0, 0)][0], host[("color", 0, 0)][0])
    assert torch.isfinite(l2["loss"]).all()
    assert torch.equal(o1[("disp", 0)], o2[("disp", 0)]) and torch.equal(l1["loss"], l2["loss"])


def test_graphed_step_replays_with_new_jitter_rows(hammer_tree, tmp_path):
    """The jitter rows are device data: two replays of the captured step on raw-colour batches with different draws give
    the loss bits of two eager steps from the same start."""
    from polardepth import functional as PF
    from polardepth.graph import GraphedTrainStep
    ds = dataset(hammer_tree, is_train=True, raw_color=True)
    batches = [{k: v.cuda() for k, v in _batch(ds, _batch_seed(g)).items()} for g in ((True, False), (False, True))]
    assert not torch.equal(batches[0]["color_jitter"], batches[1]["color_jitter"])
    PF.DropoutState.manual_seed(3)
    tr_e = _trainer(tmp_path, "eager")
    tr_e.set_train()
    losses_e = []
    for b in batches:
        tr_e.model_optimizer.zero_grad()
        _, L, _ = tr_e.process_batch(dict(b), is_train=True)
        L["loss"].backward()
        tr_e.model_optimizer.step()
        losses_e.append(L["loss"].detach().clone())
    PF.DropoutState.manual_seed(3)
    tr_g = _trainer(tmp_path, "graph")
    tr_g.set_train()
    gs = GraphedTrainStep(tr_g, batches[0], warmup=1, restore_state=True)
    losses_g = [gs.step(b).detach().clone() for b in batches]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(losses_e, losses_g)):
        assert torch.isfinite(a) and torch.equal(a, b), f"loss of step {i}: eager {a.item()!r} graph {b.item()!r}"
    assert torch.equal(tr_e.store.flat, tr_g.store.flat)
