"""pd_pose_chain / ops.pose_chain on the device against tests/pose_chain_ref.py, bit for bit: item counts on both sides of
a 64-thread group, every chain length class, both directions, the three kinds of ``present``, with and without ``init``;
the fixture's inputs; one link against ops.pose_matrix; NaN containment; reproducibility; a captured replay."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import pose_chain_ref as C
import pose_ref as P

pytestmark = pytest.mark.gpu
F32 = np.float32


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


def _links(rng, L, N):
    """Angles up to ~1.2 rad and translations up to 1: the range tests/test_pose_gpu.py draws for one matrix."""
    return rng.uniform(-0.7, 0.7, (L, N, 3)).astype(F32), rng.uniform(-1, 1, (L, N, 3)).astype(F32)


def _present(rng, kind, L, N):
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros((L, N), F32)
    p = (rng.random((L, N)) > 0.3).astype(F32)
    p[rng.integers(L), rng.integers(N)] = 0                      # at least one absent frame, whatever was drawn
    return p * rng.uniform(0.5, 2.0, (L, N)).astype(F32)         # any non-zero value means present


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("N", [1, 3, 65, 257])
def test_device_equals_the_statement_bit_for_bit(N):
    from polardepth import ops
    rng = np.random.default_rng(100 + N)
    for L in (1, 2, 3, 8):
        aa, tr = _links(rng, L, N)
        init = P.pose_matrix(*(a[0] for a in _links(rng, 1, N)), False).astype(F32)
        for direction in (-1, 1):
            for kind in ("none", "mixed", "zero"):
                present = _present(rng, kind, L, N)
                for ini in (None, init):
                    want, want_inv = C.pose_chain(aa, tr, present, ini, direction)
                    rel, rel_inv = ops.pose_chain(_cu(aa), _cu(tr), _cu(present), _cu(ini), direction)
                    assert tuple(rel.shape) == tuple(rel_inv.shape) == (L, N, 4, 4) and rel.dtype == torch.float32
                    assert not rel.requires_grad and not rel_inv.requires_grad
                    tag = (N, L, direction, kind, ini is not None)
                    assert np.array_equal(rel.cpu().numpy(), want), tag
                    assert np.array_equal(rel_inv.cpu().numpy(), want_inv), tag
                    if kind == "zero":
                        assert not rel.any() and rel_inv.reshape(L * N, 16).any(1).all()


@pytest.mark.parametrize("case", ["a", "b"])
def test_device_equals_the_statement_on_the_fixture(case):
    from polardepth import ops
    g = dict(np.load(os.path.join(GOLDEN, "g16_pose_chain.npz")))
    ids = [int(i) for i in g[f"{case}_ids"]]
    for s in (-1, 1):
        chain = sorted([f for f in ids if f * s > 0], key=abs)
        if not chain:
            continue
        aa = np.stack([g[f"{case}_aa_{f}"] for f in chain])
        tr = np.stack([g[f"{case}_tr_{f}"] for f in chain])
        present = np.stack([g[f"frame_{f}"].reshape(4, -1).sum(1) != 0 for f in chain]).astype(F32)
        want, want_inv = C.pose_chain(aa, tr, present, None, s)
        rel, rel_inv = ops.pose_chain(_cu(aa), _cu(tr), _cu(present), None, s)
        assert np.array_equal(rel.cpu().numpy(), want) and np.array_equal(rel_inv.cpu().numpy(), want_inv)
        for k, f in enumerate(chain):                            # and the reference's float32 chain is as near as the CPU test shows
            assert np.abs(rel[k].cpu().numpy().astype(np.float64) - g[f"{case}_rel_{f}"]).max() <= 1e-6


@pytest.mark.parametrize("direction", [-1, 1])
def test_one_link_is_bit_equal_to_pose_matrix(direction):
    from polardepth import ops
    aa, tr = _links(np.random.default_rng(5), 1, 131)
    rel, rel_inv = ops.pose_chain(_cu(aa), _cu(tr), None, None, direction)
    assert np.array_equal(_bits(rel[0]), _bits(ops.pose_matrix(_cu(aa[0]), _cu(tr[0]), direction < 0)))
    assert np.array_equal(_bits(rel_inv[0]), _bits(ops.pose_matrix(_cu(aa[0]), _cu(tr[0]), direction > 0)))
    # [L,N,1,3], the decoder's own layout, is the same call
    r4, _ = ops.pose_chain(_cu(aa[:, :, None]), _cu(tr[:, :, None]), None, None, direction)
    assert torch.equal(r4, rel)


def test_nan_stays_in_its_item_and_runs_are_bit_equal():
    from polardepth import ops
    rng = np.random.default_rng(6)
    L, N = 4, 70
    aa, tr = _links(rng, L, N)
    clean, clean_inv = ops.pose_chain(_cu(aa), _cu(tr), None, None, -1)
    aa2, tr2 = aa.copy(), tr.copy()
    aa2[1, 7, 0] = np.nan                                        # item 7, from link 1 on
    tr2[2, 66, 1] = np.nan                                       # item 66 (second group), from link 2 on
    rel, rel_inv = ops.pose_chain(_cu(aa2), _cu(tr2), None, None, -1)
    bad = torch.isnan(rel).reshape(L, N, 16).any(2).cpu().numpy()
    want = np.zeros((L, N), bool)
    want[1:, 7] = True
    want[2:, 66] = True
    assert np.array_equal(bad, want)
    keep = torch.from_numpy(~want).cuda()
    assert torch.equal(rel[keep], clean[keep])
    assert torch.isnan(rel_inv[1, 7]).any() and not torch.isnan(rel_inv[2, 7]).any()      # the link's own inverse only
    again, again_inv = ops.pose_chain(_cu(aa2), _cu(tr2), None, None, -1)
    assert np.array_equal(_bits(again), _bits(rel)) and np.array_equal(_bits(again_inv), _bits(rel_inv))
    # an absent frame ends a NaN too: the stored pose is sixteen zeros
    present = np.ones((L, N), F32)
    present[2, 7] = 0
    rel3, _ = ops.pose_chain(_cu(aa2), _cu(tr2), _cu(present), None, -1)
    assert torch.isnan(rel3[1, 7]).any() and not rel3[2:, 7].any()


def test_captured_replay_is_bit_equal_to_the_eager_call():
    from polardepth import ops
    rng = np.random.default_rng(7)
    L, N = 3, 65
    aa, tr = (_cu(a) for a in _links(rng, L, N))
    present = _cu(_present(rng, "mixed", L, N))
    init = _cu(P.pose_matrix(*(a[0] for a in _links(rng, 1, N)), False).astype(F32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on a side stream, as stream capture requires
        eager, eager_inv = ops.pose_chain(aa, tr, present, init, 1)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # contiguous fp32 inputs: this one kernel and nothing else
        rel, rel_inv = ops.pose_chain(aa, tr, present, init, 1)
    rel.zero_()
    rel_inv.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rel), _bits(eager)) and np.array_equal(_bits(rel_inv), _bits(eager_inv))
    # the replay reads the tensors of its capture: new parameters, new poses
    aa.copy_(aa.flip(1))
    graph.replay()
    torch.cuda.synchronize()
    again, _ = ops.pose_chain(aa, tr, present, init, 1)
    assert torch.equal(rel, again) and not torch.equal(rel, eager)
