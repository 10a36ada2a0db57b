"""The entry points of csrc/pose_loss.hip, host side (no GPU): exported symbols, SIGNATURES, the header, and every refusal
that is decided before the device is touched -- the pointers are dummies that are never dereferenced."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
N_ARGS = {"pd_pose_loss_fwd": 9, "pd_pose_loss_bwd": 9}
P = ctypes.c_void_p(64)
MAX_F = 8                                    # PD_REPROJ_MAX_FRAMES


def ptrs(n, null_at=None):
    return (ctypes.c_void_p * max(n, 1))(*[None if i == null_at else 64 for i in range(max(n, 1))])


def weights(n):
    return (ctypes.c_float * max(n, 1))(*[1.0] * max(n, 1))


def test_symbols_and_signatures():
    src = open(HEADER).read()
    so = ctypes.CDLL(_lib.lib.path)
    for name, n in N_ARGS.items():
        assert name in _lib.SIGNATURES and hasattr(so, name) and name in src, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    assert f"#define PD_REPROJ_MAX_FRAMES {MAX_F}" in src and ops.REPROJ_MAX_FRAMES == MAX_F


def test_refusals_need_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def fwd(F=2, N=4, pred=True, gt=True, w=True, vals=P, rec=None, null_at=None):
        return L.pd_pose_loss_fwd(ptrs(F, null_at) if pred else None, ptrs(F) if gt else None, F, weights(F) if w else None,
                                  None, rec, vals, N, None)

    def bwd(F=2, N=4, pred=True, gt=True, w=True, gvals=P, gT=True, null_at=None):
        return L.pd_pose_loss_bwd(gvals, ptrs(F, null_at) if pred else None, ptrs(F) if gt else None, F,
                                  weights(F) if w else None, None, ptrs(F) if gT else None, N, None)

    for call in (fwd, bwd):
        for F in (0, -1, MAX_F + 1):
            assert call(F=F) == -22 and b"frames" in err(), F
        for N in (-1, 65536):
            assert call(N=N) == -22 and b"item count" in err(), N
        for kw in ({"pred": False}, {"gt": False}, {"w": False}):
            assert call(**kw) == -22 and b"must not be null" in err(), kw
        assert call(null_at=1) == -22 and b"frame 1" in err()
    assert fwd(vals=None) == -22 and b"vals must not be null" in err()
    assert fwd(rec=ctypes.c_void_p(68)) == -22 and b"8-byte aligned" in err()
    assert bwd(gT=False) == -22 and b"must not be null" in err()
    assert bwd(gvals=None) == -22 and b"must not be null" in err()
    assert bwd(N=0) == 0 and bwd(N=0, F=MAX_F) == 0                # an empty batch launches nothing backward


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    T = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_supervision([T, T], [T, T])
    with pytest.raises(ValueError, match="as many"):
        ops.pose_supervision([T, T], [T])
    with pytest.raises(ValueError, match="frames"):
        ops.pose_supervision([], [])
    with pytest.raises(ValueError, match="frames"):
        ops.pose_supervision([T] * 9, [T] * 9)
    d = T                                    # shapes are checked before the device
    with pytest.raises(ValueError, match=r"\[N,4,4\]"):
        ops.pose_supervision([d[:, :3]], [d[:, :3]])
    with pytest.raises(ValueError, match="every pose"):
        ops.pose_supervision([d, d], [d, d[:2]])
    with pytest.raises(ValueError, match="valid must be"):
        ops.pose_supervision([d, d], [d, d], valid=torch.ones(3, 1))
    with pytest.raises(ValueError, match="frame weights"):
        ops.pose_supervision([d, d], [d, d], frame_weight=[1.0])
