"""The entry point of csrc/matching.hip, host side (no GPU): the exported symbol, SIGNATURES, the header, and every refusal that
is decided before the device is touched -- the pointers are dummies that are never dereferenced on these paths."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, matching, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
P, ODD = ctypes.c_void_p(64), ctypes.c_void_p(68)        # 16-byte aligned dummy / 4-byte aligned only


def test_symbol_signature_and_header():
    src = open(HEADER).read()
    so = ctypes.CDLL(_lib.lib.path)
    assert hasattr(so, "pd_cost_volume") and "int pd_cost_volume(" in src
    assert len(_lib.SIGNATURES["pd_cost_volume"][1]) == 21
    assert ops.COST_VOLUME_MAX_BINS == 128 and "1 <= D <= 128" in src
    # the definition is stated where pd_view_synth_fwd's is
    for phrase in ("samples ONLY where m = 1", "(float)n + 1e-7f", "FIRST index of the minimum", "binary tree"):
        assert phrase in src, phrase


def test_argument_validation_needs_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def call(cur=P, lookup=P, T=P, K=P, iK=P, bins=P, valid=None, cost=P, ldc=None, missing=None, conf=P, argmin=P, lowest=P,
             B=1, F=2, h=8, w=8, C=64, D=16, flag=0):
        return L.pd_cost_volume(cur, lookup, T, K, iK, bins, valid, cost, D if ldc is None else ldc, missing, conf, argmin,
                                lowest, B, F, h, w, C, D, flag, None)

    for C in (0, -4, 3, 6, 62):
        assert call(C=C) == -22 and b"multiple of 4" in err(), C
    for D in (0, -1, 129):
        assert call(D=D, ldc=200) == -22 and b"depth bins" in err(), D
    for F in (-1, ops.REPROJ_MAX_FRAMES + 1):
        assert call(F=F) == -22 and b"frames" in err(), F
    for ldc in (15, 0, -16):
        assert call(ldc=ldc) == -22 and b"pixel stride" in err(), ldc
    for kw in ({"B": -1}, {"B": 65536}, {"h": 0}, {"w": 0}):
        assert call(**kw) == -22 and b"bad shape" in err(), kw
    assert call(h=1 << 15, w=(1 << 15) + 1) == -22 and b"too large" in err()
    for kw in ({"cur": None}, {"K": None}, {"iK": None}, {"bins": None}, {"cost": None}, {"conf": None}, {"argmin": None},
               {"lowest": None}, {"lookup": None}, {"T": None}):
        assert call(**kw) == -22 and b"must not be null" in err(), kw
    for kw in ({"cur": ODD}, {"lookup": ODD}):
        assert call(**kw) == -22 and b"16-byte aligned" in err(), kw
    assert call(flag=2) == -22 and b"apply_confidence" in err()
    assert call(B=0) == 0                                   # an empty batch touches nothing
    assert call(B=0, ldc=80) == 0 and call(B=0, F=0, lookup=None, T=None) == 0 and call(B=0, D=128, C=4) == 0
    assert call(B=0, cur=None) == -22                       # ... but its arguments are checked


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    cur, look, T, K = torch.ones(1, 8, 6, 6), torch.ones(1, 2, 8, 6, 6), torch.eye(4).expand(1, 2, 4, 4), torch.eye(4)[None]
    bins = matching.depth_bins(0.1, 2.0, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cost_volume(cur, look, T, K, K, bins)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        matching.match_features(cur, look, T, K, K, bins)
    # the pure-torch helpers run anywhere
    cv = torch.tensor([[[[1.0, 0.0]], [[2.0, 3.0]]]])                       # [1,2,1,2]
    assert matching.compute_confidence_mask(cv).tolist() == [[[1.0, 0.0]]]
    assert matching.compute_confidence_mask(cv, 1).tolist() == [[[0.0, 1.0]]]
    d = matching.indices_to_disparity(torch.tensor([[[0, 3]]]), bins)
    assert d.shape == (1, 1, 2) and d.dtype == torch.float32 and torch.equal(d, 1 / bins[[0, 3]].view(1, 1, 2))
