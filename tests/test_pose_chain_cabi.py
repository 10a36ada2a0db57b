"""pd_pose_chain, host side (no GPU): the exported symbol, its signature against the header, every refusal that is decided
before the device is touched -- the pointers are dummies that are never dereferenced -- and the Python layer's refusals."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from polardepth import _lib, ops

HEADER = os.path.join(ROOT, "include", "polardepth.h")
P = ctypes.c_void_p(64)


def test_symbol_signature_and_header():
    src = open(HEADER).read()
    so = ctypes.CDLL(_lib.lib.path)
    assert hasattr(so, "pd_pose_chain") and "pd_pose_chain" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["pd_pose_chain"]
    decl = re.search(r"\bint\s+pd_pose_chain\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert decl, "pd_pose_chain is not declared in the header"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert [p.rsplit(" ", 1)[-1].lstrip("*") for p in params] == ["axisangle", "translation", "present", "init", "rel",
                                                                  "rel_inv", "L", "N", "direction", "stream"]
    want = [ctypes.c_void_p if "*" in p else ctypes.c_int for p in params]
    assert res is ctypes.c_int and args == want
    m = re.search(r"#define\s+PD_POSE_CHAIN_MAX_LINKS\s+(\d+)", src)
    assert m and int(m.group(1)) == 8 == ops.POSE_CHAIN_MAX_LINKS


def test_refusals_need_no_gpu():
    L = _lib.lib
    err = L.pd_last_error

    def call(aa=P, tr=P, present=P, init=P, rel=P, rel_inv=P, links=3, N=4, direction=-1):
        return L.pd_pose_chain(aa, tr, present, init, rel, rel_inv, links, N, direction, None)

    for name in ("aa", "tr", "rel", "rel_inv"):
        assert call(**{name: None}) == -22 and b"must not be null" in err(), name
    for links in (0, -1, 9, 1 << 20):
        assert call(links=links) == -22 and b"links" in err(), links
    for n in (0, -1, -(1 << 31)):
        assert call(N=n) == -22 and b"item count" in err(), n
    for d in (0, 2, -2, 64):
        assert call(direction=d) == -22 and b"direction" in err(), d
    # the optional pointers do not rescue a bad argument
    assert call(present=None, init=None, links=0) == -22 and call(present=None, init=None, direction=0) == -22


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    a = torch.zeros(2, 3, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.pose_chain(a, a)
    meta = lambda *s: torch.empty(*s, device="meta")           # shapes are judged before anything is launched
    cuda_like = lambda *s: _FakeCuda(meta(*s))
    good = cuda_like(2, 3, 3)
    for aa, tr, kw in ((cuda_like(2, 3), good, {}), (good, cuda_like(2, 3, 4), {}), (good, cuda_like(3, 3, 3), {}),
                       (cuda_like(9, 3, 3), cuda_like(9, 3, 3), {}), (cuda_like(0, 3, 3), cuda_like(0, 3, 3), {}),
                       (good, good, {"present": cuda_like(2, 4)}), (good, good, {"present": cuda_like(3, 2)}),
                       (good, good, {"init": cuda_like(3, 4, 3)}), (good, good, {"init": cuda_like(2, 4, 4)}),
                       (good, good, {"direction": 0}), (good, good, {"direction": 2})):
        with pytest.raises(ValueError, match="pose_chain"):
            ops.pose_chain(aa, tr, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.pose_chain(good, good, present=torch.zeros(2, 3))


class _FakeCuda:
    """A tensor stand-in that says it lives on the device: enough for the checks that come before the launch."""

    def __init__(self, t):
        self._t = t
        self.is_cuda = True
        self.shape = t.shape

    def dim(self):
        return self._t.dim()
