"""The four convolution wrappers of polardepth.functional -- conv_bias, conv_bias_act, padded_conv, reflect_conv_act -- through
autograd: y, dx, dw, db against PyTorch fp32 autograd on the CPU, at the smallest shapes at which each data-gradient route
(zero padding, stride-2 parity split, reflect border strips, reflect fold, 16-channel halo kernel) can still go wrong.

Tolerances are those of test_conv_gpu.py for the same kernels (max error over max magnitude): 2e-5 without an activation,
3e-5 with one; the contractions here (K <= 288) are shorter than the ones that hold them there.
tools/conv_nodes_ab.py replays CASES through `run` to compare two checkouts call by call."""
import functools

import pytest
import torch
import torch.nn.functional as F

from polardepth import functional as PF
from polardepth import ops

pytestmark = pytest.mark.gpu

CL = torch.channels_last
ACTS = {ops.ACT_NONE: lambda t: t, ops.ACT_RELU: F.relu, ops.ACT_ELU: F.elu, ops.ACT_SIGMOID: torch.sigmoid}

# wrapper, reflect, k, stride, pad, C, Co, H, W, act, data-gradient route (N = 2 everywhere)
CASES = {
    "zero_1x1_qkv": ("conv_bias", False, 1, 1, 0, 8, 8, 3, 5, ops.ACT_NONE, "zero"),
    "zero_3x3": ("conv_bias_act", False, 3, 1, 1, 8, 12, 5, 7, ops.ACT_RELU, "zero"),
    "zero_3x3_s2_odd": ("conv_bias_act", False, 3, 2, 1, 8, 12, 5, 7, ops.ACT_ELU, "zero"),
    "zero_3x3_s2_phases": ("conv_bias_act", False, 3, 2, 1, 32, 32, 4, 6, ops.ACT_NONE, "phases"),
    "zero_5x5": ("padded_conv", False, 5, 1, 2, 8, 4, 3, 4, ops.ACT_SIGMOID, "zero"),
    "reflect_3x3_border": ("reflect_conv_act", True, 3, 1, 1, 8, 4, 2, 2, ops.ACT_ELU, "border"),
    "reflect_3x3_fold": ("reflect_conv_act", True, 3, 1, 1, 8, 4, 2, 2, ops.ACT_ELU, "fold_off"),
    "reflect_3x3_co128": ("reflect_conv_act", True, 3, 1, 1, 32, 128, 3, 2, ops.ACT_RELU, "fold"),
    "reflect_3x3_halo16": ("reflect_conv_act", True, 3, 1, 1, 16, 16, 2, 2, ops.ACT_ELU, "halo"),
    "reflect_3x3_co1": ("reflect_conv_act", True, 3, 1, 1, 8, 1, 3, 3, ops.ACT_SIGMOID, "fold"),
    "reflect_5x5": ("padded_conv", True, 5, 1, 2, 8, 4, 3, 4, ops.ACT_NONE, "fold"),
}
N = 2


def _close(got, ref, tol):
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


def _tol(name):
    return 2e-5 if CASES[name][9] == ops.ACT_NONE else 3e-5


@functools.lru_cache(maxsize=None)
def _data(name):
    _, _, k, _, _, C, Co, H, W, _, _ = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 41)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5
    b = torch.randn(Co, generator=g) * 0.3
    return x, w, b, g


@functools.lru_cache(maxsize=None)
def reference(name, bias=True, const_dy=None):
    """(y, dx, dw, db, dy) of the PyTorch fp32 CPU autograd; const_dy: every element of the upstream gradient is that value."""
    _, reflect, _, s, p, _, _, _, _, act, _ = CASES[name]
    x, w, b, g = _data(name)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    xp = F.pad(xr, (p, p, p, p), mode="reflect") if reflect else xr
    y = ACTS[act](F.conv2d(xp, wr, br, stride=s, padding=0 if reflect else p))
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)) if const_dy is None else torch.full(y.shape, const_dy)
    y.backward(dy)
    return y.detach(), xr.grad, wr.grad, br.grad if bias else None, dy


def run(name, bias=True, freeze=(), x_grad=True, dy="nchw", const_dy=None, passes=1):
    """One forward and `passes` backward passes (each through a fresh graph) of case `name` on the GPU, through its public
    wrapper.  Returns (y, dx, dw, db, labels, shapes): CPU tensors (None where there is no gradient) and ops.PROFILE's
    kernel labels and shape tuples.  dy: layout in which the upstream gradient arrives."""
    wrapper, reflect, k, s, p, C, Co, H, W, act, _ = CASES[name]
    x, w, b, _ = _data(name)
    conv = torch.nn.Conv2d(C, Co, k, stride=s, padding=p, bias=bias)
    conv.weight.data = w.clone()
    if bias:
        conv.bias.data = b.clone()
    conv = conv.cuda()
    conv.weight.data = conv.weight.data.contiguous(memory_format=CL)
    conv.weight.requires_grad_("weight" not in freeze)
    if bias:
        conv.bias.requires_grad_("bias" not in freeze)
    xc = x.cuda().contiguous(memory_format=CL).requires_grad_(x_grad)
    gy = reference(name, bias, const_dy)[4].cuda()
    ops.PROFILE = []
    try:
        for _ in range(passes):
            if wrapper == "conv_bias":
                y = PF.conv_bias(xc, conv)
            elif wrapper == "conv_bias_act":
                y = PF.conv_bias_act(xc, conv, act)
            elif wrapper == "padded_conv":
                y = PF.padded_conv(xc, conv, p, reflect=reflect, act=act)
            else:
                y = PF.reflect_conv_act(xc, conv, act)
            if dy == "nchw":
                y.backward(gy.contiguous())
            elif dy == "channels_last":
                y.backward(gy.contiguous(memory_format=CL))
            elif dy == "expanded":
                (y.sum() * const_dy).backward()
            else:       # a channel slice of a wider channels_last buffer
                wide = torch.full((N, Co + 8, y.shape[2], y.shape[3]), const_dy, device="cuda").contiguous(memory_format=CL)
                y.backward(wide[:, 4:4 + Co])
        PF.sync_wgrad_stream()
        torch.cuda.synchronize()
        labels, shapes = [q[0] for q in ops.PROFILE], [q[4] for q in ops.PROFILE]
    finally:
        ops.PROFILE = None
    cpu = lambda t: None if t is None else t.detach().cpu()
    return cpu(y), cpu(xc.grad), cpu(conv.weight.grad), cpu(conv.bias.grad) if bias else None, labels, shapes


def _border_switch(monkeypatch, name):
    if CASES[name][10] == "fold_off":
        monkeypatch.setattr(PF, "USE_REFLECT_BORDER", False)
    else:
        assert PF.USE_REFLECT_BORDER


@pytest.mark.parametrize("name", list(CASES))
def test_wrapper_matches_cpu_autograd_and_accumulates(name, monkeypatch):
    """y, dx, dw, db of every case; the route the data gradient took, read from the profiler's labels and shapes; and a second
    backward through a fresh graph, which adds to the same .grad: twice the first."""
    _, _, k, _, p, C, Co, H, W, _, route = CASES[name]
    _border_switch(monkeypatch, name)
    tol = _tol(name)
    ref = reference(name)
    y, dx, dw, db, labels, shapes = run(name)
    for got, want in zip((y, dx, dw, db), ref):
        _close(got, want, tol)
    dgrad_hw = [s[3:5] for s in shapes if s[0] == "dgrad"]
    if route == "phases":
        assert "conv_dgrad_s2_phases" in labels, labels
    elif route == "border":         # pad-1 data gradient on the image's own grid (+ pd_reflect_dgrad_border)
        assert dgrad_hw == [(H, W)], shapes
    elif route in ("fold", "fold_off"):     # data gradient on the padded grid (+ the fold pass)
        assert dgrad_hw == [(H + 2 * p, W + 2 * p)], shapes
    elif route == "halo":
        assert labels.count("conv16_halo_kernel") == 2, labels       # forward and data gradient took the halo kernel
        assert labels.count("conv16_wgrad_kernel") == 1, labels      # ... and the weight / bias gradient its sibling
    y2, dx2, dw2, db2, _, _ = run(name, passes=2)
    assert torch.equal(y2, y)
    for got, want in zip((dx2, dw2, db2), ref[1:4]):
        _close(got, 2 * want, tol)


VARIANT_CASES = ["zero_3x3", "reflect_3x3_border"]


@pytest.mark.parametrize("name", VARIANT_CASES)
def test_missing_and_frozen_parameters(name):
    tol = _tol(name)
    y, dx, dw, db, _, _ = run(name, bias=False)
    ref = reference(name, bias=False)
    for got, want in zip((y, dx, dw), ref):
        _close(got, want, tol)
    assert db is None
    ref = reference(name)
    y, dx, dw, db, _, _ = run(name, freeze=("bias",))
    assert db is None
    for got, want in zip((y, dx, dw), ref):
        _close(got, want, tol)
    y, dx, dw, db, _, _ = run(name, freeze=("weight",))
    assert dw is None                       # no .grad appears on a frozen weight
    _close(dx, ref[1], tol)
    y, dx, dw, db, _, _ = run(name, x_grad=False)
    assert dx is None
    _close(dw, ref[2], tol)
    _close(db, ref[3], tol)


@pytest.mark.parametrize("name", VARIANT_CASES)
def test_upstream_gradient_layouts_give_the_same_bits(name):
    """Dense NCHW, channels_last, expanded (a scaled y.sum()) and a channel slice of a wider channels_last buffer carry the
    same values: the node's results do not depend on the layout, bit for bit."""
    ref = reference(name, const_dy=0.5)
    first = run(name, dy="nchw", const_dy=0.5)
    for got, want in zip(first[1:4], ref[1:4]):
        _close(got, want, _tol(name))
    for layout in ("channels_last", "expanded", "slice"):
        other = run(name, dy=layout, const_dy=0.5)
        for a, b in zip(first[:4], other[:4]):
            assert torch.equal(a, b), layout
