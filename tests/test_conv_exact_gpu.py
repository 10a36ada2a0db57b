"""Every convolution kernel of K2, bit for bit, on exactly summable inputs (tests/conv_cases.py: the rows, the two input classes,
the fp64 references; tests/test_conv_cases.py proves on the CPU that each row launches the instantiation it names and that its
data is exactly summable).

For every row the device result must be torch.equal to the fp64 reference rounded to fp32 -- whatever the kernel's summation
order, on the fp32 MFMA, the three-way bf16 split and the single-bf16 mode alike.  The one exception is the negative branch of
ELU (|got - expm1(z)| <= 3e-5, the suite's ELU tolerance; z >= 0 must equal z).

Every output sits in a sentinel-filled wider buffer that must be intact afterwards: forward-like outputs with a row stride of
Cout + 8 and one image row of guard pixels in front and behind, dW and dbias between 8 guard floats, BatchNorm partials
pre-filled with NaN (every row must be written, every entry an integer, the rows summing in fp64 exactly to the reference
column sums and sums of squares).  The operands must be unchanged after the call.  Calls go through polardepth.ops where it
can express the row (forward without statistics, weight gradients, the stride-2 parity launches, reflect_conv_act) and through
the C ABI otherwise (data gradients and statistics: ops allocates those outputs itself; pd_conv2d_rect; pd_conv16)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from polardepth import ops
from polardepth._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))       # the fp64 references dominate
SENT = 1.5e30
FWD_LIKE = ("fwd", "dgrad", "dgrad+addend", "rect")


def _exact(got, ref, what):
    got, ref = got.detach().cpu(), ref.detach().cpu().double().to(torch.float32)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not torch.equal(got, ref):
        bad = got != ref
        k = int(bad.flatten().to(torch.int64).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx} (flat {k}): "
                             f"got {got.flatten()[k].item()!r} ref {ref.flatten()[k].item()!r}")


def _nhwc(t):
    """fp64 [N, C, H, W] -> fp32 device tensor of the same logical shape in dense NHWC storage (canonical strides)."""
    return t.float().permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


def _act(row, t):
    return t.float().contiguous().cuda() if row.nchw else _nhwc(t)


def _vec(t):
    return None if t is None else t.float().cuda()


class Guarded:
    """[rows, cols] window with row stride ld inside a sentinel-filled buffer, `guard` floats in front and behind."""

    def __init__(self, rows, cols, ld, guard):
        self.rows, self.cols, self.ld, self.guard = rows, cols, ld, guard
        self.buf = torch.full((2 * guard + rows * ld,), SENT, dtype=torch.float32, device="cuda")

    @property
    def body(self):
        return self.buf[self.guard:self.guard + self.rows * self.ld].view(self.rows, self.ld)

    @property
    def win(self):
        return self.body[:, :self.cols]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * self.guard)

    def nchw(self, N, Ho, Wo):
        return self.body.view(N, Ho, Wo, self.ld)[..., :self.cols].permute(0, 3, 1, 2)

    def assert_intact(self, what):
        b = self.buf.clone()
        b[self.guard:self.guard + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = SENT
        stray = (b != SENT).nonzero().flatten()
        assert stray.numel() == 0, f"{what}: {stray.numel()} stray writes, first at float {int(stray[0]) - self.guard} from the output's start"


def _unchanged(pairs, what):
    for name, dev, host in pairs:
        if dev is not None:
            assert torch.equal(dev.cpu(), host), f"{what}: operand {name} changed"


def _strides(row):
    N, C, H, W = row.N, row.C, row.H, row.W
    return (C * H * W, W, 1, H * W) if row.nchw else (H * W * C, W * C, C, 1)      # sN, sH, sW, sC


# ====================================================================================================== forward-like
@pytest.mark.parametrize("v", [v for v in cc.variants() if v[0].call in FWD_LIKE], ids=cc.vid)
def test_forward_and_data_gradient_bit_exact(v):
    row, cls, role = v
    d = cc.case(row, cls, role)
    what = cc.vid(v)
    N, C, H, W, Co = row.N, row.C, row.H, row.W, row.Co
    (Ho, Wo), M, ld = row.grid, row.M, row.Co + 8
    x, w = _act(row, d["x"]), _nhwc(d["w"])
    bias, scale = _vec(d["bias"]), _vec(d["scale"])
    addbuf = add = None
    if d["addend"] is not None:
        ld_add = Co + 4 if row.addend == "view" else Co
        addbuf = torch.full((M, ld_add), SENT, dtype=torch.float32, device="cuda")
        addbuf[:, :Co] = d["addend"].float().permute(0, 2, 3, 1).reshape(M, Co).cuda()
        add = addbuf.clone()
    stats = None
    if d["stats"]:
        stats = torch.full((lib.pd_conv2d_stats_rows(M, Co), Co, 2), float("nan"), dtype=torch.float32, device="cuda")
    out = Guarded(M, Co, ld, Wo * ld)
    keep = [("x", x, x.cpu().clone()), ("w", w, w.cpu().clone()), ("bias", bias, None if bias is None else bias.cpu().clone()),
            ("addend", addbuf, None if add is None else add.cpu())]
    act = d["act"]
    sN, sH, sW, sC = _strides(row)
    sub, div = row.affine if row.affine is not None else (0.0, 1.0)
    if row.call == "fwd" and stats is None:
        with ops.conv_flags(conv=row.flags):
            ops.conv2d_fwd(x, w, bias, stride=row.stride, pad=row.ph, mode=row.mode, act=act, affine=row.affine, out=out.nchw(N, Ho, Wo),
                           out_hw=row.out_hw, out_scale=scale)
    elif row.call == "rect":
        check(lib.pd_conv2d_rect(ptr(x), ptr(w), out.ptr, N, H, W, C, sN, sH, sW, sC, Ho, Wo, Co, row.KH, row.KW, row.ph, row.pw, row.mode,
                                 ld, row.flags, stream_ptr()), what)
    elif addbuf is not None:
        check(lib.pd_conv2d_add(ptr(x), ptr(w), ptr(addbuf), addbuf.stride(0), out.ptr, N, H, W, C, sN, sH, sW, sC, Ho, Wo, Co, row.KH, row.KW,
                                row.stride, row.ph, row.mode, ld, row.flags, stream_ptr()), what)
    else:
        check(lib.pd_conv2d(ptr(x), ptr(w), ptr(bias), ptr(scale), out.ptr, ptr(stats), N, H, W, C, sN, sH, sW, sC, Ho, Wo, Co, row.KH, row.KW,
                            row.stride, row.ph, row.mode, act, int(row.affine is not None), sub, div, ld, row.flags, stream_ptr()), what)
    torch.cuda.synchronize()
    got = out.win.cpu().view(N, Ho, Wo, Co).permute(0, 3, 1, 2)
    if act == cc.ACT_ELU:
        z = d["z"]
        pos = z >= 0
        _exact(torch.where(pos, got, torch.zeros(())), torch.where(pos, z, torch.zeros((), dtype=z.dtype)), what + " (ELU, z >= 0)")
        err = torch.where(pos, torch.zeros((), dtype=z.dtype), (got.double() - torch.expm1(z)).abs())
        assert err.max() <= cc.ELU_TOL, f"{what} (ELU, z < 0): max err {err.max().item():.3e}"
    else:
        _exact(got, d["y"], what)
    out.assert_intact(what)
    _unchanged(keep, what)
    if stats is not None:
        s = stats.cpu().double()
        assert torch.isfinite(s).all(), f"{what}: {int((~torch.isfinite(s)).sum())} statistics entries not written"
        assert torch.equal(s, s.round()), f"{what}: a partial sum that is no integer"
        z = d["z"]
        _exact(s.sum(0)[:, 0].float(), z.sum((0, 2, 3)), what + " column sums")
        _exact(s.sum(0)[:, 1].float(), (z * z).sum((0, 2, 3)), what + " column sums of squares")
        assert torch.equal(s.sum(0)[:, 0], z.sum((0, 2, 3))) and torch.equal(s.sum(0)[:, 1], (z * z).sum((0, 2, 3)))


# ====================================================================================================== weight gradients
@pytest.mark.parametrize("v", [v for v in cc.variants() if v[0].call == "wgrad"], ids=cc.vid)
def test_weight_gradient_bit_exact(v):
    row, cls, role = v
    d = cc.case(row, cls, role)
    what = cc.vid(v)
    Co, C, KH, KW = row.Co, row.C, row.KH, row.KW
    x, dy = _act(row, d["x"]), _nhwc(d["w"])
    keep = [("x", x, x.cpu().clone()), ("dy", dy, dy.cpu().clone())]
    dwb, dbb = Guarded(1, Co * row.K, Co * row.K, 8), Guarded(1, Co, Co, 8)
    dw = dwb.win.view(Co, KH, KW, C).permute(0, 3, 1, 2)
    db = dbb.win.view(Co) if row.bias else None
    for rep in range(2 if (row.accumulate and cls == "E8") else 1):
        with ops.conv_flags(wgrad=row.flags):
            ops.conv2d_wgrad(x, dy, (Co, C, KH, KW), stride=row.stride, pad=row.ph, mode=row.mode, affine=row.affine, dw=dw, dbias=db,
                             accumulate=rep == 1)
        torch.cuda.synchronize()
        _exact(dw.cpu(), d["dw"] * (rep + 1), f"{what} dw (pass {rep})")
        if db is not None and not (cls == "S" and role == "wx"):
            _exact(db.cpu(), d["db"] * (rep + 1), f"{what} dbias (pass {rep})")
    dwb.assert_intact(what + " dw")
    dbb.assert_intact(what + " dbias")
    _unchanged(keep, what)


# ====================================================================================================== 16-channel tail
@pytest.mark.parametrize("v", [v for v in cc.variants() if v[0].call == "conv16"], ids=cc.vid)
def test_conv16_bit_exact(v):
    row, cls, role = v
    d = cc.case(row, cls, role)
    what = cc.vid(v)
    N, C, H, W, Co = row.N, row.C, row.H, row.W, row.Co
    (Ho, Wo), ld = row.grid, row.Co + 8
    x, w, bias = _nhwc(d["x"]), _nhwc(d["w"]), _vec(d["bias"])
    keep = [("x", x, x.cpu().clone()), ("w", w, w.cpu().clone())]
    out = Guarded(row.M, Co, ld, Wo * ld)
    check(lib.pd_conv16(ptr(x), ptr(w), ptr(bias), out.ptr, N, H, W, C, H * W * C, W * C, C, Ho, Wo, Co, ld, row.c16_mode, d["act"],
                        stream_ptr()), what)
    torch.cuda.synchronize()
    got = out.win.cpu().view(N, Ho, Wo, Co).permute(0, 3, 1, 2)
    if d["act"] == cc.ACT_ELU:
        z = d["z"]
        pos = z >= 0
        _exact(torch.where(pos, got, torch.zeros(())), torch.where(pos, z, torch.zeros((), dtype=z.dtype)), what + " (ELU, z >= 0)")
        assert torch.where(pos, torch.zeros((), dtype=z.dtype), (got.double() - torch.expm1(z)).abs()).max() <= cc.ELU_TOL, what
    else:
        _exact(got, d["y"], what)
    out.assert_intact(what)
    _unchanged(keep, what)


@pytest.mark.parametrize("v", [v for v in cc.variants() if v[0].call == "conv16_wgrad"], ids=cc.vid)
def test_conv16_weight_gradient_bit_exact(v):
    row, cls, role = v
    d = cc.case(row, cls, role)
    what = cc.vid(v)
    N, C, H, W = row.N, row.C, row.H, row.W
    x, dy = _nhwc(d["x"]), _nhwc(d["w"])
    keep = [("x", x, x.cpu().clone()), ("dy", dy, dy.cpu().clone())]
    dwb, dbb = Guarded(1, 16 * row.K, 16 * row.K, 8), Guarded(1, 16, 16, 8)
    ws = torch.empty(lib.pd_conv16_wgrad_workspace(C), dtype=torch.uint8, device="cuda")
    for rep in range(2 if (row.accumulate and cls == "E8") else 1):
        check(lib.pd_conv16_wgrad(ptr(x), ptr(dy), dwb.ptr, dbb.ptr, ptr(ws), ws.numel(), N, H, W, C, H * W * C, W * C, C, 16, rep,
                                  stream_ptr()), what)
        torch.cuda.synchronize()
        _exact(dwb.win.cpu().view(16, 3, 3, C).permute(0, 3, 1, 2), d["dw"] * (rep + 1), f"{what} dw (pass {rep})")
        if not (cls == "S" and role == "wx"):
            _exact(dbb.win.cpu().view(16), d["db"] * (rep + 1), f"{what} dbias (pass {rep})")
    dwb.assert_intact(what + " dw")
    dbb.assert_intact(what + " dbias")
    _unchanged(keep, what)


# ====================================================================================================== composite routes
def test_stride2_data_gradient_by_parity_classes_bit_exact():
    """ops.conv2d_dgrad at stride 2: pd_dgrad_s2_filters, four pd_conv2d_rect launches, pd_interleave4 (ops allocates dX: no
    guard band here; the masked transposed gather of the same gradient is a row of its own)."""
    row = next(r for r in cc.ROWS if r.call == "s2 phases")
    d = cc.case(row)
    assert ops.USE_S2_PHASES
    dy = _nhwc(d["x"])
    w_fwd = _nhwc(d["w"].permute(1, 0, 2, 3))            # the row holds the data-gradient operand [Ci, Co, kh, kw]
    ops.PROFILE = []
    try:
        dx = ops.conv2d_dgrad(dy, w_fwd, row.grid, stride=2, pad=1)
        torch.cuda.synchronize()
        labels = [p[0] for p in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert labels == ["conv_dgrad_s2_phases"], labels
    _exact(dx.cpu(), d["y"], row.id)
    assert torch.equal(dy.cpu(), d["x"].float())


@pytest.mark.parametrize("border", [True, False])
def test_reflect_conv_backward_bit_exact(border):
    """functional.reflect_conv_act with act = none: the pad-1 data gradient + pd_reflect_dgrad_border | the padded-grid data
    gradient + pd_reflect_fold, against the fp64 autograd gradient of ReflectionPad2d(1) + conv3x3."""
    from polardepth import functional as PF
    row = next(r for r in cc.ROWS if r.call == "reflect bwd")
    d = cc.case(row)
    g = torch.Generator().manual_seed(7)
    gy = torch.randint(-3, 4, tuple(d["z"].shape), generator=g).double()
    xr = d["x"].clone().requires_grad_(True)
    (F.conv2d(F.pad(xr, (1, 1, 1, 1), mode="reflect"), d["w"], d["bias"]) * gy).sum().backward()
    assert xr.grad.abs().max() < 2 ** 24
    conv = torch.nn.Conv2d(row.C, row.Co, 3).cuda()
    conv.weight.data = _nhwc(d["w"])
    conv.bias.data = _vec(d["bias"])
    xc = _nhwc(d["x"]).requires_grad_(True)
    old = PF.USE_REFLECT_BORDER
    PF.USE_REFLECT_BORDER = border
    try:
        y = PF.reflect_conv_act(xc, conv, ops.ACT_NONE)
        (y * _nhwc(gy)).sum().backward()
        PF.sync_wgrad_stream()
        torch.cuda.synchronize()
    finally:
        PF.USE_REFLECT_BORDER = old
    _exact(y.detach().cpu(), d["y"], row.id + " y")
    _exact(xc.grad.cpu(), xr.grad, row.id + f" dx (border kernel: {border})")
