"""Low-level tensor ops on the HIP library (no autograd here; see functional.py).

Activations are fp32, logically NCHW, physically NHWC (torch.channels_last); weights are
[Cout,Cin,kh,kw] logically and [Cout][kh][kw][Cin] physically (channels_last), i.e. exactly the
operand layout of the implicit-GEMM kernels -- no repacking on the forward path.
"""
import os

import torch

from ._lib import lib, check, ptr, stream_ptr

MODE_ZERO, MODE_REFLECT, MODE_TRANSPOSED = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3
CL = torch.channels_last
PROFILE = None      # bench.py sets this to a list: (kernel label, algorithmic flops, start event, end event, shape)

# Kernel family / arithmetic of the convolutions: the `flags` word of pd_conv2d* / pd_conv2d_wgrad (include/polardepth.h).
# The library reads no environment variable; this module owns the knobs and reads them ONCE, at import:
#   PD_CONV_X3=0    forward / data gradient on the fp32 MFMA only      PD_WGRAD_X3C=0   weight gradients likewise
#   PD_CONV_HALO=0  bf16-split forward / data gradient through conv_igemm_x3_kernel also where the halo-tile kernel fits
#   PD_WGRAD_ROLL=0 3x3 weight gradients with one filter row per workgroup also where the rolling-row kernel fits
# Tests and bench.py switch families in-process by assigning CONV_FLAGS / WGRAD_FLAGS (or `with conv_flags(...)`).
CONV_AUTO, CONV_FP32_MFMA, CONV_BF16X3, CONV_WGRAD_SPLIT_IN_REGS, CONV_GENERAL_KERNELS, CONV_X3_IM2COL = 0, 1, 2, 4, 8, 16
CONV_WGRAD_ROW_WORKGROUPS = 32        # one filter row per workgroup also where the rolling-row weight-gradient kernel fits (A/B, tests)
# Opt-in bf16 training mode (PD_CONV_BF16): operands rounded once to bf16, one bf16 MFMA per product, fp32 storage and epilogue,
# on the layers the single-bf16 kernels take (pd_conv2d_uses_bf16 / pd_conv2d_wgrad_uses_bf16); no environment variable selects
# it -- `with conv_flags(conv=CONV_BF16, wgrad=CONV_BF16)` or a Trainer with opt.bf16 = True.  The autograd functions fix it
# when their forward runs (functional.py: ctx.conv_bf16) and hand it to their backward's launches.
CONV_BF16 = 128
CONV_FLAGS = (CONV_FP32_MFMA if os.environ.get("PD_CONV_X3", "1") == "0" else       # pd_conv2d, _add, _rect
              CONV_X3_IM2COL if os.environ.get("PD_CONV_HALO", "1") == "0" else CONV_AUTO)   # PD_CONV_HALO=0: the per-tap gather kernel everywhere
WGRAD_FLAGS = (CONV_FP32_MFMA if os.environ.get("PD_WGRAD_X3C", "1") == "0" else     # pd_conv2d_wgrad
               CONV_X3_IM2COL if os.environ.get("PD_CONV_HALO", "1") == "0" else
               CONV_WGRAD_ROW_WORKGROUPS if os.environ.get("PD_WGRAD_ROLL", "1") == "0" else CONV_AUTO)   # PD_WGRAD_ROLL=0: one filter row per workgroup


class conv_flags:
    """Context manager: run the enclosed convolutions with the given flags (None = leave that entry point's word alone)."""

    def __init__(self, conv=None, wgrad=None):
        self.new = (conv, wgrad)

    def __enter__(self):
        global CONV_FLAGS, WGRAD_FLAGS
        self.old = (CONV_FLAGS, WGRAD_FLAGS)
        if self.new[0] is not None:
            CONV_FLAGS = int(self.new[0])
        if self.new[1] is not None:
            WGRAD_FLAGS = int(self.new[1])
        return self

    def __exit__(self, *exc):
        global CONV_FLAGS, WGRAD_FLAGS
        CONV_FLAGS, WGRAD_FLAGS = self.old
        return False


def conv_bf16_mode():
    """(forward / data gradient, weight gradient) bf16 bits of the flag words as they stand: what a convolution's forward records
    for its backward."""
    return (bool(CONV_FLAGS & CONV_BF16), bool(WGRAD_FLAGS & CONV_BF16))


def _with_bf16(word, bf16):
    """`word` with its PD_CONV_BF16 bit set to `bf16` (None: the word as it stands).  A word that asks for another arithmetic
    (fp32 MFMA, forced bf16 split) keeps it: the bit would make the word invalid."""
    if bf16 is None:
        return word
    if bf16 and not (word & (CONV_FP32_MFMA | CONV_BF16X3)):
        return word | CONV_BF16
    return word & ~CONV_BF16


def _profiled(label, flops, fn, shape=None):
    if PROFILE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    PROFILE.append((label, flops, e0, e1, shape))
    return r


# pd_conv2d_route's family code -> profiler label (the bf16-split kernels' labels name their default tile)
_IGEMM_LABELS = ("conv_igemm_kernel<{bm},{bn},{gather}>", "conv_igemm_uni_kernel<{bm},{bn}>", "conv_igemm_x3_kernel<{bm},{bn}>",
                 "conv_halo_x3_kernel<8x32,64>", "conv_halo_bf16_kernel<8x32,64>")


def _igemm_label(M, Co, vec, kind, C=0, KH=1, KW=1, stride=1, pad=0, mode=0, act=ACT_NONE, out_scale=False, out_hw=(0, 0),
                 flags=None):
    """Profiler label = the kernel pd_conv2d launches for this call, as the library's own routing answers (pd_conv2d_route)."""
    flags = CONV_FLAGS if flags is None else flags
    if not vec:     # an input the 16-byte path cannot read (strided channels, affine taps): the general kernel's scalar gather
        flags = CONV_FP32_MFMA | CONV_GENERAL_KERNELS
    r = lib.pd_conv2d_route(M, Co, C, KH, KW, stride, pad, mode, act, int(out_scale), out_hw[0], out_hw[1], flags)
    return _IGEMM_LABELS[r & 15].format(bm=r >> 12, bn=(r >> 4) & 255, gather="vec" if vec else "scalar")


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("polardepth ops need CUDA(HIP) tensors; there is no CPU fallback")


def empty_nhwc(n, c, h, w, device):
    return torch.empty((n, c, h, w), dtype=torch.float32, device=device, memory_format=CL)


def is_nhwc(t):
    n, c, h, w = t.shape
    return t.stride() == (h * w * c, 1, w * c, c) or t.is_contiguous(memory_format=CL)


def as_nhwc(t):
    return t if is_nhwc(t) else t.contiguous(memory_format=CL)


def weight_cl(w):
    """Weight in [Cout][kh][kw][Cin] storage."""
    return w if w.is_contiguous(memory_format=CL) else w.contiguous(memory_format=CL)


def conv_out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def _quad_strides(t):
    """Channel stride 1 and every other stride a whole quad: what the 16-byte gathers of the kernels need of an operand."""
    sN, sC, sH, sW = t.stride()
    return sC == 1 and sN % 4 == 0 and sH % 4 == 0 and sW % 4 == 0


def _conv16_shape(Co, C, KH, KW, stride):
    """The layer shape of the halo-tile kernels of the 16-channel decoder tail (pd_conv16, pd_conv16_wgrad)."""
    return USE_CONV16 and Co == 16 and C in (16, 32) and KH == 3 and KW == 3 and stride == 1


def conv2d_fwd(x, w, bias=None, stride=1, pad=0, mode=MODE_ZERO, act=ACT_NONE, want_stats=False,
               affine=None, out=None, out_hw=None, out_scale=None, alg_k=None):
    """y = act(conv(x, w) [* out_scale] + bias).  x: [N,C,H,W] any strides; returns channels_last [N,Co,Ho,Wo].

    out_scale: optional fp32 [Co] multiplier of the accumulator (an inference-mode BatchNorm folded into the epilogue).

    want_stats -> also returns the per-workgroup BatchNorm partials [rows, Co, 2] (sum, sum of squares
    of the pre-activation output).  affine=(sub, div) applies (x-sub)/div to in-bounds input taps.
    out: optional pre-allocated NHWC tensor whose channel slice [:, c0:c0+Co] receives the result
    (pass the sliced view; its channel stride must be 1).
    alg_k: algorithmic contraction length for the profiler's FLOP count when it differs from C*KH*KW (the
    space-to-depth stems execute K = 64*C for an algorithmic 7x7 filter: 49*C).
    """
    _require_cuda(x, w, bias, out_scale)
    global FWD_EPOCH
    FWD_EPOCH += 1
    N, C, H, W = x.shape
    Co, Ci, KH, KW = w.shape
    assert Ci == C, f"channel mismatch {Ci} vs {C}"
    w = weight_cl(w)
    Ho, Wo = conv_out_size(H, KH, stride, pad), conv_out_size(W, KW, stride, pad)
    if out_hw is not None:          # leading part of the output grid only (asymmetric padding)
        assert out_hw[0] <= Ho and out_hw[1] <= Wo
        Ho, Wo = out_hw
    if out is None:
        out = empty_nhwc(N, Co, Ho, Wo, x.device)
    assert out.shape == (N, Co, Ho, Wo) and out.stride(1) == 1
    ldy = out.stride(3)
    assert out.stride(2) == Wo * ldy and out.stride(0) == Ho * Wo * ldy
    stats = None
    if want_stats:
        rows = lib.pd_conv2d_stats_rows(N * Ho * Wo, Co)
        stats = torch.empty((rows, Co, 2), dtype=torch.float32, device=x.device)
    sub, div = (affine if affine is not None else (0.0, 1.0))
    sN, sC, sH, sW = x.stride()
    vec = C % 4 == 0 and sC == 1 and affine is None
    shape = ("fwd", N, C, H, W, Co, KH, stride, mode)
    if (_conv16_shape(Co, C, KH, KW, stride) and mode == MODE_REFLECT and pad == 1 and vec and _quad_strides(x)
            and not want_stats and out_scale is None and act in (ACT_NONE, ACT_ELU) and out_hw is None and H >= 2 and W >= 2):
        # 16-channel decoder tail: halo-tile kernel (every input pixel staged once instead of once per tap)
        _profiled("conv16_halo_kernel", 2.0 * N * Ho * Wo * Co * C * 9,
                  lambda: check(lib.pd_conv16(ptr(x), ptr(w), ptr(bias), ptr(out), N, H, W, C, sN, sH, sW, Ho, Wo, Co, ldy,
                                              0, act, stream_ptr()), "pd_conv16"), shape=shape)
        return out
    _profiled(_igemm_label(N * Ho * Wo, Co, vec, "fwd", C, KH, KW, stride, pad, mode, act, out_scale is not None, (Ho, Wo)), 2.0 * N * Ho * Wo * Co * (alg_k if alg_k is not None else C * KH * KW),
              lambda: check(lib.pd_conv2d(ptr(x), ptr(w), ptr(bias), ptr(out_scale), ptr(out), ptr(stats), N, H, W, C, sN, sH, sW, sC,
                                          Ho, Wo, Co, KH, KW, stride, pad, mode, act, int(affine is not None), sub,
                                          div, ldy, CONV_FLAGS, stream_ptr()), "pd_conv2d"), shape=shape)
    return (out, stats) if want_stats else out


# objects with .transposed(w) -> tensor | None: a parameter store hands out the data-gradient operands of ALL its
# convolution weights from one batched launch per backward pass (engine.ParamStore registers itself here).  The copies
# are valid until the next forward convolution: FWD_EPOCH counts conv2d_fwd calls, and weights cannot change between a
# forward pass and its backward pass without invalidating the gradients anyway -- no reliance on version counters
# (writes through ``p.data`` or raw pointers do not bump any).
USE_S2_PHASES = os.environ.get("PD_S2_PHASES", "1") != "0"   # stride-2 data gradient as four parity-class sub-convolutions
USE_CONV16 = os.environ.get("PD_CONV16", "1") != "0"     # halo-tile kernel for the 16-channel decoder tail
WT_PROVIDERS = []
FWD_EPOCH = 0


def weight_transposed(w):
    """[Co,Ci,kh,kw] (channels_last) -> operand of the data-gradient GEMM: [Ci][kh][kw][Co] storage,
    returned as a logical [Ci,Co,kh,kw] channels_last tensor."""
    Co, Ci, KH, KW = w.shape
    w = weight_cl(w)
    for prov in WT_PROVIDERS:
        wt = prov.transposed(w)
        if wt is not None:
            return wt
    wt = torch.empty((Ci, Co, KH, KW), dtype=torch.float32, device=w.device, memory_format=CL)
    check(lib.pd_weight_transpose(ptr(w), ptr(wt), Co, KH * KW, Ci, stream_ptr()), "pd_weight_transpose")
    return wt


def conv2d_dgrad(dy, w, in_hw, stride=1, pad=0, wt=None, addend=None, bf16=None):
    """dX of a zero-padded convolution: transposed convolution of dy (NHWC) with w.

    addend: optional tensor of dX's shape (channel stride 1) that is added in the kernel's epilogue -- the gradient of a
    residual block's skip connection, which autograd would otherwise add in a separate pass.
    bf16: the PD_CONV_BF16 bit of the forward this differentiates (None: CONV_FLAGS as it stands)."""
    _require_cuda(dy, w)
    flags = _with_bf16(CONV_FLAGS, bf16)
    dy = as_nhwc(dy)
    N, Co, Hy, Wy = dy.shape
    _, Ci, KH, KW = w.shape
    H, W = in_hw
    if wt is None:
        wt = weight_transposed(w)
    dx = empty_nhwc(N, Ci, H, W, dy.device)
    sN, sC, sH, sW = dy.stride()
    # algorithmic flops of the data gradient = those of the forward conv it differentiates
    flops, shape = 2.0 * N * Hy * Wy * Co * Ci * KH * KW, ("dgrad", N, Ci, H, W, Co, KH, stride, MODE_TRANSPOSED)
    if (USE_S2_PHASES and not (flags & CONV_GENERAL_KERNELS) and addend is None and stride == 2 and KH == 3 and KW == 3 and pad == 1 and H == 2 * Hy and W == 2 * Wy
            and Co % 32 == 0 and Ci % 4 == 0 and Ci > 16 and _quad_strides(dy)):
        # stride-2 data gradient by output parity: four stride-1 2x2 sub-filter launches + one interleave
        def _phases():
            wsub = torch.empty(9 * Ci * Co, dtype=torch.float32, device=dy.device)     # class filters 1x1, 1x2, 2x1, 2x2
            check(lib.pd_dgrad_s2_filters(ptr(wt), ptr(wsub), Ci, Co, stream_ptr()), "pd_dgrad_s2_filters")
            sub = torch.empty((4, N, Hy, Wy, Ci), dtype=torch.float32, device=dy.device)
            for c, off in enumerate((0, 1, 3, 5)):
                ph, pw = c >> 1, c & 1
                check(lib.pd_conv2d_rect(ptr(dy), wsub.data_ptr() + 4 * off * Ci * Co, ptr(sub[c]), N, Hy, Wy, Co, sN, sH, sW,
                                         sC, Hy, Wy, Ci, 1 + ph, 1 + pw, ph, pw, MODE_TRANSPOSED, Ci, flags, stream_ptr()),
                      "pd_conv2d_rect(dgrad s2 phase)")
            check(lib.pd_interleave4(ptr(sub), ptr(dx), N, Hy, Wy, Ci, stream_ptr()), "pd_interleave4")
        _profiled("conv_dgrad_s2_phases", flops, _phases, shape=shape)
        return dx
    c16_mode = 1 if (pad == 0 and H == Hy + 2 and W == Wy + 2) else (2 if (pad == 1 and H == Hy and W == Wy) else 0)
    if _conv16_shape(Co, Ci, KH, KW, stride) and addend is None and c16_mode and _quad_strides(dy) and Hy >= 2 and Wy >= 2:
        # data gradient of a 16-channel 3x3 conv (on the padded grid, or pad 1 on the same grid): halo-tile kernel
        _profiled("conv16_halo_kernel", flops,
                  lambda: check(lib.pd_conv16(ptr(dy), ptr(wt), None, ptr(dx), N, Hy, Wy, Co, sN, sH, sW, H, W, Ci, Ci, c16_mode,
                                              0, stream_ptr()), "pd_conv16(dgrad)"), shape=shape)
        return dx
    label = _igemm_label(N * H * W, Ci, True, "dgrad", Co, KH, KW, stride, pad, MODE_TRANSPOSED, out_hw=(H, W), flags=flags)
    if addend is not None:
        assert addend.shape == dx.shape and addend.stride(1) == 1 and addend.is_cuda
        ld_add = addend.stride(3)
        assert addend.stride(2) == W * ld_add and addend.stride(0) == H * W * ld_add
        _profiled(label, flops,
                  lambda: check(lib.pd_conv2d_add(ptr(dy), ptr(wt), ptr(addend), ld_add, ptr(dx), N, Hy, Wy, Co, sN, sH, sW,
                                                  sC, H, W, Ci, KH, KW, stride, pad, MODE_TRANSPOSED, Ci, flags, stream_ptr()),
                                "pd_conv2d_add(dgrad)"), shape=shape)
    else:
        _profiled(label, flops,
                  lambda: check(lib.pd_conv2d(ptr(dy), ptr(wt), None, None, ptr(dx), None, N, Hy, Wy, Co, sN, sH, sW, sC,
                                              H, W, Ci, KH, KW, stride, pad, MODE_TRANSPOSED, ACT_NONE, 0, 0.0, 1.0, Ci,
                                              flags, stream_ptr()), "pd_conv2d(dgrad)"), shape=shape)
    return dx


_ws_cache = {}


def _workspace(nbytes, device):
    """Scratch of the split reductions, one buffer per (device, stream): weight-gradient kernels run on a side
    stream next to main-stream users of the same scratch (gemm_tn in the materialised-score attention backward)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# pd_conv2d_wgrad_route's code | one-term bit -> profiler label (the one-term forms exist for the halo-tile / rolling-row kernels only)
_WGRAD_LABELS = ("conv_wgrad_kernel", "conv_wgrad_x3c_kernel", "conv_wgrad_halo_x3_kernel", "conv_wgrad_roll_x3_kernel",
                 None, None, "conv_wgrad_halo_bf16_kernel", "conv_wgrad_roll_bf16_kernel")


def conv2d_wgrad(x, dy, w_shape, stride=1, pad=0, mode=MODE_ZERO, affine=None, dw=None, dbias=None,
                 want_bias=False, accumulate=False, alg_k=None, bf16=None):
    """dW (channels_last [Co,Ci,kh,kw]) and optionally dbias of conv(x, w) given dy (NHWC).
    bf16: the PD_CONV_BF16 bit of the forward this differentiates (None: WGRAD_FLAGS as it stands)."""
    _require_cuda(x, dy)
    flags = _with_bf16(WGRAD_FLAGS, bf16)
    dy = as_nhwc(dy)
    N, C, H, W = x.shape
    Co, Ci, KH, KW = w_shape
    assert Ci == C
    Ho, Wo = dy.shape[2], dy.shape[3]
    if dw is None:
        dw = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device, memory_format=CL)
        accumulate = False
    assert dw.is_contiguous(memory_format=CL) or dw.numel() == dw.shape[0] * dw.shape[1]
    if want_bias and dbias is None:
        dbias = torch.empty(Co, dtype=torch.float32, device=x.device)
    M, K = N * Ho * Wo, KH * KW * C
    sN, sC, sH, sW = x.stride()
    shape = ("wgrad", N, C, H, W, Co, KH, stride, mode)
    fits = affine is None and _quad_strides(x) and dy.stride(3) % 4 == 0
    if _conv16_shape(Co, C, KH, KW, stride) and mode == MODE_REFLECT and pad == 1 and fits and H >= 2 and W >= 2:
        ws = _workspace(lib.pd_conv16_wgrad_workspace(C), x.device)
        _profiled("conv16_wgrad_kernel", 2.0 * M * Co * K,
                  lambda: check(lib.pd_conv16_wgrad(ptr(x), ptr(dy), ptr(dw), ptr(dbias), ptr(ws), ws.numel(), N, H, W, C,
                                                    sN, sH, sW, dy.stride(3), int(accumulate), stream_ptr()),
                                "pd_conv16_wgrad"), shape=shape)
        return (dw, dbias) if (want_bias or dbias is not None) else dw
    ws = _workspace(lib.pd_conv2d_wgrad_workspace(M, Co, K, flags), x.device)
    sub, div = (affine if affine is not None else (0.0, 1.0))
    route = lib.pd_conv2d_wgrad_route(M, Co, C, KH, KW, stride, pad, mode, H, W, Ho, Wo, flags) if fits else 0
    _profiled(_WGRAD_LABELS[route & 7], 2.0 * M * Co * (alg_k if alg_k is not None else K),
              lambda: check(lib.pd_conv2d_wgrad(ptr(x), ptr(dy), ptr(dw), ptr(dbias), ptr(ws), ws.numel(), N, H, W, C,
                                                sN, sH, sW, sC, Ho, Wo, Co, KH, KW, stride, pad, mode,
                                                int(affine is not None), sub, div, dy.stride(3), int(accumulate),
                                                flags, stream_ptr()), "pd_conv2d_wgrad"), shape=shape)
    return (dw, dbias) if (want_bias or dbias is not None) else dw


class _SSIMFn(torch.autograd.Function):
    """layers.SSIM (mode 0: the [N,C,H,W] loss map) and compute_reprojection_loss (mode 1: [N,1,H,W]) with their gradients
    w.r.t. both images (pd_ssim_fwd / pd_ssim_bwd)."""

    @staticmethod
    def forward(ctx, x, y, mode, no_ssim):
        x, y = x.float().contiguous(), y.float().contiguous()
        N, C, H, W = x.shape
        out = torch.empty((N, C if mode == 0 else 1, H, W), dtype=torch.float32, device=x.device)
        check(lib.pd_ssim_fwd(ptr(x), ptr(y), ptr(out), N, C, H, W, mode, int(no_ssim), stream_ptr()), "pd_ssim_fwd")
        ctx.args = (mode, int(no_ssim))
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        mode, no_ssim = ctx.args
        N, C, H, W = x.shape
        gout = gout.float().contiguous()
        ws = torch.empty(5 * x.numel(), dtype=torch.float32, device=x.device)
        gx = torch.empty_like(x)
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        check(lib.pd_ssim_bwd(ptr(x), ptr(y), ptr(gout), ptr(ws), ptr(gx), ptr(gy), N, C, H, W, mode, no_ssim, stream_ptr()),
              "pd_ssim_bwd")
        return gx, gy, None, None


def ssim(x, y):
    """layers.SSIM on the GPU: planar NCHW fp32 -> SSIM loss map of the same shape (differentiable in both images)."""
    _require_cuda(x, y)
    return _SSIMFn.apply(x, y, 0, False)


def reprojection_loss(pred, target, no_ssim=False):
    """trainer.py:1069-1081: [N,1,H,W] = 0.85 * mean_c SSIM(pred, target) + 0.15 * mean_c |target - pred| (differentiable)."""
    _require_cuda(pred, target)
    return _SSIMFn.apply(pred, target, 1, bool(no_ssim))


# ------------------------------------------------------------------ photometric multi-view term (csrc/reproj.hip)
REPROJ_MAX_FRAMES = 8         # PD_REPROJ_MAX_FRAMES


def _dev_ptrs(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _ViewSynthFn(torch.autograd.Function):
    """BackprojectDepth + Project3D + grid_sample(border, align_corners=True) for one source frame (pd_view_synth_fwd /
    _bwd): differentiable in depth and, where the pose requires a gradient, in T (pd_view_synth_bwd_pose, one pass for
    both) -- the source and the intrinsics are data."""

    @staticmethod
    def forward(ctx, depth, src, K, inv_K, T):
        N, C, H, W = src.shape
        warped = torch.empty_like(src)
        coords = torch.empty((N, H, W, 2), dtype=torch.float32, device=src.device)
        check(lib.pd_view_synth_fwd(ptr(depth), ptr(src), ptr(K), ptr(inv_K), ptr(T), ptr(warped), ptr(coords), N, C, H, W,
                                    stream_ptr()), "pd_view_synth_fwd")
        ctx.save_for_backward(depth, src, K, inv_K, T, coords)
        ctx.mark_non_differentiable(coords)
        return warped, coords

    @staticmethod
    def backward(ctx, gwarped, _gcoords):
        depth, src, K, inv_K, T, coords = ctx.saved_tensors
        N, C, H, W = src.shape
        if ctx.needs_input_grad[4]:
            gdepth = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
            part = torch.empty((N, lib.pd_view_synth_pose_rows(H, W), 12), dtype=torch.float64, device=src.device)
            gT = torch.empty((N, 4, 4), dtype=torch.float32, device=src.device)
            check(lib.pd_view_synth_bwd_pose(ptr(gwarped.float().contiguous()), ptr(src), ptr(coords), ptr(depth), ptr(K),
                                             ptr(inv_K), ptr(T), ptr(gdepth), ptr(part), None, ptr(gT), N, C, H, W, 0,
                                             stream_ptr()), "pd_view_synth_bwd_pose")
            return gdepth, None, None, None, gT
        gdepth = torch.empty_like(depth)
        check(lib.pd_view_synth_bwd(ptr(gwarped.float().contiguous()), ptr(src), ptr(coords), ptr(depth), ptr(K), ptr(inv_K),
                                    ptr(T), ptr(gdepth), N, C, H, W, 0, stream_ptr()), "pd_view_synth_bwd")
        return gdepth, None, None, None, None


def view_synthesis(depth, src, K, inv_K, T):
    """trainer.py:1021-1044 for one neighbouring frame: ``src`` [N,C,H,W] warped into the current view through ``depth``
    [N,1,H,W], the intrinsics ``K`` / ``inv_K`` [N,4,4] and the relative pose ``T`` [N,4,4] (current camera -> source camera).
    Returns (warped [N,C,H,W], coords [N,H,W,2]): coords are the unclamped source PIXEL coordinates (u, v) of every pixel
    (include/polardepth.h states the arithmetic).  Differentiable in depth, and in ``T`` where it requires a gradient (a
    predicted pose: ``pose_matrix`` / ``pose_head``): the pose gradient is a deterministic fp64 reduction over the pixels,
    formed in the same pass as the depth gradient.  A pose that requires no gradient costs what it did."""
    _require_cuda(depth, src, K, inv_K, T)
    if src.dim() != 4 or depth.dim() != 4 or depth.shape[1] != 1 or depth.shape[0] != src.shape[0] or \
            depth.shape[2:] != src.shape[2:]:
        raise ValueError(f"view_synthesis: depth [N,1,H,W] and src [N,C,H,W] expected, got {tuple(depth.shape)} / {tuple(src.shape)}")
    N = src.shape[0]
    for name, m in (("K", K), ("inv_K", inv_K), ("T", T)):
        if tuple(m.shape) != (N, 4, 4):
            raise ValueError(f"view_synthesis: {name} must be [{N},4,4], got {tuple(m.shape)}")
    f = lambda t: t.float().contiguous()
    return _ViewSynthFn.apply(f(depth), f(src), f(K), f(inv_K), f(T))


class _ReprojCombineFn(torch.autograd.Function):
    """trainer.py:1163-1215 (pd_reproj_combine_fwd / _bwd): returns (loss, sel, sums); differentiable in the F reproj maps."""

    @staticmethod
    def forward(ctx, identity, noise, valid, avg, *reproj):
        F = len(reproj)
        N, _, H, W = reproj[0].shape
        dev = reproj[0].device
        sel = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
        part = torch.empty((lib.pd_reproj_combine_rows(N, H, W), 2), dtype=torch.float64, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.pd_reproj_combine_fwd(_dev_ptrs(reproj), None if identity is None else _dev_ptrs(identity), F, ptr(noise),
                                        ptr(valid), ptr(sel), ptr(part), ptr(sums), ptr(loss), N, H, W, int(avg),
                                        stream_ptr()), "pd_reproj_combine_fwd")
        ctx.geom = (F, N, H, W, int(avg))
        ctx.save_for_backward(sel, sums, valid)
        ctx.mark_non_differentiable(sel, sums)
        return loss.reshape(()), sel, sums

    @staticmethod
    def backward(ctx, gloss, _gsel, _gsums):
        sel, sums, valid = ctx.saved_tensors
        F, N, H, W, avg = ctx.geom
        grads = [torch.empty((N, 1, H, W), dtype=torch.float32, device=sel.device) for _ in range(F)]
        check(lib.pd_reproj_combine_bwd(ptr(gloss.float().reshape(1).contiguous()), ptr(sel), ptr(sums), ptr(valid),
                                        _dev_ptrs(grads), F, N, H, W, avg, stream_ptr()), "pd_reproj_combine_bwd")
        return (None, None, None, None, *grads)


def reproj_combine(reproj, identity=None, noise=None, valid=None, avg=False, details=False):
    """The reduction of trainer.py:1163-1215 over the neighbouring frames: ``reproj`` (and, for automasking, ``identity``) are
    lists of F [N,1,H,W] maps of ``reprojection_loss``; ``noise`` [N,1,H,W] is added to the identity value; ``valid`` [N,F]
    marks with 0 the frames that do not exist.  Per pixel the minimum over the valid frames (``avg``: their mean), masked
    where the identity value + noise is smaller; returns sum(min * mask) / (sum(mask) + 1e-7), summed in fp64 in a fixed
    order.  ``details``: also ``sel`` [N,H,W] uint8 (winning frame, 255 = masked) and ``sums`` (2 doubles: sum, count).
    Differentiable in the reproj maps."""
    reproj = list(reproj)
    if not 1 <= len(reproj) <= REPROJ_MAX_FRAMES:
        raise ValueError(f"reproj_combine: 1 .. {REPROJ_MAX_FRAMES} frames, got {len(reproj)}")
    if identity is not None and len(identity) != len(reproj):
        raise ValueError("reproj_combine: as many identity maps as reproj maps")
    if noise is not None and identity is None:
        raise ValueError("reproj_combine: noise is added to the identity maps; there are none")
    _require_cuda(*reproj, *(identity or ()), noise, valid)
    shape = tuple(reproj[0].shape)
    if len(shape) != 4 or shape[1] != 1:
        raise ValueError(f"reproj_combine: maps must be [N,1,H,W], got {shape}")
    for t in (*reproj, *(identity or ()), *((noise,) if noise is not None else ())):
        if tuple(t.shape) != shape:
            raise ValueError(f"reproj_combine: every map must be {shape}, got {tuple(t.shape)}")
    if valid is not None and tuple(valid.shape) != (shape[0], len(reproj)):
        raise ValueError(f"reproj_combine: valid must be [{shape[0]},{len(reproj)}], got {tuple(valid.shape)}")
    f = lambda t: t.float().contiguous()
    loss, sel, sums = _ReprojCombineFn.apply(None if identity is None else [f(t).detach() for t in identity],
                                             None if noise is None else f(noise).detach(),
                                             None if valid is None else f(valid).detach(), bool(avg), *[f(t) for t in reproj])
    return (loss, sel, sums) if details else loss


# ------------------------------------------------------------------ pose network tail (csrc/pose.hip)
class _PoseMatrixFn(torch.autograd.Function):
    """transformation_from_parameters (pd_pose_matrix_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, axisangle, translation, invert):
        N = axisangle.shape[0]
        T = torch.empty((N, 4, 4), dtype=torch.float32, device=axisangle.device)
        check(lib.pd_pose_matrix_fwd(ptr(axisangle), ptr(translation), ptr(T), N, int(invert), stream_ptr()),
              "pd_pose_matrix_fwd")
        ctx.invert = int(invert)
        ctx.save_for_backward(axisangle, translation)
        return T

    @staticmethod
    def backward(ctx, gT):
        axisangle, translation = ctx.saved_tensors
        N = axisangle.shape[0]
        ga, gt = torch.empty_like(axisangle), torch.empty_like(translation)
        check(lib.pd_pose_matrix_bwd(ptr(gT.float().contiguous()), ptr(axisangle), ptr(translation), ptr(ga), ptr(gt), N,
                                     ctx.invert, stream_ptr()), "pd_pose_matrix_bwd")
        return ga, gt, None


def pose_matrix(axisangle, translation, invert=False):
    """layers.py:74-91 ``transformation_from_parameters``: ``axisangle`` and ``translation`` ([N,1,3] or [N,3]) to the 4x4
    matrix ``T`` [N,4,4] -- Trans(t) R, or with ``invert`` R^T Trans(-t) -- evaluated in fp64 and rounded once
    (include/polardepth.h states the order).  Differentiable in both."""
    _require_cuda(axisangle, translation)
    N = axisangle.shape[0]
    if axisangle.numel() != 3 * N or translation.numel() != 3 * N or translation.shape[0] != N:
        raise ValueError(f"pose_matrix: axisangle and translation must be [N,1,3] or [N,3], got {tuple(axisangle.shape)} / "
                         f"{tuple(translation.shape)}")
    f = lambda t: t.float().reshape(N, 3).contiguous()
    return _PoseMatrixFn.apply(f(axisangle), f(translation), bool(invert))


class _PoseHeadFn(torch.autograd.Function):
    """PoseDecoder's tail and both matrices of slot 0 (pd_pose_head_fwd / _bwd); x is NHWC storage of [N,Cin,h,w]."""

    @staticmethod
    def forward(ctx, x, weight, bias, invert):
        N, Cin, h, w = x.shape
        Co = weight.shape[0]
        dev = x.device
        nf = Co // 6
        aa = torch.empty((N, nf, 1, 3), dtype=torch.float32, device=dev)
        tr = torch.empty((N, nf, 1, 3), dtype=torch.float32, device=dev)
        T = torch.empty((N, 4, 4), dtype=torch.float32, device=dev)
        Ti = torch.empty((N, 4, 4), dtype=torch.float32, device=dev)
        mean = torch.empty((N, Cin), dtype=torch.float64, device=dev)
        check(lib.pd_pose_head_fwd(ptr(x), ptr(weight), ptr(bias), ptr(aa), ptr(tr), ptr(T), ptr(Ti), ptr(mean), N, h, w, Cin,
                                   Co, int(invert), stream_ptr()), "pd_pose_head_fwd")
        ctx.geom = (N, h, w, Cin, Co, int(invert))
        ctx.params = (weight, bias)
        ctx.save_for_backward(weight, mean, aa, tr)
        ctx.set_materialize_grads(False)          # an unused output hands None to the kernel, not a tensor of zeros
        return aa, tr, T, Ti

    @staticmethod
    def backward(ctx, gaa, gtr, gT, gTi):
        weight = ctx.saved_tensors[0]
        gw = torch.empty_like(weight)
        gb = torch.empty(weight.shape[0], dtype=torch.float32, device=weight.device)
        gx = pose_head_bwd(ctx.saved_tensors, ctx.geom, (gaa, gtr, gT, gTi), gw, gb, accumulate=False)
        return gx, gw, gb, None


def pose_head_bwd(saved, geom, grads, gw, gb, accumulate):
    """pd_pose_head_bwd for what _PoseHeadFn.forward saved: returns gx and writes (``accumulate``: adds to) ``gw`` / ``gb``,
    which have the storage of the 1x1 convolution's weight and bias (functional.PoseHeadFn hands in the gradient buffers)."""
    weight, mean, aa, tr = saved
    N, h, w, Cin, Co, invert = geom
    gaa, gtr, gT, gTi = (None if t is None else t.float().contiguous() for t in grads)
    gx = empty_nhwc(N, Cin, h, w, weight.device)
    ws = torch.empty((N, Co), dtype=torch.float64, device=weight.device)
    check(lib.pd_pose_head_bwd(ptr(gT), ptr(gTi), ptr(gaa), ptr(gtr), ptr(aa), ptr(tr), ptr(weight), ptr(mean), ptr(gx),
                               ptr(gw), ptr(gb), ptr(ws), N, h, w, Cin, Co, invert, int(accumulate), stream_ptr()),
          "pd_pose_head_bwd")
    return gx


def pose_head(x, weight, bias, invert=False):
    """The tail of PoseDecoder.forward (pose_decoder.py:41-50) from the input of ("pose", 2) on, in one launch: ``x``
    [N,Cin,h,w] (channels_last), ``weight`` [Co,Cin,1,1] or [Co,Cin] and ``bias`` [Co] of the 1x1 convolution, Co = 6 nf.
    Returns (axisangle [N,nf,1,3], translation [N,nf,1,3], T [N,4,4], T_inv [N,4,4]): the matrices are
    ``pose_matrix(axisangle[:, 0], translation[:, 0], invert)`` and the same with ``invert`` flipped (the reference's
    cam_T_cam / cam_T_cam_inv).  Differentiable in x, weight and bias through all four outputs."""
    _require_cuda(x, weight, bias)
    if x.dim() != 4:
        raise ValueError(f"pose_head: x must be [N,Cin,h,w], got {tuple(x.shape)}")
    Co, Cin = weight.shape[0], x.shape[1]
    if weight.numel() != Co * Cin or tuple(bias.shape) != (Co,):
        raise ValueError(f"pose_head: weight [Co,{Cin}(,1,1)] and bias [Co] expected, got {tuple(weight.shape)} / "
                         f"{tuple(bias.shape)}")
    if Cin % 64 or Cin > 1024 or Co % 6:
        raise ValueError(f"pose_head: Cin must be a multiple of 64 (<= 1024) and Co a multiple of 6, got {Cin} / {Co}")
    return _PoseHeadFn.apply(as_nhwc(x.float()), weight.float().reshape(Co, Cin).contiguous(), bias.float().contiguous(),
                             bool(invert))


POSE_CHAIN_MAX_LINKS = 8      # PD_POSE_CHAIN_MAX_LINKS


def pose_chain(axisangle, translation, present=None, init=None, direction=-1):
    """The matching-pose half of predict_poses (trainer.py:708-746) for one direction in one launch (pd_pose_chain;
    include/polardepth.h states the arithmetic).  ``axisangle`` / ``translation`` [L,N,3] (or [L,N,1,3]): link k is the pose
    network's slot-0 output for the frames ``direction * (k+1)`` and ``direction * k`` stacked in temporal order;
    ``present`` [L,N]: 0 where frame ``direction * (k+1)`` of an item does not exist; ``init`` [N,4,4]: the pose to continue
    from.  Returns ``(rel, rel_inv)`` [L,N,4,4]: ``rel[k]`` is the pose 0 -> frame ``direction * (k+1)`` -- all zeros from an
    absent frame on --, ``rel_inv[k]`` the link's OWN inverse, neither chained nor zeroed (the reference's
    ``relative_pose_inv``).  Forward only: the results carry no tape.  CPU tensors and wrong shapes are a ValueError."""
    for t in (axisangle, translation, present, init):
        if t is not None and not t.is_cuda:
            raise ValueError("pose_chain: polardepth ops need CUDA(HIP) tensors; there is no CPU fallback")
    if direction not in (-1, 1):
        raise ValueError(f"pose_chain: direction must be -1 or 1, got {direction!r}")
    if axisangle.dim() < 3 or axisangle.shape[0] < 1 or axisangle.shape[1] < 1:
        raise ValueError(f"pose_chain: axisangle must be [L,N,3] or [L,N,1,3], got {tuple(axisangle.shape)}")
    L, N = axisangle.shape[:2]
    if L > POSE_CHAIN_MAX_LINKS:
        raise ValueError(f"pose_chain: 1 .. {POSE_CHAIN_MAX_LINKS} links, got {L}")
    for name, t in (("axisangle", axisangle), ("translation", translation)):
        if tuple(t.shape) not in ((L, N, 3), (L, N, 1, 3)):
            raise ValueError(f"pose_chain: {name} must be [{L},{N},3] or [{L},{N},1,3], got {tuple(t.shape)}")
    if present is not None and tuple(present.shape) != (L, N):
        raise ValueError(f"pose_chain: present must be [{L},{N}], got {tuple(present.shape)}")
    if init is not None and tuple(init.shape) != (N, 4, 4):
        raise ValueError(f"pose_chain: init must be [{N},4,4], got {tuple(init.shape)}")
    f = lambda t: None if t is None else t.detach().float().contiguous()
    aa, tr, present, init = f(axisangle), f(translation), f(present), f(init)
    rel = torch.empty((L, N, 4, 4), dtype=torch.float32, device=aa.device)
    rel_inv = torch.empty_like(rel)
    check(lib.pd_pose_chain(ptr(aa), ptr(tr), ptr(present), ptr(init), ptr(rel), ptr(rel_inv), L, N, int(direction),
                            stream_ptr()), "pd_pose_chain")
    return rel, rel_inv


# ------------------------------------------------------------------ pose supervision (csrc/pose_loss.hip)
def _frame_weights(w):
    import ctypes
    return (ctypes.c_float * len(w))(*w)


class _PoseSupervisionFn(torch.autograd.Function):
    """pd_pose_loss_fwd / _bwd: returns (vals[:3], records | None); differentiable in the F predicted matrices."""

    @staticmethod
    def forward(ctx, T_gt, valid, weights, want_records, *T_pred):
        F = len(T_pred)
        N = T_pred[0].shape[0]
        dev = T_pred[0].device
        vals = torch.empty(3 + 2 * F, dtype=torch.float32, device=dev)
        records = torch.empty((F, N, 10), dtype=torch.float64, device=dev) if want_records else None
        check(lib.pd_pose_loss_fwd(_dev_ptrs(T_pred), _dev_ptrs(T_gt), F, _frame_weights(weights), ptr(valid), ptr(records),
                                   ptr(vals), N, stream_ptr()), "pd_pose_loss_fwd")
        ctx.geom = (F, N, tuple(weights))
        ctx.save_for_backward(valid, *T_gt, *T_pred)
        if records is not None:
            ctx.mark_non_differentiable(records)
        return vals[:3], records

    @staticmethod
    def backward(ctx, gvals, _grecords):
        F, N, weights = ctx.geom
        valid, T_gt, T_pred = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + F], ctx.saved_tensors[1 + F:]
        grads = [torch.empty((N, 4, 4), dtype=torch.float32, device=gvals.device) for _ in range(F)]
        check(lib.pd_pose_loss_bwd(ptr(gvals.float().contiguous()), _dev_ptrs(T_pred), _dev_ptrs(T_gt), F,
                                   _frame_weights(weights), ptr(valid), _dev_ptrs(grads), N, stream_ptr()), "pd_pose_loss_bwd")
        return (None, None, None, None, *grads)


def pose_supervision(T_pred, T_gt, valid=None, frame_weight=None, details=False):
    """``--supervise_pose`` of trainer.py:1267-1285 in one launch (pd_pose_loss_fwd; include/polardepth.h states the
    arithmetic): ``T_pred`` and ``T_gt`` are lists of F [N,4,4] matrices, the predicted ``cam_T_cam`` of every neighbouring
    frame and its ground-truth relative pose.  Per frame ``r_f = 0.1 * mean((rv(R_pred) - rv(R_gt))^2)`` with ``rv`` =
    ``roma.rotmat_to_rotvec`` and ``t_f = mean((t_pred - t_gt)^2)``.  Returns ``(r_loss, t_loss, total)``: the plain sums
    over the frames, which the reference logs, and ``total = sum_f frame_weight[f] (r_f + t_f)``, which it adds to the loss.

    ``frame_weight`` defaults to ``[F, F-1, ..., 1]``: the reference adds the RUNNING sums ``r_loss + t_loss`` to the total
    inside its loop over the frames, so with ``frame_ids 0 -1 1`` the first neighbour counts twice and the second once.
    ``valid`` [N,F] marks with 0 the items whose frame f does not exist: they are left out and the mean is taken over the
    present ones (the reference has no mask and supervises towards whatever its loader substituted -- a deliberate
    difference, the rule of the photometric term).  ``details``: also ``records`` [F,N,10] float64 per item, invalid ones
    included (rv_pred, rv_gt, the geodesic angle of R_pred^T R_gt in radians, |t_pred - t_gt|, |t_pred|, |t_gt|).
    Differentiable in the ``T_pred`` tensors; the ground truth receives no gradient."""
    T_pred, T_gt = list(T_pred), list(T_gt)
    F = len(T_pred)
    if not 1 <= F <= REPROJ_MAX_FRAMES:
        raise ValueError(f"pose_supervision: 1 .. {REPROJ_MAX_FRAMES} frames, got {F}")
    if len(T_gt) != F:
        raise ValueError(f"pose_supervision: as many ground-truth as predicted poses, got {len(T_gt)} / {F}")
    shape = tuple(T_pred[0].shape)
    if len(shape) != 3 or shape[1:] != (4, 4):
        raise ValueError(f"pose_supervision: poses must be [N,4,4], got {shape}")
    if shape[0] > 65535:
        raise ValueError(f"pose_supervision: at most 65535 items, got {shape[0]}")
    for t in (*T_pred, *T_gt):
        if tuple(t.shape) != shape:
            raise ValueError(f"pose_supervision: every pose must be {shape}, got {tuple(t.shape)}")
    if valid is not None and tuple(valid.shape) != (shape[0], F):
        raise ValueError(f"pose_supervision: valid must be [{shape[0]},{F}], got {tuple(valid.shape)}")
    weights = [float(F - f) for f in range(F)] if frame_weight is None else [float(w) for w in frame_weight]
    if len(weights) != F:
        raise ValueError(f"pose_supervision: {F} frame weights expected, got {len(weights)}")
    _require_cuda(*T_pred, *T_gt, valid)
    f32 = lambda t: t.float().contiguous()
    head, records = _PoseSupervisionFn.apply([f32(t).detach() for t in T_gt], None if valid is None else f32(valid).detach(),
                                             weights, bool(details), *[f32(t) for t in T_pred])
    r_loss, t_loss, total = head.unbind(0)
    return (r_loss, t_loss, total, records) if details else (r_loss, t_loss, total)


# ------------------------------------------------------------------ multi-frame cost volume (csrc/matching.hip)
COST_VOLUME_MAX_BINS = 128


def cost_volume(cur, lookup, poses, K, inv_K, bins, valid=None, out=None, apply_confidence=False, want_missing=False):
    """ManyDepth's plane sweep from known poses in one launch (pd_cost_volume; include/polardepth.h states the arithmetic).

    cur [B,C,h,w] and lookup [B,F,C,h,w] features (channels-last storage is used as it is, anything else is copied),
    poses [B,F,4,4] current -> lookup camera, K / inv_K [B,4,4] of the feature resolution, bins [D] fp32 on the device (read
    by the kernel: overwriting them in place needs no new capture), valid [B,F] or None.  A frame is also skipped where its
    pose sums to 0, the reference's "missing frame" rule.  No gradient: call it under no_grad or on detached features.

    Returns (cost, confidence, argmin, lowest[, missing]): cost a logical [B,D,h,w] channels-last tensor -- ``out`` if given,
    the sliced view [:, c0:c0+D] of a wider NHWC buffer as for conv2d_fwd(out=) -- confidence [B,h,w] fp32 0/1, argmin
    [B,h,w] int32, lowest [B,h,w] fp32 = 1 / bins[argmin], missing [B,D,h,w] uint8 (channels-last) with want_missing."""
    _require_cuda(cur, lookup, poses, K, inv_K, bins, valid, out)
    if cur.dim() != 4 or lookup.dim() != 5 or lookup.shape[0] != cur.shape[0] or lookup.shape[2:] != cur.shape[1:]:
        raise ValueError(f"cost_volume: cur [B,C,h,w] and lookup [B,F,C,h,w] expected, got {tuple(cur.shape)} / {tuple(lookup.shape)}")
    B, C, h, w = cur.shape
    F = lookup.shape[1]
    D = bins.numel()
    if C % 4 or C < 4:
        raise ValueError(f"cost_volume: the channel count must be a multiple of 4, got {C}")
    if not 1 <= D <= COST_VOLUME_MAX_BINS or bins.dim() != 1:
        raise ValueError(f"cost_volume: 1 <= D <= {COST_VOLUME_MAX_BINS} depth bins in a 1-d tensor, got {tuple(bins.shape)}")
    if F > REPROJ_MAX_FRAMES:
        raise ValueError(f"cost_volume: at most {REPROJ_MAX_FRAMES} lookup frames, got {F}")
    if tuple(poses.shape) != (B, F, 4, 4):
        raise ValueError(f"cost_volume: poses must be [{B},{F},4,4], got {tuple(poses.shape)}")
    for name, m in (("K", K), ("inv_K", inv_K)):
        if tuple(m.shape) != (B, 4, 4):
            raise ValueError(f"cost_volume: {name} must be [{B},4,4], got {tuple(m.shape)}")
    if valid is not None and tuple(valid.shape) != (B, F):
        raise ValueError(f"cost_volume: valid must be [{B},{F}], got {tuple(valid.shape)}")
    f32 = lambda t: t.detach().float().contiguous()
    cur = as_nhwc(cur.detach().float())
    lookup = lookup.detach().float()
    if lookup.stride() != (F * h * w * C, h * w * C, 1, w * C, C):
        lookup = lookup.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    poses, K, inv_K, bins = f32(poses), f32(K), f32(inv_K), f32(bins)
    dev = cur.device
    v = None
    if F:
        v = (poses.reshape(B, F, 16).sum(-1) != 0)
        if valid is not None:
            v = v & (valid != 0)
        v = v.float()
    if out is None:
        out = empty_nhwc(B, D, h, w, dev)
    if tuple(out.shape) != (B, D, h, w) or out.dtype != torch.float32 or out.stride(1) != 1:
        raise ValueError(f"cost_volume: out must be a float32 [{B},{D},{h},{w}] view with channel stride 1")
    ldc = out.stride(3)
    if out.stride(2) != w * ldc or out.stride(0) != h * w * ldc or ldc < D:
        raise ValueError(f"cost_volume: out is not a channel slice of an NHWC buffer (strides {out.stride()})")
    confidence = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    argmin = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    lowest = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    missing = torch.empty((B, h, w, D), dtype=torch.uint8, device=dev) if want_missing else None
    check(lib.pd_cost_volume(ptr(cur), ptr(lookup), ptr(poses), ptr(K), ptr(inv_K), ptr(bins), ptr(v), ptr(out), ldc,
                             ptr(missing), ptr(confidence), ptr(argmin), ptr(lowest), B, F, h, w, C, D,
                             int(bool(apply_confidence)), stream_ptr()), "pd_cost_volume")
    res = (out, confidence, argmin, lowest)
    return res + (missing.permute(0, 3, 1, 2),) if want_missing else res


# ------------------------------------------------------------------ cost-volume student's step (csrc/student.hip)
BINS_LINEAR, BINS_INVERSE = 0, 1          # PD_BINS_LINEAR / PD_BINS_INVERSE
_BINNING = {"linear": BINS_LINEAR, "inverse": BINS_INVERSE}


def _f32c16(t):
    """float32, contiguous and 16-byte aligned (a fresh allocation is; an odd view is copied)."""
    t = t.float().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def student_masks(lowest, confidence, mono_depth, aug=None, motion_masking=True, want_maps=True):
    """The consistency masks of the reference's --train_student branch in one pass (pd_student_masks; include/polardepth.h
    states the arithmetic): ``lowest`` / ``confidence`` [N,h,w] as ops.cost_volume returns them, ``mono_depth`` [N,1,4h,4w]
    the teacher's full-resolution depth, ``aug`` [N] (non-zero = augmented item) or None.  Returns (rmask [N,H,W] uint8,
    cmask [N,H,W] fp32, lowest_up [N,H,W] fp32, minmax [N,2] fp32); cmask and lowest_up are None without ``want_maps``.
    No gradient."""
    _require_cuda(lowest, confidence, mono_depth, aug)
    if lowest.dim() != 3 or confidence.shape != lowest.shape:
        raise ValueError(f"student_masks: lowest and confidence must be [N,h,w], got {tuple(lowest.shape)} / {tuple(confidence.shape)}")
    N, h, w = lowest.shape
    if tuple(mono_depth.shape) != (N, 1, 4 * h, 4 * w):
        raise ValueError(f"student_masks: mono_depth must be [{N},1,{4 * h},{4 * w}], got {tuple(mono_depth.shape)}")
    if aug is not None and aug.numel() != N:
        raise ValueError(f"student_masks: aug must hold {N} values, got {tuple(aug.shape)}")
    f32 = lambda t: t.detach().float().contiguous()
    lowest, confidence, mono = f32(lowest), f32(confidence), _f32c16(mono_depth.detach())
    aug = None if aug is None else f32(aug).reshape(N)
    dev = lowest.device
    H, W = 4 * h, 4 * w
    rmask = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    cmask = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_maps else None
    lowest_up = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_maps else None
    minmax = torch.empty((N, 2), dtype=torch.float32, device=dev)
    part = torch.empty((max(N, 1) * lib.pd_student_masks_rows(N, h, w), 2), dtype=torch.float32, device=dev)
    check(lib.pd_student_masks(ptr(lowest), ptr(confidence), ptr(mono), ptr(aug), int(bool(motion_masking)), ptr(rmask),
                               ptr(cmask), ptr(lowest_up), ptr(minmax), ptr(part), N, h, w, H, W, stream_ptr()),
          "pd_student_masks")
    return rmask, cmask, lowest_up, minmax


def depth_bins_update(minmax, tracker, floor_depth, bins, binning="linear"):
    """update_adaptive_depth_bins + compute_depth_bins on the device, in place (pd_depth_bins_update): ``minmax`` [N,2] fp32
    from student_masks, ``tracker`` 2 doubles (min, max), ``bins`` [D] fp32 -- both are overwritten where they are, so a
    cost volume that reads ``bins`` needs nothing else.  No host synchronisation."""
    _require_cuda(minmax, tracker, bins)
    if binning not in _BINNING:
        raise NotImplementedError(f"depth_binning {binning!r}: linear or inverse")
    if minmax.dim() != 2 or minmax.shape[1] != 2 or minmax.dtype != torch.float32 or not minmax.is_contiguous():
        raise ValueError(f"depth_bins_update: minmax must be a contiguous float32 [N,2], got {tuple(minmax.shape)}")
    if tracker.dtype != torch.float64 or tracker.numel() != 2 or not tracker.is_contiguous():
        raise ValueError("depth_bins_update: tracker must be 2 contiguous doubles (min, max)")
    if bins.dtype != torch.float32 or bins.dim() != 1 or not bins.is_contiguous():
        raise ValueError("depth_bins_update: bins must be a contiguous 1-d float32 tensor")
    check(lib.pd_depth_bins_update(ptr(minmax), minmax.shape[0], ptr(tracker), float(floor_depth), bins.numel(),
                                   _BINNING[binning], ptr(bins), stream_ptr()), "pd_depth_bins_update")


class _StudentCombineFn(torch.autograd.Function):
    """trainer.py:1202-1236 for one scale (pd_student_combine_fwd / _bwd): returns (loss [2], sel, sums); differentiable in
    the F reproj maps and in the multi-frame depth."""

    @staticmethod
    def forward(ctx, valid, rmask, mono, avg, multi, *reproj):
        F = len(reproj)
        N, _, H, W = reproj[0].shape
        dev = reproj[0].device
        sel = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
        part = torch.empty((lib.pd_student_combine_rows(N, H, W), 3), dtype=torch.float64, device=dev)
        sums = torch.empty(3, dtype=torch.float64, device=dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        check(lib.pd_student_combine_fwd(_dev_ptrs(reproj), F, ptr(valid), ptr(rmask), ptr(multi), ptr(mono), ptr(sel), ptr(part),
                                         ptr(sums), ptr(loss), N, H, W, int(avg), stream_ptr()), "pd_student_combine_fwd")
        ctx.geom = (F, N, H, W, int(avg))
        ctx.save_for_backward(sel, sums, valid, multi, mono)
        ctx.mark_non_differentiable(sel, sums)
        return loss, sel, sums

    @staticmethod
    def backward(ctx, gloss, _gsel, _gsums):
        sel, sums, valid, multi, mono = ctx.saved_tensors
        F, N, H, W, avg = ctx.geom
        grads = [torch.empty((N, 1, H, W), dtype=torch.float32, device=sel.device) for _ in range(F)]
        gmulti = torch.empty((N, 1, H, W), dtype=torch.float32, device=sel.device)
        check(lib.pd_student_combine_bwd(ptr(gloss.float().reshape(2).contiguous()), ptr(sel), ptr(sums), ptr(valid), ptr(multi),
                                         ptr(mono), _dev_ptrs(grads), ptr(gmulti), F, N, H, W, avg, stream_ptr()),
              "pd_student_combine_bwd")
        return (None, None, None, None, gmulti, *grads)


def student_combine(reproj, rmask, multi_depth, mono_depth, valid=None, avg=False, details=False):
    """The is_multi branch of the reference's compute_losses for one scale: ``reproj`` a list of F [N,1,H,W] maps of
    ``reprojection_loss``, ``rmask`` [N,H,W] uint8 from student_masks, ``multi_depth`` / ``mono_depth`` [N,1,H,W], ``valid``
    [N,F] or None.  Returns (reproj_loss, consistency_loss): sum(min * rmask) / (sum(rmask) + 1e-7) and
    mean(|multi - mono| * (1 - rmask)), summed in fp64 in a fixed order; ``details``: also ``sel`` [N,H,W] uint8 (winning
    frame, 255 = masked) and ``sums`` (3 doubles).  Differentiable in the reproj maps and in multi_depth; mono_depth and the
    mask are data."""
    reproj = list(reproj)
    if not 1 <= len(reproj) <= REPROJ_MAX_FRAMES:
        raise ValueError(f"student_combine: 1 .. {REPROJ_MAX_FRAMES} frames, got {len(reproj)}")
    _require_cuda(*reproj, rmask, multi_depth, mono_depth, valid)
    shape = tuple(reproj[0].shape)
    if len(shape) != 4 or shape[1] != 1 or shape[2] % 4 or shape[3] % 4:
        raise ValueError(f"student_combine: maps must be [N,1,H,W] with H and W multiples of 4, got {shape}")
    for t in (*reproj, multi_depth, mono_depth):
        if tuple(t.shape) != shape:
            raise ValueError(f"student_combine: every map must be {shape}, got {tuple(t.shape)}")
    if tuple(rmask.shape) != (shape[0], shape[2], shape[3]) or rmask.dtype != torch.uint8:
        raise ValueError(f"student_combine: rmask must be uint8 [{shape[0]},{shape[2]},{shape[3]}], got {rmask.dtype} {tuple(rmask.shape)}")
    if valid is not None and tuple(valid.shape) != (shape[0], len(reproj)):
        raise ValueError(f"student_combine: valid must be [{shape[0]},{len(reproj)}], got {tuple(valid.shape)}")
    rmask = rmask.contiguous()
    if rmask.data_ptr() % 4:
        rmask = rmask.clone()
    loss, sel, sums = _StudentCombineFn.apply(None if valid is None else valid.detach().float().contiguous(), rmask,
                                              _f32c16(mono_depth.detach()), bool(avg), _f32c16(multi_depth),
                                              *[_f32c16(t) for t in reproj])
    return (loss[0], loss[1], sel, sums) if details else (loss[0], loss[1])


# ------------------------------------------------------------------ polarimetric normals loss (csrc/polar_loss.hip)
POLAR_LOSS_COUNTERS = ("n_normal", "n_azimuth", "dolp_out", "bad", "frontal", "spec", "flipped")   # PD_PLOSS_COUNTERS, in order
POLAR_LOSS_RECORD_BYTES = 96            # PD_PLOSS_RECORD_BYTES: 4 doubles, 7 int64, 8 bytes of zero
POLAR_STATE_WINNER, POLAR_STATE_NEGATED, POLAR_STATE_BRANCH_SHIFT, POLAR_STATE_GATE_SHIFT = 7, 8, 4, 6


class PolarLossDetails:
    """What ``polar_loss(..., details=True)`` adds: ``state`` uint8 [N,H,W] (the decisions per pixel; bit layout in
    include/polardepth.h), ``sums`` float64 [4] (sum w l_n, sum w, sum w l_a, sum w), ``counters`` int64 [7]
    (POLAR_LOSS_COUNTERS) and ``maps`` fp32 [N,H,W,2] = (l_n, l_a), NaN where a pixel is not counted.  All on the device."""

    def __init__(self, state, record, maps):
        self.state, self.record, self.maps = state, record, maps

    @property
    def sums(self):
        return self.record.view(torch.float64)[:4]

    @property
    def counters(self):
        return self.record.view(torch.int64)[4:11]


class _PolarLossFn(torch.autograd.Function):
    """pd_polar_loss_fwd / _bwd: returns (values [2], state, record, maps); differentiable in the depth map."""

    @staticmethod
    def forward(ctx, depth, K, pol, xolp, ldp, valid, opts, want_maps):
        N, _, H, W = depth.shape
        dev = depth.device
        rho_min, rho_max, tilt2, sign, weighted, ray = opts
        state = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
        record = torch.zeros(POLAR_LOSS_RECORD_BYTES, dtype=torch.uint8, device=dev)
        values = torch.zeros(2, dtype=torch.float32, device=dev)
        maps = torch.empty((N, H, W, 2), dtype=torch.float32, device=dev) if want_maps else None
        ws = torch.empty((lib.pd_polar_loss_rows(N, H, W), 11), dtype=torch.float64, device=dev)
        check(lib.pd_polar_loss_fwd_ray(ptr(depth), ptr(K), ptr(pol), ptr(xolp), ldp, ptr(valid), rho_min, rho_max, tilt2, sign,
                                        weighted, ray, ptr(state), ptr(record), ptr(values), ptr(maps), ptr(ws), ws.numel() * 8,
                                        N, H, W, stream_ptr()), "pd_polar_loss_fwd_ray")
        ctx.geom = (N, H, W, ldp, sign, weighted, ray)
        ctx.save_for_backward(depth, K, pol, xolp, state, record)
        if maps is None:
            maps = torch.empty(0, dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(state, record, maps)
        return values, state, record, maps

    @staticmethod
    def backward(ctx, gvalues, _gstate, _grecord, _gmaps):
        depth, K, pol, xolp, state, record = ctx.saved_tensors
        N, H, W, ldp, sign, weighted, ray = ctx.geom
        gdepth = torch.empty_like(depth)
        check(lib.pd_polar_loss_bwd_ray(ptr(depth), ptr(K), ptr(pol), ptr(xolp), ldp, ptr(state),
                                        ptr(gvalues.float().reshape(2).contiguous()), ptr(record), sign, weighted, ray, ptr(gdepth),
                                        N, H, W, stream_ptr()), "pd_polar_loss_bwd_ray")
        return gdepth, None, None, None, None, None, None, None


def polar_loss(depth, K, pol_normals, xolp, valid=None, rho_min=0.05, rho_max=1.0, tilt_min_deg=5.0, aolp_sign=1,
               dolp_weighted=True, details=False, ray_frame=False):
    """The polarimetric normals loss of a depth map -> (L_n, L_a): what ``polar_normals_eval.polar_normals_stats`` measures as
    the angle to the best candidate and the azimuth residual, as two smooth terms on the same per-pixel decisions,
    L_n = sum w (1 - cos n_deg) / sum w and L_a = sum w sin^2(az_deg) / sum w with w = DoLP (``dolp_weighted``) or 1.  It needs
    no ground truth and no pose.  Differentiable in ``depth`` only; the winner and the branch of a pixel are data.

    depth        [N,1,H,W] fp32;  K [N,4,4] intrinsics
    pol_normals  [N,9,H,W], xolp [N,2,H,W] as ``polar_normals_stats`` takes them (padded rows are read in place)
    valid        [N,1,H,W] or [N,H,W] bool / uint8 or None: a 0 takes the pixel out altogether
    rho_min, rho_max, tilt_min_deg, aolp_sign     the evaluator's options, with the evaluator's conventions
    details      also return a ``PolarLossDetails``
    ray_frame    form both terms in the frame of each pixel's viewing ray (the minimal rotation of the ray onto the optical
                 axis, include/polardepth.h) instead of the orthographic convention of calc_normals; the gradient comes back
                 through the transposed rotation.  No gradient with respect to K"""
    import math
    from ._records import frames
    from .polar_normals_eval import _planar
    _require_cuda(depth, K, pol_normals, xolp, valid)
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"polar_loss: depth must be [N,1,H,W], got {tuple(depth.shape)}")
    N, _, H, W = depth.shape
    if tuple(K.shape) != (N, 4, 4):
        raise ValueError(f"polar_loss: K must be [{N},4,4], got {tuple(K.shape)}")
    if tuple(pol_normals.shape) != (N, 9, H, W) or tuple(xolp.shape) != (N, 2, H, W):
        raise ValueError(f"polar_loss: pol_normals must be {(N, 9, H, W)} and xolp {(N, 2, H, W)}, got "
                         f"{tuple(pol_normals.shape)} and {tuple(xolp.shape)}")
    if aolp_sign not in (1, -1):
        raise ValueError(f"polar_loss: aolp_sign must be +1 or -1, got {aolp_sign!r}")
    if not 0.0 <= float(tilt_min_deg) < 90.0:
        raise ValueError(f"polar_loss: tilt_min_deg must be in [0, 90), got {tilt_min_deg!r}")
    if valid is not None:
        valid = frames(valid, "valid", N, H, W).ne(0).to(torch.uint8).contiguous()
    opts = (float(rho_min), float(rho_max), math.sin(math.radians(float(tilt_min_deg))) ** 2, int(aolp_sign), int(bool(dolp_weighted)),
            int(bool(ray_frame)))
    if N == 0:                           # nothing to launch: both values are 0, and so is the gradient
        dev = depth.device
        values = depth.float().sum() * torch.zeros(2, dtype=torch.float32, device=dev)
        out = PolarLossDetails(torch.empty((0, H, W), dtype=torch.uint8, device=dev),
                               torch.zeros(POLAR_LOSS_RECORD_BYTES, dtype=torch.uint8, device=dev),
                               torch.empty((0, H, W, 2), dtype=torch.float32, device=dev))
        return (values[0], values[1], out) if details else (values[0], values[1])
    pol, xl, ldp = _planar(pol_normals.detach(), xolp.detach(), H, W)
    with torch.cuda.device(depth.device):
        values, state, record, maps = _PolarLossFn.apply(depth.float().contiguous(), K.detach().float().contiguous(), pol, xl, ldp,
                                                         valid, opts, bool(details))
    if details:
        return values[0], values[1], PolarLossDetails(state, record, maps)
    return values[0], values[1]


def polar_refine(*args, **kwargs):
    """``polardepth.refine.polar_refine``: the depth refined with the polarisation normals it disambiguated."""
    from .refine import polar_refine as impl
    return impl(*args, **kwargs)


# ------------------------------------------------------------------ depth-uncertainty loss (csrc/unc_loss.hip)
UNCERTAINTY_RANGE = (0.0005, 0.5)       # (b_lo, b_hi) in metres: a convention (0.5 mm .. 0.5 m, u = 0.5 -> 15.8 mm), not a measurement


class UncertaintyLossDetails:
    """What ``uncertainty_loss(..., details=True)`` adds: ``sums`` float64 [4] (sum |g - d| / b, sum log 2b, sum m, sum b) and
    ``maps`` fp32 [N,H,W,2] = (the pixel's term, b in metres), NaN where a pixel is not under the mask.  On the device."""

    def __init__(self, sums, maps):
        self.sums, self.maps = sums, maps


def uncertainty_range(b_range):
    """(b_lo, b_hi) as floats; ``None`` is UNCERTAINTY_RANGE.  0 < b_lo < b_hi < inf or ValueError."""
    import math
    lo, hi = UNCERTAINTY_RANGE if b_range is None else b_range
    lo, hi = float(lo), float(hi)
    if not (0.0 < lo < hi and math.isfinite(hi)):
        raise ValueError(f"uncertainty range must be 0 < b_lo < b_hi < inf (metres), got ({lo!r}, {hi!r})")
    return lo, hi


class _UncLossFn(torch.autograd.Function):
    """pd_unc_loss_fwd / _bwd + pd_up_gather_bwd: returns (value [1], sums [4], maps); differentiable in the depth map (unless
    detached) and in the uncertainty map."""

    @staticmethod
    def forward(ctx, depth, unc, gt, ldg, valid, opts, detach, want_maps):
        N, _, H, W = depth.shape
        hs, ws = unc.shape[2], unc.shape[3]
        dev = depth.device
        min_d, max_d, b_lo, b_hi = opts
        sums = torch.zeros(4, dtype=torch.float64, device=dev)
        value = torch.zeros(1, dtype=torch.float32, device=dev)
        maps = torch.empty((N, H, W, 2), dtype=torch.float32, device=dev) if want_maps else None
        ws_ = torch.empty((lib.pd_unc_loss_rows(N, H, W), 4), dtype=torch.float64, device=dev)
        check(lib.pd_unc_loss_fwd(ptr(depth), ptr(gt), ldg, ptr(unc), hs, ws, ptr(valid), min_d, max_d, b_lo, b_hi, ptr(sums),
                                  ptr(value), ptr(maps), ptr(ws_), ws_.numel() * 8, N, H, W, stream_ptr()), "pd_unc_loss_fwd")
        ctx.geom = (N, H, W, hs, ws, ldg, opts, detach)
        ctx.save_for_backward(depth, unc, gt, valid, sums)
        if maps is None:
            maps = torch.empty(0, dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(sums, maps)
        return value, sums, maps

    @staticmethod
    def backward(ctx, gvalue, _gsums, _gmaps):
        depth, unc, gt, valid, sums = ctx.saved_tensors
        N, H, W, hs, ws, ldg, (min_d, max_d, b_lo, b_hi), detach = ctx.geom
        st = stream_ptr()
        gdepth = torch.empty_like(depth) if (ctx.needs_input_grad[0] and not detach) else None
        gup = torch.empty((N, 1, H, W), dtype=torch.float32, device=depth.device)
        check(lib.pd_unc_loss_bwd(ptr(depth), ptr(gt), ldg, ptr(unc), hs, ws, ptr(valid), min_d, max_d, b_lo, b_hi,
                                  ptr(gvalue.float().reshape(1).contiguous()), ptr(sums), ptr(gdepth), ptr(gup), N, H, W, st),
              "pd_unc_loss_bwd")
        gunc = None
        if ctx.needs_input_grad[1]:
            gunc = torch.empty_like(unc)
            generic = int(H % hs != 0 or W % ws != 0)
            check(lib.pd_up_gather_bwd(ptr(gup), ptr(gunc), N, hs, ws, H, W, 0, generic, st), "pd_up_gather_bwd")
        return gdepth, gunc, None, None, None, None, None, None


def uncertainty_loss(depth, gt, unc, b_range=None, min_depth=0.1, max_depth=2.0, valid=None, detach_depth=False, details=False):
    """The negative log-likelihood of the ground-truth depth under a Laplace error model whose scale the network states:
    L = sum m (|gt - depth| / b + log 2b) / sum m, with log b = log b_lo + u log(b_hi / b_lo) and u the uncertainty head's
    sigmoid output sampled to the frame (bilinear, align_corners=False, inside the kernel).  Definition:
    include/polardepth.h.  Returns the scalar loss (and an ``UncertaintyLossDetails``).

    depth         [N,1,H,W] fp32 full-resolution depth in metres
    gt            [N,1,H,W] or [N,H,W] ground truth; a view whose rows are padded is read in place
    unc           [N,1,hs,ws] the head's output, hs <= H and ws <= W at any ratio
    b_range       (b_lo, b_hi) in metres, None = UNCERTAINTY_RANGE.  A convention, not a measurement
    min_depth, max_depth   the supervised term's mask, min_depth <= gt <= max_depth
    valid         [N,1,H,W] or [N,H,W] bool / uint8 or None: a 0 takes the pixel out
    detach_depth  no gradient reaches ``depth`` (it is not formed): heads trained on top of a finished network
    details       also return an ``UncertaintyLossDetails``"""
    from ._records import frames
    _require_cuda(depth, gt, unc, valid)
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"uncertainty_loss: depth must be [N,1,H,W], got {tuple(depth.shape)}")
    N, _, H, W = depth.shape
    if unc.dim() != 4 or unc.shape[0] != N or unc.shape[1] != 1 or not (0 < unc.shape[2] <= H and 0 < unc.shape[3] <= W):
        raise ValueError(f"uncertainty_loss: unc must be [{N},1,hs,ws] with hs <= {H} and ws <= {W}, got {tuple(unc.shape)}")
    b_lo, b_hi = uncertainty_range(b_range)
    gt = frames(gt.detach(), "gt", N, H, W)
    if gt.dtype != torch.float32 or gt.stride(2) != 1 or gt.stride(1) < W or (N > 1 and gt.stride(0) != H * gt.stride(1)):
        gt = gt.float().contiguous()
    ldg = gt.stride(1)
    if valid is not None:
        valid = frames(valid, "valid", N, H, W).ne(0).to(torch.uint8).contiguous()
    opts = (float(min_depth), float(max_depth), b_lo, b_hi)
    if N == 0:                           # nothing to launch: the value is 0, and so is the gradient
        dev = depth.device
        value = (depth.float().sum() + unc.float().sum()) * 0.0
        out = UncertaintyLossDetails(torch.zeros(4, dtype=torch.float64, device=dev),
                                     torch.empty((0, H, W, 2), dtype=torch.float32, device=dev))
        return (value, out) if details else value
    with torch.cuda.device(depth.device):
        value, sums, maps = _UncLossFn.apply(depth.float().contiguous(), unc.float().contiguous(), gt, int(ldg), valid, opts,
                                             bool(detach_depth), bool(details))
    if details:
        return value[0], UncertaintyLossDetails(sums, maps)
    return value[0]


def disp_to_depth(disp, size, min_depth, max_depth, clamp=False):
    """The depth read-out of evaluation: a decoder's disparity [N,1,hs,ws] -> the depth in metres [N,1,H,W] at ``size`` =
    (H, W) (pd_disp_to_depth), with ``clamp`` limited to [min_depth, max_depth] afterwards.  The loss launches the same
    kernel for all its scales itself (functional.py)."""
    disp = disp.contiguous()
    N, (H, W) = disp.shape[0], size
    depth = torch.empty((N, 1, H, W), device=disp.device)
    check(lib.pd_disp_to_depth(ptr(disp), ptr(depth), None, N, disp.shape[2], disp.shape[3], H, W, min_depth, max_depth,
                               stream_ptr()), "pd_disp_to_depth")
    return depth.clamp(min_depth, max_depth) if clamp else depth


def depth_metrics(gt, pred, min_depth, max_depth, mask=None, mask_value=0):
    """Per-image depth metrics on the device: [N,8] = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, count."""
    _require_cuda(gt, pred, mask)
    gt, pred = gt.float().contiguous(), pred.float().contiguous()
    N = gt.shape[0]
    P = gt.numel() // N
    if mask is not None:
        mask = mask.to(torch.int32).contiguous()
    ws = torch.empty(N * 64 * 8, dtype=torch.float32, device=gt.device)
    out = torch.empty((N, 8), dtype=torch.float32, device=gt.device)
    check(lib.pd_depth_metrics(ptr(gt), ptr(pred), ptr(mask), int(mask_value), ptr(ws), ptr(out), N, P,
                               float(min_depth), float(max_depth), stream_ptr()), "pd_depth_metrics")
    return out


# ------------------------------------------------------------------ 7x7/s2 stems as 4x4/s1 over space-to-depth
def s2d_input(x, affine=None):
    """[N,C,H,W] (any strides) -> channels_last [N,4C,H/2,W/2] with q = (dy*2+dx)*C + c; optional (x-sub)/div."""
    _require_cuda(x)
    N, C, H, W = x.shape
    out = empty_nhwc(N, 4 * C, H // 2, W // 2, x.device)
    sub, div = affine if affine is not None else (0.0, 1.0)
    sN, sC, sH, sW = x.stride()
    check(lib.pd_stem_s2d_input(ptr(x), ptr(out), N, C, H, W, sN, sC, sH, sW, int(affine is not None), sub, div,
                                stream_ptr()), "pd_stem_s2d_input")
    return out


def s2d_weight(w):
    """[Co,C,7,7] (channels_last) -> channels_last [Co,4C,4,4]."""
    Co, C, KH, KW = w.shape
    assert KH == 7 and KW == 7
    w = weight_cl(w)
    w2 = torch.empty((Co, 4 * C, 4, 4), dtype=torch.float32, device=w.device, memory_format=CL)
    check(lib.pd_stem_s2d_weight(ptr(w), ptr(w2), Co, C, stream_ptr()), "pd_stem_s2d_weight")
    return w2


def s2d_weight_grad(dw2, dw, accumulate=True):
    """dW2 [Co,4C,4,4] (channels_last) -> (+)= dW [Co,C,7,7] (channels_last)."""
    Co, C = dw.shape[0], dw.shape[1]
    assert dw.is_contiguous(memory_format=CL) or C == 1
    check(lib.pd_stem_s2d_weight_grad(ptr(dw2), ptr(dw), Co, C, int(accumulate), stream_ptr()),
          "pd_stem_s2d_weight_grad")
    return dw


# ------------------------------------------------------------------ dense GEMMs on the conv kernels (attention)
def gemm_nt(a, b, out=None):
    """C[M,N] = A[M,K] @ B[N,K]^T (fp32 MFMA): pd_conv2d with a 1x1 filter, A as a [1,M,1,K] NHWC image."""
    _require_cuda(a, b)
    M, K = a.shape
    Nn, Kb = b.shape
    assert K == Kb and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty((M, Nn), dtype=torch.float32, device=a.device)
    _profiled(_igemm_label(M, Nn, K % 4 == 0, "gemm", K), 2.0 * M * Nn * K,
              lambda: check(lib.pd_conv2d(ptr(a), ptr(b), None, None, ptr(out), None, 1, M, 1, K, M * K, K, K, 1,
                                          M, 1, Nn, 1, 1, 1, 0, MODE_ZERO, ACT_NONE, 0, 0.0, 1.0, out.stride(0),
                                          CONV_FLAGS, stream_ptr()), "pd_conv2d(gemm_nt)"))
    return out


def gemm_tn(dy, x):
    """C[N,K] = dY[M,N]^T @ X[M,K] (contraction over rows): pd_conv2d_wgrad with a 1x1 filter."""
    _require_cuda(dy, x)
    M, Nn = dy.shape
    Mx, K = x.shape
    assert M == Mx and dy.is_contiguous() and x.is_contiguous()
    out = torch.empty((Nn, K), dtype=torch.float32, device=x.device)
    nbytes = lib.pd_conv2d_wgrad_workspace(M, Nn, K, WGRAD_FLAGS)
    ws = _workspace(nbytes, x.device)
    _profiled("conv_wgrad_kernel", 2.0 * M * Nn * K,
              lambda: check(lib.pd_conv2d_wgrad(ptr(x), ptr(dy), ptr(out), None, ptr(ws), ws.numel(), 1, M, 1, K,
                                                M * K, K, K, 1, M, 1, Nn, 1, 1, 1, 0, MODE_ZERO, 0, 0.0, 1.0, Nn, 0,
                                                WGRAD_FLAGS, stream_ptr()), "pd_conv2d_wgrad(gemm_tn)"))
    return out


def transpose2d(a, out=None):
    """[R,C] -> [C,R] (pd_weight_transpose)."""
    R, C = a.shape
    if out is None:
        out = torch.empty((C, R), dtype=torch.float32, device=a.device)
    assert out.shape == (C, R) and out.is_contiguous() and a.is_contiguous()
    check(lib.pd_weight_transpose(ptr(a), ptr(out), R, 1, C, stream_ptr()), "pd_weight_transpose")
    return out


def softmax_rows_(x, scale):
    R, L = x.shape
    check(lib.pd_softmax_rows_fwd(ptr(x), R, L, float(scale), stream_ptr()), "pd_softmax_rows_fwd")
    return x


def softmax_rows_bwd_(p, dp, scale):
    R, L = p.shape
    check(lib.pd_softmax_rows_bwd(ptr(p), ptr(dp), R, L, float(scale), stream_ptr()), "pd_softmax_rows_bwd")
    return dp
