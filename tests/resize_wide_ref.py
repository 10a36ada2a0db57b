"""Shared by tests/test_resize_wide.py and tests/test_resize_wide_gpu.py: the cases of the 16-bit / float LANCZOS resize, their
seeded inputs, PIL's answer (computed once per case) and a NumPy restatement of the two arithmetics of Pillow's Resample.c
(ImagingResampleHorizontal_16bpc / Vertical_16bpc for mode I;16, the float case of the _32bpc pair for mode F):

    ss = 0.0; for x in taps: ss += (double)in[x] * k[x]          multiply and add rounded separately (one ufunc each)
    F:     out = (float)ss
    I;16:  v = ROUND_UP(ss); low byte = CLIP8(v % 256) with C's remainder, high byte = CLIP8(v >> 8)

with k = precompute_coeffs' w[x] / ww in double (no 8bpc normalisation), a horizontal pass, then a vertical pass; a pass
whose size does not change is skipped; the image between the passes has the mode's own type."""
import functools
import math

import numpy as np

# (Hs, Ws, Hd, Wd, hi): uint16 values in [0, hi), float32 values in [-1e4, 1e4]
CASES = [(37, 53, 16, 20, 4096),         # downscale
         (26, 34, 16, 24, 65536),        # downscale, full 16-bit range
         (19, 40, 32, 64, 65536),        # upscale
         (33, 27, 16, 24, 65536),        # downscale
         (33, 27, 33, 24, 4096),         # vertical pass skipped
         (33, 27, 16, 27, 4096)]         # horizontal pass skipped
DTYPES = ("uint16", "float32")
MODES = {"uint16": "I;16", "float32": "F"}
F_MAX = 1.0e4


def _lanczos(x):
    def sinc(v):
        if v == 0.0:
            return 1.0
        v *= math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def coeffs(in_size, out_size):
    """precompute_coeffs: (k float64 [out_size, ksize], bounds int32 [out_size, 2] = (first input index, count))"""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.float64)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ww = 0.0
        for x in range(xmax):
            w = _lanczos((x + xmin - center + 0.5) * ss)
            kk[xx, x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                kk[xx, x] /= ww
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _store(ss, dtype, stats):
    if dtype == np.float32:
        return ss.astype(np.float32)
    v = np.where(ss >= 0.0, np.trunc(ss + 0.5), np.trunc(ss - 0.5)).astype(np.int64)      # ROUND_UP, (int) truncates
    stats["over"] = int((v > 65535).sum())
    stats["under"] = int((v < 0).sum())
    low = np.clip(np.fmod(v, 256), 0, 255)        # fmod: the sign of the dividend, like C's %
    high = np.clip(v >> 8, 0, 255)                # arithmetic shift
    return (low | (high << 8)).astype(np.uint16)


def _pass(img, out_size, axis, stats):
    """one pass along `axis` (-1 horizontal, -2 vertical) of [..., H, W]"""
    src = np.moveaxis(img, axis, -1)
    kk, bounds = coeffs(src.shape[-1], out_size)
    acc = np.zeros(src.shape[:-1] + (out_size,), np.float64)
    for xx in range(out_size):
        xmin, xn = bounds[xx]
        ss = np.zeros(src.shape[:-1], np.float64)
        for x in range(xn):
            ss = ss + src[..., xmin + x].astype(np.float64) * kk[xx, x]
        acc[..., xx] = ss
    return np.ascontiguousarray(np.moveaxis(_store(acc, img.dtype, stats), -1, axis))


def restate(img, size):
    """img [..., Hs, Ws] uint16 or float32, size = (Hd, Wd) -> (resized [..., Hd, Wd], stats of the LAST pass that ran:
    over / under = outputs whose rounded sum lay above 65535 / below 0 before the bytewise store; uint16 only)"""
    assert img.dtype in (np.uint16, np.float32)
    Hd, Wd = size
    stats = {"over": 0, "under": 0}
    with np.errstate(all="ignore"):
        if Wd != img.shape[-1]:
            img = _pass(img, Wd, -1, stats)
        if Hd != img.shape[-2]:
            img = _pass(img, Hd, -2, stats)
    return img, stats


@functools.lru_cache(maxsize=None)
def planes(case, dtype):
    """[2,4,Hs,Ws] seeded planes: random values everywhere; plane [0,0] is a board of 4x4 blocks of the largest value next
    to blocks of the smallest (hard edges: the filter rings past both ends of the range); plane [1,3] holds such blocks in
    its top-left corner only.  Read-only."""
    Hs, Ws, _, _, hi = case
    rng = np.random.default_rng(sum(case))
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    board = ((yy // 4 + xx // 4) % 2).astype(bool)
    if dtype == "uint16":
        p = rng.integers(0, hi, (2, 4, Hs, Ws)).astype(np.uint16)
        top, bottom = hi - 1, 0
    else:
        p = rng.uniform(-F_MAX, F_MAX, (2, 4, Hs, Ws)).astype(np.float32)      # fractional parts, both signs
        top, bottom = F_MAX, -F_MAX
    p[0, 0] = np.where(board, top, bottom)
    p[1, 3, :12, :12] = np.where(board[:12, :12], top, bottom)
    assert np.isfinite(p.astype(np.float64)).all() and np.abs(p.astype(np.float64)).max() <= max(F_MAX, hi)
    p.setflags(write=False)
    return p


def pil_resize(plane, size):
    """Image.resize(..., Image.LANCZOS) of one [H,W] uint16 / float32 plane in mode I;16 / F"""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(plane))
    assert im.mode == MODES[str(plane.dtype)], im.mode
    out = np.asarray(im.resize((size[1], size[0]), Image.LANCZOS))
    assert out.dtype == plane.dtype and out.shape == tuple(size)
    return out


@functools.lru_cache(maxsize=None)
def pil_planes(case, dtype):
    """PIL's answer for planes(case, dtype), plane by plane: [2,4,Hd,Wd].  Read-only."""
    p = planes(case, dtype)
    out = np.stack([np.stack([pil_resize(p[b, c], case[2:4]) for c in range(4)]) for b in range(2)])
    out.setflags(write=False)
    return out


def bits(a):
    """what is compared: the values themselves for uint16, the bit patterns for float32"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
