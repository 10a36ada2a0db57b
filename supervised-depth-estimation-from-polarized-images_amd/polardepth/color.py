"""The colour half of a HAMMER item on the GPU: the ``color`` / ``color_aug`` pyramids of indoor_dataset.py:192-233 (four
successive LANCZOS resizes, torchvision 0.8.2's PIL ColorJitter on every scale for an augmented item, uint8 -> float32 / 255)
from the decoded frame, bit for bit what the PIL path of ``manydepth.datasets`` gives (tests/test_color_gpu.py).

The jitter of one item travels as a float64 row of 8 = (code, value) x 4 in the order the operations are applied
(``pack_jitter``); the kernel reads the rows from device memory, so a captured training step replays with new draws."""
import numpy as np
import torch

from ._lib import lib, check, ptr, stream_ptr
from .resize import resize_lanczos_u8

CODES = {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4}
WS_BYTES_PER_SAMPLE = 16          # sum_ws of pd_color_jitter_u8 (include/polardepth.h)


def pack_jitter(params):
    """The list ``datasets.color_jitter_params()`` returns ([(name, factor)] * 4, in order of application) -> float64 [8];
    None (a plain item) -> zeros, which the kernel copies."""
    row = np.zeros(8, np.float64)
    if params is not None:
        if len(params) > 4:
            raise ValueError(f"pack_jitter: a row holds at most 4 operations, got {len(params)}")
        for k, (name, value) in enumerate(params):
            row[2 * k] = CODES[name]
            row[2 * k + 1] = value
    return row


_WS = {}


def _workspace(B, device):
    """Zeroed once; every call leaves its sum / ticket words zero again (the entry / exit contract of sum_ws)."""
    ws = _WS.get(device.index)
    if ws is None or ws.numel() < B * WS_BYTES_PER_SAMPLE:
        ws = torch.zeros(max(B, 64) * WS_BYTES_PER_SAMPLE, dtype=torch.uint8, device=device)
        _WS[device.index] = ws
    return ws


def color_jitter_u8(x, params, want=("f32",)):
    """x: uint8 CUDA tensor [B,3,H,W]; params: float64 [B,8] rows of ``pack_jitter`` (any device; None = identity).
    want: "u8" and / or "f32" -> dict with the jittered image as uint8 and / or as float32 in [0, 1]."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8):
        raise RuntimeError("color_jitter_u8 needs a CUDA(HIP) uint8 tensor; there is no CPU fallback (PIL is the CPU path)")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"color_jitter_u8: expected [B,3,H,W], got {tuple(x.shape)}")
    want = tuple(want)
    if not want or any(w not in ("u8", "f32") for w in want):
        raise ValueError(f"color_jitter_u8: want must name 'u8' and / or 'f32', got {want!r}")
    B, _, H, W = x.shape
    x = x.contiguous()
    ws = None
    if params is not None:
        params = torch.as_tensor(params)
        if tuple(params.shape) != (B, 8) or params.dtype != torch.float64:
            raise ValueError(f"color_jitter_u8: params must be float64 [{B}, 8], got {params.dtype} {tuple(params.shape)}")
        params = params.to(x.device).contiguous()
        ws = _workspace(B, x.device)
    out = {}
    if "u8" in want:
        out["u8"] = torch.empty_like(x)
    if "f32" in want:
        out["f32"] = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.pd_color_jitter_u8(ptr(x), ptr(params), ptr(out.get("u8")), ptr(out.get("f32")), ptr(ws), B, H, W,
                                     stream_ptr()), "pd_color_jitter_u8")
    return out


def color_pyramid(raw_u8, jitter, size, num_scales=4):
    """raw_u8: uint8 CUDA [B,3,Hf,Wf], the decoded frames; jitter: float64 [B,8] or None; size = (H, W).
    Returns ("color", 0, s) and ("color_aug", 0, s), float32 [B,3,H>>s,W>>s], s < num_scales.  The resizes are successive
    (frame -> scale 0 -> scale 1 ...) and the jitter is taken of each scale's uint8 image -- the contrast mean per scale --
    as on the host.  Without jitter ``color_aug`` IS ``color`` (the same tensors)."""
    if not (isinstance(raw_u8, torch.Tensor) and raw_u8.is_cuda and raw_u8.dtype == torch.uint8):
        raise RuntimeError("color_pyramid needs a CUDA(HIP) uint8 tensor; there is no CPU fallback (PIL is the CPU path)")
    H, W = int(size[0]), int(size[1])
    out = {}
    prev = raw_u8
    for s in range(num_scales):
        prev = resize_lanczos_u8(prev, (H >> s, W >> s))
        out[("color", 0, s)] = color_jitter_u8(prev, None)["f32"]
        out[("color_aug", 0, s)] = out[("color", 0, s)] if jitter is None else color_jitter_u8(prev, jitter)["f32"]
    return out


def expand_batch(inputs, size, num_scales=4, cdofp=None, calibration=None):
    """What Trainer.process_batch / Evaluation.predict do with a raw-colour batch (HAMMER_Dataset(raw_color=True)): when
    ("color_raw", 0, 0) is there and ("color", 0, 0) is not, add the eight pyramid tensors to ``inputs``.  A colour sensor
    frame ("pol_cdofp", 0, 0) is demosaicked into ("color_raw", 0, 0) and ("pol", 0, 0) first (``polardepth.cdofp.expand``,
    ``cdofp`` = its options, ``calibration`` = the sensor's ``polardepth.calibration.Calibration``, applied before the
    demosaic): one launch, shared with ``polardepth.polar.polar_inputs``."""
    if ("pol_cdofp", 0, 0) in inputs:
        from . import cdofp as pdcdofp
        pdcdofp.expand(inputs, cdofp, calibration=calibration)
    if ("color_raw", 0, 0) in inputs and ("color", 0, 0) not in inputs:
        inputs.update(color_pyramid(inputs[("color_raw", 0, 0)], inputs.get("color_jitter"), size, num_scales))
    return inputs
