"""Frame and mask pyramids on the HIP path: what a multi-scale label-free loss reads at every level (csrc/pwc_pyramid.hip).

    frame_pyramid(frames, factors=(64, 32, 16, 8, 4))                                     -> list of float32 (N, H/f, W/f, C)
    mask_pyramid(valid, factors=(64, 32, 16, 8, 4), min_fraction=1.0, return_counts=False) -> list of torch.bool (N, H/f, W/f)
    level_flow_scale(level_flow, frame_hw)                                                 -> the `flow_scale=` of that level

PWCDCNetModule returns a differentiable flows_pyramid and every data term of pwcnet_amd/unsup.py takes `flow_scale=` with
frames "the caller has downsampled"; this module is that caller.  frame_pyramid is the block mean (area downsampling, what
UnFlow, DDFlow and ARFlow put their per-level losses on): each output element is the mean of its f x f block, the sum formed
in double and rounded to float32 once.  mask_pyramid brings an occlusion mask to the same sizes: a level pixel is kept when at
least min_fraction of its block is valid.  All requested levels come from ONE launch that reads the input once; uint8 frames are
read as they are (value v enters as the float32 nearest v / 255, fit_frames' convention).  The order of every sum is fixed by
the cell, so two calls give the same bits and an image gives the same bits alone and in a batch; for uint8 frames the sums are
exact in double (include/pwc_hip.h).  No autograd: the pyramids are constants of the loss, as the frames and the
masks are.
"""
import ctypes
import math

import torch

from . import _lib

FACTORS = (2, 4, 8, 16, 32, 64)
DEFAULT_FACTORS = (64, 32, 16, 8, 4)          # flows_pyramid's order, coarse -> fine


def _check_factors(factors, H, W, what):
    try:
        fs = tuple(factors)
    except TypeError:
        raise TypeError(f"{what}: factors must be a sequence of integers, got {factors!r}") from None
    if not 1 <= len(fs) <= len(FACTORS):
        raise ValueError(f"{what}: 1 to {len(FACTORS)} factors are required, got {fs!r}")
    for f in fs:
        if isinstance(f, bool) or not isinstance(f, int):
            raise TypeError(f"{what}: factors must be integers, got {f!r} in {fs!r}")
        if f not in FACTORS:
            raise ValueError(f"{what}: factor {f} is not one of {FACTORS}")
    if len(set(fs)) != len(fs):
        raise ValueError(f"{what}: a factor is given twice in {fs!r}")
    if H % max(fs) or W % max(fs):
        raise ValueError(f"{what}: height and width must be multiples of the largest factor {max(fs)}, got {H} x {W}")
    return fs


def _check_device(t, what):
    """The device check, the last of all: everything before it can be tested on CPU tensors."""
    if not t.is_cuda:
        raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only")


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def need_counts(factors, min_fraction):
    """The valid pixels a block needs, per factor: max(1, ceil(min_fraction * f * f)) -- exact, f * f is a power of two."""
    min_fraction = float(min_fraction)
    if not 0.0 < min_fraction <= 1.0:
        raise ValueError(f"mask_pyramid: min_fraction must lie in (0, 1], got {min_fraction}")
    return [max(1, math.ceil(min_fraction * f * f)) for f in factors]


def frame_pyramid(frames, factors=DEFAULT_FACTORS):
    """frames: (N, H, W, C) torch.uint8 or torch.float32, C = 1..4, contiguous, on the GPU.  factors: 1 to 6 distinct values out
    of 2, 4, 8, 16, 32, 64 in any order; H and W must be multiples of the largest.  Returns a list of contiguous float32
    tensors (N, H/f, W/f, C) in the order of `factors` -- the default matches flows_pyramid, coarse -> fine.  Each element is
    the mean of its f x f block, the sum formed in double, divided by f^2 and rounded to float32 once; a uint8 value v enters as
    the float32 nearest v / 255.  One launch on the current stream reads every input element once.  Two calls give the same
    bits; a NaN or Inf makes the cells that contain it non-finite and nothing else.  No autograd: the result is a constant (a
    frames tensor that requires grad is refused)."""
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"frames: expected a torch.uint8 or torch.float32 tensor, got "
                        f"{frames.dtype if isinstance(frames, torch.Tensor) else type(frames)}")
    if frames.dim() != 4 or not 1 <= frames.shape[3] <= 4 or min(frames.shape) < 1:
        raise ValueError(f"frames: expected an (N, H, W, C) tensor with 1 to 4 channels, got shape {tuple(frames.shape)}")
    N, H, W, C = frames.shape
    fs = _check_factors(factors, H, W, "frame_pyramid")
    if not frames.is_contiguous():
        raise ValueError(f"frames: a dense (contiguous) tensor is required, got strides {frames.stride()}")
    if frames.requires_grad:
        raise ValueError("frames: the pyramid has no gradient (the frames require grad); detach() them")
    _check_device(frames, "frames")
    outs = [torch.empty((N, H // f, W // f, C), dtype=torch.float32, device=frames.device) for f in fs]
    with torch.cuda.device(frames.device):
        _lib.check(_lib.lib().pwc_frame_pyramid_f32(ctypes.c_void_p(frames.data_ptr()), int(frames.dtype == torch.uint8), N, H, W, C,
                                                    (ctypes.c_int * len(fs))(*fs), _pointers(outs), len(fs),
                                                    _lib.current_stream()), "pwc_frame_pyramid_f32")
    return outs


def mask_pyramid(valid, factors=DEFAULT_FACTORS, min_fraction=1.0, return_counts=False):
    """valid: (N, H, W) torch.bool or torch.uint8 (non-zero = valid: grad_ops.mask_ptr's format), contiguous, on the GPU.
    Returns a list of contiguous torch.bool tensors (N, H/f, W/f) in the order of `factors`: a level pixel is True when at
    least max(1, ceil(min_fraction * f * f)) pixels of its f x f block are valid, counted in integers.  They go straight into
    `valid=` of the data terms.  min_fraction = 1.0 (the default) is a min-pool: a level pixel counts only where its whole block
    does; a min_fraction of 1 / 4096 or below is a max-pool.  train.py uses 0.5 -- a choice: nobody has trained with it yet.
    return_counts: also the list of int32 (N, H/f, W/f) counts.  One launch on the current stream; the masks are constants."""
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"valid: expected a torch.bool or torch.uint8 tensor, got "
                        f"{valid.dtype if isinstance(valid, torch.Tensor) else type(valid)}")
    if valid.dim() != 3 or min(valid.shape) < 1:
        raise ValueError(f"valid: expected an (N, H, W) tensor, got shape {tuple(valid.shape)}")
    N, H, W = valid.shape
    fs = _check_factors(factors, H, W, "mask_pyramid")
    need = need_counts(fs, min_fraction)
    if not valid.is_contiguous():
        raise ValueError(f"valid: a dense (contiguous) tensor is required, got strides {valid.stride()}")
    _check_device(valid, "valid")
    outs = [torch.empty((N, H // f, W // f), dtype=torch.bool, device=valid.device) for f in fs]
    counts = [torch.empty((N, H // f, W // f), dtype=torch.int32, device=valid.device) for f in fs] if return_counts else None
    with torch.cuda.device(valid.device):
        _lib.check(_lib.lib().pwc_mask_pyramid_u8(ctypes.c_void_p(valid.data_ptr()), N, H, W, (ctypes.c_int * len(fs))(*fs),
                                                  (ctypes.c_int * len(fs))(*need), _pointers(outs),
                                                  _pointers(counts) if return_counts else None, len(fs),
                                                  _lib.current_stream()), "pwc_mask_pyramid_u8")
    return (outs, counts) if return_counts else outs


def level_flow_scale(level_flow, frame_hw):
    """The `flow_scale=` that takes a flows_pyramid entry (N, h, w, 2), in px / 20 of the full frame, to pixels of its own
    level: 20 * w / W with frame_hw = (H, W) the frame's size (20 / 2^level for PWCDCNet's levels).  Host arithmetic."""
    H, W = (int(v) for v in frame_hw)
    if H < 1 or W < 1:
        raise ValueError(f"level_flow_scale: frame_hw must be positive, got {tuple(frame_hw)!r}")
    return 20.0 * level_flow.shape[2] / W
