"""Flow at any frame size: fit the frames to the network's geometry, refit the flow to the frames' grid.

PWCDCNet takes frames whose height and width are multiples of 64 (six stride-2 levels).  `fit_frames` brings frames of any
size to the next multiples of 64 -- mode "resize": half-pixel bilinear, what the PWC-Net authors do; mode "pad": the last row
and column repeated, what RAFT-style code does -- and `refit_flow` brings the flow back: resized and rescaled by W / FW and
H / FH, or cropped.  Each is ONE launch of csrc/pwc_fit.hip on plain dense tensors, in front of and behind the forward; the
model, its launch plan and the pipeline are not involved.  `flow_any_size` is the three steps in a row.

Arithmetic (include/pwc_hip.h): exact integer sample coordinates, every value formed in double and rounded to
float32 once; an axis that already fits is copied, a frame that fits on both passes through untouched.  uint8 frames are read
as they are (value v enters as the float32 nearest v / 255, the float the command lines formed on the host before): a quarter
of the bytes to upload.  No autograd: training works on crops.
"""
import collections
import ctypes

import torch

from . import _lib

MODES = {"resize": _lib.FIT_RESIZE, "pad": _lib.FIT_PAD}

FitInfo = collections.namedtuple("FitInfo", ["mode", "H", "W", "FH", "FW"])
FitInfo.__doc__ = """What fit_frames did: `mode` ("resize" / "pad"), the frames' size (H, W) and the network geometry (FH, FW).
A flow at network geometry is in network pixels: in mode "resize" u scales by W / FW and v by H / FH on the way back."""


def ceil_to(n, factor=64):
    return -(-int(n) // factor) * factor


def fit_info(H, W, mode="resize", factor=64):
    """The FitInfo of (H, W) frames (host arithmetic only)."""
    if mode not in MODES:
        raise ValueError(f"fit: unknown mode {mode!r} (one of {sorted(MODES)})")
    if int(factor) < 1 or int(H) < 1 or int(W) < 1:
        raise ValueError(f"fit: frame size {H} x {W} and factor {factor} must be positive")
    return FitInfo(mode, int(H), int(W), ceil_to(H, factor), ceil_to(W, factor))


def _check(t, what, channels, dtypes):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a torch tensor is required, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: a CUDA (HIP) tensor is required, got one on {t.device}")
    if t.dtype not in dtypes:
        raise ValueError(f"{what}: dtype {t.dtype} is not one of {[str(d) for d in dtypes]}")
    if t.dim() != 4 or t.shape[3] != channels or min(t.shape) < 1:
        raise ValueError(f"{what}: shape (N, H, W, {channels}) is required, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: a dense (contiguous) tensor is required, got strides {t.stride()}")


def fit_frames(images, mode="resize", factor=64):
    """(N, H, W, 3) uint8 or float32 frames on the GPU -> (fitted, info): fitted (N, FH, FW, 3) float32 with FH, FW the next
    multiples of `factor`, info the FitInfo that refit_flow takes.  Frames that already fit: a float32 input is returned
    itself, a uint8 one is converted (v / 255) by the same launch.  One launch on the current stream."""
    _check(images, "fit_frames", 3, (torch.uint8, torch.float32))
    N, H, W, _ = images.shape
    info = fit_info(H, W, mode, factor)
    if (info.FH, info.FW) == (H, W) and images.dtype == torch.float32:
        return images, info
    out = torch.empty((N, info.FH, info.FW, 3), dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        _lib.check(_lib.lib().pwc_fit_frames_f32(ctypes.c_void_p(images.data_ptr()), int(images.dtype == torch.uint8),
                                                 ctypes.c_void_p(out.data_ptr()), N, H, W, info.FH, info.FW, MODES[mode],
                                                 _lib.current_stream()), "pwc_fit_frames_f32")
    return out, info


def refit_flow(flow, info):
    """(N, FH, FW, 2) float32 flow at network geometry -> (N, H, W, 2) on the frames' grid, in frame pixels.  When nothing
    was fitted, `flow` itself is returned.  One launch on the current stream."""
    _check(flow, "refit_flow", 2, (torch.float32,))
    if info.mode not in MODES:
        raise ValueError(f"refit_flow: unknown mode {info.mode!r}")
    N, FH, FW, _ = flow.shape
    if (FH, FW) != (info.FH, info.FW):
        raise ValueError(f"refit_flow: the flow is {FH} x {FW}, the fit was to {info.FH} x {info.FW}")
    if (info.FH, info.FW) == (info.H, info.W):
        return flow
    out = torch.empty((N, info.H, info.W, 2), dtype=torch.float32, device=flow.device)
    with torch.cuda.device(flow.device):
        _lib.check(_lib.lib().pwc_refit_flow_f32(ctypes.c_void_p(flow.data_ptr()), ctypes.c_void_p(out.data_ptr()), N, FH, FW,
                                                 info.H, info.W, MODES[info.mode], _lib.current_stream()), "pwc_refit_flow_f32")
    return out


def flow_any_size(net, images_0, images_1, mode="resize"):
    """net(images_0, images_1) for frames of any size: fit both frames, run `net` (a PWCDCNet, or any callable with its
    signature) on the fitted frames, refit the final flow.  Returns (flows_final, flows_pyramid): flows_final is
    (N, H, W, 2) on the frames' grid in frame pixels; flows_pyramid is what `net` returned, LEFT AT NETWORK GEOMETRY
    (levels of the fitted FH x FW frames, in the network's units) -- fit_info(H, W, mode) gives the scales W / FW, H / FH.

    With a ForwardPipeline the steps are the caller's: fit_frames before submit(), refit_flow on ticket.result() after
    synchronize() (README.md)."""
    x0, info = fit_frames(images_0, mode)
    x1, info_1 = fit_frames(images_1, mode)
    if info != info_1 or x0.shape != x1.shape:
        raise ValueError(f"flow_any_size: the frames differ in shape, {tuple(images_0.shape)} and {tuple(images_1.shape)}")
    flows_final, flows_pyramid = net(x0, x1)
    return refit_flow(flows_final.contiguous(), info), flows_pyramid
