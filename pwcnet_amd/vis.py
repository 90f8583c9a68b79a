"""Flow visualisation on the HIP path: colour coding, pyramid montage, error maps (csrc/pwc_flowvis.hip).

    flow_max_radius(flows, valid=None, flow_scale=1.0)               -> (N,) float64
    flow_to_color(flows, max_rad=None, valid=None, flow_scale=1.0)   -> (N,H,W,3) uint8
    flow_error_color(flows, flows_gt, valid=None)                    -> (N,H,W,3) uint8
    pyramid_montage(frames, flows_list, flow_scales=None)            -> (N,h,W_total,3) uint8

flow_to_color is flow_io.flow_to_color (the Middlebury wheel: hue = direction, saturation = magnitude / max_rad) restated as the
same sequence of IEEE double operations on the GPU; atan2 is the only operation that may differ from numpy's, so a byte differs
from the host function's only where 255 * col lies within about 1e-11 of an integer.  flow_max_radius equals numpy's maximum bit
for bit.  flow_error_color is the log colour scale of KITTI's development kit, exact.  pyramid_montage is
infer_continuous.pyramid_montage for a batch: ONE launch writes the frame and up to seven colour-coded flows, each read nearest
neighbour at the frame's height, into one picture per image.  Flows are read in place (channel slices of wider buffers), a flow's
scale is one float32 product per component (what `f * (20.0 / 2 ** (num_levels - l))` does to a float32 array).  Unknown pixels
(flow_io.flow_valid's rule: a component that is not finite or above 1e9) and masked ones are drawn as zero flow -- white.  Every
launch goes on the current stream, nothing is copied to the host.  No autograd: pictures are constants.
"""
import math

import numpy as np
import torch

from . import _lib
from .modules import _p, as_view

WHEEL_ENTRIES = 55
MAX_MONTAGE_FLOWS = _lib.VIS_MAX_TILES - 1


def wheel():
    """(55, 3) uint8: the colour wheel the kernel reads (flow_io.color_wheel(), a constant table of the library)."""
    out = np.zeros((WHEEL_ENTRIES, 3), np.uint8)
    _lib.check(_lib.lib().pwc_flow_vis_wheel_u8(_p(out.ctypes.data)), "flow vis wheel")
    return out


def _check_flows(flows, what, like=None, like_name="flows"):
    """Type, rank and shape of a flow argument, named after it: a ValueError each."""
    if not isinstance(flows, torch.Tensor) or flows.dtype != torch.float32:
        raise ValueError(f"{what}: expected a torch.float32 tensor, got "
                         f"{flows.dtype if isinstance(flows, torch.Tensor) else type(flows)}")
    if flows.dim() != 4 or flows.shape[3] != 2:
        raise ValueError(f"{what}: expected an NHWC tensor with 2 channels, got shape {tuple(flows.shape)}")
    if min(flows.shape) <= 0:
        raise ValueError(f"{what}: empty tensor, shape {tuple(flows.shape)}")
    if like is not None and tuple(flows.shape) != tuple(like.shape):
        raise ValueError(f"{what}: expected shape {tuple(like.shape)}, {like_name}'s, got {tuple(flows.shape)}")


def _check_mask(mask, what, shape, like):
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: expected a torch.bool or torch.uint8 tensor, got "
                         f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask)}")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, {like}'s (N, H, W), got {tuple(mask.shape)}")
    if not mask.is_contiguous():
        raise ValueError(f"{what}: the mask must be contiguous")


def _check_scale(flow_scale, what="flow_scale"):
    if isinstance(flow_scale, bool) or not isinstance(flow_scale, (int, float)) or not math.isfinite(flow_scale):
        raise ValueError(f"{what}: expected a finite number, got {flow_scale!r}")
    return float(flow_scale)


def _check_device(first, **tensors):
    """The device last of all, each tensor named after its argument (compose._check_compose's order)."""
    for what, t in tensors.items():
        if t is not None and (not t.is_cuda or t.device != first.device):
            raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only, all arguments on one device")


def _check_max_rad(max_rad, N):
    """None, a non-negative finite number, or an (N,) float64 tensor (its values stay on the device: they are not read here)."""
    if max_rad is None or isinstance(max_rad, torch.Tensor):
        if max_rad is not None and (max_rad.dtype != torch.float64 or tuple(max_rad.shape) != (N,) or not max_rad.is_contiguous()):
            raise ValueError(f"max_rad: expected a contiguous ({N},) torch.float64 tensor, one radius per image, got "
                             f"{max_rad.dtype} {tuple(max_rad.shape)}")
        return
    if isinstance(max_rad, bool) or not isinstance(max_rad, (int, float)):
        raise ValueError(f"max_rad: expected None, a number or an ({N},) torch.float64 tensor, got {type(max_rad)}")
    if not math.isfinite(max_rad) or max_rad < 0:
        raise ValueError(f"max_rad: expected a finite radius >= 0, got {max_rad!r}")


def _mask_ptr(mask):
    return None if mask is None else mask.data_ptr()


def _max_radius(view, valid, flow_scale, dev):
    out = torch.empty((view.N,), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().pwc_flow_max_radius_f64(_p(view.ptr), view.cs, _p(_mask_ptr(valid)), view.N, view.H, view.W, flow_scale,
                                                  _p(out.data_ptr()), _lib.current_stream()), "flow max radius")
    return out


def _flow_tile(view, valid, max_rad, flow_scale, x0, tile_w):
    return _lib.VisTile(src=view.ptr, gt=None, valid=_mask_ptr(valid), max_rad=max_rad.data_ptr(), kind=_lib.VIS_FLOW,
                        src_cs=view.cs, gt_cs=0, src_h=view.H, src_w=view.W, x0=x0, tile_w=tile_w, flow_scale=flow_scale)


def _launch(tiles, N, out_h, out_w, dev):
    out = torch.empty((N, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    table = (_lib.VisTile * len(tiles))(*tiles)
    _lib.check(_lib.lib().pwc_flow_vis_tiles_u8(_lib.ctypes.cast(table, _lib.ctypes.c_void_p), len(tiles), N, out_h, out_w,
                                                _p(out.data_ptr()), _lib.current_stream()), "flow vis tiles")
    return out


def flow_max_radius(flows, valid=None, flow_scale=1.0):
    """(N,) float64 on the device: per image the largest sqrt(u u + v v) of flows * flow_scale over the pixels that are known
    (flow_io.flow_valid: both components finite, |.| <= 1e9) and, where valid is given, set in it; 0 for an image without one.
    flows: (N,H,W,2) float32, a channel slice of a wider buffer is read in place; valid: (N,H,W) torch.bool / torch.uint8,
    contiguous.  The product with flow_scale is one float32 product, the radius a double: numpy's value bit for bit, the same
    bits from every call, alone and in a batch (pwc_flow_max_radius_f64: an integer atomic max on the bits)."""
    _check_flows(flows, "flows")
    _check_mask(valid, "valid", tuple(flows.shape[:3]), "flows")
    flow_scale = _check_scale(flow_scale)
    _check_device(flows, flows=flows, valid=valid)
    fv, flows = as_view(flows.detach(), "flows")
    return _max_radius(fv, valid, flow_scale, flows.device)


def flow_to_color(flows, max_rad=None, valid=None, flow_scale=1.0):
    """(N,H,W,3) torch.uint8 RGB: flow_io.flow_to_color of every image of flows * flow_scale, on the GPU.
    max_rad: None -- each image's own maximum (flow_max_radius(flows, valid, flow_scale): what the host function does per
    field); a number -- that radius for every image; an (N,) torch.float64 tensor on the device -- one per image (finite and
    >= 0: a tensor's values are not read back to be checked).  A pixel beyond max_rad is drawn at 0.75 of its hue.  Unknown
    pixels and those valid rules out are zero flow: white.  flows, valid, flow_scale as in flow_max_radius."""
    _check_flows(flows, "flows")
    N, H, W, _ = flows.shape
    _check_mask(valid, "valid", (N, H, W), "flows")
    flow_scale = _check_scale(flow_scale)
    _check_max_rad(max_rad, N)
    _check_device(flows, flows=flows, valid=valid, max_rad=max_rad if isinstance(max_rad, torch.Tensor) else None)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    if max_rad is None:
        max_rad = _max_radius(fv, valid, flow_scale, dev)
    elif not isinstance(max_rad, torch.Tensor):
        max_rad = torch.full((N,), float(max_rad), dtype=torch.float64, device=dev)
    return _launch([_flow_tile(fv, valid, max_rad, flow_scale, 0, W)], N, H, W, dev)


def flow_error_color(flows, flows_gt, valid=None):
    """(N,H,W,3) torch.uint8 RGB: the error of flows against flows_gt on the log colour scale of KITTI's development kit.
    With d = flows - flows_gt in double, n_err = min(|d| / 3, (|d| / |flows_gt|) / 0.05) (|d| / 3 where the ground truth is
    zero): the bins [0, 1/16) .. [8, 16), [16, inf) from dark blue to dark red; n_err >= 1 is a Fl-all outlier, the warm bins.
    A pixel whose ground truth is unknown or ruled out by valid is black, one whose prediction is unknown where the ground truth
    is known gets the last bin.  Both flows (N,H,W,2) float32, read in place; valid as in flow_max_radius.  Exact."""
    _check_flows(flows, "flows")
    _check_flows(flows_gt, "flows_gt", flows)
    N, H, W, _ = flows.shape
    _check_mask(valid, "valid", (N, H, W), "flows")
    _check_device(flows, flows=flows, flows_gt=flows_gt, valid=valid)
    fv, flows = as_view(flows.detach(), "flows")
    gv, flows_gt = as_view(flows_gt.detach(), "flows_gt")
    tile = _lib.VisTile(src=fv.ptr, gt=gv.ptr, valid=_mask_ptr(valid), max_rad=None, kind=_lib.VIS_ERROR, src_cs=fv.cs,
                        gt_cs=gv.cs, src_h=H, src_w=W, x0=0, tile_w=W, flow_scale=1.0)
    return _launch([tile], N, H, W, flows.device)


def pyramid_montage(frames, flows_list, flow_scales=None):
    """(N,h,W_total,3) torch.uint8: infer_continuous.pyramid_montage for a batch -- the frame, then every flow of flows_list
    colour-coded by its OWN per-image maximum and read nearest neighbour at the frame's height h, side by side; one launch.
    frames: (N,h,w,3), contiguous, torch.uint8 (copied) or torch.float32 in [0,1] (rint(255 x), clamped; NaN is 0);
    flows_list: 1 to 7 (N,Hl,Wl,2) float32 tensors (coarse -> fine), read in place; flow_scales: None or one number per flow
    (level_flow_scale's 20 / 2^(num_levels - l): one float32 product per component).  A flow of Hl x Wl takes
    h * Wl // Hl columns; row y reads row y * Hl // h, column x of the tile column x * Wl // (h * Wl // Hl)."""
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"frames: expected a torch.uint8 or torch.float32 tensor, got "
                        f"{frames.dtype if isinstance(frames, torch.Tensor) else type(frames)}")
    if frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) < 1:
        raise ValueError(f"frames: expected an (N, h, w, 3) tensor, got shape {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError(f"frames: a dense (contiguous) tensor is required, got strides {frames.stride()}")
    if not isinstance(flows_list, (list, tuple)) or not 1 <= len(flows_list) <= MAX_MONTAGE_FLOWS:
        raise ValueError(f"flows_list: expected a list of 1 to {MAX_MONTAGE_FLOWS} (N,H,W,2) tensors, got "
                         f"{len(flows_list) if isinstance(flows_list, (list, tuple)) else type(flows_list)}")
    N, h, w, _ = frames.shape
    for l, f in enumerate(flows_list):
        _check_flows(f, f"flows_list[{l}]")
        if f.shape[0] != N:
            raise ValueError(f"flows_list[{l}]: expected a batch of {N}, the frames', got shape {tuple(f.shape)}")
        if h * f.shape[2] // f.shape[1] < 1:
            raise ValueError(f"flows_list[{l}]: a {f.shape[1]} x {f.shape[2]} flow has no column at the frames' height {h}")
    if flow_scales is None:
        flow_scales = [1.0] * len(flows_list)
    if not isinstance(flow_scales, (list, tuple)) or len(flow_scales) != len(flows_list):
        raise ValueError(f"flow_scales: expected None or {len(flows_list)} numbers, one per flow")
    flow_scales = [_check_scale(s, f"flow_scales[{l}]") for l, s in enumerate(flow_scales)]
    _check_device(frames, frames=frames, **{f"flows_list[{l}]": f for l, f in enumerate(flows_list)})
    dev = frames.device
    tiles = [_lib.VisTile(src=frames.data_ptr(), gt=None, valid=None, max_rad=None,
                          kind=_lib.VIS_FRAME_U8 if frames.dtype == torch.uint8 else _lib.VIS_FRAME_F32, src_cs=3, gt_cs=0,
                          src_h=h, src_w=w, x0=0, tile_w=w, flow_scale=1.0)]
    keep, x0 = [], w
    for f, s in zip(flows_list, flow_scales):
        fv, f = as_view(f.detach(), "flows_list")
        rad = _max_radius(fv, None, s, dev)
        keep.append((f, rad))
        tile_w = h * fv.W // fv.H
        tiles.append(_flow_tile(fv, None, rad, s, x0, tile_w))
        x0 += tile_w
    return _launch(tiles, N, h, x0, dev)
