"""Motion-compensated temporal filtering of a clip on the HIP path (csrc/pwc_temporal.hip).

    temporal_filter(frames, flows_fw, flows_bw, radius=2, sigma=10.0, patch=1, ...)   -> (filtered (n,H,W,C), support (n,H,W) uint8)
    plan_windows(T, radius, batch)                                                     -> [(clip_start, clip_stop, out_start, out_stop)]

Every pixel of a frame is averaged with what its trajectory through the `radius` frames after and before it shows: a neighbour
is read where the consecutive flows say the pixel went (track_points' step, in double, rounded to float32 once per step),
weighs 1 / (1 + d^2 / sigma^2) by the mean squared difference d^2 of the (2 patch + 1)^2 patches around the two positions, and is
dropped -- with everything beyond it on that side -- where the walk leaves the frame, meets an unknown flow (compose_flows'
all-four-corners rule) or fails the forward-backward check (fb_valid's inequality).  The exact sequence of operations is in
include/pwc_hip.h, "temporal filter"; the kernel equals its numpy restatement bit for bit (tests/temporal_ref.py).  No autograd.

sigma = 10 grey levels, patch = 1 and radius = 2 are choices: nobody has tuned them, and nobody has measured the denoising
quality on real footage.
"""
import math

import numpy as np
import torch

from . import _lib
from .interp import _check_mask
from .modules import _p, as_view
from .motion import _check_device, _ptr
from .unsup import _check_nhwc

MAX_RADIUS = _lib.TEMPORAL_MAX_RADIUS
MAX_PATCH = _lib.TEMPORAL_MAX_PATCH


def add_cli_arguments(ap):
    """The --denoise flags of infer_continuous.py (all default off)."""
    ap.add_argument("--denoise", type=int, default=0, metavar="R",
                    help="also write <fname>_denoised.png for every frame: the frame averaged with its R = 1 .. 8 neighbours on "
                         "either side along the flow, on the GPU (the reversed pairs are run too) [0: off]")
    ap.add_argument("--denoise_sigma", type=float, default=10.0, metavar="S",
                    help="--denoise: a neighbour weighs 1 / (1 + d^2 / S^2), d its patch's rms difference in grey levels [10]")
    ap.add_argument("--denoise_patch", type=int, default=1, metavar="P", help="--denoise: patches of (2 P + 1)^2 pixels, P = 0 .. 2 [1]")
    ap.add_argument("--denoise_no_fb", action="store_true", help="--denoise: do not drop neighbours that fail the forward-backward check")


def check_cli_arguments(ap, args):
    """The flags' rules as argparse errors; returns temporal_filter's keyword arguments, None without --denoise."""
    if not 0 <= args.denoise <= MAX_RADIUS:
        ap.error(f"--denoise must be in 1 .. {MAX_RADIUS} (0: off), got {args.denoise}")
    if not (args.denoise_sigma > 0.0 and math.isfinite(args.denoise_sigma)):
        ap.error(f"--denoise_sigma must be positive and finite, got {args.denoise_sigma}")
    if not 0 <= args.denoise_patch <= MAX_PATCH:
        ap.error(f"--denoise_patch must be in 0 .. {MAX_PATCH}, got {args.denoise_patch}")
    if args.denoise == 0:
        return None
    return dict(radius=args.denoise, sigma=args.denoise_sigma, patch=args.denoise_patch, fb_check=not args.denoise_no_fb)


def _check_int(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{what}: expected an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def plan_windows(T, radius, batch):
    """[(clip_start, clip_stop, out_start, out_stop), ...]: how a sequence of T frames is fed to temporal_filter `batch` output
    frames at a time.  Piece n produces the frames out_start .. out_stop - 1 from the clip clip_start .. clip_stop - 1, which holds
    `radius` frames of context on either side, clipped at the ends of the sequence:
        temporal_filter(frames[cs:ce], flows_fw[cs:ce - 1], flows_bw[cs:ce - 1], radius, out_range=(os - cs, oe - cs))
    gives the bits of frames os .. oe - 1 of one call over the whole sequence.  Host only."""
    T = _check_int(T, "T", 1, 1 << 30)
    radius = _check_int(radius, "radius", 1, MAX_RADIUS)
    batch = _check_int(batch, "batch", 1, 1 << 30)
    return [(max(o - radius, 0), min(min(o + batch, T) + radius, T), o, min(o + batch, T)) for o in range(0, T, batch)]


def _check_temporal(frames, flows_fw, flows_bw, radius, sigma, patch, alpha1, alpha2, max_distance, valids_fw, valids_bw, out_range):
    """Types, shapes and values of temporal_filter's arguments, each named after its argument; the device last of all.
    Returns (T, H, W, C, radius, patch, sigma, max_distance, i0, i1)."""
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"frames: expected a torch.uint8 or torch.float32 tensor, got "
                        f"{frames.dtype if isinstance(frames, torch.Tensor) else type(frames)}")
    if frames.dim() != 4 or frames.shape[3] not in (1, 3):
        raise ValueError(f"frames: expected a (T,H,W,C) tensor with 1 or 3 channels, got shape {tuple(frames.shape)}")
    T, H, W, C = frames.shape
    if T <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"frames: empty tensor, shape {tuple(frames.shape)}")
    for what, f in (("flows_fw", flows_fw), ("flows_bw", flows_bw)):
        if f is None and T == 1:
            continue
        _check_nhwc(f, what, (2,))
        if tuple(f.shape) != (T - 1, H, W, 2):
            raise ValueError(f"{what}: expected shape {(T - 1, H, W, 2)}, one flow per consecutive pair of frames, got {tuple(f.shape)}")
    if T > 1:
        _check_mask(valids_fw, "valids_fw", T - 1, H, W)
        _check_mask(valids_bw, "valids_bw", T - 1, H, W)
    radius = _check_int(radius, "radius", 1, MAX_RADIUS)
    patch = _check_int(patch, "patch", 0, MAX_PATCH)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (
            float(sigma) > 0.0 and math.isfinite(float(sigma)) and 0.0 < float(sigma) * float(sigma) < math.inf):
        raise ValueError(f"sigma: expected a positive finite number of grey levels, got {sigma!r}")
    if max_distance is not None and (isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating))
                                     or not (float(max_distance) > 0.0 and math.isfinite(float(max_distance)))):
        raise ValueError(f"max_distance: expected None or a positive finite number of grey levels, got {max_distance!r}")
    for what, v in (("alpha1", alpha1), ("alpha2", alpha2)):
        if not float(v) >= 0.0:
            raise ValueError(f"{what}: expected a non-negative number, got {v!r}")
    if out_range is None:
        i0, i1 = 0, T
    else:
        try:
            i0, i1 = out_range
        except (TypeError, ValueError):
            raise ValueError(f"out_range: expected None or a pair (start, stop) of frame indices, got {out_range!r}") from None
        for v in (i0, i1):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"out_range: expected a pair of integers, got {out_range!r}")
        if not 0 <= i0 < i1 <= T:
            raise ValueError(f"out_range: expected 0 <= start < stop <= {T}, the frames of the clip, got {out_range!r}")
    _check_device(frames, frames=frames, flows_fw=flows_fw, flows_bw=flows_bw, valids_fw=valids_fw, valids_bw=valids_bw)
    return T, H, W, C, radius, patch, float(sigma), 0.0 if max_distance is None else float(max_distance), int(i0), int(i1)


def temporal_filter(frames, flows_fw, flows_bw, radius=2, sigma=10.0, patch=1, fb_check=True, alpha1=0.01, alpha2=0.5,
                    max_distance=None, valids_fw=None, valids_bw=None, out_range=None):
    """(filtered (n,H,W,C) in the frames' dtype, support (n,H,W) torch.uint8): the clip's frames averaged with their temporal
    neighbours along the motion (pwc_temporal_filter: one launch on the current stream, no workspace, no host synchronisation).

    frames: (T,H,W,C) torch.uint8, or float32 in [0, 1] (read as grey levels 255 v, a NaN as 0, nothing clamped), C = 1 or 3, on
    the GPU.  flows_fw: (T-1,H,W,2) float32 in pixels, flows_fw[j] the flow from frame j to frame j + 1; flows_bw: the same
    shape, flows_bw[j] the flow from frame j + 1 to frame j; channel slices of wider buffers are read in place; read detached.
    Both may be None where T = 1.  valids_fw, valids_bw: (T-1,H,W) torch.bool / torch.uint8, contiguous, None = every pixel; a flow
    that fails flow_io.flow_valid's rule (a NaN, an Inf, the sentinel 1e10) is unknown as well.
    For every output pixel the walk goes k = 1 .. radius frames forwards along flows_fw, then backwards along flows_bw, one
    track_points step per frame.  A step that leaves the frame, reads an unknown or masked flow at any of its four corners or
    -- with fb_check -- fails alpha1 (|f|^2 + |b|^2) + alpha2 >= |f + b|^2 against the opposite flow ends that side of the walk:
    the frame it would have reached and every farther one contribute nothing.  A reached frame contributes its bilinear sample
    with the weight 1 / (1 + d^2 / sigma^2), d^2 the mean over the (2 patch + 1)^2 offsets inside the frame and the channels of
    the squared grey-level difference between the centre frame's patch and the neighbour's, sampled around where the walk
    stands; with max_distance (grey levels) the weight is 0 where d > max_distance.  The pixel itself weighs 1.
    filtered: the weighted mean; uint8 frames round to even and clamp.  support: how many of the up to 2 radius neighbours
    entered with a weight above 0.  out_range = (start, stop): only those frames of the clip are produced (plan_windows feeds a
    long sequence by such pieces and gives the bits of one call).  T = 1 returns the input, support 0.  Two calls give the same
    bits.  sigma, patch and radius are untuned choices; nobody has measured the denoising quality on real footage.  No autograd:
    the outputs never require grad."""
    T, H, W, C, radius, patch, sigma, max_distance, i0, i1 = _check_temporal(
        frames, flows_fw, flows_bw, radius, sigma, patch, alpha1, alpha2, max_distance, valids_fw, valids_bw, out_range)
    frames = frames.detach().contiguous()
    fv = bv = None
    if T > 1:
        fv, flows_fw = as_view(flows_fw.detach(), "flows_fw")
        bv, flows_bw = as_view(flows_bw.detach(), "flows_bw")
    else:
        valids_fw = valids_bw = None
    dev = frames.device
    filtered = torch.empty((i1 - i0, H, W, C), dtype=frames.dtype, device=dev)
    support = torch.empty((i1 - i0, H, W), dtype=torch.uint8, device=dev)
    dtype = _lib.TEMPORAL_F32 if frames.dtype == torch.float32 else _lib.TEMPORAL_U8
    _lib.check(_lib.lib().pwc_temporal_filter(_p(frames.data_ptr()), dtype, C, None if fv is None else _p(fv.ptr),
                                              2 if fv is None else fv.cs, None if bv is None else _p(bv.ptr),
                                              2 if bv is None else bv.cs, _ptr(valids_fw), _ptr(valids_bw), T, H, W, radius, patch,
                                              sigma, max_distance, 1 if fb_check else 0, float(alpha1), float(alpha2), i0, i1,
                                              _p(filtered.data_ptr()), _p(support.data_ptr()), _lib.current_stream()),
               "temporal filter")
    return filtered, support
