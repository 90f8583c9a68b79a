"""Point tracking on the HIP path: query points carried through the consecutive flows of a sequence (csrc/pwc_track.hip).

    track_points(flows_fw, points, flows_bw=None, start=None, status=None, ...)   -> (tracks (T+1,P,2), status (T+1,P) uint8)
    grid_points(H, W, stride, offset=None)                                         -> (P,2) float32 queries of a regular grid

A point steps from frame t to frame t + 1 by the flow sampled bilinearly where it stands (fb_valid's sample, in double, rounded to
float32 once per step).  Its status at every frame is one of UNSEEN (the frame is not covered by the track), VISIBLE, LEFT (out of
frame), OCCLUDED (the forward-backward check against flows_bw failed: UnFlow's rule, fb_valid's) and UNKNOWN (a flow it had to
read is masked out or fails flow_io.flow_valid's rule for the .flo sentinel -- at any of the four corners, whatever their
weights, as compose_flows decides).  The exact sequence of operations is in include/pwc_hip.h, "point tracking"; the kernel
equals its numpy restatement bit for bit (tests/track_ref.py).  No autograd.
"""
import numpy as np
import torch

from . import _lib
from .modules import _p, as_view
from .unsup import _check_distill_mask, _check_nhwc

UNSEEN, VISIBLE, LEFT, OCCLUDED, UNKNOWN = (_lib.TRACK_UNSEEN, _lib.TRACK_VISIBLE, _lib.TRACK_LEFT, _lib.TRACK_OCCLUDED,
                                            _lib.TRACK_UNKNOWN)
STATUS_NAMES = ("UNSEEN", "VISIBLE", "LEFT", "OCCLUDED", "UNKNOWN")
_DIRECTIONS = {"forward": _lib.TRACK_FORWARD, "both": _lib.TRACK_BOTH}


def _check_vector(t, what, dtype, shape):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{what}: expected a {dtype} tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t)}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, one entry per point, got {tuple(t.shape)}")


def _check_track(flows_fw, points, flows_bw, start, status, valids_fw, valids_bw, direction, alpha1, alpha2):
    """Types and shapes of track_points' arguments, each named after its argument; the device last of all."""
    _check_nhwc(flows_fw, "flows_fw", (2,))
    T, H, W, _ = flows_fw.shape
    if T <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows_fw: empty tensor, shape {tuple(flows_fw.shape)}")
    if flows_bw is not None:
        _check_nhwc(flows_bw, "flows_bw", (2,))
        if tuple(flows_bw.shape) != tuple(flows_fw.shape):
            raise ValueError(f"flows_bw: expected shape {tuple(flows_fw.shape)}, flows_fw's, got {tuple(flows_bw.shape)}")
    _check_distill_mask(valids_fw, "valids_fw", (T, H, W), "flows_fw")
    _check_distill_mask(valids_bw, "valids_bw", (T, H, W), "flows_fw")
    if valids_bw is not None and flows_bw is None:
        raise ValueError("valids_bw: a mask of flows_bw, which is not given")
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32:
        raise TypeError(f"points: expected a torch.float32 tensor, got {points.dtype if isinstance(points, torch.Tensor) else type(points)}")
    if points.dim() != 2 or points.shape[1] != 2 or points.shape[0] < 1:
        raise ValueError(f"points: expected shape (P, 2) with P >= 1, (x, y) per point, got {tuple(points.shape)}")
    P = points.shape[0]
    _check_vector(start, "start", torch.int32, (P,))
    _check_vector(status, "status", torch.uint8, (P,))
    if direction not in _DIRECTIONS:
        raise ValueError(f"direction: expected 'forward' or 'both', got {direction!r}")
    if direction == "both" and flows_bw is None:
        raise ValueError("direction: 'both' steps towards frame 0 along flows_bw, which is not given")
    for what, v in (("alpha1", alpha1), ("alpha2", alpha2)):
        if not float(v) >= 0.0:
            raise ValueError(f"{what}: expected a non-negative number, got {v!r}")
    if start is not None and int(start.min()) < 0:
        raise ValueError(f"start: expected frame indices >= 0, got {int(start.min())}")
    for what, t in dict(flows_fw=flows_fw, points=points, flows_bw=flows_bw, start=start, status=status, valids_fw=valids_fw,
                        valids_bw=valids_bw).items():
        if t is not None and (not t.is_cuda or t.device != flows_fw.device):
            raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only, all arguments on one device")


def _ptr(t):
    return None if t is None else _p(t.data_ptr())


def track_points(flows_fw, points, flows_bw=None, start=None, status=None, valids_fw=None, valids_bw=None, direction="forward",
                 alpha1=0.01, alpha2=0.5, stop_on_occlusion=True):
    """(tracks (T+1,P,2) float32, status (T+1,P) torch.uint8), time-major: where the P query points are in each of the T + 1
    frames of a sequence, and what is known about them there (pwc_track_points_f32, one launch, a lane per point).

    flows_fw: (T,H,W,2) float32, the flows t -> t + 1 in pixels; channel slices of wider buffers are read in place.  flows_bw:
    the flows t + 1 -> t, same shape: with it every step is checked (alpha1, alpha2: fb_valid's) and a failing point is
    OCCLUDED -- terminal with stop_on_occlusion, else it keeps stepping from where it is and may become VISIBLE again.
    valids_fw, valids_bw: (T,H,W) torch.bool / torch.uint8, contiguous, None = every pixel.  points: (P,2) float32 (x, y), the
    flow's channel order, pixel centres at the integers, sub-pixel positions welcome.  start: (P,) int32, the frame each query
    is given in (None: 0); a point is VISIBLE there (LEFT where the query is outside the frame) and UNSEEN before -- or, with
    direction="both" (needs flows_bw), also tracked down to frame 0 along flows_bw, checked against flows_fw.  start > T: not
    in this call, UNSEEN throughout.  status: (P,) uint8, the streaming form -- where it is not UNSEEN the point enters frame
    0 in that state at points[p] and start[p] is ignored: feed tracks[-1], status[-1] of one call and start - T to the next
    and the pieces equal one call over the whole sequence, bit for bit.
    A point that leaves the frame (LEFT) or meets a masked-out or unknown flow at any of the four pixels around it (UNKNOWN)
    stays where it was, in that state, for the rest of the track.  Every value is computed in double in a fixed order and
    rounded to float32 once per step (include/pwc_hip.h, "point tracking").  No autograd: the flows are read detached, the
    outputs never require grad."""
    _check_track(flows_fw, points, flows_bw, start, status, valids_fw, valids_bw, direction, alpha1, alpha2)
    fv, flows_fw = as_view(flows_fw.detach(), "flows_fw")
    bv, flows_bw = (None, None) if flows_bw is None else as_view(flows_bw.detach(), "flows_bw")
    points = points.detach().contiguous()
    start = None if start is None else start.contiguous()
    status = None if status is None else status.contiguous()
    T, H, W, P = fv.N, fv.H, fv.W, points.shape[0]
    dev = flows_fw.device
    tracks = torch.empty((T + 1, P, 2), dtype=torch.float32, device=dev)
    out_status = torch.empty((T + 1, P), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().pwc_track_points_f32(_p(fv.ptr), fv.cs, None if bv is None else _p(bv.ptr), 2 if bv is None else bv.cs,
                                               _ptr(valids_fw), _ptr(valids_bw), T, H, W, _p(points.data_ptr()), _ptr(start),
                                               _ptr(status), P, _DIRECTIONS[direction], float(alpha1), float(alpha2),
                                               1 if stop_on_occlusion else 0, _p(tracks.data_ptr()), _p(out_status.data_ptr()),
                                               _lib.current_stream()), "track points")
    return tracks, out_status


def grid_points(H, W, stride, offset=None):
    """The (P,2) float32 queries (x, y) of a regular grid over an H x W frame, row by row: x = ox, ox + stride, ... < W and
    y = oy, oy + stride, ... < H.  offset: an integer or (ox, oy); None: stride // 2, the centres of stride x stride cells.
    Host side: a CPU tensor, `.cuda()` it for track_points."""
    for what, v in (("H", H), ("W", W), ("stride", stride)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{what}: expected a positive integer, got {v!r}")
    if offset is None:
        offset = stride // 2
    ox, oy = (offset, offset) if isinstance(offset, (int, np.integer)) else tuple(offset)
    for what, v, size in (("offset x", ox, W), ("offset y", oy, H)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < size:
            raise ValueError(f"offset: expected integers inside the frame, got {what} = {v!r}")
    ys, xs = np.meshgrid(np.arange(oy, H, stride), np.arange(ox, W, stride), indexing="ij")
    return torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32))
