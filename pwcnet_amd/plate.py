"""The background plate of a clip on the HIP path: the frames registered on one canvas by the camera's motion and voted per pixel,
and every frame against that plate (csrc/pwc_plate.hip).

    plate_path(matrices, ok=None, anchor=0)                          -> (to_frame (T+1,3,3) float64 numpy, reach (T+1,) bool)
    plate_canvas(to_frame, reach, H, W, margin=0, max_side=4096)     -> (x0, y0, Hc, Wc)
    canvas_matrices(to_frame, x0, y0)                                -> (matrices, frame_matrices), (T+1,3,3) float64 numpy each
    background_plate(frames, matrices, canvas, mode="median", ...)   -> (plate (Hc,Wc,C), count (Hc,Wc) uint8)
    plate_difference(frames, plate, count, matrices, threshold, ...) -> (difference float32, foreground bool, known bool)

plate_path chains fit_motion's pair-to-pair matrices into one matrix per frame, from the anchor frame's coordinates to that
frame's; plate_canvas is the box all reachable frames cover in anchor coordinates; canvas_matrices shifts the path onto that
box.  background_plate samples every frame at every canvas pixel (warp_frames' bilinear sample, in double) and writes per
channel the LOWER median -- or the mean -- of the samples that exist there: what moves on its own is voted out, and the canvas
is larger than a frame where the camera moves.  plate_difference holds every frame against the plate sampled where the frame
looks: an appearance-based foreground mask, independent of moving_regions' flow-based one.  The exact sequence of operations is
in include/pwc_hip.h, "background plate"; the kernels equal their numpy restatement bit for bit (tests/plate_ref.py).  No
autograd.

The lower median and min_count = 1 are choices: nobody has measured the quality of the plate on real footage.

All five take projective=True for the matrices of homography.fit_homography (a camera that pans or tilts): the helpers then chain
and invert full 3 x 3 matrices normalised to [2][2] = 1, and the two ops divide per pixel, (M p) / (m6 x + m7 y + m8), with no
sample where that divisor is not positive (include/pwc_hip.h, "projective motion").  The default False is every call as it was.
"""
import math

import numpy as np
import torch

from . import _lib
from .interp import _check_mask
from .modules import _p
from .motion import _check_device, _check_matrices, _ptr

MODES = {"median": _lib.PLATE_MEDIAN, "mean": _lib.PLATE_MEAN}
MAX_FRAMES = _lib.PLATE_MAX_FRAMES


def add_cli_arguments(ap):
    """The --plate flags of infer_continuous.py (all default off)."""
    ap.add_argument("--plate", action="store_true",
                    help="--motion: also write plate.png and plate_count.png: the frames registered on one canvas by the dominant "
                         "motion and, per pixel, their temporal median, built on the GPU [off]")
    ap.add_argument("--plate_mode", choices=sorted(MODES), default="median", help="--plate: the lower median or the mean [median]")
    ap.add_argument("--plate_anchor", type=int, default=0, metavar="A", help="--plate: the frame whose coordinates the canvas has [0]")
    ap.add_argument("--plate_frames", type=int, default=32, metavar="K",
                    help=f"--plate: at most K <= {MAX_FRAMES} reachable frames, evenly spaced, the anchor among them [32]")
    ap.add_argument("--plate_margin", type=int, default=0, metavar="M", help="--plate: grow the canvas by M pixels on every side [0]")
    ap.add_argument("--plate_max_side", type=int, default=4096, metavar="S", help="--plate: refuse a canvas with a side above S [4096]")
    ap.add_argument("--plate_inliers", action="store_true",
                    help="--plate: only pixels that move with the camera are candidates (motion_residual's inlier mask of each "
                         "frame's pair; the last frame has none)")
    ap.add_argument("--plate_foreground", type=float, default=None, metavar="T",
                    help="--plate: also write <fname>_fg.png for every reachable frame: white where the frame differs from the "
                         "plate by more than T grey levels, grey 128 where the plate is unknown [off]")


def check_cli_arguments(ap, args, nframes):
    """The flags' rules as argparse errors; True with --plate."""
    if not args.plate:
        return False
    if args.motion is None:
        ap.error("--plate needs --motion MODEL")
    if not 0 <= args.plate_anchor < nframes:
        ap.error(f"--plate_anchor must be a frame of the sequence, 0 .. {nframes - 1}, got {args.plate_anchor}")
    if not 1 <= args.plate_frames <= MAX_FRAMES:
        ap.error(f"--plate_frames must be in 1 .. {MAX_FRAMES}, got {args.plate_frames}")
    if args.plate_margin < 0:
        ap.error(f"--plate_margin must be at least 0, got {args.plate_margin}")
    if args.plate_max_side < 1:
        ap.error(f"--plate_max_side must be at least 1, got {args.plate_max_side}")
    if args.plate_foreground is not None and not args.plate_foreground >= 0.0:
        ap.error(f"--plate_foreground must be non-negative, got {args.plate_foreground}")
    return True


def _check_int(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{what}: expected an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def _host_matrices(matrices, what, rows=None):
    if isinstance(matrices, torch.Tensor):
        matrices = matrices.detach().cpu().numpy()
    M = np.asarray(matrices, np.float64)
    if M.ndim != 3 or M.shape[1:] != (3, 3) or (rows is not None and M.shape[0] != rows):
        raise ValueError(f"{what}: expected shape ({'T' if rows is None else rows}, 3, 3), got {M.shape}")
    return M


def _check_projective(projective):
    if not isinstance(projective, (bool, np.bool_)):
        raise TypeError(f"projective: expected a bool, got {projective!r}")
    return bool(projective)


def _normalised(M):
    """M divided by its [2][2] entry, or None where that entry is not finite and positive or the result is not finite."""
    with np.errstate(all="ignore"):
        if not (np.isfinite(M[2, 2]) and M[2, 2] > 0.0):
            return None
        M = M / M[2, 2]
    return M if np.isfinite(M).all() else None


def plate_path(matrices, ok=None, anchor=0, projective=False):
    """(to_frame (T + 1,3,3) float64 numpy, reach (T + 1,) bool): for every frame of a sequence of T + 1 the matrix that takes a
    pixel (x, y, 1) of the ANCHOR frame to where that frame holds it, from the T motions between neighbours.  Host numpy float64.

    matrices: (T,3,3), fit_motion's (a tensor or an array), M_t taking frame t to frame t + 1.  to_frame[anchor] = I,
    to_frame[t + 1] = M_t to_frame[t] going forwards and to_frame[t] = inv(M_t) to_frame[t + 1] going backwards, the last row set
    to 0 0 1 after every step.  ok: (T,) bool, fit_motion's, None = all True.  Where ok[t] is False -- or M_t is not finite or
    cannot be inverted on the way back -- the chain is broken between frames t and t + 1: every frame beyond the break, seen from
    the anchor, has reach False and the identity.
    projective=True: matrices are fit_homography's; the full 3 x 3 products are kept, divided by their [2][2] entry after every
    step, and a step whose [2][2] entry is not finite and positive breaks the chain as well."""
    projective = _check_projective(projective)
    M = _host_matrices(matrices, "matrices")
    T = M.shape[0]
    if ok is None:
        ok = np.ones(T, bool)
    else:
        if isinstance(ok, torch.Tensor):
            ok = ok.detach().cpu().numpy()
        ok = np.asarray(ok).astype(bool)
        if ok.shape != (T,):
            raise ValueError(f"ok: expected shape {(T,)}, one flag per matrix, got {ok.shape}")
    anchor = _check_int(anchor, "anchor", 0, T)
    to_frame = np.tile(np.eye(3), (T + 1, 1, 1))
    reach = np.zeros(T + 1, bool)
    reach[anchor] = True
    for t in range(anchor, T):
        if not (ok[t] and np.isfinite(M[t]).all()):
            break
        step = M[t] @ to_frame[t]
        if projective:
            step = _normalised(step)
            if step is None:
                break
        else:
            step[2] = (0.0, 0.0, 1.0)
        to_frame[t + 1] = step
        reach[t + 1] = True
    for t in range(anchor - 1, -1, -1):
        if not (ok[t] and np.isfinite(M[t]).all()):
            break
        try:
            inverse = np.linalg.inv(M[t])
        except np.linalg.LinAlgError:
            break
        if not np.isfinite(inverse).all():
            break
        step = inverse @ to_frame[t + 1]
        if projective:
            step = _normalised(step)
            if step is None:
                break
        else:
            step[2] = (0.0, 0.0, 1.0)
        to_frame[t] = step
        reach[t] = True
    return to_frame, reach


def _check_path(to_frame, reach):
    P = _host_matrices(to_frame, "to_frame")
    if isinstance(reach, torch.Tensor):
        reach = reach.detach().cpu().numpy()
    reach = np.asarray(reach).astype(bool)
    if reach.shape != (P.shape[0],):
        raise ValueError(f"reach: expected shape {(P.shape[0],)}, one flag per frame, got {reach.shape}")
    return P, reach


def plate_canvas(to_frame, reach, H, W, margin=0, max_side=4096, projective=False):
    """(x0, y0, Hc, Wc): the integer box, in the anchor frame's coordinates, that the reachable frames cover -- canvas pixel
    (x, y) is the anchor's (x + x0, y + y0).  Host only.

    The four corners (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1) of every frame with reach[t] are carried to anchor
    coordinates by inv(to_frame[t]); x0 = floor(min x) - margin, x1 = ceil(max x) + margin, Wc = x1 - x0 + 1, likewise in y.
    ValueError where no frame is reachable or a side is above max_side (a path that drifts: lower --plate_frames or raise it).
    projective=True: the corners are carried with the division, (x, y) = (q0, q1) / q2 for q = inv(to_frame[t]) corner; a frame
    with a corner at q2 <= 0 (behind the horizon), or whose matrix cannot be inverted, counts as not reached."""
    projective = _check_projective(projective)
    P, reach = _check_path(to_frame, reach)
    H, W = _check_int(H, "H", 1, 1 << 30), _check_int(W, "W", 1, 1 << 30)
    margin = _check_int(margin, "margin", 0, 1 << 30)
    max_side = _check_int(max_side, "max_side", 1, 1 << 30)
    if not reach.any():
        raise ValueError("reach: no frame is reachable")
    corners = np.array([[0.0, 0.0, 1.0], [W - 1.0, 0.0, 1.0], [0.0, H - 1.0, 1.0], [W - 1.0, H - 1.0, 1.0]]).T
    xs, ys = [], []
    for t in np.nonzero(reach)[0]:
        if projective:
            try:
                q = np.linalg.inv(P[t]) @ corners
            except np.linalg.LinAlgError:
                continue
            if not (q[2] > 0.0).all():
                continue
            q = q / q[2]
        else:
            q = np.linalg.inv(P[t]) @ corners
        xs.append(q[0])
        ys.append(q[1])
    if not xs:
        raise ValueError("reach: no frame is reachable in front of the horizon")
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    if not (np.isfinite(xs).all() and np.isfinite(ys).all()):
        raise ValueError("to_frame: a reachable frame's corners are not finite on the canvas")
    x0, x1 = math.floor(xs.min()) - margin, math.ceil(xs.max()) + margin
    y0, y1 = math.floor(ys.min()) - margin, math.ceil(ys.max()) + margin
    Hc, Wc = y1 - y0 + 1, x1 - x0 + 1
    if Hc > max_side or Wc > max_side:
        raise ValueError(f"canvas: {Hc} x {Wc} (H x W) has a side above max_side = {max_side}")
    return int(x0), int(y0), int(Hc), int(Wc)


def canvas_matrices(to_frame, x0, y0, projective=False):
    """(matrices, frame_matrices), (T + 1,3,3) float64 numpy each: matrices[t] = to_frame[t] @ [[1,0,x0],[0,1,y0],[0,0,1]] takes a
    CANVAS pixel to its position in frame t (what background_plate wants), frame_matrices[t] = inv(matrices[t]) takes a pixel of
    frame t to the canvas (what plate_difference wants); last rows 0 0 1.  A matrix that cannot be inverted gives NaNs, which
    both kernels read as "this frame sees nothing".  Host only.
    projective=True: the full 3 x 3 matrices, each divided by its [2][2] entry; NaNs where that entry is not finite and positive
    (what background_plate and plate_difference want with projective=True)."""
    projective = _check_projective(projective)
    P = _host_matrices(to_frame, "to_frame")
    for what, v in (("x0", x0), ("y0", y0)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"{what}: expected a finite number, got {v!r}")
    shift = np.array([[1.0, 0.0, float(x0)], [0.0, 1.0, float(y0)], [0.0, 0.0, 1.0]])
    matrices = P @ shift
    if projective:
        frame_matrices = np.full_like(matrices, np.nan)
        for t in range(P.shape[0]):
            forward = _normalised(matrices[t])
            matrices[t] = np.nan if forward is None else forward
            if forward is None:
                continue
            try:
                inverse = _normalised(np.linalg.inv(forward))
            except np.linalg.LinAlgError:
                continue
            if inverse is not None:
                frame_matrices[t] = inverse
        return matrices, frame_matrices
    matrices[:, 2] = (0.0, 0.0, 1.0)
    frame_matrices = np.full_like(matrices, np.nan)
    for t in range(P.shape[0]):
        try:
            frame_matrices[t] = np.linalg.inv(matrices[t])
        except np.linalg.LinAlgError:
            continue
    frame_matrices[:, 2] = (0.0, 0.0, 1.0)
    return matrices, frame_matrices


def _check_frames(frames):
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"frames: expected a torch.uint8 or torch.float32 tensor, got "
                        f"{frames.dtype if isinstance(frames, torch.Tensor) else type(frames)}")
    if frames.dim() != 4 or not 1 <= frames.shape[3] <= 4 or min(frames.shape) < 1:
        raise ValueError(f"frames: expected a (T, H, W, C) tensor with 1 to 4 channels, got shape {tuple(frames.shape)}")
    return tuple(frames.shape)


def _device_matrices(matrices, T, device):
    if isinstance(matrices, np.ndarray):
        if matrices.dtype != np.float64:
            raise TypeError(f"matrices: expected a float64 array, got {matrices.dtype}")
        if matrices.shape != (T, 3, 3):
            raise ValueError(f"matrices: expected shape {(T, 3, 3)}, one matrix per image, got {matrices.shape}")
        return torch.from_numpy(np.array(matrices, order="C")).to(device)       # (a copy: the array may be read-only)
    _check_matrices(matrices, T)
    return matrices


def background_plate(frames, matrices, canvas, mode="median", use=None, masks=None, min_count=1, projective=False):
    """(plate (Hc,Wc,C) in the frames' dtype, count (Hc,Wc) torch.uint8): the clip's frames on one canvas, voted per pixel
    (pwc_plate_build: one launch on the current stream, no workspace, no host synchronisation).

    frames: (T,H,W,C) torch.uint8 or torch.float32, C = 1 .. 4, T = 1 .. 64, on the GPU (made contiguous).  matrices: (T,3,3)
    torch.float64 or a numpy array (canvas_matrices'), each taking a CANVAS pixel (x, y, 1) to its position in frame t.  canvas:
    (Hc, Wc).  use: (T,) bools, None = every frame.  masks: (T,H,W) torch.bool / torch.uint8, contiguous, None = every pixel.
    Frame t has a sample at a canvas pixel where use[t] holds, its matrix is affine (last row exactly 0 0 1) and finite, the
    position is inside [0, W - 1] x [0, H - 1], all four corners of the bilinear sample are inside the mask (compose_flows'
    rule) and, for float frames, finite.  mode "median": per channel the LOWER median of the samples, each rounded as
    warp_frames rounds (the element of rank (n - 1) // 2 of n; floats ordered with -0 < +0, the output is one of the samples'
    bit patterns); "mean": the mean of the unrounded samples, added in frame order, rounded once.  count: n, the samples a pixel
    has; where n < min_count (>= 1) the plate is 0.  Two calls give the same bits.  The lower median and min_count = 1 are
    choices nobody has measured on real footage.
    projective=True (pwc_plate_build_projective): matrices are canvas_matrices' with projective=True; the position is (M p) / D,
    D = m6 x + m7 y + m8; a frame has no sample where D is not positive or one of its nine entries is not finite.  Affine matrices
    give the bits of projective=False.  No autograd: the outputs never require grad."""
    projective = _check_projective(projective)
    T, H, W, C = _check_frames(frames)
    if T > MAX_FRAMES:
        raise ValueError(f"frames: expected at most {MAX_FRAMES} frames, got {T}")
    matrices = _device_matrices(matrices, T, frames.device)
    try:
        Hc, Wc = canvas
    except (TypeError, ValueError):
        raise ValueError(f"canvas: expected a pair (Hc, Wc), got {canvas!r}") from None
    Hc, Wc = _check_int(Hc, "canvas", 1, 1 << 30), _check_int(Wc, "canvas", 1, 1 << 30)
    if mode not in MODES:
        raise ValueError(f"mode: expected one of {sorted(MODES)}, got {mode!r}")
    if use is not None:
        if isinstance(use, torch.Tensor):
            use = use.detach().cpu().numpy()
        use = np.asarray(use)
        if use.shape != (T,) or use.dtype.kind not in "bui":
            raise ValueError(f"use: expected {T} booleans, one per frame, got shape {use.shape}, dtype {use.dtype}")
        use = np.ascontiguousarray(use != 0).astype(np.uint8)
    _check_mask(masks, "masks", T, H, W)
    min_count = _check_int(min_count, "min_count", 1, 255)
    _check_device(frames, frames=frames, matrices=matrices, masks=masks)
    frames = frames.detach().contiguous()                                  # (a view is copied: the kernel reads dense frames)
    matrices = matrices.detach().contiguous()
    use_t = None if use is None else torch.from_numpy(use).to(frames.device)
    plate = torch.empty((Hc, Wc, C), dtype=frames.dtype, device=frames.device)
    count = torch.empty((Hc, Wc), dtype=torch.uint8, device=frames.device)
    dtype = _lib.MOTION_U8 if frames.dtype == torch.uint8 else _lib.MOTION_F32
    entry = _lib.lib().pwc_plate_build_projective if projective else _lib.lib().pwc_plate_build
    _lib.check(entry(_p(frames.data_ptr()), dtype, C, _p(matrices.data_ptr()), _ptr(use_t), _ptr(masks), T, H, W, Hc, Wc, MODES[mode],
                     min_count, _p(plate.data_ptr()), _p(count.data_ptr()), _lib.current_stream()), "background plate")
    return plate, count


def plate_difference(frames, plate, count, matrices, threshold, min_count=1, projective=False):
    """(difference (T,H,W) float32, foreground (T,H,W) torch.bool, known (T,H,W) torch.bool): every frame against the plate
    sampled where the frame looks (pwc_plate_difference: one launch, a lane per frame pixel).

    frames: (T,H,W,C) as background_plate's (any T).  plate (Hc,Wc,C) in the frames' dtype and count (Hc,Wc) torch.uint8:
    background_plate's.  matrices: (T,3,3) torch.float64 or a numpy array (canvas_matrices' frame_matrices), each taking a
    FRAME pixel (x, y, 1) to its position on the canvas.  A pixel is known where its matrix is affine and finite, the position
    is on the canvas, all four corners of the bilinear sample have count >= min_count and, for floats, everything read is
    finite.  difference: the largest absolute difference over the channels between the frame's value and the plate's
    (unrounded) sample, in the frames' units; 0 where not known.  foreground: known and difference > threshold (>= 0).
    projective=True (pwc_plate_difference_projective): matrices are canvas_matrices' frame_matrices with projective=True; a
    pixel is not known where D = m6 x + m7 y + m8 is not positive or an entry of its matrix is not finite.  No autograd."""
    projective = _check_projective(projective)
    T, H, W, C = _check_frames(frames)
    if not isinstance(plate, torch.Tensor) or plate.dtype != frames.dtype:
        raise TypeError(f"plate: expected a {frames.dtype} tensor, the frames' dtype, got "
                        f"{plate.dtype if isinstance(plate, torch.Tensor) else type(plate)}")
    if plate.dim() != 3 or plate.shape[2] != C or min(plate.shape) < 1:
        raise ValueError(f"plate: expected an (Hc, Wc, {C}) tensor, got shape {tuple(plate.shape)}")
    Hc, Wc = plate.shape[:2]
    if not isinstance(count, torch.Tensor) or count.dtype != torch.uint8:
        raise TypeError(f"count: expected a torch.uint8 tensor, got {count.dtype if isinstance(count, torch.Tensor) else type(count)}")
    if tuple(count.shape) != (Hc, Wc):
        raise ValueError(f"count: expected shape {(Hc, Wc)}, the plate's, got {tuple(count.shape)}")
    matrices = _device_matrices(matrices, T, frames.device)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not float(threshold) >= 0.0:
        raise ValueError(f"threshold: expected a non-negative number, got {threshold!r}")
    min_count = _check_int(min_count, "min_count", 1, 255)
    _check_device(frames, frames=frames, plate=plate, count=count, matrices=matrices)
    frames, plate, count = frames.detach().contiguous(), plate.detach().contiguous(), count.contiguous()
    matrices = matrices.detach().contiguous()
    difference = torch.empty((T, H, W), dtype=torch.float32, device=frames.device)
    foreground = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device)
    known = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device)
    dtype = _lib.MOTION_U8 if frames.dtype == torch.uint8 else _lib.MOTION_F32
    entry = _lib.lib().pwc_plate_difference_projective if projective else _lib.lib().pwc_plate_difference
    _lib.check(entry(_p(frames.data_ptr()), dtype, C, _p(plate.data_ptr()), _p(count.data_ptr()), _p(matrices.data_ptr()), T, H, W, Hc,
                     Wc, min_count, float(threshold), _p(difference.data_ptr()), _p(foreground.data_ptr()), _p(known.data_ptr()),
                     _lib.current_stream()), "plate difference")
    return difference, foreground.view(torch.bool), known.view(torch.bool)


def select_frames(reach, anchor, limit):
    """The indices of at most `limit` reachable frames, evenly spaced over the reachable ones, the anchor among them (sorted)."""
    idx = np.nonzero(np.asarray(reach).astype(bool))[0]
    if len(idx) > limit:
        idx = idx[np.unique(np.round(np.linspace(0, len(idx) - 1, limit)).astype(int))]
        if anchor not in idx:
            idx[np.argmin(np.abs(idx - anchor))] = anchor
    return [int(i) for i in idx]
