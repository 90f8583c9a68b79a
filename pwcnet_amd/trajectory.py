"""Scale chain and camera trajectory on the HIP path: one unit of length for the pairs of a sequence, and the camera's path through
it (csrc/pwc_trajectory.hip).

    camera_trajectory(flows, rotation, translation, intrinsics, depth, known, min_samples=64, state=None)
        -> (trajectory (T+1,3,4) f64, scales (T,) f64, segment (T,) int32, info, state)
    flow_trajectory(flows, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0, min_parallax=0.25, min_samples=64, state=None, refine=0)
        -> (depth, known, trajectory, scales, segment, info, state)

flows are the T consecutive flows of ONE sequence, pair j being frames j -> j + 1.  pose.flow_depth gives every pair a pose with
|t| = 1 and a depth map in that pair's own baseline.  A rigid point that pair j - 1 and pair j both see has two depths in camera j,
one in each pair's baseline; the lower median of their ratio over the image -- an exact whole-image selection by histogram passes,
no sort -- links the two scales, and the running product of the links puts the whole sequence in one unit.  The exact sequence of
operations is in include/pwc_hip.h, "scale chain and camera trajectory"; the kernels equal their numpy restatement bit for bit
(tests/trajectory_ref.py).  No host synchronisation.  No autograd.

Units: scales[j] is pair j's baseline in the baseline of the FIRST pair of its segment; depth[j] * scales[j] is pair j's depth in
that unit, and so is every length of trajectory.  trajectory[i] = [A | c] is world-to-camera, X_cam_i = A X_world + c, the world
being the first camera of frame i's segment; the camera's centre is -A^T c.
Segments: a seam is linked where both pairs' poses are ok, it has at least min_samples samples and its ratio is usable.  A pair whose
pose is ok behind a seam that is not linked starts a new segment: scale 1, [I | 0] at its first frame (that frame's row shows the
start of the new segment, not the end of the old one).  A pair whose pose is not ok has scale 0 and segment -1, and the frame after
it holds [I | 0].  Segments do not share a unit.
What this cannot do:
  * A point that moves ALONG its epipolar line has a consistent, wrong depth in both pairs and counts as a sample.
  * A pair in which the camera only rotates has no pose (camera_pose's ok False): it breaks the chain, nothing bridges it.
  * The scale is a running product: its error multiplies up over a long clip.  No loop closure, no refinement of any kind.
min_samples = 64 is a choice nobody has tuned on real video, as are sampling the depth (not the inverse depth) bilinearly and
restarting at a broken seam; nobody has measured the trajectory on network flows of real footage.
"""
import numpy as np
import torch

from . import _lib
from .modules import _p, as_view
from .motion import _check_device, _check_flows, _ptr
from .pose import _check_pose, _intrinsics, flow_depth

MAX_PIXELS = _lib.TRAJECTORY_MAX_PIXELS
_STATE = ("flow", "rotation", "translation", "intrinsics", "depth", "known", "row", "scale", "segment")


def _check_map(t, what, dtypes, shape):
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise TypeError(f"{what}: expected a {' / '.join(str(d) for d in dtypes)} tensor, got "
                        f"{t.dtype if isinstance(t, torch.Tensor) else type(t)}")
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: expected shape {shape}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous tensor")


def _check_state(state, H, W):
    if not isinstance(state, dict) or any(k not in state for k in _STATE):
        raise TypeError(f"state: expected the state an earlier call returned (a dict with {', '.join(_STATE)}), got "
                        f"{sorted(state) if isinstance(state, dict) else type(state)}")
    if not isinstance(state["flow"], torch.Tensor) or state["flow"].dtype != torch.float32:
        raise TypeError(f"state['flow']: expected a torch.float32 tensor, got "
                        f"{state['flow'].dtype if isinstance(state['flow'], torch.Tensor) else type(state['flow'])}")
    if tuple(state["flow"].shape) != (H, W, 2):
        raise ValueError(f"state['flow']: expected shape {(H, W, 2)}, the flows', got {tuple(state['flow'].shape)}")
    _check_pose(state["rotation"][None], state["translation"][None], 1)
    _check_map(state["intrinsics"], "state['intrinsics']", (torch.float64,), (4,))
    _check_map(state["depth"], "state['depth']", (torch.float32,), (H, W))
    _check_map(state["known"], "state['known']", (torch.bool, torch.uint8), (H, W))
    _check_map(state["row"], "state['row']", (torch.float64,), (3, 4))
    _check_map(state["scale"], "state['scale']", (torch.float64,), (1,))
    _check_map(state["segment"], "state['segment']", (torch.int32,), (2,))


def camera_trajectory(flows, rotation, translation, intrinsics, depth, known, min_samples=64, state=None):
    """(trajectory (T+1,3,4) torch.float64, scales (T,) torch.float64, segment (T,) torch.int32, info, state): the baseline scale
    chained across the T pairs of ONE sequence and the camera's path (pwc_scale_links_f32: two memsets and six launches;
    pwc_camera_trajectory_f64: one launch; no host synchronisation).

    flows: (T,H,W,2) float32 in pixels, on the GPU, the consecutive flows j -> j + 1; a channel slice of a wider buffer is read in
    place; read detached.  rotation (T,3,3), translation (T,3): torch.float64, camera_pose's.  intrinsics: fx fy cx cy, camera_pose's.
    depth (T,H,W) float32 and known (T,H,W) torch.bool / torch.uint8: triangulate_depth's, contiguous, computed with valid=inlier
    (flow_depth does) -- a pixel that moves on its own would be a sample otherwise.  H W <= 2^26, T <= 65535.
    Per pixel of pair j - 1 with known set: the point's depth Z1 in camera j in pair j - 1's baselines (the triangulation again) over
    pair j's depth sampled bilinearly at where the pixel lands (compose_flows' rule: in the frame and ALL FOUR corners known), rounded
    to float32; info["ratio"][j] is the LOWER median of these over the image, info["samples"][j] their number.  ratio[j] =
    b_j / b_(j-1) multiplies scales[j - 1] to give scales[j].  info["linked"][j]: both poses ok (rotation not all zeros), samples[j]
    >= min_samples and the ratio finite and positive.  scales, segment, trajectory: see the module's text -- lengths in the baseline
    of the segment's first pair, depth[j] * scales[j] the depth in that unit, [I | 0] at every segment start, scale 0 and segment -1
    for a pair without a pose.  info: {"ratio": (T,) float32, "samples": (T,) int32, "linked": (T,) bool}; index 0 is the seam to
    `state`'s pair, 0 / 0 / False without one.
    state: None, or what an earlier call returned -- the last pair's flow, pose, intrinsics, depth and known (views of the
    arguments, not copies: clone what you overwrite), the last trajectory row, the last scale and (segment, segments opened).  A
    sequence fed in batches of any size with state=state gives the bits of one call (track_points' streaming contract); row 0 of a
    call replaces the last row of the call before, the frame they share.
    Two calls give the same bits.  min_samples = 64 is a choice nobody has tuned on real video; a mover along its epipolar line, a
    rotation-only pair and the drift of a running product are the module text's limits.  No autograd."""
    T, H, W = _check_flows(flows, None)
    _check_pose(rotation, translation, T)
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or min_samples < 1:
        raise ValueError(f"min_samples: expected an integer of at least 1, got {min_samples!r}")
    _check_map(depth, "depth", (torch.float32,), (T, H, W))
    _check_map(known, "known", (torch.bool, torch.uint8), (T, H, W))
    if H * W > MAX_PIXELS or T > _lib.TRAJECTORY_MAX_PAIRS:
        raise ValueError(f"flows: {T} pairs of {H} x {W} are beyond what the selection indexes ({MAX_PIXELS} pixels, "
                         f"{_lib.TRAJECTORY_MAX_PAIRS} pairs)")
    k = _intrinsics(intrinsics, T)
    others = dict(flows=flows, rotation=rotation, translation=translation, depth=depth, known=known, intrinsics=k if k.is_cuda else None)
    if state is not None:
        _check_state(state, H, W)
        others.update({f"state['{key}']": state[key] for key in _STATE})
    _check_device(flows, **others)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    k = k.to(dev).contiguous()
    rotation, translation = rotation.detach().contiguous(), translation.detach().contiguous()
    depth = depth.detach()
    L = _lib.lib()
    prev = [None, 2, None, None, None, None]
    chain = [None, None, None, None]
    if state is not None:
        pv, pflow = as_view(state["flow"].detach()[None], "state['flow']")
        held = [pflow, state["rotation"].contiguous(), state["translation"].contiguous(), state["intrinsics"]]
        prev = [_p(pv.ptr), pv.cs, _p(held[1].data_ptr()), _p(held[2].data_ptr()), _p(held[3].data_ptr()), _p(state["known"].data_ptr())]
        chain = [prev[2], _p(state["row"].data_ptr()), _p(state["scale"].data_ptr()), _p(state["segment"].data_ptr())]
    nbytes = L.pwc_scale_links_workspace_bytes(T, H, W, 0 if state is None else 1)
    if nbytes == 0:
        raise _lib.PwcHipError(f"scale links failed: {T} pairs of {H} x {W} are beyond what the selection indexes")
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
    ratio = torch.empty((T,), dtype=torch.float32, device=dev)
    samples = torch.empty((T,), dtype=torch.int32, device=dev)
    _lib.check(L.pwc_scale_links_f32(_p(fv.ptr), fv.cs, _p(rotation.data_ptr()), _p(translation.data_ptr()), _p(k.data_ptr()),
                                     _p(depth.data_ptr()), _p(known.data_ptr()), T, H, W, *prev, _p(ws.data_ptr()), ws.numel() * 8,
                                     _p(ratio.data_ptr()), _p(samples.data_ptr()), _lib.current_stream()), "scale links")
    trajectory = torch.empty((T + 1, 3, 4), dtype=torch.float64, device=dev)
    scales = torch.empty((T,), dtype=torch.float64, device=dev)
    segment = torch.empty((T,), dtype=torch.int32, device=dev)
    linked = torch.empty((T,), dtype=torch.uint8, device=dev)
    segment_state = torch.empty((2,), dtype=torch.int32, device=dev)
    _lib.check(L.pwc_camera_trajectory_f64(_p(rotation.data_ptr()), _p(translation.data_ptr()), _p(ratio.data_ptr()),
                                           _p(samples.data_ptr()), T, int(min_samples), *chain, _p(trajectory.data_ptr()),
                                           _p(scales.data_ptr()), _p(segment.data_ptr()), _p(linked.data_ptr()),
                                           _p(segment_state.data_ptr()), _lib.current_stream()), "camera trajectory")
    state = {"flow": flows[T - 1], "rotation": rotation[T - 1], "translation": translation[T - 1], "intrinsics": k[T - 1],
             "depth": depth[T - 1], "known": known[T - 1], "row": trajectory[T], "scale": scales[T - 1:], "segment": segment_state}
    return trajectory, scales, segment, {"ratio": ratio, "samples": samples, "linked": linked.view(torch.bool)}, state


def flow_trajectory(flows, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0, min_parallax=0.25, min_samples=64, state=None,
                    refine=0):
    """(depth, known, trajectory, scales, segment, info, state): from the consecutive flows of ONE sequence to its depth maps and the
    camera's path in one call -- flow_depth(flows, intrinsics, valid, iters, scale, threshold, min_parallax), then
    camera_trajectory(flows, rotation, translation, intrinsics, depth, known, min_samples, state), nothing in between.

    depth (T,H,W) float32 stays in each pair's OWN baseline, 1e10 where known is False: depth[j] * scales[j] is the depth in the
    unit of pair j's segment.  info is camera_trajectory's with flow_depth's added ("rotation", "translation", "ok" and its info).
    The limits are camera_trajectory's and flow_depth's; every threshold here is a choice nobody has tuned on real video.  No
    autograd.  refine = K > 0 is flow_depth's: the poses are refined by K passes of refine_pose before the depth maps and the chain;
    0, the default, is the call as it was."""
    depth, known, rotation, translation, ok, depth_info = flow_depth(flows, intrinsics, valid=valid, iters=iters, scale=scale,
                                                                     threshold=threshold, min_parallax=min_parallax, refine=refine)
    trajectory, scales, segment, info, state = camera_trajectory(flows, rotation, translation, intrinsics, depth, known,
                                                                 min_samples=min_samples, state=state)
    info = dict(depth_info, rotation=rotation, translation=translation, ok=ok, **info)
    return depth, known, trajectory, scales, segment, info, state
