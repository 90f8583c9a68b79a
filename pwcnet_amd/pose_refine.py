"""Refinement of the relative pose on the HIP path: camera_pose's closed form fitted to the Sampson distance of its inliers
(csrc/pwc_pose_refine.hip).

    refine_pose(flows, rotation, translation, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0)
        -> (rotation (N,3,3) f64, translation (N,3) f64, ok (N,) bool, info {"samples", "best_pass", "cost" (N, iters+1), "weight_sum"})

camera_pose decomposes an algebraic eight-point fit: eight unknowns where the calibrated problem has five, and the wrong error.
refine_pose takes that pose as its start and runs a reweighted Gauss-Newton fit of the five parameters -- a rotation update by the
Cayley map and a step of the unit translation in its tangent plane -- to the Sampson distance in pixels, over the pixels that are
inliers of the INPUT pose.  The pixel set is fixed for the whole call, so the costs of the passes are comparable, and the pose of
the pass with the lowest cost is returned: it never fits that set worse than the input did, in the op's own robust cost.  The
exact sequence of operations is in include/pwc_hip.h, "pose refinement"; the kernels equal their numpy restatement bit for bit
(tests/pose_refine_ref.py).  No autograd.

What this cannot do: what the closed form cannot -- a point that moves along its epipolar line satisfies the constraint, a camera
that only rotates has no pose upstream (ok False, zeros here); it refines one pair at a time and no structure: it is no bundle
adjustment over a sequence; a bad start stays bad, because the input pose chooses the pixel set.
"""
import numpy as np
import torch

from . import _lib
from .modules import _p, as_view
from .motion import _check_device, _check_flows, _ptr
from .pose import _check_pose, _intrinsics


def refine_pose(flows, rotation, translation, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0):
    """(rotation (N,3,3) torch.float64, translation (N,3) torch.float64, ok (N,) torch.bool, info): the pose of camera_pose refined
    on the Sampson distance of its inliers (pwc_pose_refine_f64: iters + 1 sums launches and iters + 1 solve launches, no host
    synchronisation).

    flows, valid, intrinsics: camera_pose's.  rotation (N,3,3), translation (N,3): torch.float64, camera_pose's.  The pixel set is
    fixed for the call: the pixels whose flow is known, that `valid` admits and whose Sampson distance to the INPUT pose is at most
    `threshold` px (inf: every known pixel).  Each of the iters + 1 passes sums, over that set and under the pass's pose, the
    Gauss-Newton system of the five parameters with the Cauchy weight 1 / (1 + d^2 / scale^2) and the robust cost sum w d^2; the
    first iters passes solve it (an L D L^T elimination, a pivot must exceed 1e-9 times the trace) and step.  Returned is the pose
    of the pass with the lowest cost, ties to the earlier pass: iters = 0 returns the input bit for bit with its cost, and
    cost[best_pass] <= cost[0] always.  X' = rotation X + translation as camera_pose has it; translation has unit length, so depths
    stay in BASELINES and each pair of a sequence keeps its own scale.
    ok[n] is False, and rotation, translation, cost and weight_sum all zeros, where the image's input rotation is all zeros
    (camera_pose's ok False -- a camera that only rotates ends here), an intrinsic is not usable, or fewer than 5 pixels take part.
    A failed pivot or a value that is not finite freezes an image: it keeps its best pose so far and its later costs are 0.
    info: {"samples": (N,) int32, the pixels of the set, "best_pass": (N,) int32, "cost": (N, iters+1) float64, "weight_sum": (N,)
    float64, of the best pass}.
    An image's result does not depend on its neighbours in the batch; two calls give the same bits.  scale = 1.0 px, threshold =
    1.0 px, iters = 4, the pivot rule and the Jacobian that holds the Sampson gradient fixed inside a pass are choices nobody has
    tuned on real video.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    _check_pose(rotation, translation, N)
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= _lib.MOTION_MAX_ITERS:
        raise ValueError(f"iters: expected an integer in 0 .. {_lib.MOTION_MAX_ITERS}, got {iters!r}")
    if not float(scale) > 0.0:
        raise ValueError(f"scale: expected a positive number of pixels, got {scale!r}")
    if not float(threshold) >= 0.0:
        raise ValueError(f"threshold: expected a non-negative number, got {threshold!r}")
    k = _intrinsics(intrinsics, N)
    _check_device(flows, flows=flows, valid=valid, rotation=rotation, translation=translation, intrinsics=k if k.is_cuda else None)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    k = k.to(dev).contiguous()
    rotation, translation = rotation.detach().contiguous(), translation.detach().contiguous()
    L = _lib.lib()
    nbytes = L.pwc_pose_refine_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise _lib.PwcHipError(f"pose refinement failed: {N} flows of {H} x {W} are beyond what the grid indexes")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    refined = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    moved = torch.empty((N, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((N,), dtype=torch.uint8, device=dev)
    samples = torch.empty((N,), dtype=torch.int32, device=dev)
    best_pass = torch.empty((N,), dtype=torch.int32, device=dev)
    cost = torch.empty((N, int(iters) + 1), dtype=torch.float64, device=dev)
    weight_sum = torch.empty((N,), dtype=torch.float64, device=dev)
    _lib.check(L.pwc_pose_refine_f64(_p(fv.ptr), fv.cs, _ptr(valid), _p(k.data_ptr()), _p(rotation.data_ptr()), _p(translation.data_ptr()),
                                     N, H, W, int(iters), float(scale), float(threshold), _p(ws.data_ptr()), nbytes, _p(refined.data_ptr()),
                                     _p(moved.data_ptr()), _p(ok.data_ptr()), _p(samples.data_ptr()), _p(best_pass.data_ptr()),
                                     _p(cost.data_ptr()), _p(weight_sum.data_ptr()), _lib.current_stream()), "pose refinement")
    return refined, moved, ok.view(torch.bool), {"samples": samples, "best_pass": best_pass, "cost": cost, "weight_sum": weight_sum}
