"""Relative pose and depth from flow on the HIP path: with a calibration, how the camera moved between the two frames of a flow
field and how far away every rigid pixel is (csrc/pwc_pose.hip).

    camera_pose(flows, matrices, intrinsics, valid=None, threshold=1.0)          -> (rotation (N,3,3) f64, translation (N,3) f64, ok, info)
    triangulate_depth(flows, rotation, translation, intrinsics, valid=None,
                      min_parallax=0.25, return_parallax=False)                  -> (depth (N,H,W) f32, known (N,H,W) bool[, parallax])
    flow_depth(flows, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0,
               min_parallax=0.25, refine=0)                                      -> (depth, known, rotation, translation, ok, info)

fit_fundamental says which pixels belong to the rigid scene.  With the intrinsics fx fy cx cy of the camera, in pixels of the
flow's grid and the same for both frames, its matrix becomes the essential matrix E = K^T F K = [t]x R, whose closed-form
decomposition gives four candidate poses; the one under which the scene lies in front of both cameras is chosen by a vote of the
inlier pixels, and every pixel is then triangulated.  X' = R X + t takes a point of the first camera's frame to the second's.
The exact sequence of operations is in include/pwc_hip.h, "relative pose and depth"; the kernels equal their numpy restatement bit
for bit (tests/pose_ref.py).  No autograd.

Units: the length of a two-view translation cannot be observed, so translation has unit length and every depth is in BASELINES,
multiples of the distance the camera moved between the two frames.  Each pair of a sequence has its own baseline and therefore its
own scale: depths of different pairs are not comparable until pwcnet_amd.trajectory has chained the scales.
What this cannot do:
  * A camera that only rotates (or a flat scene) leaves F undetermined: fit_fundamental's ok is False upstream, its matrix is all
    zeros, and camera_pose then gives ok False and triangulate_depth an all-unknown map.
  * A pixel that moves on its own has no meaningful depth; triangulate_depth does not test the epipolar constraint, the caller
    passes valid=inlier from epipolar_residual (flow_depth does).
  * Near the epipole the parallax is small and the depth is noise: min_parallax switches those pixels off.
threshold = 1.0 px, min_parallax = 0.25 px and the rule that the winning candidate must hold more than half the voters are
choices: nobody has tuned them on real video, and nobody has measured the depth quality on network flows of real footage.
"""
import numpy as np
import torch

from . import _lib
from .fundamental import epipolar_residual, fit_fundamental
from .modules import _p, as_view
from .motion import _check_device, _check_flows, _check_matrices, _ptr


def _intrinsics(intrinsics, N):
    """(N,4) float64 from a (4,) or (N,4) sequence, numpy array or tensor: fx fy cx cy (on whatever device it came on)."""
    if isinstance(intrinsics, torch.Tensor):
        k = intrinsics.detach().to(torch.float64)
    else:
        try:
            k = torch.from_numpy(np.array(intrinsics, dtype=np.float64))
        except (TypeError, ValueError) as e:
            raise TypeError(f"intrinsics: expected four numbers fx fy cx cy, or N rows of them, got {type(intrinsics)}") from e
    if tuple(k.shape) == (4,):
        k = k[None].expand(N, 4)
    if tuple(k.shape) != (N, 4):
        raise ValueError(f"intrinsics: expected shape (4,) or {(N, 4)}: fx fy cx cy per image, got {tuple(k.shape)}")
    return k


def _check_pose(rotation, translation, N):
    for what, t, shape in (("rotation", rotation, (N, 3, 3)), ("translation", translation, (N, 3))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise TypeError(f"{what}: expected a torch.float64 tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t)}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: expected shape {shape}, one per image, got {tuple(t.shape)}")


def camera_pose(flows, matrices, intrinsics, valid=None, threshold=1.0):
    """(rotation (N,3,3) torch.float64, translation (N,3) torch.float64, ok (N,) torch.bool, info): the relative pose of the two
    frames of every flow of a batch (pwc_camera_pose_f64: a decompose, a vote and a select launch, no host synchronisation).

    flows, valid: as fit_fundamental's.  matrices: (N,3,3) torch.float64, fit_fundamental's.  intrinsics: fx fy cx cy in pixels
    of the flow's grid, a (4,) or (N,4) sequence, numpy array or tensor; both frames share them.  E = K^T F K is decomposed in
    closed form (a cyclic Jacobi decomposition of E^T E, the singular values forced to (1, 1, 0)) into the four textbook
    candidates; every pixel whose flow is known, that `valid` admits and whose Sampson distance to F is at most `threshold` px
    (epipolar_residual's inlier rule) votes for each candidate under which it lies in front of both cameras.
    X' = rotation X + translation takes a point of the first camera's frame to the second's.  translation has unit length: the
    baseline of two views cannot be observed, and each pair of a sequence has its own.  ok[n] is False, and rotation and
    translation all zeros, where the image's F is all zeros (fit_fundamental's ok False: a camera that only rotates gives that
    upstream), an intrinsic is not finite or a focal length not positive, a value is not finite, nobody votes, or the winner
    does not hold strictly more than half the voters.  info: {"votes": (N,4) int32 in the order (R_a, +t), (R_a, -t), (R_b, +t),
    (R_b, -t), "voters": (N,) int32, "singular": (N,2) float64, the second and third singular value of E over the first -- (1, 0)
    for an essential matrix --, "essential": (N,3,3) float64, K^T F K as computed}.
    An image's result does not depend on its neighbours in the batch; two calls give the same bits.  threshold = 1.0 px and the
    half-the-voters rule are choices nobody has tuned on real video.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    _check_matrices(matrices, N)
    if not float(threshold) >= 0.0:
        raise ValueError(f"threshold: expected a non-negative number, got {threshold!r}")
    k = _intrinsics(intrinsics, N)
    _check_device(flows, flows=flows, valid=valid, matrices=matrices, intrinsics=k if k.is_cuda else None)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    k = k.to(dev).contiguous()
    matrices = matrices.detach().contiguous()
    L = _lib.lib()
    nbytes = L.pwc_camera_pose_workspace_bytes(N)
    if nbytes == 0:
        raise _lib.PwcHipError(f"camera pose failed: a batch of {N} flows is beyond what the grid indexes")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    rotation = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    translation = torch.empty((N, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((N,), dtype=torch.uint8, device=dev)
    votes = torch.empty((N, 4), dtype=torch.int32, device=dev)
    voters = torch.empty((N,), dtype=torch.int32, device=dev)
    singular = torch.empty((N, 2), dtype=torch.float64, device=dev)
    essential = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    _lib.check(L.pwc_camera_pose_f64(_p(fv.ptr), fv.cs, _ptr(valid), _p(matrices.data_ptr()), _p(k.data_ptr()), N, H, W, float(threshold),
                                     _p(ws.data_ptr()), nbytes, _p(rotation.data_ptr()), _p(translation.data_ptr()), _p(ok.data_ptr()),
                                     _p(votes.data_ptr()), _p(voters.data_ptr()), _p(singular.data_ptr()), _p(essential.data_ptr()),
                                     _lib.current_stream()), "camera pose")
    return rotation, translation, ok.view(torch.bool), {"votes": votes, "voters": voters, "singular": singular, "essential": essential}


def triangulate_depth(flows, rotation, translation, intrinsics, valid=None, min_parallax=0.25, return_parallax=False):
    """(depth (N,H,W) float32, known (N,H,W) torch.bool[, parallax (N,H,W) float32]): every pixel's depth in the FIRST camera under
    the pose of camera_pose (pwc_triangulate_depth_f32, one launch, a lane per pixel).

    flows, valid, intrinsics: camera_pose's.  rotation (N,3,3), translation (N,3): torch.float64, camera_pose's.  depth is in
    BASELINES (|translation| = 1), computed in double and rounded once; each pair of a sequence has its own baseline, so the
    depths of different pairs are not comparable.  parallax is the distance in pixels between where the pixel lands and where a
    point at infinity on the same ray would land; the relative error of the depth is about the flow's error over it.
    known is False and depth 1e10 where the flow is unknown, valid is 0, the image's rotation is all zeros (camera_pose's ok
    False -- a camera that only rotates ends here, through fit_fundamental's ok False upstream), its intrinsics are not usable,
    the point would lie behind either camera, or parallax < min_parallax.
    The epipolar constraint is NOT tested: a pixel that moves on its own gets a meaningless depth.  Pass valid=inlier from
    epipolar_residual (flow_depth does).  min_parallax = 0.25 px is a choice nobody has tuned on real video.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    _check_pose(rotation, translation, N)
    if not float(min_parallax) >= 0.0:
        raise ValueError(f"min_parallax: expected a non-negative number, got {min_parallax!r}")
    k = _intrinsics(intrinsics, N)
    _check_device(flows, flows=flows, valid=valid, rotation=rotation, translation=translation, intrinsics=k if k.is_cuda else None)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    k = k.to(dev).contiguous()
    rotation, translation = rotation.detach().contiguous(), translation.detach().contiguous()
    depth = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    known = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    parallax = torch.empty((N, H, W), dtype=torch.float32, device=dev) if return_parallax else None
    _lib.check(_lib.lib().pwc_triangulate_depth_f32(_p(fv.ptr), fv.cs, _ptr(valid), _p(rotation.data_ptr()), _p(translation.data_ptr()),
                                                    _p(k.data_ptr()), N, H, W, float(min_parallax), _p(depth.data_ptr()),
                                                    _p(known.data_ptr()), _ptr(parallax), _lib.current_stream()), "triangulate depth")
    if return_parallax:
        return depth, known.view(torch.bool), parallax
    return depth, known.view(torch.bool)


def flow_depth(flows, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0, min_parallax=0.25, refine=0):
    """(depth, known, rotation, translation, ok, info): depth from flow in one call -- fit_fundamental(flows, valid, iters, scale),
    epipolar_residual(flows, matrices, valid, threshold), camera_pose(flows, matrices, intrinsics, valid, threshold) and
    triangulate_depth(flows, rotation, translation, intrinsics, valid=inlier, min_parallax), nothing in between.

    depth (N,H,W) float32 in BASELINES, 1e10 where known (N,H,W) torch.bool is False: each pair of a sequence has its own scale.
    ok is camera_pose's; info is camera_pose's with "matrices", "fit_ok", "distance" and "inlier" added.  A camera that only rotates
    gives fit_fundamental's ok False upstream, hence ok False and an all-unknown map.  iters, scale: fit_fundamental's; threshold,
    min_parallax and the half-the-voters rule are choices nobody has tuned on real video.  No autograd.

    refine = K > 0 runs pwcnet_amd.refine_pose(flows, rotation, translation, intrinsics, valid, iters=K, scale, threshold) between
    camera_pose and triangulate_depth: rotation, translation and the depth are then the refined pose's, an image whose refinement is
    not ok keeps camera_pose's, and info gains "closed_rotation", "closed_translation" (camera_pose's) and "refine_ok", "samples",
    "best_pass", "cost", "weight_sum" (refine_pose's).  refine = 0, the default, is the call as it was: the same launches, the same
    bits."""
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
        raise ValueError(f"refine: expected a non-negative integer, the passes of refine_pose, got {refine!r}")
    matrices, fit_ok, _ = fit_fundamental(flows, valid=valid, iters=iters, scale=scale)
    distance, inlier = epipolar_residual(flows, matrices, valid=valid, threshold=threshold)
    rotation, translation, ok, info = camera_pose(flows, matrices, intrinsics, valid=valid, threshold=threshold)
    if refine > 0:
        from .pose_refine import refine_pose
        closed_rotation, closed_translation = rotation, translation
        refined, moved, refine_ok, refine_info = refine_pose(flows, rotation, translation, intrinsics, valid=valid, iters=refine,
                                                             scale=scale, threshold=threshold)
        rotation = torch.where(refine_ok[:, None, None], refined, closed_rotation)
        translation = torch.where(refine_ok[:, None], moved, closed_translation)
        info = dict(info, closed_rotation=closed_rotation, closed_translation=closed_translation, refine_ok=refine_ok, **refine_info)
    depth, known = triangulate_depth(flows, rotation, translation, intrinsics, valid=inlier, min_parallax=min_parallax)
    info = dict(info, matrices=matrices, fit_ok=fit_ok, distance=distance, inlier=inlier)
    return depth, known, rotation, translation, ok, info
