"""Epipolar camera motion on the HIP path: the fundamental matrix that explains most of a flow field, every pixel's Sampson distance
to it, and what breaks it as regions (csrc/pwc_fundamental.hip).

    fit_fundamental(flows, valid=None, iters=4, scale=1.0)               -> (matrices (N,3,3) float64, ok (N,) bool, info)
    epipolar_residual(flows, matrices, valid=None, threshold=1.0)        -> (distance (N,H,W) float32, inlier (N,H,W) bool)
    epipolar_regions(flows, matrices, valid=None, threshold=1.0, **kw)   -> (labels, count, regions, distance, inlier)

fit_motion and fit_homography are point maps: exact for a camera that rotates or a scene that is flat.  A camera that translates
through a scene with depth -- a dolly, a drone, a car -- produces parallax, which no point map explains; what still holds for
everything rigid is the epipolar constraint p'^T F p = 0, and what moves on its own is what breaks it.  fit_fundamental is the
reweighted normalised eight-point fit, wholly on the device: 2 (iters + 1) launches on the current stream and no host
synchronisation between the passes.  The exact sequence of operations is in include/pwc_hip.h, "epipolar motion"; the kernels
equal their numpy restatement bit for bit (tests/fundamental_ref.py).  No autograd.

What the model cannot do:
  * An object that moves ALONG its epipolar line passes the test: a car ahead driving the way the camera drives is such an object.
  * A camera that only rotates (or a flat scene) leaves F undetermined: ok is then False, info["eigen"] shows how close a clip is
    to that, and the homography (fit_homography) is the model to use.  Nothing here switches models by itself.
threshold = 1.0 px, scale = 1.0 px, iters = 4, the rule that a second-smallest eigenvalue at or below 1e-9 of the trace is
degenerate and the 10 Jacobi sweeps are choices: nobody has tuned them on real video.  From the plain least-squares start a small
block of outliers can capture the fit when the parallax is weak -- a limit of the start, not of the kernel.
"""
import numpy as np
import torch

from . import _lib
from .modules import _p, as_view
from .motion import MAX_ITERS, _check_device, _check_flows, _check_matrices, _ptr
from .regions import label_regions


def fit_fundamental(flows, valid=None, iters=4, scale=1.0):
    """(matrices (N,3,3) torch.float64, ok (N,) torch.bool, info): the fundamental matrix of every flow of a batch
    (pwc_fundamental_fit_f64: iters + 1 passes of a sums launch and a solve launch).

    flows, valid, iters, scale and the known-pixel rule: fit_homography's.  Each known pixel gives one row of the eight-point
    system in normalised coordinates; pass 0 weighs them 1, a later pass by the Cauchy weight of the pixel's Sampson distance to
    the pass before, in pixels, over the gradient factor g that turns the algebraic error into the geometric one; a pixel whose g
    is not positive there is left out of that pass.  The solve is a cyclic Jacobi eigen-decomposition (10 sweeps) of the 9 x 9
    moment matrix; the matrix is forced to rank 2.
    matrices[n] satisfies p'^T F p = 0 for a rigid point seen at p = (x, y, 1) in the first frame and p' = p + flow in the second;
    Frobenius norm 1, the entry of largest magnitude positive.  ok[n] is False, and the matrix all zeros, where the image is
    degenerate: fewer than 8 known pixels, a value that is not finite, or a second-smallest eigenvalue not above 1e-9 of the
    trace -- the flow is then a homography's (a camera that only rotates, a flat scene) and F is not determined; use
    fit_homography there.  info: {"count": (N,) int32 known pixels, "weight_sum": (N,) float64 of the last pass, "eigen": (N,2)
    float64, the two smallest eigenvalues over the trace (how close the clip is to degenerate), "epipole": (N,3) float64, the
    homogeneous epipole of the first frame in pixels, F e = 0}.
    An object that moves along its epipolar line satisfies the constraint and cannot be told from the scene.  An image's result
    does not depend on its neighbours in the batch; two calls give the same bits.  scale = 1.0, iters = 4, the 1e-9 rule and the
    sweep count are choices nobody has tuned on real video.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"iters: expected an integer in 0 .. {MAX_ITERS}, got {iters!r}")
    if not float(scale) > 0.0:
        raise ValueError(f"scale: expected a positive number, got {scale!r}")
    _check_device(flows, flows=flows, valid=valid)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    L = _lib.lib()
    nbytes = L.pwc_fundamental_fit_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise _lib.PwcHipError(f"fit fundamental failed: a batch of {N} flows of {H} x {W} is beyond what the sums index")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    matrices = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((N,), dtype=torch.uint8, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    weight_sum = torch.empty((N,), dtype=torch.float64, device=dev)
    eigen = torch.empty((N, 2), dtype=torch.float64, device=dev)
    epipole = torch.empty((N, 3), dtype=torch.float64, device=dev)
    _lib.check(L.pwc_fundamental_fit_f64(_p(fv.ptr), fv.cs, _ptr(valid), N, H, W, int(iters), float(scale), _p(ws.data_ptr()), nbytes,
                                         _p(matrices.data_ptr()), _p(ok.data_ptr()), _p(count.data_ptr()), _p(weight_sum.data_ptr()),
                                         _p(eigen.data_ptr()), _p(epipole.data_ptr()), _lib.current_stream()), "fit fundamental")
    return matrices, ok.view(torch.bool), {"count": count, "weight_sum": weight_sum, "eigen": eigen, "epipole": epipole}


def epipolar_residual(flows, matrices, valid=None, threshold=1.0):
    """(distance (N,H,W) float32, inlier (N,H,W) torch.bool): every pixel's Sampson distance to the epipolar constraint of
    `matrices`, in pixels, and the pixels that satisfy it (pwc_epipolar_residual_f32, one launch, a lane per pixel).

    flows, valid: as fit_fundamental's.  matrices: (N,3,3) torch.float64, fit_fundamental's.  distance = |p'^T F p| / sqrt(g),
    computed in double in pixel coordinates and rounded once; inlier where distance <= threshold (of the double, before the
    rounding).  distance holds 1e10 and inlier is False where the flow is unknown, valid is 0, g is not positive, or the image's
    matrix is all zeros (fit_fundamental's ok False).  A pixel that moves along its epipolar line is an inlier whatever its speed.
    threshold = 1.0 px is a choice nobody has tuned on real video.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    _check_matrices(matrices, N)
    if not float(threshold) >= 0.0:
        raise ValueError(f"threshold: expected a non-negative number, got {threshold!r}")
    _check_device(flows, flows=flows, valid=valid, matrices=matrices)
    fv, flows = as_view(flows.detach(), "flows")
    matrices = matrices.detach().contiguous()
    distance = torch.empty((N, H, W), dtype=torch.float32, device=flows.device)
    inlier = torch.empty((N, H, W), dtype=torch.uint8, device=flows.device)
    _lib.check(_lib.lib().pwc_epipolar_residual_f32(_p(fv.ptr), fv.cs, _ptr(valid), _p(matrices.data_ptr()), N, H, W, float(threshold),
                                                    _p(distance.data_ptr()), _p(inlier.data_ptr()), _lib.current_stream()),
               "epipolar residual")
    return distance, inlier.view(torch.bool)


def epipolar_regions(flows, matrices, valid=None, threshold=1.0, **label_kw):
    """(labels, count, regions, distance, inlier): what breaks the epipolar constraint, as objects -- epipolar_residual followed by
    label_regions(inlier, invert=True, flows=flows, ...), nothing in between.

    flows, matrices, valid, threshold: epipolar_residual's.  label_kw: connectivity, min_area, max_regions of label_regions.  A
    region is a connected set of pixels whose flow is known and lies more than `threshold` px off its epipolar line; unknown
    pixels fall out through the flow rule, pixels that `valid` excludes do not (they are no inliers): mask the flow itself to
    drop them.  regions["mean"] is the region's mean flow ITSELF, in pixels: no point map exists to subtract.  The output feeds
    track_regions unchanged.  An object that moves along its epipolar line -- a car ahead driving the way the camera drives --
    is not found; where the camera only rotates, ok is False, every pixel of that image is a region candidate, and
    moving_regions with fit_homography is the tool.  Nothing here judges segmentation quality on real video."""
    unknown = set(label_kw) - {"connectivity", "min_area", "max_regions"}
    if unknown:
        raise TypeError(f"epipolar_regions: unexpected keyword arguments {sorted(unknown)}")
    distance, inlier = epipolar_residual(flows, matrices, valid=valid, threshold=threshold)
    labels, count, regions = label_regions(inlier, flows=flows, invert=True, **label_kw)
    return labels, count, regions, distance, inlier
