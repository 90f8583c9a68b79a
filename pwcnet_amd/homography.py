"""Projective camera motion on the HIP path: the homography that explains most of a flow field (csrc/pwc_homography.hip).

    fit_homography(flows, valid=None, iters=4, scale=1.0)    -> (matrices (N,3,3) float64, ok (N,) bool, info)

fit_motion stops at six unknowns; a camera that pans or tilts produces a homography, p' = (M p) / (m6 x + m7 y + 1), whose
division bends a wide frame at its ends.  fit_homography is the reweighted normalised direct linear transform, wholly on the
device: 2 (iters + 1) launches on the current stream and no host synchronisation between the passes.  The exact sequence of
operations is in include/pwc_hip.h, "projective motion"; the kernels equal their numpy restatement bit for bit
(tests/homography_ref.py).  Its matrices are what motion_residual, warp_frames, moving_regions, background_plate, plate_difference
and the host helpers take with projective=True.  No autograd.

scale = 1.0 px, iters = 4 and the rule that a pixel behind the horizon of the pass before is left out are choices: nobody has
tuned them on real video.  From the plain least-squares start a block of outliers of about 15 % of the pixels is voted out in
4 passes; one of 26 % (35 % of the width) is not -- a limit of the start, not of the kernel.
"""
import numpy as np
import torch

from . import _lib
from .modules import _p, as_view
from .motion import MAX_ITERS, _check_device, _check_flows, _ptr


def fit_homography(flows, valid=None, iters=4, scale=1.0):
    """(matrices (N,3,3) torch.float64, ok (N,) torch.bool, info): the dominant homography of every flow of a batch
    (pwc_homography_fit_f64: iters + 1 passes of a sums launch and a solve launch).

    flows, valid, iters, scale, the known-pixel rule and info: fit_motion's.  Each known pixel gives the two rows of the direct
    linear transform in normalised coordinates; pass 0 weighs them 1, a later pass by the Cauchy weight of the pixel's geometric
    residual against the pass before, in pixels, over D^2 (the factor that turns the algebraic error into the geometric one); a
    pixel whose D = g6 xh + g7 yh + 1 is not positive there is left out of that pass.
    matrices[n] takes a pixel (x, y, 1) of the first frame to where the model sends it after the division, p' = (M p) / D with
    D = m6 x + m7 y + 1 (the [2][2] entry is 1): the model flow at p is p' - p.  ok[n] is False where the image is degenerate --
    fewer than 4 known pixels, normal equations whose pivot is not above 1e-9 of the weight sum (pixels on one line), a result
    that is not finite -- or where D is not positive at one of the four frame corners (the horizon would cross the frame); its
    matrix is then the identity.  An image's result does not depend on its neighbours in the batch; two calls give the same
    bits.  scale = 1.0 and iters = 4 are choices nobody has tuned on real video.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"iters: expected an integer in 0 .. {MAX_ITERS}, got {iters!r}")
    if not float(scale) > 0.0:
        raise ValueError(f"scale: expected a positive number, got {scale!r}")
    _check_device(flows, flows=flows, valid=valid)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    L = _lib.lib()
    nbytes = L.pwc_homography_fit_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise _lib.PwcHipError(f"fit homography failed: a batch of {N} flows of {H} x {W} is beyond what the sums index")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    matrices = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((N,), dtype=torch.uint8, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    weight_sum = torch.empty((N,), dtype=torch.float64, device=dev)
    _lib.check(L.pwc_homography_fit_f64(_p(fv.ptr), fv.cs, _ptr(valid), N, H, W, int(iters), float(scale), _p(ws.data_ptr()), nbytes,
                                        _p(matrices.data_ptr()), _p(ok.data_ptr()), _p(count.data_ptr()), _p(weight_sum.data_ptr()),
                                        _lib.current_stream()), "fit homography")
    return matrices, ok.view(torch.bool), {"count": count, "weight_sum": weight_sum}
