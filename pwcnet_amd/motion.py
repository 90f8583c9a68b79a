"""Dominant motion on the HIP path: the one parametric motion that explains most of a flow field, the flow it leaves, and frames
warped by it (csrc/pwc_motion.hip).

    fit_motion(flows, valid=None, model="affine", iters=4, scale=1.0)    -> (matrices (N,3,3) float64, ok (N,) bool, info)
    motion_residual(flows, matrices, valid=None, threshold=3.0)          -> (residual (N,H,W,2) float32, inlier (N,H,W) bool)
    warp_frames(frames, matrices)                                        -> (out (N,H,W,C), covered (N,H,W) bool)
    smooth_path(matrices, radius)                                        -> (T+1,3,3) float64 numpy, the matrices warp_frames wants

The last three take projective=True for the matrices of homography.fit_homography: the position of a pixel is then
(M p) / (m6 x + m7 y + m8), and there is none where that divisor is not positive (include/pwc_hip.h, "projective motion").

fit_motion is a robust fit (iteratively reweighted least squares with the Cauchy weight) of a translation, a similarity or an
affine motion to every flow of a batch, wholly on the device: 2 (iters + 1) launches on the current stream and no host
synchronisation between the passes.  The exact sequence of operations is in include/pwc_hip.h, "dominant motion"; the kernels
equal their numpy restatement bit for bit (tests/motion_ref.py).  No autograd.

scale = 1.0 px and iters = 4 are choices: nobody has tuned them on real video.
"""
import numpy as np
import torch

from . import _lib
from .interp import _check_mask
from .modules import _p, as_view
from .unsup import _check_nhwc

MODELS = {"translation": _lib.MOTION_TRANSLATION, "similarity": _lib.MOTION_SIMILARITY, "affine": _lib.MOTION_AFFINE}
MAX_ITERS = _lib.MOTION_MAX_ITERS


def _check_flows(flows, valid):
    _check_nhwc(flows, "flows", (2,))
    N, H, W, _ = flows.shape
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows: empty tensor, shape {tuple(flows.shape)}")
    _check_mask(valid, "valid", N, H, W)
    return N, H, W


def _check_matrices(matrices, N):
    if not isinstance(matrices, torch.Tensor) or matrices.dtype != torch.float64:
        raise TypeError(f"matrices: expected a torch.float64 tensor, got "
                        f"{matrices.dtype if isinstance(matrices, torch.Tensor) else type(matrices)}")
    if tuple(matrices.shape) != (N, 3, 3):
        raise ValueError(f"matrices: expected shape {(N, 3, 3)}, one matrix per image, got {tuple(matrices.shape)}")


def _check_device(first, **others):
    for what, t in others.items():
        if t is not None and (not t.is_cuda or t.device != first.device):
            raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only, all arguments on one device")


def _ptr(t):
    return None if t is None else _p(t.data_ptr())


def fit_motion(flows, valid=None, model="affine", iters=4, scale=1.0):
    """(matrices (N,3,3) torch.float64, ok (N,) torch.bool, info): the dominant motion of every flow of a batch
    (pwc_motion_fit_f64: iters + 1 passes of a sums launch and a solve launch).

    flows: (N,H,W,2) float32 in pixels, on the GPU; a channel slice of a wider buffer is read in place; read detached.  valid:
    (N,H,W) torch.bool / torch.uint8, contiguous, None = every pixel; a pixel whose flow fails flow_io.flow_valid's rule is left
    out as well.  model: "translation" (2 unknowns), "similarity" (4: rotation, uniform scale, shift) or "affine" (6).  iters:
    0 .. 64 reweighting passes after the plain least-squares pass; scale: the Cauchy scale in pixels -- a pixel whose residual
    against the pass before is r weighs 1 / (1 + |r|^2 / scale^2).
    matrices[n] takes a pixel (x, y, 1) of the first frame to where the model sends it, p' = M p: the model flow at p is
    M p - p.  ok[n] is False where the image is degenerate -- fewer known pixels than 1 / 2 / 3, or normal equations whose
    pivot is not above 1e-9 of the weight sum (a row of pixels cannot hold a rotation) -- and its matrix is then the identity.
    info: {"count": (N,) int32 known pixels, "weight_sum": (N,) float64, the sum of the weights of the last pass}.
    An image's result does not depend on its neighbours in the batch; two calls give the same bits.  scale = 1.0 and iters = 4
    are choices nobody has tuned on real video.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    if model not in MODELS:
        raise ValueError(f"model: expected one of {sorted(MODELS)}, got {model!r}")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"iters: expected an integer in 0 .. {MAX_ITERS}, got {iters!r}")
    if not float(scale) > 0.0:
        raise ValueError(f"scale: expected a positive number, got {scale!r}")
    _check_device(flows, flows=flows, valid=valid)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    L = _lib.lib()
    nbytes = L.pwc_motion_fit_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise _lib.PwcHipError(f"fit motion failed: a batch of {N} flows of {H} x {W} is beyond what the sums index")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    matrices = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((N,), dtype=torch.uint8, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    weight_sum = torch.empty((N,), dtype=torch.float64, device=dev)
    _lib.check(L.pwc_motion_fit_f64(_p(fv.ptr), fv.cs, _ptr(valid), N, H, W, MODELS[model], int(iters), float(scale),
                                    _p(ws.data_ptr()), nbytes, _p(matrices.data_ptr()), _p(ok.data_ptr()), _p(count.data_ptr()),
                                    _p(weight_sum.data_ptr()), _lib.current_stream()), "fit motion")
    return matrices, ok.view(torch.bool), {"count": count, "weight_sum": weight_sum}


def motion_residual(flows, matrices, valid=None, threshold=3.0, projective=False):
    """(residual (N,H,W,2) float32, inlier (N,H,W) torch.bool): the flow with the motion of `matrices` taken out, and the pixels
    that move with it (pwc_motion_residual_f32, one launch, a lane per pixel).

    flows, valid: as fit_motion's.  matrices: (N,3,3) torch.float64, fit_motion's.  residual = flow - (M p - p), computed in
    double and rounded once; inlier where |residual|^2 <= threshold^2 (of the double, before the rounding).  An unknown pixel
    holds the .flo sentinel 1e10 in both components and is no inlier (compose_flows' convention), and so does every pixel of an
    image whose matrix is not affine (last row other than exactly 0 0 1) or not finite.
    projective=True (pwc_motion_residual_projective_f32): matrices are fit_homography's; residual = flow - (pos - p) with the
    projective position pos = (M p) / D, D = m6 x + m7 y + m8; the sentinel and no inlier where D is not positive, and everywhere
    in an image one of whose nine entries is not finite.  An affine matrix gives the bits of projective=False.  No autograd."""
    N, H, W = _check_flows(flows, valid)
    _check_matrices(matrices, N)
    if not isinstance(projective, (bool, np.bool_)):
        raise TypeError(f"projective: expected a bool, got {projective!r}")
    if not float(threshold) >= 0.0:
        raise ValueError(f"threshold: expected a non-negative number, got {threshold!r}")
    _check_device(flows, flows=flows, valid=valid, matrices=matrices)
    fv, flows = as_view(flows.detach(), "flows")
    matrices = matrices.detach().contiguous()
    residual = torch.empty((N, H, W, 2), dtype=torch.float32, device=flows.device)
    inlier = torch.empty((N, H, W), dtype=torch.uint8, device=flows.device)
    entry = _lib.lib().pwc_motion_residual_projective_f32 if projective else _lib.lib().pwc_motion_residual_f32
    _lib.check(entry(_p(fv.ptr), fv.cs, _ptr(valid), _p(matrices.data_ptr()), N, H, W, float(threshold), _p(residual.data_ptr()),
                     _p(inlier.data_ptr()), _lib.current_stream()), "motion residual")
    return residual, inlier.view(torch.bool)


def warp_frames(frames, matrices, projective=False):
    """(out (N,H,W,C) in the frames' dtype, covered (N,H,W) torch.bool): every frame resampled through its matrix
    (pwc_warp_affine, one launch, a lane per four output pixels).

    frames: (N,H,W,C) torch.uint8 or torch.float32, C = 1 .. 4, on the GPU (made contiguous).  matrices: (N,3,3) torch.float64 or
    a numpy array (smooth_path's), each taking an OUTPUT pixel (x, y, 1) to its position in the source frame.  A position inside
    [0, W - 1] x [0, H - 1] is sampled bilinearly with clamped corners (fb_valid's sample, in double) and rounded once -- to
    float32, or rint clamped to [0, 255] for bytes.  Elsewhere, and everywhere in an image whose matrix is not affine (last row
    other than exactly 0 0 1) or not finite, the output is 0 and covered is False.
    projective=True (pwc_warp_projective): the source position is (M p) / D, D = m6 x + m7 y + m8; not covered where D is not
    positive, and everywhere in an image one of whose nine entries is not finite.  An affine matrix gives the bits of
    projective=False.  No autograd."""
    if not isinstance(projective, (bool, np.bool_)):
        raise TypeError(f"projective: expected a bool, got {projective!r}")
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"frames: expected a torch.uint8 or torch.float32 tensor, got "
                        f"{frames.dtype if isinstance(frames, torch.Tensor) else type(frames)}")
    if frames.dim() != 4 or not 1 <= frames.shape[3] <= 4 or min(frames.shape) < 1:
        raise ValueError(f"frames: expected an (N, H, W, C) tensor with 1 to 4 channels, got shape {tuple(frames.shape)}")
    N, H, W, C = frames.shape
    if isinstance(matrices, np.ndarray):
        if matrices.dtype != np.float64:
            raise TypeError(f"matrices: expected a float64 array, got {matrices.dtype}")
        matrices = torch.from_numpy(np.ascontiguousarray(matrices)).to(frames.device)
    _check_matrices(matrices, N)
    _check_device(frames, frames=frames, matrices=matrices)
    frames = frames.detach().contiguous()
    matrices = matrices.detach().contiguous()
    out = torch.empty_like(frames)
    covered = torch.empty((N, H, W), dtype=torch.uint8, device=frames.device)
    dtype = _lib.MOTION_U8 if frames.dtype == torch.uint8 else _lib.MOTION_F32
    entry = _lib.lib().pwc_warp_projective if projective else _lib.lib().pwc_warp_affine
    _lib.check(entry(_p(frames.data_ptr()), dtype, C, _p(matrices.data_ptr()), N, H, W, _p(out.data_ptr()), _p(covered.data_ptr()),
                     _lib.current_stream()), "warp frames")
    return out, covered.view(torch.bool)


def smooth_path(matrices, radius, projective=False):
    """(T + 1, 3, 3) float64 numpy: the stabilising matrices A_t of a sequence of T + 1 frames from the T motions between them,
    one per frame, the matrices warp_frames wants.  Host numpy float64.

    matrices: (T,3,3), fit_motion's (a tensor or an array), M_t taking frame t to frame t + 1.  The path is P_0 = I,
    P_t = M_(t-1) P_(t-1): where a pixel of frame 0 is in frame t.  Pbar_t is the mean of the six affine entries of P over
    [t - radius, t + radius], clipped to the sequence, and A_t = P_t inv(Pbar_t) takes a pixel of the stabilised frame t to
    where frame t holds it.  radius = 0 gives identities.
    The entry-wise mean of affine matrices is a choice: it is not a geodesic mean (it does not average rotations as rotations),
    it is what is cheap and behaves for the small motions between neighbouring frames.
    projective=True: matrices are fit_homography's; the full 3 x 3 products are chained and inverted, every P_t, mean and A_t
    divided by its [2][2] entry, and Pbar_t is the mean of the eight normalised entries (the ninth is 1); warp_frames wants the
    result with projective=True.  A path whose [2][2] entry reaches 0 gives non-finite matrices, which warp_frames covers
    nothing with."""
    if not isinstance(projective, (bool, np.bool_)):
        raise TypeError(f"projective: expected a bool, got {projective!r}")
    if isinstance(matrices, torch.Tensor):
        matrices = matrices.detach().cpu().numpy()
    M = np.asarray(matrices, np.float64)
    if M.ndim != 3 or M.shape[1:] != (3, 3):
        raise ValueError(f"matrices: expected shape (T, 3, 3), got {M.shape}")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius < 0:
        raise ValueError(f"radius: expected a non-negative integer, got {radius!r}")
    T = M.shape[0]
    P = np.empty((T + 1, 3, 3), np.float64)
    P[0] = np.eye(3)
    for t in range(T):
        P[t + 1] = M[t] @ P[t]
        if projective:
            with np.errstate(all="ignore"):
                P[t + 1] = P[t + 1] / P[t + 1, 2, 2]
    A = np.empty_like(P)
    for t in range(T + 1):
        mean = P[max(0, t - radius):min(T, t + radius) + 1].mean(axis=0)
        if projective:
            try:
                with np.errstate(all="ignore"):
                    A[t] = P[t] @ np.linalg.inv(mean)
                    A[t] = A[t] / A[t, 2, 2]
            except np.linalg.LinAlgError:
                A[t] = np.nan
            continue
        mean[2] = (0.0, 0.0, 1.0)
        A[t] = P[t] @ np.linalg.inv(mean)
        A[t, 2] = (0.0, 0.0, 1.0)
    return A
