"""Frame interpolation on the HIP path: the frames between two frames, from the two flows between them (csrc/pwc_interp.hip).

    interpolate_frames(frames_0, frames_1, flows_fw, flows_bw, times, ...)   -> (frames_t (N,M,H,W,3), source (N,M,H,W) uint8)

Both frames are splatted forward to every time t asked for -- frame 0 along t * flows_fw, frame 1 along (1 - t) * flows_bw -- as
forward_splat(mode="average") does it, every source pixel weighted by how well its flow's match agrees with it (Niklaus & Liu's
softmax splatting with the photometric error as the metric: w = exp(-min(alpha * e, 10))), and the two arrivals are blended
(1 - t, t).  A target that too little of a frame reaches (its unweighted range below min_range) takes the other frame's arrival
alone; one that neither reaches is a hole and takes the cross-fade of the two co-located pixels.  `source` says which: 3 both,
1 frame 0 only, 2 frame 1 only, 0 a hole.  One memset, one scatter launch and one resolve launch per call whatever M is; the
weight of a source pixel is formed once for all M times.  The sums are 64-bit fixed point of 2^-36 steps, so two calls give the
same bits; the exact sequence of operations is in include/pwc_hip.h, "frame interpolation", and tests/interp_ref.py restates it
in numpy.  No autograd.

alpha = 20, the clamp at 10 and min_range = 0.5 are choices: nobody has tuned them on real video.
"""
import ctypes

import torch

from . import _lib
from .grad_ops import mask_ptr
from .modules import _p, _pixel_dense, as_view
from .unsup import _check_nhwc

MAX_TIMES = _lib.INTERP_MAX_TIMES
SOURCE_HOLE, SOURCE_FRAME_0, SOURCE_FRAME_1, SOURCE_BOTH = 0, 1, 2, 3


def _check_times(times):
    if isinstance(times, (int, float)) and not isinstance(times, bool):
        times = [times]
    try:
        times = [float(t) for t in times]
    except (TypeError, ValueError):
        raise TypeError(f"times: expected a float or a sequence of floats, got {times!r}") from None
    if not 1 <= len(times) <= MAX_TIMES:
        raise ValueError(f"times: expected 1 to {MAX_TIMES} times, got {len(times)}")
    for t in times:
        if not 0.0 <= t <= 1.0:
            raise ValueError(f"times: expected times in [0, 1], got {t!r}")
    return times


def _check_frames(frames_0, frames_1, N, H, W):
    for what, f in (("frames_0", frames_0), ("frames_1", frames_1)):
        if not isinstance(f, torch.Tensor) or f.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"{what}: expected a torch.uint8 or torch.float32 tensor, got "
                            f"{f.dtype if isinstance(f, torch.Tensor) else type(f)}")
        if f.dim() != 4 or f.shape[3] != 3:
            raise ValueError(f"{what}: expected an (N,H,W,3) tensor, got shape {tuple(f.shape)}")
        if tuple(f.shape[:3]) != (N, H, W):
            raise ValueError(f"{what}: expected (N,H,W) {(N, H, W)}, the flows', got {tuple(f.shape[:3])}")
    if frames_0.dtype != frames_1.dtype:
        raise TypeError(f"frames_1: expected frames_0's dtype {frames_0.dtype}, got {frames_1.dtype}")


def _check_weights(w, what, N, H, W):
    if w is None:
        return
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32:
        raise TypeError(f"{what}: expected a torch.float32 tensor, got {w.dtype if isinstance(w, torch.Tensor) else type(w)}")
    if tuple(w.shape) != (N, H, W):
        raise ValueError(f"{what}: expected (N,H,W) {(N, H, W)}, the flows', got {tuple(w.shape)}")


def _check_mask(valid, what, N, H, W):
    """mask_ptr's type, shape and layout rules, named after the argument; the device comes later."""
    if valid is None:
        return
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what}: expected a torch.bool or torch.uint8 tensor, got "
                        f"{valid.dtype if isinstance(valid, torch.Tensor) else type(valid)}")
    if tuple(valid.shape) != (N, H, W):
        raise ValueError(f"{what}: expected shape {(N, H, W)}, the flows' (N, H, W), got {tuple(valid.shape)}")
    if not valid.is_contiguous():
        raise ValueError(f"{what}: the mask must be contiguous")


def _check_interp(frames_0, frames_1, flows_fw, flows_bw, times, alpha, min_range, valid_fw, valid_bw, weights_fw, weights_bw,
                  max_workspace_bytes):
    """Types, shapes and values of interpolate_frames' arguments, then the device, last of all.  Returns the list of times."""
    _check_nhwc(flows_fw, "flows_fw", (2,))
    _check_nhwc(flows_bw, "flows_bw", (2,))
    N, H, W, _ = flows_fw.shape
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows_fw: empty tensor, shape {tuple(flows_fw.shape)}")
    if tuple(flows_bw.shape) != tuple(flows_fw.shape):
        raise ValueError(f"flows_bw: expected shape {tuple(flows_fw.shape)}, flows_fw's, got {tuple(flows_bw.shape)}")
    _check_frames(frames_0, frames_1, N, H, W)
    times = _check_times(times)
    for what, v in (("alpha", alpha), ("min_range", min_range)):
        if not float(v) >= 0.0:
            raise ValueError(f"{what}: expected a non-negative number, got {v!r}")
    _check_mask(valid_fw, "valid_fw", N, H, W)
    _check_mask(valid_bw, "valid_bw", N, H, W)
    _check_weights(weights_fw, "weights_fw", N, H, W)
    _check_weights(weights_bw, "weights_bw", N, H, W)
    if isinstance(max_workspace_bytes, bool) or not isinstance(max_workspace_bytes, int) or max_workspace_bytes < 1:
        raise ValueError(f"max_workspace_bytes: expected a positive integer, got {max_workspace_bytes!r}")
    for what, t in dict(flows_fw=flows_fw, flows_bw=flows_bw, frames_0=frames_0, frames_1=frames_1, valid_fw=valid_fw,
                        valid_bw=valid_bw, weights_fw=weights_fw, weights_bw=weights_bw).items():
        if t is not None and (not t.is_cuda or t.device != flows_fw.device):
            raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only, all arguments on one device")
    return times


def workspace_bytes(N, M, H, W):
    """8 * (N * M * H * W * 10 + 1): the accumulators of one call (plain arithmetic, no library call)."""
    return 8 * (N * M * H * W * 10 + 1)


def plan_slices(N, M, H, W, max_workspace_bytes):
    """The pieces [(n0, n1, m0, m1)] a call is cut into so that each piece's workspace fits max_workspace_bytes: whole images
    along N while one image with all M times fits, else one image at a time cut along M.  ValueError where a single image-time
    does not fit."""
    if workspace_bytes(1, 1, H, W) > max_workspace_bytes:
        raise ValueError(f"max_workspace_bytes: one {H} x {W} image at one time needs {workspace_bytes(1, 1, H, W)} bytes of "
                         f"workspace, more than {max_workspace_bytes}")
    if workspace_bytes(1, M, H, W) <= max_workspace_bytes:
        step = max(n for n in range(1, N + 1) if workspace_bytes(n, M, H, W) <= max_workspace_bytes)
        return [(n0, min(n0 + step, N), 0, M) for n0 in range(0, N, step)]
    step = max(m for m in range(1, M + 1) if workspace_bytes(1, m, H, W) <= max_workspace_bytes)
    return [(n, n + 1, m0, min(m0 + step, M)) for n in range(N) for m0 in range(0, M, step)]


def _frame_view(f):
    """(address, channel stride, the tensor kept alive): float32 frames as as_view reads them, uint8 frames contiguous."""
    if f.dtype == torch.uint8:
        f = f.contiguous()
        return f.data_ptr(), 3, f
    v, f = as_view(f, "frames")
    return v.ptr, v.cs, f


def interpolate_frames(frames_0, frames_1, flows_fw, flows_bw, times, *, alpha=20.0, min_range=0.5, valid_fw=None, valid_bw=None,
                       weights_fw=None, weights_bw=None, max_workspace_bytes=1 << 30):
    """(frames_t (N,M,H,W,3) in the frames' dtype, source (N,M,H,W) torch.uint8): the frames at the M `times` between frames_0
    (t = 0) and frames_1 (t = 1) (pwc_interp_frames: a memset, one scatter launch, one resolve launch per piece).

    frames_0, frames_1: (N,H,W,3), both torch.uint8 (a byte v is v / 255) or both torch.float32 in [0, 1] (a channel slice of a
    wider buffer is read in place).  flows_fw: (N,H,W,2) float32, the flow 0 -> 1 in pixels; flows_bw: the flow 1 -> 0; channel
    slices of wider buffers are read in place, both are read detached.  times: a float or a sequence of 1 to 16 floats in
    [0, 1].  valid_fw, valid_bw: (N,H,W) torch.bool / torch.uint8 SOURCE masks (grad_ops.mask_ptr's format), None = all; a pixel
    whose flow fails flow_io.flow_valid's rule is skipped as well.

    Every source pixel p of frame 0 is sent to p + t * flows_fw[p], every source pixel of frame 1 to p + (1 - t) * flows_bw[p],
    bilinearly onto the four pixels around that point (each corner inside the frame on its own, forward_splat's rule), with the
    weight w = exp(-min(alpha * e, 10)): e is the mean over the channels of |own[p] - other(p + flow[p])|, the other frame
    sampled bilinearly (fb_valid's sample); where the flow points out of the other frame the match is unverified and w =
    exp(-10), the lowest weight -- such a pixel fills a place nothing else claims and yields to anything that has a match.
    weights_fw, weights_bw: (N,H,W) float32 replace that weight (a negative or non-finite one skips the pixel):
    torch.ones(...) is plain average splatting, a metric of the caller's own -- built from fb_valid, say -- goes the same way;
    keep them below 2^26, beyond it every output element is NaN (float32) or 0 (uint8) and every source code 0.
    Per target and direction, range = the sum of the bilinear weights alone (range_map's), covered iff range >= min_range and
    the weighted sum is positive, c = the weighted mean colour.  frames_t = (1 - t) c0 + t c1 where both cover (source 3), c0
    (1), c1 (2), and (1 - t) frames_0 + t frames_1 at the same pixel where neither does (0).  float32 frames are rounded once,
    uint8 is rint(255 v) clamped.

    The workspace is 80 bytes per output pixel.  Where that exceeds max_workspace_bytes the call is cut into slices along N, and
    where one image with all its times is still too large, along M (plan_slices); a single image-time that does not fit raises
    ValueError.  A time's sums never meet another's and an image's never another image's: the pieces give the whole call's
    bits.  alpha = 20, the clamp at 10 and min_range = 0.5 are choices nobody has tuned on real video.  No autograd."""
    times = _check_interp(frames_0, frames_1, flows_fw, flows_bw, times, alpha, min_range, valid_fw, valid_bw, weights_fw,
                          weights_bw, max_workspace_bytes)
    N, H, W, _ = flows_fw.shape
    M = len(times)
    dev = flows_fw.device
    pieces = plan_slices(N, M, H, W, max_workspace_bytes)
    for what, v in (("valid_fw", valid_fw), ("valid_bw", valid_bw)):
        if v is not None:
            mask_ptr(v, N, H, W, dev)
    fv, flows_fw = as_view(flows_fw.detach(), "flows_fw")
    bv, flows_bw = as_view(flows_bw.detach(), "flows_bw")
    p0, cs0, frames_0 = _frame_view(frames_0.detach())
    p1, cs1, frames_1 = _frame_view(frames_1.detach())
    weights_fw = None if weights_fw is None else weights_fw.detach().contiguous()
    weights_bw = None if weights_bw is None else weights_bw.detach().contiguous()
    u8 = frames_0.dtype == torch.uint8
    esize = 1 if u8 else 4
    dtype = _lib.INTERP_U8 if u8 else _lib.INTERP_F32
    frames_t = torch.empty((N, M, H, W, 3), dtype=frames_0.dtype, device=dev)
    source = torch.empty((N, M, H, W), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    ws = torch.empty((max(workspace_bytes(n1 - n0, m1 - m0, H, W) for n0, n1, m0, m1 in pieces) // 8,), dtype=torch.int64,
                     device=dev)
    hw = H * W

    def at(base, n0, unit):
        return None if base is None else _p(base + n0 * hw * unit)

    for n0, n1, m0, m1 in pieces:
        whole = m0 == 0 and m1 == M
        out = frames_t[n0:n1] if whole else torch.empty((n1 - n0, m1 - m0, H, W, 3), dtype=frames_0.dtype, device=dev)
        src = source[n0:n1] if whole else torch.empty((n1 - n0, m1 - m0, H, W), dtype=torch.uint8, device=dev)
        table = (ctypes.c_double * (m1 - m0))(*times[m0:m1])
        _lib.check(L.pwc_interp_frames(
            at(p0, n0, cs0 * esize), dtype, cs0, at(p1, n0, cs1 * esize), dtype, cs1, at(fv.ptr, n0, 4 * fv.cs), fv.cs,
            at(bv.ptr, n0, 4 * bv.cs), bv.cs, at(None if valid_fw is None else valid_fw.data_ptr(), n0, 1),
            at(None if valid_bw is None else valid_bw.data_ptr(), n0, 1),
            at(None if weights_fw is None else weights_fw.data_ptr(), n0, 4),
            at(None if weights_bw is None else weights_bw.data_ptr(), n0, 4), n1 - n0, H, W, table, m1 - m0, float(alpha),
            float(min_range), _p(ws.data_ptr()), 8 * ws.numel(), _p(out.data_ptr()), _p(src.data_ptr()), _lib.current_stream()),
            "interpolate frames")
        if not whole:
            frames_t[n0:n1, m0:m1] = out
            source[n0:n1, m0:m1] = src
    return frames_t, source
