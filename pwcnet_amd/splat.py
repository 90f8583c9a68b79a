"""Forward splatting on the HIP path: the pixels of a frame moved to where a flow sends them (csrc/pwc_splat.hip).

    forward_splat(x, flows, weights=None, valid=None, flow_scale=1.0, mode="sum" | "average")  -> (out (N,H,W,C), coverage (N,H,W))
    splat_grad(x, flows, g_out, g_cov, ...)                                                     -> (dx, dweights, dflows)
    range_map(flows, flow_scale=1.0, valid=None)                                                -> (N,H,W) float32
    range_valid(flows_fw, flows_bw, min_range=0.5, flow_scale=1.0)                              -> (mask_fw, mask_bw) torch.bool

Every other geometric op of the package gathers along the flow (WarpingLayer, the data terms, fb_valid); this one scatters.
Source pixel (y, x) has the target point (x + flow_scale * flows[..., 0], y + flow_scale * flows[..., 1]); it contributes iff its
mask passes and the point lies in (-1, W) x (-1, H) (a NaN or Inf flow contributes nothing); each of the four pixels around the
point that lies inside the frame receives (bilinear weight) * weight * x -- a point half a pixel outside still splats onto the
border, nothing is clamped (UFlow's compute_range_map, Niklaus & Liu's softmax splatting; include/pwc_hip.h, "forward
splatting").  Several sources share a target: the sums are 64-bit fixed point of 2^-36 steps, so the order in which the atomics
land cannot change a bit and a training step stays bit reproducible.  A contribution that is not finite or reaches 2^26 makes
every output element NaN (a flag, no fault).  The gradient is a gather.  No double backward.
"""
import torch

from . import _lib
from .grad_ops import mask_ptr
from .modules import _p, _pixel_dense, as_view
from .unsup import _check_gpu, _check_nhwc, _dflow_view

MODES = ("sum", "average")


def _check_mode(mode, what):
    if mode not in MODES:
        raise ValueError(f"{what}: mode must be 'sum' or 'average', got {mode!r}")
    return mode == "average"


def _check_splat(x, flows, weights, valid, what):
    """Types and shapes of a splat's arguments, then the device, last of all."""
    _check_nhwc(flows, "flows", (2,))
    N, H, W, _ = flows.shape
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows: empty tensor, shape {tuple(flows.shape)}")
    others = {}
    if x is not None:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise TypeError(f"x: expected a torch.float32 tensor, got {x.dtype if isinstance(x, torch.Tensor) else type(x)}")
        if x.dim() != 4 or not 1 <= x.shape[3] <= 64:
            raise ValueError(f"x: expected an NHWC tensor with 1 to 64 channels, got shape {tuple(x.shape)}")
        if tuple(x.shape[:3]) != (N, H, W):
            raise ValueError(f"x: expected (N,H,W) {(N, H, W)}, the flows', got {tuple(x.shape[:3])}")
        others["x"] = x
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
            raise TypeError(f"weights: expected a torch.float32 tensor, got "
                            f"{weights.dtype if isinstance(weights, torch.Tensor) else type(weights)}")
        if tuple(weights.shape) != (N, H, W):
            raise ValueError(f"weights: expected (N,H,W) {(N, H, W)}, the flows', got {tuple(weights.shape)}")
        others["weights"] = weights
    if valid is not None:
        mask_ptr(valid, N, H, W, flows.device)
    _check_gpu(flows, **others)


def _splat_forward(x, flows, weights, valid, flow_scale, normalize):
    """The launch: (out or None, coverage, workspace).  The workspace holds the accumulators; the average mode's gradient reads it."""
    N, H, W, _ = flows.shape
    dev = flows.device
    vp = None if valid is None else mask_ptr(valid, N, H, W, dev)
    fv, flows = as_view(flows, "flows")
    xv = None
    if x is not None:
        xv, x = as_view(x, "x")
    if weights is not None:
        weights = weights.contiguous()
    C = 0 if xv is None else xv.C
    L = _lib.lib()
    ws = torch.empty((L.pwc_splat_workspace_bytes(N, H, W, C) // 8,), dtype=torch.int64, device=dev)
    out = None if xv is None else torch.empty((N, H, W, C), dtype=torch.float32, device=dev)
    cov = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    _lib.check(L.pwc_splat_f32(_p(xv.ptr) if xv is not None else None, xv.cs if xv is not None else 0, _p(fv.ptr), fv.cs,
                               float(flow_scale), _p(weights.data_ptr()) if weights is not None else None, vp, N, H, W, C,
                               1 if normalize else 0, _p(ws.data_ptr()), 8 * ws.numel(),
                               _p(out.data_ptr()) if out is not None else None, C, _p(cov.data_ptr()), _lib.current_stream()),
               "splat")
    return out, cov, ws, (x, flows, weights)


def _dense_like(t, shape, dev, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{what}: expected a torch.float32 tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t)}")
    if tuple(t.shape) != tuple(shape) or t.device != dev:
        raise ValueError(f"{what}: expected shape {tuple(shape)} on {dev}, got {tuple(t.shape)} on {t.device}")
    return t


def splat_grad(x, flows, g_out=None, g_cov=None, weights=None, valid=None, flow_scale=1.0, mode="sum", dx=None, dweights=None,
               dflows=None, accumulate=False, need=(True, True, True), _workspace=None):
    """(dx, dweights, dflows) (+)= the gradient of (g_out * out).sum() + (g_cov * coverage).sum() of forward_splat(x, flows,
    weights, valid, flow_scale, mode) w.r.t. x, weights and flows (pwc_splat_grad_f32: a gather, one launch).  g_out: (N,H,W,C),
    g_cov: (N,H,W), either may be None (zeros).  d* None: new tensors; accumulate: added onto them, pixels that do not contribute
    are left alone (without it they get exact zeros).  need: which of the three are computed (the others come back None);
    x None (a range map) has no dx, weights None gives dweights with respect to a weight of 1.  mode "average" needs the
    forward's accumulators: the forward is run again here unless the autograd function hands its own over.  What the autograd
    backward of forward_splat calls."""
    normalize = _check_mode(mode, "splat_grad")
    _check_splat(x, flows, weights, valid, "splat_grad")
    N, H, W, _ = flows.shape
    dev = flows.device
    C = 0 if x is None else x.shape[3]
    need_dx, need_dw, need_df = (bool(n) for n in need)
    need_dx = need_dx and C > 0
    if not (need_dx or need_dw or need_df):
        return None, None, None
    flows = flows.detach()
    x = None if x is None else x.detach()
    weights = None if weights is None else weights.detach()
    if normalize and _workspace is None:
        _workspace = _splat_forward(x, flows, weights, valid, flow_scale, True)[2]
    vp = None if valid is None else mask_ptr(valid, N, H, W, dev)
    fv, flows = as_view(flows, "flows")
    xv = gv = None
    if x is not None:
        xv, x = as_view(x, "x")
    if weights is not None:
        weights = weights.contiguous()
    if g_out is not None and C > 0:
        gv, g_out = as_view(_dense_like(g_out, (N, H, W, C), dev, "g_out"), "g_out")
    if g_cov is not None:
        g_cov = _dense_like(g_cov, (N, H, W), dev, "g_cov").contiguous()
    dxv = dfv = None
    if need_dx:
        if dx is None:
            dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dev)
        _dense_like(dx, (N, H, W, C), dev, "dx")
        if not _pixel_dense(dx):
            raise ValueError(f"dx: expected a pixel-dense tensor, got strides {dx.stride()}")
        dxv = as_view(dx, "dx")[0]
    else:
        dx = None
    if need_dw:
        if dweights is None:
            dweights = torch.empty((N, H, W), dtype=torch.float32, device=dev)
        _dense_like(dweights, (N, H, W), dev, "dweights")
        if not dweights.is_contiguous():
            raise ValueError("dweights: the tensor must be contiguous")
    else:
        dweights = None
    if need_df:
        dfv, dflows = _dflow_view(dflows, fv, dev)
    else:
        dflows = None
    _lib.check(_lib.lib().pwc_splat_grad_f32(
        _p(xv.ptr) if xv is not None else None, xv.cs if xv is not None else 0, _p(fv.ptr), fv.cs, float(flow_scale),
        _p(weights.data_ptr()) if weights is not None else None, vp, N, H, W, C, 1 if normalize else 0,
        _p(gv.ptr) if gv is not None else None, gv.cs if gv is not None else 0,
        _p(g_cov.data_ptr()) if g_cov is not None else None,
        _p(_workspace.data_ptr()) if normalize else None, 8 * _workspace.numel() if normalize else 0,
        _p(dxv.ptr) if dxv is not None else None, dxv.cs if dxv is not None else 0,
        _p(dweights.data_ptr()) if dweights is not None else None,
        _p(dfv.ptr) if dfv is not None else None, dfv.cs if dfv is not None else 0, 1 if accumulate else 0,
        _lib.current_stream()), "splat grad")
    return dx, dweights, dflows


class _ForwardSplat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flows, weights, valid, flow_scale, normalize):
        ctx.set_materialize_grads(False)
        out, cov, ws, (x, flows, weights) = _splat_forward(x, flows, weights, valid, flow_scale, normalize)
        ctx.has = (x is not None, weights is not None)
        ctx.save_for_backward(*[t for t in (x, flows, weights) if t is not None], *([ws] if normalize else []))
        ctx.valid, ctx.consts = valid, (flow_scale, normalize)
        if out is None:
            out = cov.new_empty((0,))
            ctx.mark_non_differentiable(out)
        return out, cov

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_cov):
        need = tuple(ctx.needs_input_grad[:3])
        if (g_out is None and g_cov is None) or not any(need):
            return (None,) * 6
        flow_scale, normalize = ctx.consts
        saved = list(ctx.saved_tensors)
        x = saved.pop(0) if ctx.has[0] else None
        flows = saved.pop(0)
        weights = saved.pop(0) if ctx.has[1] else None
        ws = saved.pop(0) if normalize else None
        dx, dw, df = splat_grad(x, flows, g_out if x is not None else None, g_cov, weights, ctx.valid, flow_scale,
                                "average" if normalize else "sum", need=(need[0], need[2], need[1]), _workspace=ws)
        return dx, df, dw, None, None, None


def forward_splat(x, flows, weights=None, valid=None, flow_scale=1.0, mode="sum"):
    """(out (N,H,W,C) float32, coverage (N,H,W) float32): x splatted along flow_scale * flows.
    x: (N,H,W,C), C = 1..64 (a channel slice of a wider buffer is read in place); flows: (N,H,W,2); weights: (N,H,W) float32, the
    weight of each SOURCE pixel, None = 1; valid: (N,H,W) torch.bool / torch.uint8 source mask (grad_ops.mask_ptr's format), None =
    all.  Source pixel p contributes iff valid[p] and its target point (x + flow_scale * u, y + flow_scale * v) lies in
    (-1, W) x (-1, H); each of the four pixels around the point that is inside the frame receives b * weights[p] * x[p], b its
    bilinear weight -- every corner on its own, nothing is clamped, a NaN or Inf flow contributes nothing.
        mode "sum":      out[t] = the sum of b * weights * x over what reaches t  (summation splatting),
        mode "average":  that sum divided by coverage[t] where coverage[t] > 0, else 0,
        coverage[t]      = the sum of b * weights: the splatted weights, in either mode.
    Softmax splatting (Niklaus & Liu) is forward_splat(x, flows, weights=torch.exp(alpha * z), mode="average"); keep alpha * z
    below about 17, a contribution of 2^26 or more is out of the fixed point's range.  Forward warping of a frame (or of a flow: x =
    flows) to time t is flow_scale=t.
    Differentiable with respect to x, weights and flows (pwc_splat_grad_f32, a gather); the mask is a constant.  The sums are
    64-bit fixed point of 2^-36 steps: two calls give the same bits, a contribution below 2^-37 vanishes, and a contribution that
    is not finite or reaches 2^26 makes every element of out and coverage NaN."""
    normalize = _check_mode(mode, "forward_splat")
    if x is None:
        raise TypeError("forward_splat: x is None; range_map(flows) is the splat without a frame")
    _check_splat(x, flows, weights, valid, "forward_splat")
    return _ForwardSplat.apply(x, flows, weights, valid, float(flow_scale), normalize)


def range_map(flows, flow_scale=1.0, valid=None):
    """(N,H,W) float32: how many pixels land on each pixel under flow_scale * flows, bilinearly -- the coverage of a splat with no
    frame and weights 1 (Wang et al. 2018, UFlow's compute_range_map).  range_map(flows_bw) is, per pixel of frame 0, how much of
    frame 1 arrives there: about 1 where the pixel is visible in frame 1, 0 where it is occluded.  Differentiable with respect to
    flows; valid masks the SOURCE pixels."""
    _check_splat(None, flows, None, valid, "range_map")
    return _ForwardSplat.apply(None, flows, None, valid, float(flow_scale), False)[1]


def range_valid(flows_fw, flows_bw, min_range=0.5, flow_scale=1.0):
    """(mask_fw, mask_bw), torch.bool (N,H,W), contiguous -- they go straight into `valid=` of the data terms, as fb_valid's do.
        mask_fw = range_map(flows_bw) >= min_range    the frame-0 pixels that something of frame 1 lands on,
        mask_bw = range_map(flows_fw) >= min_range.
    Both are constants (computed under no_grad).  Unlike fb_valid's check this does not confuse "occluded" with "the flow is still
    wrong": a poor flow still covers most of the frame.  The data terms take boolean masks, hence a threshold and not Wang et
    al.'s soft weight 1 - clip(range, 0, 1).  min_range = 0.5 is a choice: nobody has trained with it yet.  A NaN range (the
    poison flag) gives False."""
    min_range = float(min_range)
    if not min_range >= 0.0:
        raise ValueError(f"range_valid: min_range must be non-negative, got {min_range}")
    _check_nhwc(flows_fw, "flows_fw", (2,))
    _check_nhwc(flows_bw, "flows_bw", (2,))
    if tuple(flows_bw.shape) != tuple(flows_fw.shape):
        raise ValueError(f"flows_bw: expected (N,H,W) {tuple(flows_fw.shape[:3])}, flows_fw's, got {tuple(flows_bw.shape[:3])}")
    _check_splat(None, flows_fw, None, None, "range_valid")
    _check_gpu(flows_fw, flows_bw=flows_bw)
    with torch.no_grad():
        mask_fw = range_map(flows_bw.detach(), flow_scale) >= min_range
        mask_bw = range_map(flows_fw.detach(), flow_scale) >= min_range
    return mask_fw, mask_bw
