"""Losses that need no ground-truth flow, on the HIP path: the photometric warp term and the edge-aware smoothness term.

    photometric_sums(images_0, images_1, flows, ...)  -> (sums (N,), counts (N,) int32)
    photometric_loss(...)                              -> sums.sum() / (C * counts.sum().clamp(min=1))
    smoothness_sums(flows, images=None, ...)           -> sums (N,)
    smoothness_loss(...)                               -> sums.sum() / (N * H * W)

    census_sums(images_0, images_1, flows, ...)        -> (sums (N,), counts (N,) int32)
    census_loss(...)                                    -> sums.sum() / counts.sum().clamp(min=1)

    ssim_sums(images_0, images_1, flows, ...)          -> (sums (N,), counts (N,) int32)
    ssim_loss(...)                                      -> sums.sum() / (C * counts.sum().clamp(min=1))

    fb_valid(flows_fw, flows_bw, ...)                   -> (mask_fw, mask_bw) torch.bool (N,H,W) [, counts_fw, counts_bw int32 (N,)]
    fb_consistency_sums(flows_fw, flows_bw, ...)        -> (sums_fw, counts_fw, sums_bw, counts_bw)
    fb_consistency_loss(...)                            -> (sums_fw.sum() + sums_bw.sum()) / (2 * (counts_fw.sum() + counts_bw.sum()).clamp(min=1))

    flow_distill_sums(student, teacher, offset, ...)    -> (sums (N,), counts (N,) int32)
    flow_distill_loss(...)                              -> sums.sum() / (2 * counts.sum().clamp(min=1))

With rho(d) = (d^2 + eps^2)^q: the photometric term of a pixel is sum_c rho(images_0 - bilinear sample of images_1 at the pixel
moved by flow_scale * flow), over the pixels that are valid (`valid`, grad_ops.mask_ptr's format, e.g. an occlusion mask of the
caller's) and whose sample point lies inside the frame; the smoothness term is the sum of exp(-alpha * mean_c |d image|) *
rho(d flow) over the forward differences along x and y (include/pwc_hip.h, "self-supervised losses").
`sums` is differentiable with respect to `flows` (pwc_photometric_grad_f32 / pwc_flow_smoothness_grad_f32: gathers, bit
reproducible), so the losses compose with PWCDCNetModule; the images are constants -- an image that requires grad is refused.
The census term compares the local intensity ORDER in a (2 radius + 1)^2 window of the grey images instead of the intensities
(csrc/pwc_census.hip; the formulas are in census_sums' docstring), so a brightness change between the frames does not pull the flow.
The SSIM term is (1 - SSIM) / 2 of images_0 and the warped images_1 in the same windows, per channel (csrc/pwc_ssim.hip; ssim_sums'
docstring): the data term of UFlow / ARFlow, 0.15 * photometric_loss(q=0.5) + 0.85 * ssim_loss.
No double backward.
fb_valid makes the occlusion masks that go into `valid`: the forward-backward consistency check of two flows (csrc/pwc_fbcheck.hip;
the definition is in its docstring).  It is not differentiable: the masks are constants.
smoothness_*(order=2) penalises the SECOND difference of the flow (a constant slope is free), and fb_consistency_* is UnFlow's
third term: rho of f + g, the quantity fb_valid thresholds, at the pixels the masks keep, differentiable with respect to BOTH
flows (the gradient with respect to the sampled flow is a scatter, added in 64-bit fixed point: bit reproducible).
flow_distill_* is the self-supervision term: rho of a student flow minus a teacher flow of the same direction, the teacher a
wider field read in place through a window (csrc/pwc_distill.hip), differentiable with respect to the student only.
"""
import torch

from . import _lib
from .grad_ops import mask_ptr
from .modules import _p, _pixel_dense, as_view


def _check_rho(eps, q, what):
    eps, q = float(eps), float(q)
    if not eps > 0.0:
        raise ValueError(f"{what}: eps must be positive, got {eps}")
    if not 0.0 < q <= 1.0:
        raise ValueError(f"{what}: q must be in (0, 1], got {q}")
    return eps, q


def _check_nhwc(t, what, channels):
    """dtype (TypeError) and shape (ValueError) of an NHWC float32 argument -- mask_ptr's exception types.  The device is checked
    last of all (_check_gpu), so that every other fault of a call is reported whatever machine it is made on."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{what}: expected a torch.float32 tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t)}")
    if t.dim() != 4 or t.shape[3] not in channels:
        raise ValueError(f"{what}: expected an NHWC tensor with {' or '.join(str(c) for c in channels)} channels, "
                         f"got shape {tuple(t.shape)}")


def _check_image(t, what, like):
    _check_nhwc(t, what, (1, 2, 3, 4))
    if tuple(t.shape[:3]) != tuple(like.shape[:3]):
        raise ValueError(f"{what}: expected (N,H,W) {tuple(like.shape[:3])}, the flows', got {tuple(t.shape[:3])}")
    if t.requires_grad:
        raise ValueError(f"{what}: gradients with respect to the images are not implemented (the image requires grad); "
                         "detach it")


def _check_gpu(flows, **others):
    for what, t in dict(flows=flows, **others).items():
        if not t.is_cuda or t.device != flows.device:
            raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only, all arguments on one device")


def _dflow_view(dflow, fv, dev):
    """The gradient's destination: a new dense tensor, or the caller's (N,H,W,2) tensor / channel slice of a wider buffer."""
    if dflow is None:
        dflow = torch.empty((fv.N, fv.H, fv.W, 2), dtype=torch.float32, device=dev)
    _check_nhwc(dflow, "dflow", (2,))
    _check_gpu(dflow)
    if tuple(dflow.shape) != (fv.N, fv.H, fv.W, 2) or dflow.device != dev or not _pixel_dense(dflow):
        raise ValueError(f"dflow: expected a pixel-dense {(fv.N, fv.H, fv.W, 2)} tensor on {dev}, got {tuple(dflow.shape)} "
                         f"strides {dflow.stride()} on {dflow.device}")
    return as_view(dflow, "dflow")[0], dflow


def photometric_grad(images_0, images_1, flows, dsums, dflow=None, flow_scale=1.0, valid=None, eps=1e-3, q=0.5,
                     accumulate=False):
    """dflow (+)= the gradient of (dsums * photometric_sums(...)[0]).sum() w.r.t. flows (pwc_photometric_grad_f32); dsums:
    (N,) on the GPU.  dflow None: a new tensor; accumulate: added onto dflow, pixels that do not contribute are left alone
    (without it they get 0).  Returns dflow.  What the autograd backward of photometric_sums calls."""
    vp = None if valid is None else mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
    fv, flows = as_view(flows, "flows")
    v0, images_0 = as_view(images_0, "images_0")
    v1, images_1 = as_view(images_1, "images_1")
    up = torch.empty((fv.N,), dtype=torch.float32, device=flows.device).copy_(dsums)       # contiguous float32, its own
    dv, dflow = _dflow_view(dflow, fv, flows.device)
    _lib.check(_lib.lib().pwc_photometric_grad_f32(_p(v0.ptr), v0.cs, _p(v1.ptr), v1.cs, _p(fv.ptr), fv.cs, float(flow_scale),
                                                   vp, fv.N, fv.H, fv.W, v0.C, float(eps), float(q), _p(up.data_ptr()),
                                                   _p(dv.ptr), dv.cs, 1 if accumulate else 0, _lib.current_stream()),
               "photometric grad")
    return dflow


def _check_order(order, what):
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"{what}: order must be 1 or 2, got {order!r}")
    return int(order)


def smoothness_grad(flows, dsums, dflow=None, images=None, alpha=10.0, eps=1e-3, q=0.5, accumulate=False, order=1):
    """dflow (+)= the gradient of (dsums * smoothness_sums(...)).sum() w.r.t. flows (pwc_flow_smoothness_grad_f32, order 2:
    pwc_flow_smoothness2_grad_f32)."""
    order = _check_order(order, "smoothness_grad")
    fv, flows = as_view(flows, "flows")
    iv = None
    if images is not None:
        iv, images = as_view(images, "images")
    up = torch.empty((fv.N,), dtype=torch.float32, device=flows.device).copy_(dsums)
    dv, dflow = _dflow_view(dflow, fv, flows.device)
    L = _lib.lib()
    entry = L.pwc_flow_smoothness_grad_f32 if order == 1 else L.pwc_flow_smoothness2_grad_f32
    _lib.check(entry(_p(fv.ptr), fv.cs, _p(iv.ptr) if iv is not None else None, iv.cs if iv is not None else 0,
                     iv.C if iv is not None else 0, float(alpha), float(eps), float(q), fv.N, fv.H, fv.W, _p(up.data_ptr()),
                     _p(dv.ptr), dv.cs, 1 if accumulate else 0, _lib.current_stream()), "flow smoothness grad")
    return dflow


def _check_census(radius, scale, c1, c2, eps, q, what):
    eps, q = _check_rho(eps, q, what)
    if isinstance(radius, bool) or not isinstance(radius, int) or radius not in (1, 2, 3):
        raise ValueError(f"{what}: radius must be 1, 2 or 3, got {radius!r}")
    scale, c1, c2 = float(scale), float(c1), float(c2)
    for name, v in (("scale", scale), ("c1", c1), ("c2", c2)):
        if not v > 0.0:
            raise ValueError(f"{what}: {name} must be positive, got {v}")
    return radius, scale, c1, c2, eps, q


def _check_census_tensors(images_0, images_1, flows, valid):
    _check_nhwc(flows, "flows", (2,))
    _check_image(images_0, "images_0", flows)
    _check_image(images_1, "images_1", flows)
    if images_0.shape[3] != images_1.shape[3]:
        raise ValueError(f"images_0 has {images_0.shape[3]} channels, images_1 {images_1.shape[3]}")
    if valid is not None:
        mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
    _check_gpu(flows, images_0=images_0, images_1=images_1)


def census_grad(images_0, images_1, flows, dsums, dflow=None, flow_scale=1.0, valid=None, radius=3, scale=255.0, c1=0.81,
                c2=0.1, eps=1e-2, q=0.4, accumulate=False):
    """dflow (+)= the gradient of (dsums * census_sums(...)[0]).sum() w.r.t. flows (pwc_census_grad_f32); dsums: (N,) on the
    GPU.  dflow None: a new tensor; accumulate: added onto dflow, out-of-frame pixels are left alone (without it they get 0).
    Returns dflow.  What the autograd backward of census_sums calls."""
    radius, scale, c1, c2, eps, q = _check_census(radius, scale, c1, c2, eps, q, "census_grad")
    _check_census_tensors(images_0, images_1, flows, valid)
    vp = None if valid is None else mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
    fv, flows = as_view(flows, "flows")
    v0, images_0 = as_view(images_0, "images_0")
    v1, images_1 = as_view(images_1, "images_1")
    L = _lib.lib()
    up = torch.empty((fv.N,), dtype=torch.float32, device=flows.device).copy_(dsums)       # contiguous float32, its own
    dv, dflow = _dflow_view(dflow, fv, flows.device)
    ws = torch.empty((max(L.pwc_census_workspace_floats(fv.N, fv.H, fv.W, 1), 1),), dtype=torch.float32, device=flows.device)
    _lib.check(L.pwc_census_grad_f32(_p(v0.ptr), v0.cs, _p(v1.ptr), v1.cs, _p(fv.ptr), fv.cs, float(flow_scale), vp, fv.N, fv.H,
                                     fv.W, v0.C, radius, scale, c1, c2, eps, q, _p(up.data_ptr()), _p(ws.data_ptr()), ws.numel(),
                                     _p(dv.ptr), dv.cs, 1 if accumulate else 0, _lib.current_stream()), "census grad")
    return dflow


class _CensusSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, images_0, images_1, flow_scale, valid, consts):
        ctx.set_materialize_grads(False)
        radius, scale, c1, c2, eps, q = consts
        vp = None if valid is None else mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
        fv, flows = as_view(flows, "flows")
        v0, images_0 = as_view(images_0, "images_0")
        v1, images_1 = as_view(images_1, "images_1")
        L = _lib.lib()
        dev = flows.device
        sums = torch.empty((fv.N,), dtype=torch.float32, device=dev)
        counts = torch.empty((fv.N,), dtype=torch.int32, device=dev)
        ws = torch.empty((max(L.pwc_census_workspace_floats(fv.N, fv.H, fv.W, 0), 1),), dtype=torch.float32, device=dev)
        _lib.check(L.pwc_census_sums_f32(_p(v0.ptr), v0.cs, _p(v1.ptr), v1.cs, _p(fv.ptr), fv.cs, flow_scale, vp, fv.N, fv.H,
                                         fv.W, v0.C, radius, scale, c1, c2, eps, q, _p(ws.data_ptr()), ws.numel(),
                                         _p(sums.data_ptr()), _p(counts.data_ptr()), _lib.current_stream()), "census sums")
        ctx.save_for_backward(flows, images_0, images_1)
        ctx.valid, ctx.consts = valid, (flow_scale,) + tuple(consts)
        ctx.mark_non_differentiable(counts)
        return sums, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsums, _dcounts):
        if dsums is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        flows, images_0, images_1 = ctx.saved_tensors
        flow_scale, radius, scale, c1, c2, eps, q = ctx.consts
        dflow = census_grad(images_0, images_1, flows, dsums, None, flow_scale, ctx.valid, radius, scale, c1, c2, eps, q)
        return dflow, None, None, None, None, None


def _check_ssim(radius, c1, c2, what):
    if isinstance(radius, bool) or not isinstance(radius, int) or radius not in (1, 2, 3):
        raise ValueError(f"{what}: radius must be 1, 2 or 3, got {radius!r}")
    c1, c2 = float(c1), float(c2)
    for name, v in (("c1", c1), ("c2", c2)):
        if not v > 0.0:
            raise ValueError(f"{what}: {name} must be positive, got {v}")
    return radius, c1, c2


def ssim_grad(images_0, images_1, flows, dsums, dflow=None, flow_scale=1.0, valid=None, radius=1, c1=1e-4, c2=9e-4,
              accumulate=False):
    """dflow (+)= the gradient of (dsums * ssim_sums(...)[0]).sum() w.r.t. flows (pwc_ssim_grad_f32); dsums: (N,) on the GPU.
    dflow None: a new tensor; accumulate: added onto dflow, pixels that are out of frame or have no contributing centre within
    `radius` are left alone (without it they get 0).  Returns dflow.  What the autograd backward of ssim_sums calls."""
    radius, c1, c2 = _check_ssim(radius, c1, c2, "ssim_grad")
    _check_census_tensors(images_0, images_1, flows, valid)
    vp = None if valid is None else mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
    fv, flows = as_view(flows, "flows")
    v0, images_0 = as_view(images_0, "images_0")
    v1, images_1 = as_view(images_1, "images_1")
    L = _lib.lib()
    up = torch.empty((fv.N,), dtype=torch.float32, device=flows.device).copy_(dsums)       # contiguous float32, its own
    dv, dflow = _dflow_view(dflow, fv, flows.device)
    ws = torch.empty((max(L.pwc_ssim_workspace_floats(fv.N, fv.H, fv.W, v0.C, 1), 1),), dtype=torch.float32, device=flows.device)
    _lib.check(L.pwc_ssim_grad_f32(_p(v0.ptr), v0.cs, _p(v1.ptr), v1.cs, _p(fv.ptr), fv.cs, float(flow_scale), vp, fv.N, fv.H,
                                   fv.W, v0.C, radius, c1, c2, _p(up.data_ptr()), _p(ws.data_ptr()), ws.numel(), _p(dv.ptr), dv.cs,
                                   1 if accumulate else 0, _lib.current_stream()), "ssim grad")
    return dflow


class _SsimSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, images_0, images_1, flow_scale, valid, consts):
        ctx.set_materialize_grads(False)
        radius, c1, c2 = consts
        vp = None if valid is None else mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
        fv, flows = as_view(flows, "flows")
        v0, images_0 = as_view(images_0, "images_0")
        v1, images_1 = as_view(images_1, "images_1")
        L = _lib.lib()
        dev = flows.device
        sums = torch.empty((fv.N,), dtype=torch.float32, device=dev)
        counts = torch.empty((fv.N,), dtype=torch.int32, device=dev)
        ws = torch.empty((max(L.pwc_ssim_workspace_floats(fv.N, fv.H, fv.W, v0.C, 0), 1),), dtype=torch.float32, device=dev)
        _lib.check(L.pwc_ssim_sums_f32(_p(v0.ptr), v0.cs, _p(v1.ptr), v1.cs, _p(fv.ptr), fv.cs, flow_scale, vp, fv.N, fv.H, fv.W,
                                       v0.C, radius, c1, c2, _p(ws.data_ptr()), ws.numel(), _p(sums.data_ptr()),
                                       _p(counts.data_ptr()), _lib.current_stream()), "ssim sums")
        ctx.save_for_backward(flows, images_0, images_1)
        ctx.valid, ctx.consts = valid, (flow_scale,) + tuple(consts)
        ctx.mark_non_differentiable(counts)
        return sums, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsums, _dcounts):
        if dsums is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        flows, images_0, images_1 = ctx.saved_tensors
        flow_scale, radius, c1, c2 = ctx.consts
        dflow = ssim_grad(images_0, images_1, flows, dsums, None, flow_scale, ctx.valid, radius, c1, c2)
        return dflow, None, None, None, None, None


class _PhotometricSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, images_0, images_1, flow_scale, valid, eps, q):
        ctx.set_materialize_grads(False)
        vp = None if valid is None else mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
        fv, flows = as_view(flows, "flows")
        v0, images_0 = as_view(images_0, "images_0")
        v1, images_1 = as_view(images_1, "images_1")
        L = _lib.lib()
        dev = flows.device
        sums = torch.empty((fv.N,), dtype=torch.float32, device=dev)
        counts = torch.empty((fv.N,), dtype=torch.int32, device=dev)
        ws = torch.empty((max(L.pwc_photometric_workspace_floats(fv.N, fv.H, fv.W), 1),), dtype=torch.float32, device=dev)
        _lib.check(L.pwc_photometric_sums_f32(_p(v0.ptr), v0.cs, _p(v1.ptr), v1.cs, _p(fv.ptr), fv.cs, flow_scale, vp,
                                              fv.N, fv.H, fv.W, v0.C, eps, q, _p(ws.data_ptr()), ws.numel(),
                                              _p(sums.data_ptr()), _p(counts.data_ptr()), _lib.current_stream()),
                   "photometric sums")
        ctx.save_for_backward(flows, images_0, images_1)
        ctx.valid, ctx.consts = valid, (flow_scale, eps, q)
        ctx.mark_non_differentiable(counts)
        return sums, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsums, _dcounts):
        if dsums is None or not ctx.needs_input_grad[0]:
            return (None,) * 7
        flows, images_0, images_1 = ctx.saved_tensors
        flow_scale, eps, q = ctx.consts
        dflow = photometric_grad(images_0, images_1, flows, dsums, None, flow_scale, ctx.valid, eps, q)
        return dflow, None, None, None, None, None, None


class _SmoothnessSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows, images, alpha, eps, q, order=1):
        ctx.set_materialize_grads(False)
        fv, flows = as_view(flows, "flows")
        iv = None
        if images is not None:
            iv, images = as_view(images, "images")
        L = _lib.lib()
        dev = flows.device
        sums = torch.empty((fv.N,), dtype=torch.float32, device=dev)
        ws = torch.empty((max(L.pwc_flow_smoothness_workspace_floats(fv.N, fv.H, fv.W), 1),), dtype=torch.float32, device=dev)
        entry = L.pwc_flow_smoothness_sums_f32 if order == 1 else L.pwc_flow_smoothness2_sums_f32
        _lib.check(entry(_p(fv.ptr), fv.cs, _p(iv.ptr) if iv is not None else None, iv.cs if iv is not None else 0,
                         iv.C if iv is not None else 0, alpha, eps, q, fv.N, fv.H, fv.W, _p(ws.data_ptr()), ws.numel(),
                         _p(sums.data_ptr()), _lib.current_stream()), "flow smoothness sums")
        if images is None:
            ctx.save_for_backward(flows)
        else:
            ctx.save_for_backward(flows, images)
        ctx.consts = (alpha, eps, q, order)
        return sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsums):
        if dsums is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        flows, *images = ctx.saved_tensors
        alpha, eps, q, order = ctx.consts
        dflow = smoothness_grad(flows, dsums, None, images[0] if images else None, alpha, eps, q, order=order)
        return dflow, None, None, None, None, None


def photometric_sums(images_0, images_1, flows, flow_scale=1.0, valid=None, eps=1e-3, q=0.5):
    """(sums (N,) float32, counts (N,) int32): per image, the sum over the contributing pixels of sum_c rho(images_0 -
    images_1 sampled at the pixel moved by flow_scale * flows), rho(d) = (d^2 + eps^2)^q, and the number of contributing
    pixels -- valid ones (valid: (N,H,W) torch.bool / torch.uint8, None = all) whose sample point is inside the frame.
    images: (N,H,W,C), C = 1..4, at the flows' resolution; flows: (N,H,W,2).  flow_scale: 20 / 2^level takes the pyramid
    flows (px / 20 at the level's size) with images the caller has downsampled.  sums is differentiable w.r.t. flows."""
    eps, q = _check_rho(eps, q, "photometric_sums")
    _check_nhwc(flows, "flows", (2,))
    _check_image(images_0, "images_0", flows)
    _check_image(images_1, "images_1", flows)
    if images_0.shape[3] != images_1.shape[3]:
        raise ValueError(f"images_0 has {images_0.shape[3]} channels, images_1 {images_1.shape[3]}")
    if valid is not None:
        mask_ptr(valid, flows.shape[0], flows.shape[1], flows.shape[2], flows.device)
    _check_gpu(flows, images_0=images_0, images_1=images_1)
    return _PhotometricSums.apply(flows, images_0, images_1, float(flow_scale), valid, eps, q)


def photometric_loss(images_0, images_1, flows, flow_scale=1.0, valid=None, eps=1e-3, q=0.5):
    """0-dim: the mean of rho over the contributing pixels and the channels; 0 when no pixel contributes."""
    sums, counts = photometric_sums(images_0, images_1, flows, flow_scale, valid, eps, q)
    return sums.sum() / (images_0.shape[3] * counts.sum().clamp(min=1)).to(torch.float32)


def smoothness_sums(flows, images=None, alpha=10.0, eps=1e-3, q=0.5, order=1):
    """sums (N,) float32: per image, sum over x < W - 1 of exp(-alpha * mean_c |images[y,x+1] - images[y,x]|) * sum_k
    rho(flows[y,x+1,k] - flows[y,x,k]) plus the same along y.  images: (N,H,W,C), C = 1..4, at the flows' resolution, a
    constant; None: every weight is 1.  Differentiable w.r.t. flows.
    order=2 (UnFlow's second-order smoothness): sum over the centres 1 <= x <= W - 2 of exp(-alpha * mean_c |images[y,x+1] -
    images[y,x-1]|) * sum_k rho(flows[y,x-1,k] - 2 flows[y,x,k] + flows[y,x+1,k]) plus the same along y -- a constant slope of
    the flow is free.  W < 3 gives no x terms, H < 3 no y terms (both: 0).  Any other order: ValueError."""
    eps, q = _check_rho(eps, q, "smoothness_sums")
    order = _check_order(order, "smoothness_sums")
    alpha = float(alpha)
    if not alpha >= 0.0:
        raise ValueError(f"smoothness_sums: alpha must be non-negative, got {alpha}")
    _check_nhwc(flows, "flows", (2,))
    if images is not None:
        _check_image(images, "images", flows)
        _check_gpu(flows, images=images)
    _check_gpu(flows)
    return _SmoothnessSums.apply(flows, images, alpha, eps, q, order)


def smoothness_loss(flows, images=None, alpha=10.0, eps=1e-3, q=0.5, order=1):
    """0-dim: smoothness_sums(...).sum() / (N * H * W), for both orders."""
    sums = smoothness_sums(flows, images, alpha, eps, q, order)
    return sums.sum() / float(flows.shape[0] * flows.shape[1] * flows.shape[2])


def census_sums(images_0, images_1, flows, flow_scale=1.0, valid=None, radius=3, scale=255.0, c1=0.81, c2=0.1, eps=1e-2, q=0.4):
    """(sums (N,) float32, counts (N,) int32) of the soft census (ternary) term.  Grey planes a = scale * mean_c images_0 and
    b = scale * mean_c (images_1 sampled at the pixel moved by flow_scale * flows, photometric_sums' sample; 0 where the sample
    point is out of frame or the flow is not finite).  Over the K = (2 radius + 1)^2 - 1 offsets o != 0 of the window:
        t0 = a(p+o) - a(p),  t1 = b(p+o) - b(p),  tau(t) = t / sqrt(c1 + t^2),  d = (tau(t0) - tau(t1))^2,
        h(p) = (1/K) sum_o d / (c2 + d),
    sums[n] = the sum of rho(h(p)) = (h^2 + eps^2)^q over the contributing pixels, counts[n] their number.  A pixel contributes
    when it is at least `radius` pixels from every border (no padding), its sample point is inside the frame, and valid[p] is
    set (valid: (N,H,W) torch.bool / torch.uint8, None = all).  UNLIKE photometric_sums, `valid` and the in-frame test select
    CENTRES only: the neighbours in a contributing centre's window are always read, so the images must hold numbers at masked
    pixels too.  H <= 2 radius or W <= 2 radius: counts and sums are 0, no error.  images: (N,H,W,C), C = 1..4, in [0, 1] with
    the default scale (the constants are UnFlow's, for 0..255 grey values); radius: 1, 2 or 3.  sums is differentiable w.r.t.
    flows (pwc_census_grad_f32: a gather, bit reproducible); the images are constants."""
    consts = _check_census(radius, scale, c1, c2, eps, q, "census_sums")
    _check_census_tensors(images_0, images_1, flows, valid)
    return _CensusSums.apply(flows, images_0, images_1, float(flow_scale), valid, consts)


def census_loss(images_0, images_1, flows, flow_scale=1.0, valid=None, radius=3, scale=255.0, c1=0.81, c2=0.1, eps=1e-2, q=0.4):
    """0-dim: the mean of rho(h) over the contributing pixels; 0 when no pixel contributes."""
    sums, counts = census_sums(images_0, images_1, flows, flow_scale, valid, radius, scale, c1, c2, eps, q)
    return sums.sum() / counts.sum().clamp(min=1).to(torch.float32)


def ssim_sums(images_0, images_1, flows, flow_scale=1.0, valid=None, radius=1, c1=1e-4, c2=9e-4):
    """(sums (N,) float32, counts (N,) int32) of the SSIM term, the data term of UFlow / ARFlow.  x = images_0, y = images_1
    sampled at the pixel moved by flow_scale * flows (photometric_sums' sample and in-frame rule; a flow that is not finite is
    out of frame).  Per channel, over the n = (2 radius + 1)^2 pixels of the window of centre p, in double and centred:
        mu_x = mean x,  mu_y = mean y,  s_x = mean (x - mu_x)^2,  s_y = mean (y - mu_y)^2,  s_xy = mean (x - mu_x)(y - mu_y),
        SSIM = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_x + s_y + c2)),  term(p, c) = (1 - SSIM) / 2,
    no clamp, no eps and no q (the term is not passed through rho).  sums[n] = the sum of term(p, c) over the contributing
    centres and the channels, counts[n] the number of contributing centres.  A centre contributes when it is at least `radius`
    pixels from every border (no padding), valid[p] is set (valid: (N,H,W) torch.bool / torch.uint8, None = all), and every
    pixel of the window must be in frame: UNLIKE census_sums, where a neighbour is always read, one out-of-frame or non-finite
    pixel switches off every window it belongs to (a zero inside a window would wreck its means and variances).  `valid` still
    selects centres only, so the images must hold numbers at masked pixels.  H <= 2 radius or W <= 2 radius: counts and sums
    are 0, no error.  images: (N,H,W,C), C = 1..4, nominally in [0, 1] (c1 = 0.01^2, c2 = 0.03^2 are SSIM's constants for that
    range); radius: 1 (the 3 x 3 window of UFlow / ARFlow), 2 or 3.  sums is differentiable w.r.t. flows (pwc_ssim_grad_f32: a
    gather, bit reproducible); the images are constants."""
    consts = _check_ssim(radius, c1, c2, "ssim_sums")
    _check_census_tensors(images_0, images_1, flows, valid)
    return _SsimSums.apply(flows, images_0, images_1, float(flow_scale), valid, consts)


def ssim_loss(images_0, images_1, flows, flow_scale=1.0, valid=None, radius=1, c1=1e-4, c2=9e-4):
    """0-dim: the mean of (1 - SSIM) / 2 over the contributing centres and the channels; 0 when no centre contributes."""
    sums, counts = ssim_sums(images_0, images_1, flows, flow_scale, valid, radius, c1, c2)
    return sums.sum() / (images_0.shape[3] * counts.sum().clamp(min=1)).to(torch.float32)


def fb_valid(flows_fw, flows_bw, flow_scale=1.0, alpha1=0.01, alpha2=0.5, valid_fw=None, valid_bw=None, return_counts=False):
    """(mask_fw, mask_bw), torch.bool (N,H,W), contiguous -- mask_ptr's format, they go straight into `valid=` of the data terms;
    with return_counts also (counts_fw, counts_bw), int32 (N,): the number of True pixels per image (exact, bit reproducible).
    flows_fw: the flow 0 -> 1, flows_bw: the flow 1 -> 0, both (N,H,W,2) float32 (channel slices of wider buffers are read in
    place).  With f = flow_scale * flows_fw[p] and g = flow_scale * (flows_bw sampled bilinearly at p moved by f,
    photometric_sums' sample), mask_fw[p] is True iff valid_fw[p] (where given) and the sample point is inside the frame and
        |f + g|^2 <= alpha1 * (|f|^2 + |g|^2) + alpha2
    (UnFlow's check and constants); a NaN or Inf anywhere in it gives False.  mask_bw: the same with the roles swapped.  A pixel
    that valid_* rules out reads neither flow.  alpha2 is in px^2 at the flows' resolution AFTER flow_scale: flow_scale =
    20 / 2^level takes the pyramid flows with the same alpha2 in that level's pixels.  Not differentiable -- the masks are
    constants, as in UnFlow; flows that require grad are read detached.  With census_loss remember that `valid` selects the
    CENTRES only: an occluded neighbour in a visible centre's window is still read."""
    alpha1, alpha2 = float(alpha1), float(alpha2)
    for name, v in (("alpha1", alpha1), ("alpha2", alpha2)):
        if not v >= 0.0:
            raise ValueError(f"fb_valid: {name} must be non-negative, got {v}")
    _check_nhwc(flows_fw, "flows_fw", (2,))
    _check_nhwc(flows_bw, "flows_bw", (2,))
    if tuple(flows_bw.shape) != tuple(flows_fw.shape):
        raise ValueError(f"flows_bw: expected (N,H,W) {tuple(flows_fw.shape[:3])}, flows_fw's, got {tuple(flows_bw.shape[:3])}")
    N, H, W, _ = flows_fw.shape
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows_fw: empty tensor, shape {tuple(flows_fw.shape)}")
    vp_fw = None if valid_fw is None else mask_ptr(valid_fw, N, H, W, flows_fw.device)
    vp_bw = None if valid_bw is None else mask_ptr(valid_bw, N, H, W, flows_fw.device)
    _check_gpu(flows_fw, flows_bw=flows_bw)
    fa, flows_fw = as_view(flows_fw.detach(), "flows_fw")
    fb, flows_bw = as_view(flows_bw.detach(), "flows_bw")
    L = _lib.lib()
    dev = flows_fw.device
    mask_fw = torch.empty((N, H, W), dtype=torch.bool, device=dev)
    mask_bw = torch.empty((N, H, W), dtype=torch.bool, device=dev)
    counts_fw = counts_bw = ws = None
    if return_counts:
        counts_fw = torch.empty((N,), dtype=torch.int32, device=dev)
        counts_bw = torch.empty((N,), dtype=torch.int32, device=dev)
        ws = torch.empty((max(L.pwc_fb_workspace_floats(N, H, W), 1),), dtype=torch.float32, device=dev)
    _lib.check(L.pwc_fb_valid_u8(_p(fa.ptr), fa.cs, _p(fb.ptr), fb.cs, float(flow_scale), vp_fw, vp_bw, N, H, W, alpha1, alpha2,
                                 _p(mask_fw.data_ptr()), _p(mask_bw.data_ptr()),
                                 _p(counts_fw.data_ptr()) if return_counts else None,
                                 _p(counts_bw.data_ptr()) if return_counts else None,
                                 _p(ws.data_ptr()) if return_counts else None, ws.numel() if return_counts else 0,
                                 _lib.current_stream()), "fb valid")
    if return_counts:
        return mask_fw, mask_bw, counts_fw, counts_bw
    return mask_fw, mask_bw


def _check_fb_pair(flows_fw, flows_bw, valid_fw, valid_bw):
    """fb_valid's tensor checks; the masks' addresses."""
    _check_nhwc(flows_fw, "flows_fw", (2,))
    _check_nhwc(flows_bw, "flows_bw", (2,))
    if tuple(flows_bw.shape) != tuple(flows_fw.shape):
        raise ValueError(f"flows_bw: expected (N,H,W) {tuple(flows_fw.shape[:3])}, flows_fw's, got {tuple(flows_bw.shape[:3])}")
    N, H, W, _ = flows_fw.shape
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows_fw: empty tensor, shape {tuple(flows_fw.shape)}")
    vp_fw = None if valid_fw is None else mask_ptr(valid_fw, N, H, W, flows_fw.device)
    vp_bw = None if valid_bw is None else mask_ptr(valid_bw, N, H, W, flows_fw.device)
    _check_gpu(flows_fw, flows_bw=flows_bw)
    return vp_fw, vp_bw


def _upstream(dsums, N, dev):
    """The upstream gradient of a direction as N contiguous float32 of its own; None (the sums were not used): zeros."""
    if dsums is None:
        return torch.zeros((N,), dtype=torch.float32, device=dev)
    return torch.empty((N,), dtype=torch.float32, device=dev).copy_(dsums)


def fb_consistency_grad(flows_fw, flows_bw, dsums_fw, dsums_bw, dflow_fw=None, dflow_bw=None, flow_scale=1.0, valid_fw=None,
                        valid_bw=None, eps=1e-3, q=0.5, accumulate=False):
    """(dflow_fw, dflow_bw) (+)= the gradient of (dsums_fw * sums_fw).sum() + (dsums_bw * sums_bw).sum() of
    fb_consistency_sums(...) w.r.t. flows_fw and flows_bw (pwc_fb_consistency_grad_f32); dsums_*: (N,) on the GPU.  dflow_* None:
    new tensors; accumulate: added onto them (without it every pixel is written, 0 where nothing reaches it).  Bit reproducible;
    a contribution outside the fixed point's range or a non-finite dsums makes the dflow it reaches all NaN (include/pwc_hip.h).
    What the autograd backward of fb_consistency_sums calls."""
    eps, q = _check_rho(eps, q, "fb_consistency_grad")
    vp_fw, vp_bw = _check_fb_pair(flows_fw, flows_bw, valid_fw, valid_bw)
    fa, flows_fw = as_view(flows_fw.detach(), "flows_fw")
    fb, flows_bw = as_view(flows_bw.detach(), "flows_bw")
    L = _lib.lib()
    dev = flows_fw.device
    up_fw, up_bw = _upstream(dsums_fw, fa.N, dev), _upstream(dsums_bw, fa.N, dev)
    da, dflow_fw = _dflow_view(dflow_fw, fa, dev)
    db, dflow_bw = _dflow_view(dflow_bw, fa, dev)
    ws = torch.empty((L.pwc_fb_consistency_grad_workspace_bytes(fa.N, fa.H, fa.W) // 8,), dtype=torch.int64, device=dev)
    _lib.check(L.pwc_fb_consistency_grad_f32(_p(fa.ptr), fa.cs, _p(fb.ptr), fb.cs, float(flow_scale), vp_fw, vp_bw, fa.N, fa.H,
                                             fa.W, eps, q, _p(up_fw.data_ptr()), _p(up_bw.data_ptr()), _p(ws.data_ptr()),
                                             8 * ws.numel(), _p(da.ptr), da.cs, _p(db.ptr), db.cs, 1 if accumulate else 0,
                                             _lib.current_stream()), "fb consistency grad")
    return dflow_fw, dflow_bw


class _FbConsistencySums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows_fw, flows_bw, flow_scale, valid_fw, valid_bw, eps, q):
        ctx.set_materialize_grads(False)
        N, H, W, _ = flows_fw.shape
        vp_fw = None if valid_fw is None else mask_ptr(valid_fw, N, H, W, flows_fw.device)
        vp_bw = None if valid_bw is None else mask_ptr(valid_bw, N, H, W, flows_fw.device)
        fa, flows_fw = as_view(flows_fw, "flows_fw")
        fb, flows_bw = as_view(flows_bw, "flows_bw")
        L = _lib.lib()
        dev = flows_fw.device
        sums_fw, sums_bw = (torch.empty((N,), dtype=torch.float32, device=dev) for _ in range(2))
        counts_fw, counts_bw = (torch.empty((N,), dtype=torch.int32, device=dev) for _ in range(2))
        ws = torch.empty((max(L.pwc_fb_consistency_workspace_floats(N, H, W), 1),), dtype=torch.float32, device=dev)
        _lib.check(L.pwc_fb_consistency_sums_f32(_p(fa.ptr), fa.cs, _p(fb.ptr), fb.cs, flow_scale, vp_fw, vp_bw, N, H, W, eps, q,
                                                 _p(ws.data_ptr()), ws.numel(), _p(sums_fw.data_ptr()), _p(counts_fw.data_ptr()),
                                                 _p(sums_bw.data_ptr()), _p(counts_bw.data_ptr()), _lib.current_stream()),
                   "fb consistency sums")
        ctx.save_for_backward(flows_fw, flows_bw)
        ctx.valid, ctx.consts = (valid_fw, valid_bw), (flow_scale, eps, q)
        ctx.mark_non_differentiable(counts_fw, counts_bw)
        return sums_fw, counts_fw, sums_bw, counts_bw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsums_fw, _dcounts_fw, dsums_bw, _dcounts_bw):
        if (dsums_fw is None and dsums_bw is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 7
        flows_fw, flows_bw = ctx.saved_tensors
        flow_scale, eps, q = ctx.consts
        dflow_fw, dflow_bw = fb_consistency_grad(flows_fw, flows_bw, dsums_fw, dsums_bw, None, None, flow_scale, ctx.valid[0],
                                                 ctx.valid[1], eps, q)
        return (dflow_fw if ctx.needs_input_grad[0] else None, dflow_bw if ctx.needs_input_grad[1] else None, None, None, None,
                None, None)


def fb_consistency_sums(flows_fw, flows_bw, flow_scale=1.0, valid_fw=None, valid_bw=None, eps=1e-3, q=0.5):
    """(sums_fw (N,) float32, counts_fw (N,) int32, sums_bw, counts_bw): UnFlow's forward-backward consistency term.  With f =
    flow_scale * flows_fw[p] and g = flow_scale * (flows_bw sampled bilinearly at p moved by f) -- fb_valid's f and g -- pixel p
    contributes to the forward direction iff valid_fw[p] (where given; usually fb_valid's mask_fw) and its sample point is inside
    the frame, and
        sums_fw[n] = sum over the contributing pixels of rho(f0 + g0) + rho(f1 + g1),  rho(d) = (d^2 + eps^2)^q,
    counts_fw[n] their number (exact).  The backward direction: the same with the roles swapped.  A pixel its mask rules out
    reads no flow of its own direction.  Both sums are differentiable with respect to BOTH flows (pwc_fb_consistency_grad_f32:
    a flow is reached where it stands and at the corners the other direction samples; bit reproducible); the masks are
    constants and the counts carry no gradient.  No double backward."""
    eps, q = _check_rho(eps, q, "fb_consistency_sums")
    _check_fb_pair(flows_fw, flows_bw, valid_fw, valid_bw)
    return _FbConsistencySums.apply(flows_fw, flows_bw, float(flow_scale), valid_fw, valid_bw, eps, q)


def fb_consistency_loss(flows_fw, flows_bw, flow_scale=1.0, valid_fw=None, valid_bw=None, eps=1e-3, q=0.5):
    """0-dim: the mean of rho over the contributing pixels of both directions and the two components; 0 when none contributes."""
    sums_fw, counts_fw, sums_bw, counts_bw = fb_consistency_sums(flows_fw, flows_bw, flow_scale, valid_fw, valid_bw, eps, q)
    return (sums_fw.sum() + sums_bw.sum()) / (2 * (counts_fw.sum() + counts_bw.sum()).clamp(min=1)).to(torch.float32)


def _check_distill_mask(mask, what, shape, like):
    """dtype (TypeError), shape and layout (ValueError) of a mask of the distillation term, named after its argument."""
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what}: expected a torch.bool or torch.uint8 tensor, got "
                        f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask)}")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, {like}'s (N, H, W), got {tuple(mask.shape)}")
    if not mask.is_contiguous():
        raise ValueError(f"{what}: the mask must be contiguous")


def _check_distill(student, teacher, offset, teacher_valid, exclude):
    """The tensor checks of the distillation term, the device last; (y0, x0)."""
    _check_nhwc(student, "student", (2,))
    _check_nhwc(teacher, "teacher", (2,))
    N, h, w, _ = student.shape
    if N <= 0 or h <= 0 or w <= 0:
        raise ValueError(f"student: empty tensor, shape {tuple(student.shape)}")
    if teacher.shape[0] != N:
        raise ValueError(f"teacher: expected a batch of {N}, the student's, got shape {tuple(teacher.shape)}")
    try:
        y0, x0 = offset
    except (TypeError, ValueError):
        raise ValueError(f"offset: expected a pair (y0, x0) of integers, got {offset!r}") from None
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (y0, x0)):
        raise ValueError(f"offset: expected a pair (y0, x0) of integers, got {offset!r}")
    H, W = teacher.shape[1:3]
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"offset: the {h} x {w} student at {(y0, x0)} does not lie inside the {H} x {W} teacher")
    _check_distill_mask(teacher_valid, "teacher_valid", (N, H, W), "the teacher")
    _check_distill_mask(exclude, "exclude", (N, h, w), "the student")
    for what, t in (("student", student), ("teacher", teacher), ("teacher_valid", teacher_valid), ("exclude", exclude)):
        if t is not None and (not t.is_cuda or t.device != student.device):
            raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only, all arguments on one device")
    return y0, x0


def _distill_call(entry, student, teacher, y0, x0, teacher_valid, exclude, eps, q, *tail):
    sv, student = as_view(student, "student")
    tv, teacher = as_view(teacher, "teacher")
    rc = entry(_p(sv.ptr), sv.cs, _p(tv.ptr), tv.cs, sv.N, sv.H, sv.W, tv.H, tv.W, y0, x0,
               None if teacher_valid is None else _p(teacher_valid.data_ptr()),
               None if exclude is None else _p(exclude.data_ptr()), eps, q, *tail, _lib.current_stream())
    return rc, sv, student, teacher


def flow_distill_grad(student, teacher, dsums, dstudent=None, offset=(0, 0), teacher_valid=None, exclude=None, eps=1e-3, q=0.5,
                      accumulate=False):
    """dstudent (+)= the gradient of (dsums * flow_distill_sums(...)[0]).sum() w.r.t. student (pwc_flow_distill_grad_f32); dsums:
    (N,) on the GPU.  dstudent None: a new tensor; a (N,h,w,2) tensor or channel slice of a wider buffer is written in place;
    accumulate: added onto dstudent, pixels that do not contribute are left alone (without it they get 0).  Returns dstudent.
    What the autograd backward of flow_distill_sums calls."""
    eps, q = _check_rho(eps, q, "flow_distill_grad")
    y0, x0 = _check_distill(student, teacher, offset, teacher_valid, exclude)
    student, teacher = student.detach(), teacher.detach()
    sv = as_view(student, "student")[0]
    up = torch.empty((sv.N,), dtype=torch.float32, device=student.device).copy_(dsums)       # contiguous float32, its own
    dv, dstudent = _dflow_view(dstudent, sv, student.device)
    rc = _distill_call(_lib.lib().pwc_flow_distill_grad_f32, student, teacher, y0, x0, teacher_valid, exclude, eps, q,
                       _p(up.data_ptr()), _p(dv.ptr), dv.cs, 1 if accumulate else 0)[0]
    _lib.check(rc, "flow distill grad")
    return dstudent


class _FlowDistillSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, offset, teacher_valid, exclude, eps, q):
        ctx.set_materialize_grads(False)
        L = _lib.lib()
        dev = student.device
        N, h, w, _ = student.shape
        sums = torch.empty((N,), dtype=torch.float32, device=dev)
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        ws = torch.empty(((L.pwc_flow_distill_workspace_bytes(N, h, w) + 7) // 8 + 1,), dtype=torch.float64, device=dev)
        rc, _, student, teacher = _distill_call(L.pwc_flow_distill_sums_f32, student, teacher, offset[0], offset[1], teacher_valid,
                                                exclude, eps, q, _p(sums.data_ptr()), _p(counts.data_ptr()), _p(ws.data_ptr()),
                                                8 * ws.numel())
        _lib.check(rc, "flow distill sums")
        ctx.save_for_backward(student, teacher)
        ctx.masks, ctx.consts = (teacher_valid, exclude), (offset, eps, q)
        ctx.mark_non_differentiable(counts)
        return sums, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsums, _dcounts):
        if dsums is None or not ctx.needs_input_grad[0]:
            return (None,) * 7
        student, teacher = ctx.saved_tensors
        offset, eps, q = ctx.consts
        dstudent = flow_distill_grad(student, teacher, dsums, None, offset, ctx.masks[0], ctx.masks[1], eps, q)
        return dstudent, None, None, None, None, None, None


def flow_distill_sums(student, teacher, offset=(0, 0), teacher_valid=None, exclude=None, eps=1e-3, q=0.5):
    """(sums (N,) float32, counts (N,) int32) of the self-supervision (distillation) term of DDFlow / SelFlow / UFlow / ARFlow:
    the flow of a narrow view, `student` (N,h,w,2), against the flow the network gave on a wider view, `teacher` (N,H,W,2), read
    in place through the h x w window at offset = (y0, x0): student pixel p = (y, x) pairs with teacher pixel P = (y + y0, x + x0)
    -- nothing is cropped or copied, channel slices of wider buffers are read where they are.  p contributes iff teacher_valid[P]
    (where given: (N,H,W) torch.bool / torch.uint8, read through the same window), not exclude[p] (where given: (N,h,w)), both
    teacher components are finite with |.| <= 1e9 (flow_io.flow_valid's rule) and both student components are finite;
        sums[n] = sum over the contributing pixels of rho(student[p,0] - teacher[P,0]) + rho(student[p,1] - teacher[P,1]),
    rho(d) = (d^2 + eps^2)^q, every pixel in double, the sum in double and rounded once; counts[n] their number (exact).  Both
    flows in the same unit: the window moves no flow vector.  sums is differentiable w.r.t. student (pwc_flow_distill_grad_f32: a
    gather, bit reproducible); the teacher is detached here, whatever it carries, and the masks are constants.  No double
    backward."""
    eps, q = _check_rho(eps, q, "flow_distill_sums")
    y0, x0 = _check_distill(student, teacher, offset, teacher_valid, exclude)
    return _FlowDistillSums.apply(student, teacher.detach(), (y0, x0), teacher_valid, exclude, eps, q)


def flow_distill_loss(student, teacher, offset=(0, 0), teacher_valid=None, exclude=None, eps=1e-3, q=0.5):
    """0-dim: the mean of rho over the contributing pixels and the two components; 0 when no pixel contributes."""
    sums, counts = flow_distill_sums(student, teacher, offset, teacher_valid, exclude, eps, q)
    return sums.sum() / (2 * counts.sum().clamp(min=1)).to(torch.float32)
