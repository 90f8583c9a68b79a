"""Flow composition on the HIP path: long-range flow from the flows of consecutive pairs (csrc/pwc_compose.hip).

    compose_flows(flows_ab, flows_bc, valid_ab=None, valid_bc=None)         -> (flows_ac (N,H,W,2), valid_ac (N,H,W) torch.bool)
    compose_grad(flows_ab, flows_bc, g, valid_ab=None, valid_bc=None, ...)  -> (dflow_ab, dflow_bc)
    chain_flows(flows, valids=None, span=None)                              -> (flows, valid)

flows_ac[p] = f + flows_bc sampled bilinearly at p + f, f = flows_ab[p] (fb_valid's sample, in double, rounded once).  Pixel p
is valid iff valid_ab[p] (where given), f is known (both components finite with |.| <= 1e9: flow_io.flow_valid's rule for the
.flo sentinel), the sample point is inside the frame, and all four corners it reads are valid in valid_bc (where given) and
known -- whatever their weights.  An invalid pixel holds the sentinel (1e10, 1e10), so flow_io.write_flo, evaluate.py and a
further compose_flows treat it as unknown.  Differentiable with respect to BOTH flows: the gradient into flows_ab is a gather,
the one into flows_bc a scatter whose sums are 64-bit fixed point at a step relative to the largest upstream gradient of the
image, so two calls give the same bits, an image gives the same bits alone and in a batch, and an upstream gradient of any scale
(a loss mean puts it near 1 / (N H W)) keeps its 36 bits (include/pwc_hip.h, "flow composition").  No double backward.
"""
import torch

from . import _lib
from .modules import _p, as_view
from .unsup import _check_distill_mask, _check_nhwc, _dflow_view


def _check_compose(flows_ab, flows_bc, valid_ab, valid_bc, device=True, **others):
    """Types and shapes of a composition's arguments, each named after its argument; the device (where asked) last of all."""
    _check_nhwc(flows_ab, "flows_ab", (2,))
    _check_nhwc(flows_bc, "flows_bc", (2,))
    N, H, W, _ = flows_ab.shape
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows_ab: empty tensor, shape {tuple(flows_ab.shape)}")
    if tuple(flows_bc.shape) != tuple(flows_ab.shape):
        raise ValueError(f"flows_bc: expected (N,H,W) {(N, H, W)}, flows_ab's, got {tuple(flows_bc.shape[:3])}")
    _check_distill_mask(valid_ab, "valid_ab", (N, H, W), "flows_ab")
    _check_distill_mask(valid_bc, "valid_bc", (N, H, W), "flows_ab")
    for what, t in others.items():
        _check_nhwc(t, what, (2,))
        if tuple(t.shape) != tuple(flows_ab.shape):
            raise ValueError(f"{what}: expected shape {tuple(flows_ab.shape)}, flows_ab's, got {tuple(t.shape)}")
    for what, t in dict(flows_ab=flows_ab, flows_bc=flows_bc, valid_ab=valid_ab, valid_bc=valid_bc, **others).items():
        if device and t is not None and (not t.is_cuda or t.device != flows_ab.device):
            raise ValueError(f"{what}: the tensor is on {t.device}; pwcnet_amd runs on the GPU only, all arguments on one device")


def _mask_p(mask):
    return None if mask is None else _p(mask.data_ptr())


def _compose_forward(flows_ab, flows_bc, valid_ab, valid_bc):
    """The launch: (flows_ac, valid_ac, the flows as the kernel read them)."""
    av, flows_ab = as_view(flows_ab, "flows_ab")
    bv, flows_bc = as_view(flows_bc, "flows_bc")
    dev = flows_ab.device
    out = torch.empty((av.N, av.H, av.W, 2), dtype=torch.float32, device=dev)
    valid = torch.empty((av.N, av.H, av.W), dtype=torch.bool, device=dev)
    _lib.check(_lib.lib().pwc_flow_compose_f32(_p(av.ptr), av.cs, _p(bv.ptr), bv.cs, _mask_p(valid_ab), _mask_p(valid_bc), av.N,
                                               av.H, av.W, _p(out.data_ptr()), 2, _p(valid.data_ptr()), _lib.current_stream()),
               "flow compose")
    return out, valid, flows_ab, flows_bc


def compose_grad(flows_ab, flows_bc, g, valid_ab=None, valid_bc=None, dflow_ab=None, dflow_bc=None, accumulate=False):
    """(dflow_ab, dflow_bc) (+)= the gradient of (g * flows_ac).sum() over the valid pixels of compose_flows(flows_ab, flows_bc,
    valid_ab, valid_bc) w.r.t. both flows (pwc_flow_compose_grad_f32); g: (N,H,W,2), it is not read at an invalid pixel.
    dflow_* None: new tensors; a (N,H,W,2) tensor or channel slice of a wider buffer is written in place; accumulate: added onto
    them -- exactly what a plain call writes -- and pixels nothing reaches are left alone (without it they get exact zeros).  Bit
    reproducible; a non-finite g at a valid pixel of an image makes that image's dflow_bc all NaN.  What the autograd backward
    of compose_flows calls."""
    _check_compose(flows_ab, flows_bc, valid_ab, valid_bc, g=g)
    av, flows_ab = as_view(flows_ab.detach(), "flows_ab")
    bv, flows_bc = as_view(flows_bc.detach(), "flows_bc")
    gv, g = as_view(g.detach(), "g")
    dev = flows_ab.device
    da, dflow_ab = _dflow_view(dflow_ab, av, dev)
    db, dflow_bc = _dflow_view(dflow_bc, av, dev)
    L = _lib.lib()
    ws = torch.empty((L.pwc_flow_compose_grad_workspace_bytes(av.N, av.H, av.W) // 8,), dtype=torch.int64, device=dev)
    _lib.check(L.pwc_flow_compose_grad_f32(_p(av.ptr), av.cs, _p(bv.ptr), bv.cs, _mask_p(valid_ab), _mask_p(valid_bc), av.N, av.H,
                                           av.W, _p(gv.ptr), gv.cs, _p(ws.data_ptr()), 8 * ws.numel(), _p(da.ptr), da.cs,
                                           _p(db.ptr), db.cs, 1 if accumulate else 0, _lib.current_stream()), "flow compose grad")
    return dflow_ab, dflow_bc


class _ComposeFlows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flows_ab, flows_bc, valid_ab, valid_bc):
        ctx.set_materialize_grads(False)
        out, valid, flows_ab, flows_bc = _compose_forward(flows_ab, flows_bc, valid_ab, valid_bc)
        ctx.save_for_backward(flows_ab, flows_bc)
        ctx.masks = (valid_ab, valid_bc)
        ctx.mark_non_differentiable(valid)
        return out, valid

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gvalid):
        if g is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None
        flows_ab, flows_bc = ctx.saved_tensors
        dflow_ab, dflow_bc = compose_grad(flows_ab, flows_bc, g, ctx.masks[0], ctx.masks[1])
        return (dflow_ab if ctx.needs_input_grad[0] else None, dflow_bc if ctx.needs_input_grad[1] else None, None, None)


def compose_flows(flows_ab, flows_bc, valid_ab=None, valid_bc=None):
    """(flows_ac (N,H,W,2) float32, valid_ac (N,H,W) torch.bool, contiguous -- it goes straight into `valid=` of the data terms
    and into the next compose_flows): the flow a -> c from the flows a -> b and b -> c of frames of one size, both in pixels.
    flows_*: (N,H,W,2) float32, channel slices of wider buffers are read in place; valid_*: (N,H,W) torch.bool / torch.uint8,
    contiguous, None = every pixel.  With f = flows_ab[p] and q = p + f,
        flows_ac[p] = f + (flows_bc sampled bilinearly at q)    (in double, rounded once),
    and p is valid iff valid_ab[p], f is known (finite, |.| <= 1e9), q lies in [0, W - 1] x [0, H - 1], and each of the four
    pixels around q (clamped to the frame) is valid in valid_bc and known, whatever its weight.  An invalid pixel holds the
    .flo sentinel (1e10, 1e10) and reads nothing the rule excludes: a NaN there reaches no output.  Differentiable with
    respect to both flows (pwc_flow_compose_grad_f32: bit reproducible, per image); the masks are constants, the gradient at an
    invalid pixel is not read.  fb_valid's mask as valid_ab keeps occluded pixels out of a chain.  No double backward."""
    _check_compose(flows_ab, flows_bc, valid_ab, valid_bc)
    return _ComposeFlows.apply(flows_ab, flows_bc, valid_ab, valid_bc)


def _known(flows, valid):
    """The mask of a chain of one flow: compose_flows' rule for f without a second flow (span 1; no kernel of its own)."""
    known = (flows.detach().abs() <= 1e9).all(dim=3)
    return known if valid is None else known & valid.to(torch.bool)


def chain_flows(flows, valids=None, span=None):
    """Long-range flow from consecutive flows, by repeated compose_flows; (flows, valid) as compose_flows gives them.
        chain_flows([f01, f12, ..., ], valids=None)     a list of L (N,H,W,2) tensors i -> i+1: the left fold 0 -> L, (N,H,W,2);
                                                        valids: None or a list of L masks (each (N,H,W) or None);
        chain_flows(flows, valids=None, span=K)         flows: ONE (T,H,W,2) tensor of the consecutive flows i -> i+1 of a
                                                        sequence: the (T-K+1,H,W,2) flows i -> i+K, 1 <= K <= T; valids: None or
                                                        a (T,H,W) mask.
    The second form makes K - 1 batched calls on batch slices (step k composes acc[:T-k] with flows[k:]), nothing is copied.
    Each step's mask goes in as the next valid_ab, so a pixel lost once stays unknown.  Differentiable with respect to every
    flow.  A chain of one flow is that flow and the mask of its known pixels."""
    if span is None:
        if not isinstance(flows, (list, tuple)) or len(flows) < 1:
            raise TypeError(f"flows: expected a non-empty list of (N,H,W,2) tensors (or one (T,H,W,2) tensor and span=K), got "
                            f"{type(flows)}")
        if valids is None:
            valids = [None] * len(flows)
        if not isinstance(valids, (list, tuple)) or len(valids) != len(flows):
            raise ValueError(f"valids: expected None or a list of {len(flows)} masks, one per flow")
        if len(flows) == 1:
            _check_compose(flows[0], flows[0], valids[0], None, device=False)
            return flows[0], _known(flows[0], valids[0])
        acc, mask = compose_flows(flows[0], flows[1], valids[0], valids[1])
        for f, v in zip(flows[2:], valids[2:]):
            acc, mask = compose_flows(acc, f, mask, v)
        return acc, mask
    if isinstance(span, bool) or not isinstance(span, int):
        raise TypeError(f"span: expected an integer, got {span!r}")
    _check_nhwc(flows, "flows", (2,))
    T = flows.shape[0]
    if not 1 <= span <= T:
        raise ValueError(f"span: expected 1 <= span <= {T}, the number of flows, got {span}")
    _check_distill_mask(valids, "valids", tuple(flows.shape[:3]), "flows")
    _check_compose(flows, flows, None, None, device=False)
    if span == 1:
        return flows, _known(flows, valids)
    acc, mask = flows, valids
    for k in range(1, span):
        acc, mask = compose_flows(acc[:T - k], flows[k:], None if mask is None else mask[:T - k],
                                  None if valids is None else valids[k:])
    return acc, mask
