"""PWCDCNet as a differentiable torch.nn.Module: the training forward and the hand-written HIP backward of
pwcnet_amd.train behind one torch.autograd.Function, so that any loss written in torch ops reaches the weights (and,
when asked, the images) with `loss.backward()`, and torch.optim steps the parameters.

The parameters are ONE flat nn.Parameter with the Trainer's layout (every TensorFlow variable a 16-byte aligned view,
`variables()`): the kernels read the weights in place, and each backward hands autograd one fresh flat gradient.  Each
forward keeps its activations on its own tape (train._Tape) in the autograd context, so any number of forwards may wait
for their backward; the tape is released by the backward.

Limits: H and W multiples of 64 (as for the Trainer); the bilinear warp only; output_level 4 or 5 (the gradient of the
final x2^(6 - output_level) resize supports factors up to 4); no double backward; no DistributedDataParallel.
PWCDCNet / ForwardPipeline stay the inference fast path.
"""
import torch

from . import grad_ops as G
from .modules import resize_bilinear
from .train import _Net
from .weights import init_weights


class _PWCDCNetFunction(torch.autograd.Function):
    """(flat, images_0, images_1) -> (flows_final, *flows_pyramid) on the training forward; backward on the HIP
    gradient kernels from arbitrary upstream gradients."""

    @staticmethod
    def forward(ctx, flat, images_0, images_1, net):
        ctx.set_materialize_grads(False)
        tape = net._forward(images_0, images_1)
        final, pyr = _final_and_pyramid(net, tape)
        ctx.net, ctx.tape = net, tape
        ctx.save_for_backward(flat)             # (the backward reads the weights: autograd refuses if they changed since)
        return (final, *pyr)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dfinal, *dpyr):
        net, tape = ctx.net, ctx.tape
        flat, = ctx.saved_tensors
        if tape is None:
            raise RuntimeError("PWCDCNetModule: backward through the same forward twice (retain_graph is not supported)")
        ctx.tape = None                                   # the activations go once this backward has been enqueued
        # the backward adds into the level gradients: copies, never autograd's own tensors
        dflows = [torch.zeros_like(p) if d is None else torch.empty_like(p).copy_(d) for p, d in zip(tape.flows_pyramid, dpyr)]
        if dfinal is not None:
            dfinal = dfinal.to(torch.float32).contiguous()
            tape.keep.append(dfinal)
        need_images = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        d_images = None
        if need_images:
            d_images = torch.empty((2 * tape.N, tape.H, tape.W, 3), dtype=torch.float32, device=net.device)
        grads = torch.zeros_like(flat)
        net._backward_from(tape, dflows, grads, dfinal=dfinal, d_images=d_images)
        di0 = d_images[:tape.N] if ctx.needs_input_grad[1] else None
        di1 = d_images[tape.N:] if ctx.needs_input_grad[2] else None
        return grads if ctx.needs_input_grad[0] else None, di0, di1, None


def _final_and_pyramid(net, tape):
    """flows_final (px) and copies of the pyramid flows (px / 20): the tape keeps its own tensors, the caller gets
    tensors that nothing else refers to."""
    pyr = [p.clone() for p in tape.flows_pyramid]
    up = 2 ** (net.num_levels - net.output_level)
    last = tape.flows_pyramid[-1]
    final = resize_bilinear(last, (last.shape[1] * up, last.shape[2] * up), mul=20.0)
    return final, pyr


class PWCDCNetModule(torch.nn.Module):
    """Differentiable PWCDCNet (reference model.py:74-134) on the HIP training kernels.

    forward(images_0, images_1) -> (flows_final (N,H,W,2) px, flows_pyramid [5 x (N,h,w,2)] px / 20): the shapes and
    units of PWCDCNet.__call__.  Gradients reach `flat` (every variable) and, when they require grad, both images."""

    def __init__(self, num_levels=6, search_range=4, warp_type="bilinear", use_dc=False, output_level=4,
                 name="pwcdcnet", f16x2=True, f16x2_dgrad=False, seed=0, device="cuda", normalize_features=False,
                 norm_eps=1e-16):
        super().__init__()
        if warp_type != "bilinear":
            raise ValueError(f"PWCDCNetModule: warp_type {warp_type!r} has no flow gradient; use 'bilinear'")
        if num_levels != 6 or search_range != 4:
            raise ValueError("PWCDCNetModule: num_levels 6 and search_range 4 only (the training kernels' configuration)")
        if not 0 <= output_level < num_levels or 2 ** (num_levels - output_level) > 4:
            raise ValueError(f"PWCDCNetModule: output_level {output_level} not supported: flows_final's resize factor "
                             f"2^{num_levels - output_level} is above 4 (output_level 4 or 5)")
        self._net = _Net(num_levels, search_range, warp_type, use_dc, output_level, name, f16x2, f16x2_dgrad, device,
                         normalize_features, norm_eps)
        self.flat = torch.nn.Parameter(self._net.params)
        self.load_weights(init_weights(self._net.specs, seed=seed))
        G._lib.lib()                                    # fail loudly without the HIP library

    # ------------------------------------------------------------------ variables
    def _bind(self):
        """The flat parameter's current storage is what the kernels read."""
        self._net.params = self.flat.detach()
        return self._net

    def variables(self):
        """{TF variable name: view of `flat`} (kernels (3,3,cin,cout), biases (cout,)); views share flat's gradient."""
        return {k: self._net._view(self.flat, k) for k in self._net.views}

    def load_weights(self, weights):
        """weights: {TF variable name: array}, the names of PWCDCNet.load_weights / Trainer.state_dict."""
        with torch.no_grad():
            self._bind().load_weights(weights)

    def tf_state_dict(self):
        """{TF variable name: numpy array}: loads into PWCDCNet.load_weights and Trainer.load_weights."""
        return self._bind().state_dict()

    # ------------------------------------------------------------------ forward
    def forward(self, images_0, images_1):
        net = self._bind()
        for t in (images_0, images_1):
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[-1] == 3):
                raise ValueError("PWCDCNetModule: images must be (N,H,W,3) float32 tensors on the GPU")
        if images_0.shape != images_1.shape:
            raise ValueError(f"PWCDCNetModule: image shapes differ: {tuple(images_0.shape)} vs {tuple(images_1.shape)}")
        if images_0.shape[1] % 64 or images_0.shape[2] % 64:
            raise ValueError("PWCDCNetModule: H and W must be multiples of 64")
        if torch.is_grad_enabled() and (self.flat.requires_grad or images_0.requires_grad or images_1.requires_grad):
            final, *pyr = _PWCDCNetFunction.apply(self.flat, images_0, images_1, net)
            return final, pyr
        tape = net._forward(images_0.detach(), images_1.detach())       # the same forward, nothing kept
        return _final_and_pyramid(net, tape)
