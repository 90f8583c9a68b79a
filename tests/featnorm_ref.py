"""float64 torch restatement of the cost-volume feature normalisation ("Feature normalisation") and of the model
that uses it.  TEST INFRASTRUCTURE ONLY, CPU, differentiated by torch.autograd.

    feature_norm(f0, f1, eps)   one layer norm over the two maps of every pair: (y0, y1, mean, rstd)
    NormPWCDCNet                oracle.torch_ref.TorchPWCDCNet whose levels normalise their pair BEFORE the warp and the cost
                                volume; the estimator's concat keeps the raw features_0
"""
import numpy as np
import torch

from oracle import torch_ref as tr

EPS = 1e-16


def feature_norm(f0, f1, eps=EPS):
    """f0, f1: (N, h, w, C) float64.  Two passes, as the definition reads: mean, then the biased variance of the residuals."""
    assert f0.dtype == torch.float64 and f1.dtype == torch.float64 and f0.shape == f1.shape
    N = f0.shape[0]
    x = torch.cat([f0.reshape(N, -1), f1.reshape(N, -1)], dim=1)
    M = x.shape[1]
    mean = x.sum(dim=1, keepdim=True) / M
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / M
    rstd = 1.0 / torch.sqrt(var + eps)
    sh = (N, 1, 1, 1)
    return (f0 - mean.view(sh)) * rstd.view(sh), (f1 - mean.view(sh)) * rstd.view(sh), mean.view(N), rstd.view(N)


def feature_norm_np(f0, f1, eps=EPS):
    """The same on float32 numpy maps: float64 numpy (y0, y1, mean, rstd)."""
    y0, y1, mean, rstd = feature_norm(torch.from_numpy(np.asarray(f0, np.float64)), torch.from_numpy(np.asarray(f1, np.float64)), eps)
    return y0.numpy(), y1.numpy(), mean.numpy(), rstd.numpy()


def feature_norm_grads(f0, f1, g0, g1, eps=EPS):
    """autograd through feature_norm: float64 numpy (d f0, d f1) for upstream g0, g1; plus the three terms' absolute sum
    A = |rstd g| + |rstd a| + |rstd xh b| per element of (f0, f1) -- the scale of the gradient kernel's rounding."""
    a0 = torch.tensor(np.asarray(f0, np.float64), requires_grad=True)
    a1 = torch.tensor(np.asarray(f1, np.float64), requires_grad=True)
    t0, t1 = torch.from_numpy(np.asarray(g0, np.float64)), torch.from_numpy(np.asarray(g1, np.float64))
    y0, y1, _, rstd = feature_norm(a0, a1, eps)
    ((y0 * t0).sum() + (y1 * t1).sum()).backward()
    N = a0.shape[0]
    M = 2 * a0[0].numel()
    sh = (N, 1, 1, 1)
    with torch.no_grad():
        ga = ((t0.reshape(N, -1).sum(1) + t1.reshape(N, -1).sum(1)) / M).view(sh)
        gb = (((t0 * y0).reshape(N, -1).sum(1) + (t1 * y1).reshape(N, -1).sum(1)) / M).view(sh)
        r = rstd.view(sh)
        A0 = r * (t0.abs() + ga.abs() + (y0 * gb).abs())
        A1 = r * (t1.abs() + ga.abs() + (y1 * gb).abs())
    return a0.grad.numpy(), a1.grad.numpy(), A0.numpy(), A1.numpy()


class NormPWCDCNet(tr.TorchPWCDCNet):
    """TorchPWCDCNet with normalize_features: every level correlates the normalised pair (normalise first, then warp); the
    estimator, the context network and the up-sampling see the raw features.  self.level_stats: per level (mean, rstd, std / |mean|
    minimum over the pairs) of the last call."""

    def __init__(self, weights, eps=EPS, **kw):
        super().__init__(weights, **kw)
        self.eps = eps
        self.level_stats = []

    def __call__(self, images_0, images_1):
        pyr0, pyr1 = self.extractor(images_0), self.extractor(images_1)
        self.level_stats = []
        flows_pyramid, flows_up, feats_up = [], None, None
        for l, (f0, f1) in enumerate(zip(pyr0, pyr1)):
            y0, y1, mean, rstd = feature_norm(f0, f1, self.eps)
            with torch.no_grad():
                self.level_stats.append((mean.clone(), rstd.clone(), float(((1.0 / rstd) / mean.abs()).min())))
            f1w = y1 if l == 0 else tr.bilinear_warp(y1, flows_up * self.SCALES[l])
            cv = tr.cost_volume(y0, f1w, self.s_range)
            if l < self.output_level:
                flows, flows_up, feats_up = self.estimator(l, cv, f0, flows_up, feats_up, False)
            else:
                flows, feats = self.estimator(l, cv, f0, flows_up, feats_up, True)
                flows = self.context(flows, feats)
                flows_pyramid.append(flows)
                up = 2 ** (self.num_levels - self.output_level)
                h, w = flows.shape[1:3]
                return tr.resize_legacy(flows, (h * up, w * up)) * 20.0, flows_pyramid
            flows_pyramid.append(flows)


# ---------------------------------------------------------------- seeded inputs shared by the host and the GPU tests
def lrelu_maps(shape, seed, shift=0.0):
    """Two leaky-relu-like float32 maps (N, h, w, C): a normal draw through max(0.1 x, x), |mean| rstd about 1; `shift` is added
    (the caller picks it so that |mean| rstd lands where the case wants it)."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        x = rs.normal(0.6, 1.0, size=shape)
        out.append((np.maximum(0.1 * x, x) + shift).astype(np.float32))
    return out


# inputs of the model tests: (kernel gain, image seed, image shift, ground-truth seed) -- those of tests/test_gpu_grad.py's step
# tests at 2 x 64 x 128, so that its bounds for the un-normalised model are the yardstick
MODEL_SHAPE = (2, 64, 128)
MODEL_INPUTS = (1.25, 61, (3, -2), 62)
LOSS_WEIGHTS = (0.32, 0.08, 0.02, 0.01, 0.005)


def model_inputs(use_dc):
    from tests import util
    gain, s_im, shift, s_gt = MODEL_INPUTS
    N, H, W = MODEL_SHAPE
    w = util.model_weights(use_dc, gain=gain)
    im0, im1 = util.smooth_images(N, H, W, seed=s_im, shift=shift)
    gt = util.flow_field(N, H, W, seed=s_gt, sigma=2.0, outliers=False).astype(np.float32)
    return w, im0, im1, gt


_MODEL_REF = {}


def model_reference(use_dc):
    """One float64 forward + backward of the normalised model on model_inputs (multiscale loss), computed once per process:
    dict(w, im0, im1, gt, final, pyr, loss, grads {variable: tensor}, d_im0, d_im1, level_stats)."""
    if use_dc not in _MODEL_REF:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        w, im0, im1, gt = model_inputs(use_dc)
        wt = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in w.items()}
        r0 = torch.tensor(np.asarray(im0, np.float64), requires_grad=True)
        r1 = torch.tensor(np.asarray(im1, np.float64), requires_grad=True)
        net = NormPWCDCNet(wt, use_dc=use_dc)
        final, pyr = net(r0, r1)
        loss = tr.multiscale_loss(torch.from_numpy(gt.astype(np.float64)), pyr, LOSS_WEIGHTS)
        loss.backward()
        _MODEL_REF[use_dc] = dict(w=w, im0=im0, im1=im1, gt=gt, final=final.detach().numpy(), pyr=[p.detach() for p in pyr],
                                  loss=float(loss.detach()), grads={k: v.grad for k, v in wt.items()}, d_im0=r0.grad, d_im1=r1.grad,
                                  level_stats=net.level_stats)
    return _MODEL_REF[use_dc]
