"""pwcnet_amd.PWCDCNetModule: the training forward and the HIP backward behind torch.autograd.

- arbitrary cotangents on flows_final and every pyramid level against torch.autograd on the float64 restatement
  (oracle/torch_ref.py), every variable and both images;
- the same parameter gradients as Trainer.backward, bit for bit, for the multiscale loss's cotangents;
- one tape per forward: two forwards, one backward;
- the library calls: the narrow stride-2 image gradient runs once per backward, and only when asked for;
- a torch.optim training loop on a loss written in torch ops, whose weights then load into PWCDCNet.

Errors are relative to the reference's largest magnitude (per variable / per image).  Every bound is 10x the worst error
measured on an MI355X, rounded up to two digits; the comments give that error and where it is."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as tr
from tests import util

pytestmark = pytest.mark.gpu

LOSS_WEIGHTS = (0.32, 0.08, 0.02, 0.01, 0.005)

# (use_dc, (N, H, W)) -> (variable gradient bound, image gradient bound)
COTANGENT_BOUNDS = {
    (False, (2, 64, 128)): (1.4e-5, 1.4e-5),   # 1.36e-6 fp_extractor/conv2d/bias (images below that)
    (True, (2, 64, 128)): (1.6e-5, 1.6e-5),    # 1.52e-6 optflow_4/conv2d_3/kernel (images below that)
    # sign-following extractor; 7.2e-4 context/conv2d_2/kernel, images 6.0e-3 (images_0).  The per-element image gradient
    # sums every path back to the pixel; with O(1) cotangents on all 384x448 pixels of flows_final, the estimators' and the
    # context's own leaky-relu branches and the warps' floor cells, which follow the fp32 forward's flows and are not
    # pinned to float64's, move single pixels' sums.  The 64x128 cases and test_gpu_dgrad_s2_narrow.py hold the tight bounds.
    (False, (4, 384, 448)): (7.3e-3, 6e-2),
}


def gpu(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t.requires_grad_(grad)


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def rel_err(got, ref):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-12)


def smooth_cotangent(shape, seed):
    """A random field, smooth on the scale of 4 pixels (bilinear-free: block values plus a small ramp)."""
    N, h, w, c = shape
    rs = np.random.RandomState(seed)
    hb, wb = -(-h // 4), -(-w // 4)
    base = rs.uniform(-1, 1, size=(N, hb, wb, c))
    g = np.kron(base, np.ones((1, 4, 4, 1)))[:, :h, :w]
    g += 0.25 * np.sin(np.arange(w) / 3.0)[None, None, :, None]
    return g.astype(np.float32)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    return pwcnet_amd


def _module_grads(M, w, im0, im1, cots, use_dc=False):
    net = M.PWCDCNetModule(use_dc=use_dc)
    net.load_weights(w)
    i0, i1 = gpu(im0, True), gpu(im1, True)
    final, pyr = net(i0, i1)
    torch.autograd.backward([final, *pyr], [gpu(c) for c in cots])
    torch.cuda.synchronize()
    g = {k: net._net._view(net.flat.grad, k) for k in net._net.views}
    return net, g, i0.grad, i1.grad


def _report(tag, errs):
    ranked = sorted(errs.items(), key=lambda kv: -kv[1])
    print(f"\n[{tag}] worst {ranked[0][1]:.2e} ({ranked[0][0]}), median {float(np.median(list(errs.values()))):.2e}")
    for k, e in ranked[:4]:
        print(f"    {e:.2e}  {k}")


def _check(key, errs):
    g_bound, i_bound = COTANGENT_BOUNDS[key]
    _report(key, errs)
    bad = {k: f"{e:.3e}" for k, e in errs.items() if e > (i_bound if k.startswith("images") else g_bound)}
    assert not bad, f"relative gradient error above the bounds {g_bound:.1e} / {i_bound:.1e}: {bad}"


def _cotangents(N, H, W, n_levels=5, seed=100):
    cots = [smooth_cotangent((N, H, W, 2), seed)]
    for l in range(n_levels):
        s = 2 ** (6 - l)
        cots.append(smooth_cotangent((N, H // s, W // s, 2), seed + 1 + l))
    return cots


@pytest.mark.parametrize("use_dc", [False, True])
def test_arbitrary_cotangents_vs_float64_autograd(M, use_dc):
    N, H, W = 2, 64, 128
    w = util.model_weights(use_dc, gain=1.25)
    im0, im1 = util.smooth_images(N, H, W, seed=61, shift=(3, -2))
    cots = _cotangents(N, H, W)
    wt = {k: t64(v) for k, v in w.items()}
    r0, r1 = t64(im0), t64(im1)
    final, pyr = tr.TorchPWCDCNet(wt, use_dc=use_dc)(r0, r1)
    torch.autograd.backward([final, *pyr], [t64(c, False) for c in cots])
    _, g, d0, d1 = _module_grads(M, w, im0, im1, cots, use_dc)
    errs = {k: rel_err(g[k], wt[k].grad) for k in wt}
    errs["images_0"], errs["images_1"] = rel_err(d0, r0.grad), rel_err(d1, r1.grad)
    _check((use_dc, (N, H, W)), errs)


def test_arbitrary_cotangents_at_the_cli_crop(M):
    """384x448, batch 4, non-DC: the float64 reference takes the extractor's leaky-relu branches from the fp32 forward
    (test_gpu_grad._SignFollowingNet; at this size an element or two of the extractor sit within fp32 rounding of zero)."""
    from tests.test_gpu_grad import _SignFollowingNet
    N, H, W = 4, 384, 448
    w = util.model_weights(False, gain=1.2)
    im0, im1 = util.smooth_images(N, H, W, seed=91, shift=(4, -3))
    cots = _cotangents(N, H, W, seed=200)
    net, g, d0, d1 = _module_grads(M, w, im0, im1, cots)
    tape = net._net._forward(gpu(im0), gpu(im1))
    signs = [torch.from_numpy(c.y_t.cpu().numpy() > 0) for c in tape.ext]
    wt = {k: t64(v) for k, v in w.items()}
    ref = _SignFollowingNet(wt, signs, N)
    r0, r1 = t64(im0), t64(im1)
    final, pyr = ref(r0, r1)
    torch.autograd.backward([final, *pyr], [t64(c, False) for c in cots])
    print(f"extractor leaky-relu branches that differ from float64: { {k: n for k, n in ref.flips.items() if n} }")
    assert sum(ref.flips.values()) <= 16, ref.flips
    errs = {k: rel_err(g[k], wt[k].grad) for k in wt}
    errs["images_0"], errs["images_1"] = rel_err(d0, r0.grad), rel_err(d1, r1.grad)
    _check((False, (N, H, W)), errs)


@pytest.mark.parametrize("use_dc", [False, True])
def test_multiscale_cotangents_give_the_trainers_gradients_bit_for_bit(M, use_dc):
    from pwcnet_amd import grad_ops as G
    from pwcnet_amd.modules import as_view
    from pwcnet_amd.train import Trainer
    N, H, W = 2, 64, 128
    w = util.model_weights(use_dc, gain=1.25)
    im0, im1 = util.smooth_images(N, H, W, seed=61, shift=(3, -2))
    gt = util.flow_field(N, H, W, seed=62, sigma=2.0, outliers=False).astype(np.float32)
    g0, g1, ggt = gpu(im0), gpu(im1), gpu(gt)
    tn = Trainer(weights=LOSS_WEIGHTS, gamma=0.0, use_dc=use_dc)
    tn.load_weights(w)
    tn.forward(g0, g1)
    tn.backward(ggt)
    net = M.PWCDCNetModule(use_dc=use_dc)
    net.load_weights(w)
    _, pyr = net(g0, g1)
    cots = []
    for l, p in enumerate(pyr):
        d = torch.empty_like(p)
        G.flow_norm_grad(as_view(p.detach())[0], as_view(ggt)[0], as_view(d)[0], gt_div=20.0, ord=2, scale=LOSS_WEIGHTS[l] / N)
        cots.append(d)
    torch.autograd.backward(pyr, cots)
    torch.cuda.synchronize()
    assert torch.equal(net.flat.grad, tn.grads)


def _loss(out, target):
    final, pyr = out
    return (final - target).abs().mean() + 0.1 * sum((p * p).mean() for p in pyr)


def test_two_forwards_one_backward(M):
    """Each forward keeps its own tape: loss(net(a, b)) + loss(net(b, a)) with one backward gives the sum of the two
    separate backwards, and the tapes are released by the backward."""
    N, H, W = 2, 64, 128
    net = M.PWCDCNetModule()
    net.load_weights(util.model_weights(False, gain=1.25))
    im0, im1 = util.smooth_images(N, H, W, seed=61, shift=(3, -2))
    a, b = gpu(im0, True), gpu(im1, True)
    target = gpu(util.flow_field(N, H, W, seed=5, sigma=2.0, outliers=False))

    def grads(pairs):
        net.zero_grad(set_to_none=True)
        a.grad = b.grad = None
        sum(_loss(net(x, y), target) for x, y in pairs).backward()
        torch.cuda.synchronize()
        return net.flat.grad.clone(), a.grad.clone(), b.grad.clone()

    grads([(a, b)])                                       # warm-up: workspaces
    net.zero_grad(set_to_none=True)
    a.grad = b.grad = None
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    both = grads([(a, b), (b, a)])
    ab = grads([(a, b)])
    ba = grads([(b, a)])
    for got, x, y in zip(both, ab, ba):
        assert torch.equal(got, x + y)
    del both, ab, ba
    net.zero_grad(set_to_none=True)
    a.grad = b.grad = None
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - m0
    print(f"\nallocated after the backwards: {grown / 2 ** 20:+.2f} MiB")
    assert grown <= 4 * 2 ** 20, grown


def test_library_calls_of_the_image_gradient(M, monkeypatch):
    from pwcnet_amd import _lib
    from pwcnet_amd import grad_ops as G
    from tests.test_gpu_dispatch import _Recorder
    N, H, W = 2, 64, 128
    net = M.PWCDCNetModule()
    net.load_weights(util.model_weights(False))
    im0, im1 = util.smooth_images(N, H, W)
    target = gpu(util.flow_field(N, H, W, seed=5, sigma=2.0, outliers=False))
    dgrads = []
    orig = G.conv3x3_dgrad

    def spy(dy, w, dx, *a, **k):
        dgrads.append(dx.C)
        return orig(dy, w, dx, *a, **k)

    monkeypatch.setattr(G, "conv3x3_dgrad", spy)

    def narrow_calls(grad0, grad1):
        rec = _Recorder(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", rec)
        dgrads.clear()
        try:
            _loss(net(gpu(im0, grad0), gpu(im1, grad1)), target).backward()
            torch.cuda.synchronize()
        finally:
            monkeypatch.setattr(_lib, "_lib", rec._handle)
        return sum(1 for name, _ in rec.calls if name == "pwc_conv3x3_dgrad_s2_narrow_f32")

    assert narrow_calls(True, True) == 1 and 3 not in dgrads, dgrads
    assert narrow_calls(True, False) == 1 and 3 not in dgrads, dgrads
    assert narrow_calls(False, False) == 0 and 3 not in dgrads, dgrads


def test_torch_optim_training_loop_and_weights_round_trip(M):
    N, H, W = 2, 64, 64
    net = M.PWCDCNetModule()
    net.load_weights(util.model_weights(False, gain=1.1))
    im0, im1 = util.smooth_images(N, H, W, seed=63, shift=(2, 1))
    g0, g1 = gpu(im0), gpu(im1)
    gt = torch.zeros((N, H, W, 2), device="cuda")
    gt[..., 0], gt[..., 1] = 2.0, 1.0                      # the true motion of smooth_images(shift=(2, 1))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        final, _ = net(g0, g1)
        loss = torch.linalg.vector_norm(final - gt, dim=-1).mean()          # EPE
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("EPE:", [round(x, 4) for x in losses])
    assert losses[-1] < 0.9 * losses[0], losses
    ref = M.PWCDCNet()
    ref.load_weights(net.tf_state_dict())
    with torch.no_grad():
        final, pyr = net(g0, g1)
    e_final, e_pyr = ref(g0, g1)
    for a, b in zip([final, *pyr], [e_final, *e_pyr]):
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))
    v = net.variables()
    assert sorted(v) == sorted(net.tf_state_dict()) and v["pwcdcnet/context/conv2d_6/bias"].shape == (2,)
