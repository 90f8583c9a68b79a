"""GPU tests of the training path: every backward kernel and the assembled train step
against torch.autograd on the float64 CPU restatement of the forward (oracle/torch_ref.py).

Tolerances are relative to the largest reference gradient (fp32 kernels vs a float64 reference)."""
import time

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def go():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import grad_ops
    return grad_ops


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, size=shape).astype(np.float32)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def close(got, exp, rel=2e-5):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got
    exp = exp.detach().cpu().double().numpy() if isinstance(exp, torch.Tensor) else exp
    assert got.shape == exp.shape, (got.shape, exp.shape)
    tol = rel * max(float(np.abs(exp).max()), 1e-6)
    err = float(np.abs(got - exp).max())
    assert err <= tol, f"max abs err {err:.3e} > tol {tol:.3e} (max |ref| {float(np.abs(exp).max()):.3e})"


def View(*a):
    from pwcnet_amd.modules import View as _V
    return _V(*a)


def V(t):
    from pwcnet_amd.modules import as_view
    return as_view(t)[0]


def test_lrelu_grad_and_channel_sums(go):
    y, dy = rnd((2, 5, 7, 16), 1), rnd((2, 5, 7, 16), 2)
    gy, gdy = gpu(y), gpu(dy)
    go.lrelu_grad_(V(gy), V(gdy))
    close(gdy, dy * np.where(y > 0, 1.0, 0.1))
    out = torch.zeros(16, device="cuda")
    go.channel_sums(V(gdy), out, gdy.device)
    close(out, gdy.cpu().numpy().reshape(-1, 16).sum(0), rel=1e-5)
    # fused form, awkward channel counts and pixel counts
    for (n, h, w, c) in [(2, 33, 47, 96), (1, 7, 16, 192), (3, 20, 31, 2), (1, 64, 64, 300)]:
        y2, d2 = rnd((n, h, w, c), 3 + c), rnd((n, h, w, c), 4 + c)
        g2y, g2d = gpu(y2), gpu(d2)
        o2 = torch.zeros(c, device="cuda")
        go.lrelu_grad_channel_sums_(V(g2y), V(g2d), o2, g2d.device)
        exp = d2 * np.where(y2 > 0, 1.0, 0.1)
        close(g2d, exp)
        close(o2, exp.reshape(-1, c).astype(np.float64).sum(0), rel=2e-5)


@pytest.mark.parametrize("k", [2, 4])
def test_resize_grad(go, k):
    x = rnd((2, 5, 6, 8), 3)
    dy = rnd((2, 5 * k, 6 * k, 8), 4)
    xt = t64(x)
    (tr.resize_legacy(xt, (5 * k, 6 * k)) * t64(dy, False)).sum().backward()
    dx = torch.zeros((2, 5, 6, 8), device="cuda")
    gdy = gpu(dy)                       # (Views do not own memory: keep every tensor alive in a variable)
    go.resize_grad(V(gdy), V(dx))
    close(dx, xt.grad)
    go.resize_grad(V(gdy), V(dx), mul=0.5, accumulate=True)
    close(dx, 1.5 * xt.grad)


def test_warp_grad(go):
    N, H, W, C = 2, 12, 20, 8
    x, dy = rnd((N, H, W, C), 5), rnd((N, H, W, C), 6)
    flow = util.flow_field(N, H, W, seed=7, sigma=2.0) + 0.137     # keep away from exact integers
    scale = 1.25
    xt, ft = t64(x), t64(flow)
    (tr.bilinear_warp(xt, ft * scale) * t64(dy, False)).sum().backward()
    dx = torch.zeros((N, H, W, C), device="cuda")
    dfl = torch.zeros((N, H, W, 2), device="cuda")
    gx, gfl, gdy = gpu(x), gpu(flow), gpu(dy)
    go.warp_grad(V(gx), V(gfl), scale, V(gdy), V(dx), V(dfl))
    close(dx, xt.grad, rel=1e-5)
    close(dfl, ft.grad, rel=1e-4)


def test_warp_grad_is_bit_reproducible(go):
    """Hundreds of source pixels collapse onto a few corners (a flow field that points at one spot): the default
    scatter (64-bit fixed-point integer atomics) gives the same bits on every run and matches autograd; it also
    accumulates into a non-zero dx."""
    N, H, W, C = 2, 40, 56, 32
    x, dy = rnd((N, H, W, C), 15), rnd((N, H, W, C), 16)
    gy, gx_ = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    flow = np.stack([(20.3 - gx_) * 0.97, (17.6 - gy) * 0.97], axis=2)[None].repeat(N, 0).astype(np.float32)
    flow += rnd((N, H, W, 2), 17) * 0.3
    xt, ft = t64(x), t64(flow)
    (tr.bilinear_warp(xt, ft) * t64(dy, False)).sum().backward()
    gx, gfl, gdy = gpu(x), gpu(flow), gpu(dy)
    outs = []
    for _ in range(4):
        dx = torch.zeros((N, H, W, C), device="cuda")
        go.warp_grad(V(gx), V(gfl), 1.0, V(gdy), V(dx), None)
        torch.cuda.synchronize()
        outs.append(dx.clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    close(outs[0], xt.grad, rel=1e-5)
    base = gpu(rnd((N, H, W, C), 18))
    dx = base.clone()
    go.warp_grad(V(gx), V(gfl), 1.0, V(gdy), V(dx), None)
    close(dx - base, xt.grad, rel=2e-5)      # (fp32 cancellation of the base in dx - base)
    dxa = torch.zeros((N, H, W, C), device="cuda")
    go.warp_grad(V(gx), V(gfl), 1.0, V(gdy), V(dxa), None, deterministic=False)      # fp32 atomics: same sums up to order
    close(dxa, xt.grad, rel=1e-5)


def test_warp_grad_deterministic_form_does_not_hide_divergence(go):
    """the fixed-point scatter maps NaN to 0 and saturates Inf -- a non-finite (or > 2^26) upstream gradient
    must come out as NaN in dx, not as finite numbers."""
    N, H, W, C = 1, 12, 20, 8
    rs = np.random.RandomState(3)
    x, dy = rs.randn(N, H, W, C).astype(np.float32), rs.randn(N, H, W, C).astype(np.float32)
    fl = (rs.randn(N, H, W, 2) * 2).astype(np.float32)
    for bad in (np.nan, np.inf, 1e9):
        d = dy.copy(); d[0, 5, 7, 3] = bad
        gx, gfl, gdy = gpu(x), gpu(fl), gpu(d)
        dx = torch.zeros((N, H, W, C), device="cuda")
        go.warp_grad(V(gx), V(gfl), 1.0, V(gdy), V(dx), None)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx).all()), bad
    gx, gfl, gdy = gpu(x), gpu(fl), gpu(dy)
    dx = torch.zeros((N, H, W, C), device="cuda")
    go.warp_grad(V(gx), V(gfl), 1.0, V(gdy), V(dx), None)
    assert bool(torch.isfinite(dx).all())


def test_train_step_is_bit_reproducible():
    """Two trainers from the same weights on the same batch: identical losses and identical parameters after 3 steps
    (fixed-order reductions everywhere, integer atomics in the warp gradient)."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from pwcnet_amd.train import Trainer
    N, H, W = 2, 64, 128
    w = util.model_weights(False, gain=1.25)
    im0, im1 = util.smooth_images(N, H, W, seed=71, shift=(3, -2))
    gt = util.flow_field(N, H, W, seed=72, sigma=2.0, outliers=False).astype(np.float32)
    g0, g1, ggt = gpu(im0), gpu(im1), gpu(gt)
    runs = []
    for _ in range(2):
        tn = Trainer(weights=(0.32, 0.08, 0.02, 0.01, 0.005), gamma=4e-4, lr=1e-3)
        tn.load_weights(w)
        losses = [float(tn.step(g0, g1, ggt)) for _ in range(3)]
        runs.append((losses, tn.state_dict()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert np.array_equal(np.asarray(runs[0][1][k]), np.asarray(runs[1][1][k])), k


@pytest.mark.parametrize("N,H,W,C", [(1, 9, 11, 8), (2, 16, 24, 32), (1, 8, 8, 20)])
def test_cost_volume_grad(go, N, H, W, C):
    f0, f1, dcv = rnd((N, H, W, C), 8), rnd((N, H, W, C), 9), rnd((N, H, W, 81), 10)
    a, b = t64(f0), t64(f1)
    cv = tr.cost_volume(a, b)
    (cv * t64(dcv, False)).sum().backward()
    df0 = torch.zeros((N, H, W, C), device="cuda")
    df1 = torch.zeros((N, H, W, C), device="cuda")
    g0, g1, gcv, gdcv = gpu(f0), gpu(f1), gpu(cv.detach().numpy()), gpu(dcv)
    go.cost_volume_grad(V(g0), V(g1), V(gcv), V(gdcv), V(df0), V(df1))
    close(df0, a.grad)
    close(df1, b.grad)
    # cv / dcv as 16-byte aligned slices of wider buffers (the estimator layouts): the float4 path
    wcv = torch.zeros((N, H, W, 96), device="cuda"); wcv[..., 4:85] = gcv
    wd = torch.zeros((N, H, W, 100), device="cuda"); wd[..., 8:89] = gdcv
    vcv = View(wcv.data_ptr() + 16, 96, N, H, W, 81)
    vd = View(wd.data_ptr() + 32, 100, N, H, W, 81)
    df0b = torch.zeros((N, H, W, C), device="cuda")
    df1b = torch.zeros((N, H, W, C), device="cuda")
    go.cost_volume_grad(V(g0), V(g1), vcv, vd, V(df0b), V(df1b))
    assert torch.equal(df0b, df0) and torch.equal(df1b, df1)


def test_flow_norm_grad(go):
    N, H, W = 2, 16, 24
    pred, gt = rnd((N, 4, 6, 2), 11), rnd((N, H, W, 2), 12) * 20
    pt = t64(pred)
    loss = 0.32 * tr.L2loss(tr.resize_nearest(t64(gt, False) / 20.0, (4, 6)), pt)
    loss.backward()
    dp = torch.zeros((N, 4, 6, 2), device="cuda")
    gpred, ggt = gpu(pred), gpu(gt)
    go.flow_norm_grad(V(gpred), V(ggt), V(dp), gt_div=20.0, ord=2, scale=0.32 / N)
    close(dp, pt.grad)


@pytest.mark.parametrize("stride,dil,H,W,cin,cout", [
    (1, 1, 12, 16, 16, 32), (1, 1, 9, 11, 48, 16), (2, 1, 12, 16, 3, 16), (2, 1, 8, 8, 32, 64),
    (1, 4, 16, 16, 64, 64), (1, 1, 6, 10, 160, 128), (1, 1, 7, 9, 32, 2), (1, 16, 20, 36, 96, 64)])
def test_conv_wgrad_and_dgrad(go, stride, dil, H, W, cin, cout):
    N = 2
    x, k, b = rnd((N, H, W, cin), 13), rnd((3, 3, cin, cout), 14) * 0.2, rnd((cout,), 15)
    Ho, Wo = -(-H // stride), -(-W // stride)
    dy = rnd((N, Ho, Wo, cout), 16)
    xt, kt, bt = t64(x), t64(k), t64(b)
    (tr.conv3x3_same(xt, kt, bt, stride, dil) * t64(dy, False)).sum().backward()
    gx, gdy = gpu(x), gpu(dy)
    dw = torch.zeros((3, 3, cin, cout), device="cuda")
    go.conv3x3_wgrad(V(gx), V(gdy), dw, cin, stride, dil)
    close(dw, kt.grad, rel=3e-5)
    db = torch.zeros((cout,), device="cuda")
    go.channel_sums(V(gdy), db, gdy.device)
    close(db, bt.grad, rel=1e-5)
    if cin % 4 == 0:
        dx = torch.zeros((N, H, W, cin), device="cuda")
        gk = gpu(k)
        keep = []
        go.conv3x3_dgrad(V(gdy), gk, V(dx), stride, dil, keep=keep, dy_tensor=gdy)
        torch.cuda.synchronize()
        close(dx, xt.grad, rel=3e-5)


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e-8])
def test_conv_dgrad_of_small_gradients(go, scale):
    """upstream gradients of 1e-6 .. 1e-8 (what a multiscale loss averaged over a batch hands to the deep layers) at a
    shape the F16-pipe kernel would take (8 x 56 x 128, 128 -> 128).  The data gradient runs on the fp32 kernels by default
    (grad_ops.F16X2_DGRAD = False) and meets a float64 convolution at fp32 accuracy at every scale; with the split kernel
    switched on the error grows as the scale falls (the fp16 pairs leave the normal range): recorded, not asserted to be small."""
    N, H, W, cin, cout = 8, 56, 128, 128, 128
    k = rnd((3, 3, cin, cout), 24) * 0.05
    dy = rnd((N, H, W, cout), 26) * scale
    wt = np.flip(k, (0, 1)).transpose(0, 1, 3, 2).copy()
    ref = tr.conv3x3_same(t64(dy[:1], False), t64(wt, False), None, 1, 1).numpy()
    gdy, gk = gpu(dy), gpu(k)
    errs = {}
    for flag in (False, True):
        go.F16X2_DGRAD = flag
        try:
            dx = torch.zeros((N, H, W, cin), device="cuda")
            go.conv3x3_dgrad(V(gdy), gk, V(dx), 1, 1, keep=[], dy_tensor=gdy)
            torch.cuda.synchronize()
        finally:
            go.F16X2_DGRAD = False
        errs[flag] = float(np.abs(dx[:1].double().cpu().numpy() - ref).max()) / float(np.abs(ref).max())
    print(f"dgrad at |dy| ~ {scale:g}: relative error fp32 kernels {errs[False]:.2e}, F16-pipe split {errs[True]:.2e}")
    assert errs[False] <= 3e-5, errs
    if scale == 1.0:
        assert errs[True] <= 3e-5, errs


@pytest.mark.parametrize("N,dil,H,W,cin,cout", [
    (2, 1, 64, 128, 128, 128), (2, 4, 64, 128, 96, 64), (4, 1, 50, 70, 40, 36), (1, 16, 112, 256, 96, 64),
    (2, 2, 33, 47, 64, 100), (3, 1, 28, 64, 160, 32), (8, 8, 24, 20, 32, 32), (2, 1, 96, 160, 16, 16), (1, 1, 130, 77, 16, 16), (1, 1, 32, 64, 2112, 64)])
def test_conv_wgrad_lds_staged_kernel(go, N, dil, H, W, cin, cout):
    """Shapes the LDS-staged weight-gradient kernel takes (stride 1, >= 32 channels, enough 64-pixel tiles): full and
    ragged tiles, every tile shape (64x1 ... 8x8), dilation sub-lattices that do not divide the image."""
    x, dy = rnd((N, H, W, cin), 23), rnd((N, H, W, cout), 24)
    xt = t64(x, False)
    kt = torch.zeros((3, 3, cin, cout), dtype=torch.float64, requires_grad=True)
    (tr.conv3x3_same(xt, kt, torch.zeros(cout, dtype=torch.float64), 1, dil) * t64(dy, False)).sum().backward()
    gx, gdy = gpu(x), gpu(dy)
    dw = torch.full((3, 3, cin, cout), 7.0, device="cuda")
    go.conv3x3_wgrad(V(gx), V(gdy), dw, cin, 1, dil)
    close(dw, kt.grad, rel=3e-5)
    # fixed summation order (k-split partials, pixel parts): bit-identical on every run
    for _ in range(3):
        again = torch.full((3, 3, cin, cout), -3.0, device="cuda")
        go.conv3x3_wgrad(V(gx), V(gdy), again, cin, 1, dil)
        assert torch.equal(again, dw)
    # strided views (the dense-connection buffers): x and dy as channel slices of wider tensors
    if cin % 8 == 0:
        wide_x = torch.zeros((N, H, W, cin + 16), device="cuda"); wide_x[..., 8:8 + cin] = gx
        wide_d = torch.zeros((N, H, W, cout + 8), device="cuda"); wide_d[..., 4:4 + cout] = gdy
        vx = View(wide_x.data_ptr() + 32, cin + 16, N, H, W, cin)
        vd = View(wide_d.data_ptr() + 16, cout + 8, N, H, W, cout)
        dw2 = torch.zeros((3, 3, cin, cout), device="cuda")
        go.conv3x3_wgrad(vx, vd, dw2, cin, 1, dil)
        close(dw2, kt.grad, rel=3e-5)


def test_conv_wgrad_with_channel_map(go):
    """input in a padded physical layout (ChannelLayout): gradient comes back in the variable's logical order."""
    N, H, W = 1, 10, 12
    phys2log = np.array([0, 1, 2, -1, 3, 4, 5, 6, 7, 8, -1, -1, 9, 10, -1, -1], np.int32)    # 11 logical in 16 physical
    xl = rnd((N, H, W, 11), 17)
    xp = np.zeros((N, H, W, 16), np.float32)
    xp[..., phys2log >= 0] = xl[..., phys2log[phys2log >= 0]]
    k, dy = rnd((3, 3, 11, 32), 18), rnd((N, H, W, 32), 19)
    xt, kt = t64(xl), t64(k)
    (tr.conv3x3_same(xt, kt, torch.zeros(32, dtype=torch.float64)) * t64(dy, False)).sum().backward()
    dw = torch.zeros((3, 3, 11, 32), device="cuda")
    gxp, gdy, gmap = gpu(xp), gpu(dy), torch.from_numpy(phys2log).cuda()
    go.conv3x3_wgrad(V(gxp), V(gdy), dw, 11, 1, 1, cin_map=gmap)
    close(dw, kt.grad, rel=3e-5)


def test_adam_step(go):
    n = 1000
    p, g = rnd((n,), 20), rnd((n,), 21)
    m, v = np.abs(rnd((n,), 22)) * 0.1, np.abs(rnd((n,), 23)) * 0.01
    gp, gg, gm, gv = gpu(p), gpu(g), gpu(m), gpu(v)
    import math
    step, lr, gamma = 7, 1e-4, 4e-4
    lr_t = lr * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
    go.adam_step_(gp, gg, gm, gv, lr_t, l2_gamma=gamma)
    pt, mt, vt = tr.adam_step(t64(p, False), t64(g, False) + gamma * t64(p, False), t64(m, False), t64(v, False), step, lr)
    close(gp, pt, rel=1e-6)
    close(gm, mt, rel=1e-6)
    close(gv, vt, rel=3e-6)


# ------------------------------------------------------------------ assembled training step
LOSS_WEIGHTS = (0.32, 0.08, 0.02, 0.01, 0.005)

# (N, H, W) -> (kernel gain, image seed, gt seed, image shift) of the step tests' inputs
_STEP_INPUTS = {
    (2, 64, 128): (1.25, 61, 62, (3, -2)),
    (4, 384, 448): (1.2, 91, 92, (4, -3)),
    (1, 448, 1024): (1.2, 81, 82, (4, -3)),
}

# Bounds of the step tests: (gradient, pyramid, loss), each relative to the reference's largest magnitude -- the gradient
# bound per variable.  Every bound is max(10 x the worst error measured on an MI355X, 1e-5), rounded up to two digits and
# capped at 1e-4 (64x128) / 6.5e-4 (448x1024); the comments give the measured worst gradient error and its variable.
# Key: (use_dc, loss, (N, H, W), f16x2).
STEP_BOUNDS = {
    (False, "multiscale", (2, 64, 128), True): (1e-5, 1e-5, 1e-5),       # 7.5e-7 fp_extractor/conv2d_9/kernel
    (True, "multiscale", (2, 64, 128), True): (1e-5, 1.6e-5, 1e-5),      # 8.9e-7 fp_extractor/conv2d_3/kernel
    (False, "robust", (2, 64, 128), True): (1.8e-5, 1e-5, 1e-5),         # 1.75e-6 fp_extractor/conv2d/bias
    (True, "robust", (2, 64, 128), True): (1e-5, 1.6e-5, 1e-5),          # 8.8e-7 fp_extractor/conv2d_3/kernel
    (False, "multiscale", (2, 64, 128), False): (1e-5, 1e-5, 1e-5),      # 7.5e-7 fp_extractor/conv2d_9/kernel
    (False, "multiscale", (4, 384, 448), True): (3.7e-4, 1.4e-5, 1e-5),  # 3.7e-5 fp_extractor/conv2d/bias (sign-following)
    (False, "multiscale", (4, 384, 448), False): (1.2e-4, 1.5e-5, 1e-5),  # 1.2e-5 context/conv2d/bias (sign-following)
    (False, "multiscale", (1, 448, 1024), True): (6.5e-4, 1.7e-5, 1e-5),  # 7.3e-5 fp_extractor/conv2d/kernel (cap)
}
# the first Adam step's gradients (64x64, batch 2, constant gt): same rule (7.5e-7 fp_extractor/conv2d/kernel)
ADAM_STEP_GRAD_BOUND = 1e-5


def _ref_grads(w, im0, im1, gt, weights, use_dc=False, loss="multiscale"):
    wt = {k: t64(v) for k, v in w.items()}
    _, pyr = tr.TorchPWCDCNet(wt, use_dc=use_dc)(t64(im0, False), t64(im1, False))
    if loss == "multiscale":
        loss = tr.multiscale_loss(t64(gt, False), pyr, weights)
    else:
        loss = tr.multirobust_loss(t64(gt, False), pyr, weights, epsilon=0.02, q=0.4)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in wt.items()}, [p.detach() for p in pyr]


@pytest.fixture(scope="module")
def step_ref():
    """The float64 autograd reference of one training step, computed once per module and shared by the tests below:
    step_ref(use_dc, loss, (N, H, W)) -> dict of the inputs, the loss, the pyramid, every variable's gradient and the
    CPU seconds the reference took."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    cache = {}

    def get(use_dc, loss, shape):
        key = (use_dc, loss, shape)
        if key not in cache:
            gain, s_im, s_gt, shift = _STEP_INPUTS[shape]
            N, H, W = shape
            w = util.model_weights(use_dc, gain=gain)
            im0, im1 = util.smooth_images(N, H, W, seed=s_im, shift=shift)
            gt = util.flow_field(N, H, W, seed=s_gt, sigma=2.0, outliers=False).astype(np.float32)
            t0 = time.perf_counter()
            ref_loss, ref_g, ref_pyr = _ref_grads(w, im0, im1, gt, LOSS_WEIGHTS, use_dc, loss)
            cache[key] = dict(w=w, im0=im0, im1=im1, gt=gt, loss=ref_loss, grads=ref_g, pyr=ref_pyr,
                              cpu_s=time.perf_counter() - t0, threads=torch.get_num_threads())
        return cache[key]
    return get


def _rel_err(got, ref):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-12)


def _run_step(ref, use_dc=False, loss="multiscale", f16x2=True):
    """One Trainer forward + backward on ref's inputs: (trainer, worst pyramid level error, loss error, gradients), the
    errors relative to the reference's largest magnitude."""
    from pwcnet_amd.train import Trainer
    tn = Trainer(weights=LOSS_WEIGHTS, gamma=0.0, lr=1e-4, use_dc=use_dc, loss=loss, epsilon=0.02, q=0.4, f16x2=f16x2)
    tn.load_weights(ref["w"])
    pyr = tn.forward(gpu(ref["im0"]), gpu(ref["im1"]))
    pyr_err = max(_rel_err(a, b) for a, b in zip(pyr, ref["pyr"]))
    ggt = gpu(ref["gt"])
    loss_err = abs(float(tn.loss_value(ggt)) - ref["loss"]) / abs(ref["loss"])
    tn.backward(ggt)
    torch.cuda.synchronize()
    return tn, pyr_err, loss_err, tn.gradients()


def _step_errors(ref, use_dc=False, loss="multiscale", f16x2=True):
    """(worst pyramid level error, loss error, {variable: relative gradient error}) of one Trainer step."""
    _, pyr_err, loss_err, got = _run_step(ref, use_dc, loss, f16x2)
    return pyr_err, loss_err, {k: _rel_err(got[k], r) for k, r in ref["grads"].items()}


class _SignFollowingNet(tr.TorchPWCDCNet):
    """The float64 restatement, except that every extractor leaky-relu takes the branch the given fp32 activations took
    (signs[k]: (2N, h, w, c) booleans of extractor conv k, both frames stacked as the Trainer stacks them).  Counts the
    elements where that differs from the float64 pre-activation's own sign in self.flips[k]."""

    def __init__(self, weights, signs, N):
        super().__init__(weights)
        self.signs, self.N, self.frame, self.flips = signs, N, 0, {}

    def extractor(self, images):
        sl = slice(self.frame * self.N, (self.frame + 1) * self.N)
        self.frame += 1
        pyr, x, k = [], images, 0
        for l in range(self.num_levels):
            for j in range(3):
                n = f"{self.name}/fp_extractor/conv2d" + ("" if k == 0 else f"_{k}")
                y = tr.conv3x3_same(x, self.w[n + "/kernel"], self.w[n + "/bias"], 2 if j == 0 else 1)
                pos = self.signs[k][sl]
                self.flips[k] = self.flips.get(k, 0) + int((pos != (y.detach() > 0)).sum())
                x = torch.where(pos, y, 0.1 * y)
                k += 1
            pyr.append(x)
        return pyr[::-1]


def _sign_following_grads(ref, tn):
    """Float64 autograd of the multiscale step with the extractor's leaky-relu branches of tn's forward: {k: gradient},
    {extractor conv: elements whose branch differs from float64's}."""
    N = ref["im0"].shape[0]
    signs = [torch.from_numpy(c.y_t.cpu().numpy() > 0) for c in tn.ext]
    wt = {k: t64(v) for k, v in ref["w"].items()}
    net = _SignFollowingNet(wt, signs, N)
    _, pyr = net(t64(ref["im0"], False), t64(ref["im1"], False))
    tr.multiscale_loss(t64(ref["gt"], False), pyr, LOSS_WEIGHTS).backward()
    return {k: v.grad for k, v in wt.items()}, {k: n for k, n in net.flips.items() if n}


def _report(tag, pyr_err, loss_err, errs):
    ranked = sorted(errs.items(), key=lambda kv: -kv[1])
    print(f"\n[{tag}] pyramid {pyr_err:.2e}, loss {loss_err:.2e}; gradients of {len(ranked)} variables: "
          f"worst {ranked[0][1]:.2e} ({ranked[0][0]}), median {float(np.median(list(errs.values()))):.2e}")
    for k, e in ranked[:4]:
        print(f"    {e:.2e}  {k}")


def _check_step(key, pyr_err, loss_err, errs):
    g_bound, p_bound, l_bound = STEP_BOUNDS[key]
    _report(key, pyr_err, loss_err, errs)
    assert pyr_err <= p_bound, f"pyramid: relative error {pyr_err:.3e} > {p_bound:.1e}"
    assert loss_err <= l_bound, f"loss: relative error {loss_err:.3e} > {l_bound:.1e}"
    bad = {k: f"{e:.3e}" for k, e in errs.items() if e > g_bound}
    assert not bad, f"relative gradient error above {g_bound:.1e}: {bad}"


@pytest.mark.parametrize("use_dc,loss", [(False, "multiscale"), (True, "multiscale"), (False, "robust"), (True, "robust")])
def test_train_step_gradients_vs_autograd(step_ref, use_dc, loss):
    """Whole backward (loss gradient, context, 5 estimators -- plain and densely connected --, cost volumes, warps,
    resizes, shared-weight extractor) against torch.autograd on the float64 restatement: every variable's gradient, at
    the bounds of STEP_BOUNDS."""
    shape = (2, 64, 128)
    _check_step((use_dc, loss, shape, True), *_step_errors(step_ref(use_dc, loss, shape), use_dc, loss))


def test_train_step_gradients_with_the_fp32_forward(step_ref):
    """Trainer(f16x2=False): the training forward on the fp32 convolution kernels instead of the F16-pipe ones (non-DC,
    multiscale, 64x128; the F16-pipe kernels take no layer at this size, so both forwards measure alike here -- the
    384x448 test runs both as well)."""
    shape = (2, 64, 128)
    _check_step((False, "multiscale", shape, False), *_step_errors(step_ref(False, "multiscale", shape), f16x2=False))


@pytest.mark.parametrize("f16x2", [True, False])
def test_train_step_gradients_at_the_cli_crop(step_ref, f16x2):
    """train.py's own geometry: 384x448 crops at its default batch of 4.  The estimator levels are 6x7, 12x14, 24x28,
    48x56 and 96x112: widths 7, 14 and 28 leave ragged 8x8 tiles along W in the cost-volume gradient and ragged
    weight-gradient tiles, which neither 64x128 (powers of two) nor 448x1024 (ragged heights only) reach.  Every variable
    of a non-DC multiscale step against float64 autograd; the float64 reference takes about 4 s on 16 CPU threads (8 s
    on 8), so batch 4 it is.

    Against the plain reference the worst error is 3.8e-4 (fp_extractor/conv2d_7/kernel, then conv2d/kernel 3.5e-4): ONE
    leaky-relu branch differs -- an element of fp_extractor/conv2d_7's output (extractor level 2, 48x56, first frame)
    whose float64 pre-activation is 8.7e-9 against a layer maximum of 0.18, below what fp32 resolves, comes out on the
    other side of zero in the fp32 forward, and its gradient is 10x off.  That is the forward's rounding, not the
    backward's: the bound applies to float64 autograd of the same branches (the extractor's leaky-relus take the fp32
    forward's signs; worst 3.7e-5, fp_extractor/conv2d/bias, with the F16-pipe forward; 1.2e-5, context/conv2d/bias,
    with the fp32 one), and the plain reference's error is reported."""
    shape = (4, 384, 448)
    ref = step_ref(False, "multiscale", shape)
    print(f"\n384x448 batch 4: float64 reference {ref['cpu_s']:.1f} s on {ref['threads']} CPU threads")
    tn, pyr_err, loss_err, got = _run_step(ref, f16x2=f16x2)
    plain = {k: _rel_err(got[k], r) for k, r in ref["grads"].items()}
    _report("384x448 plain reference (not asserted)", pyr_err, loss_err, plain)
    grads, flips = _sign_following_grads(ref, tn)
    print(f"extractor leaky-relu branches that differ from float64 (conv index: elements): {flips}")
    assert sum(flips.values()) <= 16, flips                   # (a wrong forward would differ in many)
    _check_step((False, "multiscale", shape, f16x2), pyr_err, loss_err, {k: _rel_err(got[k], r) for k, r in grads.items()})


def test_train_step_gradients_full_size_spot_check(step_ref):
    """One 448x1024 pair (the geometry `bench.py --mode train` times: LDS-staged weight-gradient tiling with its k-split
    over pixel chunks, Winograd data gradients, full-size cost-volume / warp gradients): every variable against float64
    autograd on the torch restatement.  The worst, 7.3e-5 on fp_extractor/conv2d/kernel (no leaky-relu branch differs
    in the extractor), is fp32 summation over the 229 376 output pixels of the first conv, whose kernel gradient is a
    small difference of large sums; 10x that is above the 6.5e-4 cap, so the cap is the bound."""
    shape = (1, 448, 1024)
    ref = step_ref(False, "multiscale", shape)
    print(f"\n448x1024 batch 1: float64 reference {ref['cpu_s']:.1f} s on {ref['threads']} CPU threads")
    _check_step((False, "multiscale", shape, True), *_step_errors(ref))


def _mutate(case):
    """(name of the grad_ops function, replacement) that perturbs one term of the backward at one level (64x128 step:
    levels 0..4 are 1x2, 2x4, 4x8, 8x16, 16x32)."""
    from pwcnet_amd import grad_ops as G
    from pwcnet_amd.weights import SCALES
    keep = []
    if case == "warp_dflow":
        # (a) the warp's flow gradient at level 4 (flow_scale 5), x 0.9.  At x 0.99 no level moves any variable by more
        # than 3e-6 (dropping that term altogether moves level 2 by 5e-5, levels 3 / 4 by 3e-4): enlarged to 10 %.
        orig = G.warp_grad

        def f(x, flow, flow_scale, dy, dx=None, dflow=None, dflow_accumulate=False, deterministic=True):
            if flow_scale != SCALES[4] or dflow is None:
                return orig(x, flow, flow_scale, dy, dx, dflow, dflow_accumulate, deterministic)
            orig(x, flow, flow_scale, dy, dx, None, deterministic=deterministic)
            t = torch.zeros((flow.N, flow.H, flow.W, 2), device="cuda")
            keep.append(t)
            orig(x, flow, flow_scale, dy, None, V(t))
            G.add_(V(t), dflow, alpha=0.9, accumulate=dflow_accumulate)
        return "warp_grad", f
    if case == "cv_grad":
        # (b) the cost volume's feature gradients at level 3 x 0.99.  (Replaces slope 0.11 in the cost volume's leaky-relu
        # mask, which no step here can see: every in-image cost-volume entry of these inputs is positive at every level
        # -- the entries <= 0 are exactly the zero padding -- so the slope multiplies nothing.  test_gpu_grad_ops.py's
        # sweeps, with features of both signs, pin the slope.)
        orig = G.cost_volume_grad

        def f(f0, f1w, cv, dcv, df0=None, df1w=None, accumulate=False, search_range=4, slope=0.1):
            if f0.H != 8:
                return orig(f0, f1w, cv, dcv, df0, df1w, accumulate, search_range, slope)
            for d, which in ((df0, 0), (df1w, 1)):
                if d is not None:
                    t = torch.zeros((d.N, d.H, d.W, d.C), device="cuda")
                    keep.append(t)
                    orig(f0, f1w, cv, dcv, V(t) if which == 0 else None, V(t) if which == 1 else None, False, search_range, slope)
                    G.add_(V(t), d, alpha=0.99, accumulate=accumulate)
        return "cost_volume_grad", f
    if case == "feat_up_mul":                # (c) level 3's feat_up resize gradient x 0.99
        orig = G.resize_grad

        def f(dy, dx, mul=1.0, accumulate=False):
            return orig(dy, dx, 0.99 * mul if (dy.H == 8 and dy.C > 2) else mul, accumulate)
        return "resize_grad", f
    if case == "flow_norm_scale":            # (d) the loss gradient of level 4 (weight 0.005) x 1.01
        orig = G.flow_norm_grad

        def f(pred, gt, dpred, gt_div=1.0, ord=2, scale=1.0, accumulate=False):
            return orig(pred, gt, dpred, gt_div, ord, 1.01 * scale if pred.H == 16 else scale, accumulate)
        return "flow_norm_grad", f
    if case == "lrelu_slope":                # (e) leaky-relu slope 0.105 in the backward of optflow_3/conv2d_2 (8x16, 96 out)
        orig = G.lrelu_grad_channel_sums_

        def f(y, dy, out, device, slope=0.1, accumulate=False):
            hit = y.N == 2 and y.H == 8 and y.C == 96
            return orig(y, dy, out, device, 0.105 if hit else slope, accumulate)
        return "lrelu_grad_channel_sums_", f
    raise ValueError(case)


@pytest.mark.parametrize("case", ["warp_dflow", "cv_grad", "feat_up_mul", "flow_norm_scale", "lrelu_slope"])
def test_train_step_check_sees_a_one_percent_error(step_ref, monkeypatch, case):
    """The bounds of test_train_step_gradients_vs_autograd are tight enough to see a subtle backward bug: each case
    perturbs one term of one level by about 1 % (10 % for the warp's flow gradient, see _mutate; the Trainer calls the
    grad_ops functions as G.<name> at run time), and the same check must then fail for at least one variable."""
    from pwcnet_amd import grad_ops as G
    key = (False, "multiscale", (2, 64, 128), True)
    ref = step_ref(*key[:3])
    name, fn = _mutate(case)
    monkeypatch.setattr(G, name, fn)
    pyr_err, loss_err, errs = _step_errors(ref)
    _report(f"mutation {case}", pyr_err, loss_err, errs)
    worst = max(errs.values())
    assert worst > STEP_BOUNDS[key][0], f"{case}: worst relative gradient error {worst:.3e} is inside the bound"


def test_train_step_reduces_the_loss_and_matches_adam():
    """A few optimisation steps on one batch: the loss goes down; after the first step every variable equals
    tf.train.AdamOptimizer's formula applied to that step's gradient plus gamma * var, that gradient matches float64
    autograd, the padding floats of the flat buffer stay zero, and three variables also match Adam on the reference
    gradients directly."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from pwcnet_amd.train import Trainer
    N, H, W = 2, 64, 64
    w = util.model_weights(False, gain=1.1)
    im0, im1 = util.smooth_images(N, H, W, seed=63, shift=(2, 1))
    gt = np.zeros((N, H, W, 2), np.float32)
    gt[..., 0], gt[..., 1] = 2.0, 1.0                       # the true motion of smooth_images(shift=(2, 1))
    gamma, lr = 4e-4, 1e-3
    _, ref_g, _ = _ref_grads(w, im0, im1, gt, LOSS_WEIGHTS)
    tn = Trainer(weights=LOSS_WEIGHTS, gamma=gamma, lr=lr)
    tn.load_weights(w)
    g0, g1, ggt = gpu(im0), gpu(im1), gpu(gt)
    losses = [float(tn.step(g0, g1, ggt))]
    after = tn.state_dict()
    got_g = tn.gradients()                                  # the step's gradients (the optimiser does not clear them)
    errs = {k: _rel_err(got_g[k], ref_g[k]) for k in ref_g}
    _report("64x64 first step", 0.0, 0.0, errs)
    bad = {k: f"{e:.3e}" for k, e in errs.items() if e > ADAM_STEP_GRAD_BOUND}
    assert not bad, f"relative gradient error above {ADAM_STEP_GRAD_BOUND:.1e}: {bad}"
    assert sorted(after) == sorted(ref_g)
    for k in sorted(ref_g):
        p = t64(w[k], False)
        g = t64(got_g[k], False) + gamma * p
        exp, _, _ = tr.adam_step(p, g, torch.zeros_like(g), torch.zeros_like(g), 1, lr)
        close(after[k], exp, rel=1e-5)
    used = torch.zeros(tn.params.numel(), dtype=torch.bool)
    for off, shape in tn.views.values():
        used[off:off + int(np.prod(shape))] = True
    assert int(torch.count_nonzero(tn.params.cpu()[~used])) == 0, "padding floats of the flat buffer moved"
    for k in ("pwcdcnet/context/conv2d_6/kernel", "pwcdcnet/optflow_2/conv2d/kernel", "pwcdcnet/fp_extractor/conv2d_4/bias"):
        g = ref_g[k] + gamma * t64(w[k], False)
        exp, _, _ = tr.adam_step(t64(w[k], False), g, torch.zeros_like(g), torch.zeros_like(g), 1, lr)
        close(after[k], exp, rel=1e-4)
    for _ in range(7):
        losses.append(float(tn.step(g0, g1, ggt)))
    print("losses:", [round(x, 4) for x in losses])
    assert tn.global_step == 8 and losses[-1] < 0.9 * losses[0]


@pytest.mark.parametrize("use_dc", [False, True])
def test_trainer_forward_equals_inference_forward(use_dc):
    """The training forward (activations kept, weights from the flat buffer) and PWCDCNet.__call__ are the same
    function, with and without dense connections."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import pwcnet_amd
    from pwcnet_amd.train import Trainer, piecewise_lr
    w = util.model_weights(use_dc)
    im0, im1 = util.smooth_images(2, 64, 128, seed=64)
    tn = Trainer(use_dc=use_dc)
    tn.load_weights(w)
    pyr = tn.forward(gpu(im0), gpu(im1))
    net = pwcnet_amd.PWCDCNet(use_dc=use_dc)
    net.load_weights(w)
    _, ref = net(gpu(im0), gpu(im1))
    for a, b in zip(pyr, ref):
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))
    with pytest.raises(ValueError, match="missing"):
        tn.load_weights({})
    # reference train.py:82-88
    assert piecewise_lr(1e-4, 0) == 1e-4 and piecewise_lr(1e-4, 200000) == 1e-4 and piecewise_lr(1e-4, 200001) == 5e-5
    assert piecewise_lr(1e-4, 360000) == 1e-4 / 16 and piecewise_lr(1e-4, 360000, scheduling=False) == 1e-4


@pytest.mark.parametrize("extra,use_dc", [((), False), (("--use-dc", "--loss", "robust"), True)])
def test_train_cli_synthetic_epoch_writes_a_restorable_bundle(tmp_path, extra, use_dc):
    """train.py (counterpart of the reference's train.py): two short epochs on synthetic translating textures;
    every epoch prints loss / validation EPE and writes a TF-format bundle that PWCDCNet can restore."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import os, subprocess, sys
    import pwcnet_amd
    from pwcnet_amd import ckpt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "train.py"), "-d", "synthetic", "--synthetic_pairs", "20",
                          "-e", "2", "-b", "4", "--crop_shape", "64", "128", "--lr", "3e-4", "--model_dir", str(tmp_path / "model"), *extra],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 2 and "EPE/val" in lines[0] and "global_step 8" in lines[1], out.stdout[-1500:]
    w = ckpt.load_weights(str(tmp_path / "model" / "model_2.ckpt"))
    net = pwcnet_amd.PWCDCNet(use_dc=use_dc)
    net.load_weights(w)
    im0, im1 = util.smooth_images(1, 64, 128, seed=65)
    final, _ = net(gpu(im0), gpu(im1))
    assert torch.isfinite(final).all()
