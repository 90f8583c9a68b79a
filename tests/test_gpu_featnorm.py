"""Cost-volume feature normalisation on the GPU (pwc_featnorm.hip, FeatureNormLayer, PWCDCNet / Trainer / PWCDCNetModule /
ForwardPipeline with normalize_features=True, train.py --normalize_features) against the float64 restatement of
tests/featnorm_ref.py.

Forward bound, per element: |got - ref| <= 2^-24 |ref| + 2^-40 (1 + |mean| rstd).
  The kernel forms y = ((double)x - mean) * rstd in doubles and rounds it once to float32: half an ulp, at most 2^-24 |y|.  What is
  left is the difference between the kernel's double y and the restatement's.  Both take their moments from sums of M <= 2^17
  doubles in some order: mean carries a relative error of a few 2^-53 log2 M, i.e. an absolute error of y of that times
  |mean| rstd; rstd carries the variance's -- the shifted one-pass variance loses (|mean - K| rstd)^2 ulps, K a sample of the pair,
  a few hundred ulps = 2^-45 at most for the inputs here -- times |y| <= 2^3.  2^-40 (1 + |mean| rstd) is 2^5 above either, and
  2^-16 of the float32 rounding it stands beside: a kernel that took its moments in float32, or the variance from unshifted
  sums at |mean| rstd = 2^10 (an error of rstd of 2^-33 to 2^-31 relative), does not pass.
Backward bound, per element: |got - ref| <= 2^-23 A, A = |rstd g| + |rstd a| + |rstd xh b| (the splat tests' rule): every term is a
  double, the sum is rounded once (2^-24 |d| <= 2^-24 A), the sums a and b differ from the restatement's by summation order only.
Model bounds: flows_final within 1e-3 px of the float64 model (the project's parity tolerance); gradients at the bounds
  tests/test_gpu_grad.py and tests/test_gpu_autograd.py assert for the un-normalised model on the same weights and frames.
Measured figures: profiles/featnorm_gpu_test_figures.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import featnorm_ref as R
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w, C) at N = 2: level 0 of a 64 x 128 frame (one workgroup); odd extents with a tail; the scalar path; several workgroups per
# pair and the second reduction stage (16 and 56 parts); the scalar path with several workgroups and a last group of one value
SHAPES = [(1, 2, 192), (5, 7, 16), (3, 5, 3), (16, 32, 32), (28, 64, 32), (9, 31, 15)]


@pytest.fixture(scope="module")
def fn():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd.modules import FeatureNormLayer
    return FeatureNormLayer


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def V(t):
    from pwcnet_amd.modules import as_view
    return as_view(t)[0]


def _inputs(shape, kind, seed):
    """(f0, f1) float32 numpy, (N, h, w, C).  "lrelu": |mean| rstd about 1.  "shifted": moved so that |mean| rstd = 2^10."""
    f0, f1 = R.lrelu_maps(shape, seed)
    if kind == "shifted":
        both = np.concatenate([f0.reshape(shape[0], -1), f1.reshape(shape[0], -1)], axis=1).astype(np.float64)
        s = (1024.0 * both.std(axis=1) - both.mean(axis=1)).astype(np.float32).reshape(-1, 1, 1, 1)      # per pair
        f0, f1 = (f0 + s).astype(np.float32), (f1 + s).astype(np.float32)
    return f0, f1


def _forward_check(tag, got0, got1, f0, f1, eps=R.EPS):
    y0, y1, mean, rstd = R.feature_norm_np(f0, f1, eps)
    worst, mr = 0.0, float(np.abs(mean * rstd).max())
    for got, ref in ((got0, y0), (got1, y1)):
        got = got.detach().cpu().double().numpy()
        tol = 2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * (1.0 + np.abs(mean * rstd)).reshape(-1, 1, 1, 1)
        err = np.abs(got - ref)
        worst = max(worst, float((err / tol).max()))
    print(f"featnorm forward {tag}: |mean| rstd {mr:.4g}, worst error / bound {worst:.3f}")
    assert worst <= 1.0, (tag, worst)
    return mean, rstd


def _run(fn, g0, g1, eps=R.EPS):
    y0, y1, stats = fn(eps)(g0, g1, with_stats=True)
    torch.cuda.synchronize()
    return y0, y1, stats


@pytest.mark.parametrize("kind", ["lrelu", "shifted"])
@pytest.mark.parametrize("h,w,C", SHAPES)
def test_forward_against_float64(fn, h, w, C, kind):
    f0, f1 = _inputs((2, h, w, C), kind, seed=h * 1000 + C)
    y0, y1, stats = _run(fn, gpu(f0), gpu(f1))
    mean, rstd = _forward_check(f"{h}x{w}x{C} {kind}", y0, y1, f0, f1)
    if kind == "shifted":
        assert 1000.0 <= float(np.abs(mean * rstd).min()) <= 1050.0
    st = stats.cpu().numpy()
    assert np.abs(st[:, 0] - mean).max() <= 2.0 ** -40 * np.abs(mean).max() and np.abs(st[:, 1] / rstd - 1).max() <= 2.0 ** -30


@pytest.mark.parametrize("h,w,C", SHAPES)
def test_forward_on_the_shared_frame_view(fn, h, w, C):
    """f1 is f0 plus one frame of an N + 1 tensor (PWCDCNet's sequence path): pair n is frames n and n + 1."""
    from pwcnet_amd.modules import View
    N = 2
    frames = R.lrelu_maps((N + 1, h, w, C), seed=77 + C)[0]
    t = gpu(frames)
    y = torch.empty((2, N, h, w, C), device="cuda")
    stats = torch.empty((N, 2), dtype=torch.float64, device="cuda")
    layer = fn()
    ws = layer.workspace(N, h, w, C, "cuda")
    layer._run(View(t.data_ptr(), C, N, h, w, C), View(t.data_ptr() + 4 * h * w * C, C, N, h, w, C), V(y[0]), V(y[1]), stats, ws)
    torch.cuda.synchronize()
    _forward_check(f"{h}x{w}x{C} shared frames", y[0], y[1], frames[:N], frames[1:])
    a0, a1, _ = _run(fn, t[:N].clone(), t[1:].clone())
    assert torch.equal(a0, y[0]) and torch.equal(a1, y[1])


@pytest.mark.parametrize("C,cs", [(32, 48), (16, 18), (6, 8)])
def test_forward_on_channel_slices(fn, C, cs):
    """Maps that are channel slices of wider buffers: 16-byte path (stride 48), scalar path by stride (18) and by C (6) -- the
    same bits as dense maps (the order of the sums does not depend on how a group is fetched)."""
    N, h, w = 2, 20, 33
    f0, f1 = _inputs((N, h, w, C), "lrelu", seed=cs)
    wide = torch.full((2, N, h, w, cs), 7.0, device="cuda")
    wide[0, ..., :C], wide[1, ..., :C] = gpu(f0), gpu(f1)
    out = torch.full((2, N, h, w, cs), -3.0, device="cuda")
    a0, a1, _ = _run(fn, wide[0, ..., :C], wide[1, ..., :C])             # (as_view keeps a pixel-dense slice where it is)
    _forward_check(f"slices C {C} stride {cs}", a0, a1, f0, f1)
    b0, b1, _ = _run(fn, gpu(f0), gpu(f1))
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    from pwcnet_amd.modules import View
    stats = torch.empty((N, 2), dtype=torch.float64, device="cuda")
    layer = fn()
    layer._run(V(wide[0, ..., :C]), V(wide[1, ..., :C]), View(out[0].data_ptr(), cs, N, h, w, C), View(out[1].data_ptr(), cs, N, h, w, C),
               stats, layer.workspace(N, h, w, C, "cuda"))
    torch.cuda.synchronize()
    assert torch.equal(out[0, ..., :C], b0) and torch.equal(out[1, ..., :C], b1)
    assert bool((out[..., C:] == -3.0).all())                              # nothing is written behind the channels


@pytest.mark.parametrize("h,w,C", SHAPES)
def test_backward_against_autograd(fn, h, w, C):
    from pwcnet_amd import grad_ops as G
    N = 2
    f0, f1 = _inputs((N, h, w, C), "lrelu", seed=h * 100 + C)
    g0, g1 = R.lrelu_maps((N, h, w, C), seed=h * 100 + C + 1, shift=-0.3)
    r0, r1, A0, A1 = R.feature_norm_grads(f0, f1, g0, g1)
    t0, t1, u0, u1 = gpu(f0), gpu(f1), gpu(g0), gpu(g1)
    _, _, stats = _run(fn, t0, t1)
    d = torch.full((2, N, h, w, C), 9.0, device="cuda")
    G.feature_norm_grad(V(t0), V(t1), V(u0), V(u1), stats, V(d[0]), V(d[1]))
    torch.cuda.synchronize()
    worst = 0.0
    for got, ref, A in ((d[0], r0, A0), (d[1], r1, A1)):
        worst = max(worst, float((np.abs(got.cpu().double().numpy() - ref) / (2.0 ** -23 * A)).max()))
    print(f"featnorm backward {h}x{w}x{C}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst
    # accumulate adds exactly what the plain call writes; two calls give the same bits
    base = gpu(R.lrelu_maps((2 * N, h, w, C), seed=5)[0]).view(2, N, h, w, C)
    acc = base.clone()
    G.feature_norm_grad(V(t0), V(t1), V(u0), V(u1), stats, V(acc[0]), V(acc[1]), accumulate=True)
    again = torch.empty_like(d)
    G.feature_norm_grad(V(t0), V(t1), V(u0), V(u1), stats, V(again[0]), V(again[1]))
    torch.cuda.synchronize()
    assert torch.equal(acc, base + d) and torch.equal(again, d)


@pytest.mark.parametrize("h,w,C", SHAPES)
def test_exactness(fn, h, w, C):
    """What needs no tolerance: a batch against its images run singly, two calls, the scale (norm_eps = 0), a constant pair, a NaN."""
    from pwcnet_amd import grad_ops as G
    N = 2
    f0, f1 = _inputs((N, h, w, C), "lrelu", seed=h + 31 * C)
    t0, t1 = gpu(f0), gpu(f1)
    y0, y1, stats = _run(fn, t0, t1)
    z0, z1, stats2 = _run(fn, t0, t1)
    assert torch.equal(y0, z0) and torch.equal(y1, z1) and torch.equal(stats, stats2)
    g = gpu(R.lrelu_maps((2 * N, h, w, C), seed=9)[0])
    d = torch.empty((2, N, h, w, C), device="cuda")
    G.feature_norm_grad(V(t0), V(t1), V(g[:N]), V(g[N:]), stats, V(d[0]), V(d[1]))
    for n in range(N):
        s0, s1, st = _run(fn, t0[n:n + 1].clone(), t1[n:n + 1].clone())
        assert torch.equal(s0[0], y0[n]) and torch.equal(s1[0], y1[n]) and torch.equal(st[0], stats[n])
        ds = torch.empty((2, 1, h, w, C), device="cuda")
        G.feature_norm_grad(V(t0[n:n + 1]), V(t1[n:n + 1]), V(g[n:n + 1]), V(g[N + n:N + n + 1]), st, V(ds[0]), V(ds[1]))
        torch.cuda.synchronize()
        assert torch.equal(ds[0, 0], d[0, n]) and torch.equal(ds[1, 0], d[1, n])
    # norm_eps = 0: x and 4 x normalise to the same bits
    a0, a1, _ = _run(fn, t0, t1, eps=0.0)
    b0, b1, _ = _run(fn, 4.0 * t0, 4.0 * t1, eps=0.0)
    assert torch.equal(a0, b0) and torch.equal(a1, b1) and bool(torch.isfinite(a0).all())
    # a constant pair gives zeros (the default eps keeps rstd finite)
    c = torch.full((N, h, w, C), 0.1, device="cuda")
    c0, c1, cst = _run(fn, c, c.clone())
    assert not bool(c0.any()) and not bool(c1.any()) and float(cst[0, 0]) == float(np.float32(0.1)) and float(cst[0, 1]) == 1e8
    # a NaN in pair 0 stays in pair 0
    bad = t1.clone()
    bad[0, h // 2, w // 2, C // 2] = float("nan")
    n0, n1, _ = _run(fn, t0, bad)
    assert bool(torch.isnan(n0[0]).all()) and bool(torch.isnan(n1[0]).all())
    assert torch.equal(n0[1], y0[1]) and torch.equal(n1[1], y1[1])


# ------------------------------------------------------------------ model forward
def _net(use_dc, w, attrs=None, **kw):
    import pwcnet_amd
    net = pwcnet_amd.PWCDCNet(use_dc=use_dc, **kw)
    for k, v in (attrs or {}).items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    net.load_weights(w)
    return net


def _flows_check(tag, net, ref, im0, im1):
    final, pyr = net(gpu(im0), gpu(im1))
    net.synchronize()
    assert net.fallback_reason is None
    err = float(np.abs(final.cpu().double().numpy() - ref).max())
    print(f"featnorm model {tag}: max |flow| {float(np.abs(ref).max()):.2f} px, flows_final error {err:.3e} px")
    assert err <= 1e-3, (tag, err)
    return final, pyr


@pytest.mark.parametrize("use_dc", [False, True])
@pytest.mark.parametrize("variant", ["default", "f16x2=False", "coarse_cv=False", "concat_cv=False", "three_operand=False",
                                     "use_plans=False"])
def test_model_forward_against_the_float64_model(fn, use_dc, variant):
    """2 x 64 x 128, every correlation route fed with normalised operands: the block-per-workgroup and coarse kernels (default),
    the fp32 forms (f16x2=False), the matrix-pipe concat kernel (coarse_cv=False), the separate warp + cost volume launches
    (concat_cv=False), the one-buffer estimator input (three_operand=False), and the eager forward (use_plans=False)."""
    ref = R.model_reference(use_dc)
    kw, attrs = {}, {}
    if variant == "three_operand=False":
        attrs["three_operand"] = False
    elif variant != "default":
        k, v = variant.split("=")
        kw[k] = v == "True"
    net = _net(use_dc, ref["w"], attrs, normalize_features=True, **kw)
    _flows_check(f"use_dc={use_dc} {variant}", net, ref["final"], ref["im0"], ref["im1"])
    if variant == "default":                       # a second call replays the launch plan: the same bits
        a, _ = net(gpu(ref["im0"]), gpu(ref["im1"]))
        b, _ = net(gpu(ref["im0"]), gpu(ref["im1"]))
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,H,W", [(2, 128, 192), (2, 256, 384)])
def test_model_forward_at_larger_levels(fn, N, H, W):
    """2 x 128 x 192: levels up to 32 x 48.  No level this small takes the three-operand estimator input (its first conv goes to
    the F16-pipe kernel from 2 x 64 x 96 pixels on), so 2 x 256 x 384 is run as well, where level 4 does: the row-walking
    correlation kernel writes [cv | flow] records from normalised operands, the first conv reads the RAW features_0."""
    w = util.model_weights(False, gain=1.25)
    im0, im1 = util.smooth_images(N, H, W, seed=61, shift=(3, -2))
    net = _net(False, w, normalize_features=True)
    three = [l for l in range(1, 5) if net._three_operand_level(l, N, H >> (6 - l), W >> (6 - l), [192, 128, 96, 64, 32][l], list(range(32)))]
    print(f"featnorm model {N}x{H}x{W}: three-operand levels {three}")
    if (N, H, W) == (2, 256, 384) and not three:
        pytest.skip("no level of 2 x 256 x 384 takes the three-operand route on this build")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        ref, _ = R.NormPWCDCNet({k: torch.from_numpy(v).double() for k, v in w.items()})(
            torch.from_numpy(im0).double(), torch.from_numpy(im1).double())
    _flows_check(f"{N}x{H}x{W}", net, ref.numpy(), im0, im1)


@pytest.mark.parametrize("use_dc", [False, True])
def test_flag_off_is_the_plain_model_and_the_pipeline_is_the_plain_call(fn, use_dc):
    import pwcnet_amd
    ref = R.model_reference(use_dc)
    g0, g1 = gpu(ref["im0"]), gpu(ref["im1"])
    plain = _net(use_dc, ref["w"])
    off = _net(use_dc, ref["w"], normalize_features=False, norm_eps=1e-3)
    a, ap = plain(g0, g1)
    b, bp = off(g0, g1)
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(ap, bp))
    on = _net(use_dc, ref["w"], normalize_features=True)
    c, cp = on(g0, g1)
    assert float((c - a).abs().max()) > 1e-3
    pipe = pwcnet_amd.ForwardPipeline(depth=2, use_dc=use_dc, normalize_features=True)
    pipe.load_weights(ref["w"])
    tickets = [pipe.submit(g0, g1) for _ in range(3)]
    pipe.synchronize()
    for t in tickets:
        f, p = t.result()
        assert torch.equal(f, c) and all(torch.equal(x, y) for x, y in zip(p, cp))


def test_sequence_form_equals_two_tensors(fn):
    """frames[:-1], frames[1:] of one tensor (the extractor runs N + 1 frames once; f1 of a pair is the next frame's map) against
    the same pairs as two separate tensors."""
    w = util.model_weights(False, gain=1.25)
    N, H, W = 2, 64, 128
    a, b = util.smooth_images(N + 1, H, W, seed=33, shift=(2, 1))
    frames = gpu(0.5 * (a + b))
    net = _net(False, w, normalize_features=True)
    assert net._frames_shared(V(frames[:-1]), V(frames[1:]))
    s, sp = net(frames[:-1], frames[1:])
    t, tp = net(frames[:-1].clone(), frames[1:].clone())
    net.synchronize()
    assert torch.equal(s, t) and all(torch.equal(x, y) for x, y in zip(sp, tp))


# ------------------------------------------------------------------ model gradients
def _rel_err(got, ref):
    from tests.test_gpu_grad import _rel_err as f
    return f(got, ref)


def _report(tag, errs):
    ranked = sorted(errs.items(), key=lambda kv: -kv[1])
    print(f"featnorm gradients {tag}: worst {ranked[0][1]:.2e} ({ranked[0][0]}), median {float(np.median(list(errs.values()))):.2e}")


def _trainer_step(ref, use_dc, normalize):
    from pwcnet_amd.train import Trainer
    tn = Trainer(weights=R.LOSS_WEIGHTS, gamma=0.0, lr=1e-4, use_dc=use_dc, normalize_features=normalize)
    tn.load_weights(ref["w"])
    pyr = tn.forward(gpu(ref["im0"]), gpu(ref["im1"]))
    ggt = gpu(ref["gt"])
    loss = float(tn.loss_value(ggt))
    tn.backward(ggt)
    torch.cuda.synchronize()
    return tn, pyr, loss


@pytest.mark.parametrize("use_dc", [False, True])
def test_trainer_gradients_against_float64_autograd(fn, use_dc):
    """Every variable of a multiscale step at the bounds tests/test_gpu_grad.py asserts for the un-normalised model at this shape
    (STEP_BOUNDS: gradient per variable, pyramid, loss; each relative to the reference's largest magnitude)."""
    from tests.test_gpu_grad import STEP_BOUNDS
    g_bound, p_bound, l_bound = STEP_BOUNDS[(use_dc, "multiscale", R.MODEL_SHAPE, True)]
    ref = R.model_reference(use_dc)
    tn, pyr, loss = _trainer_step(ref, use_dc, True)
    pyr_err = max(_rel_err(a, b) for a, b in zip(pyr, ref["pyr"]))
    loss_err = abs(loss - ref["loss"]) / abs(ref["loss"])
    got = tn.gradients()
    errs = {k: _rel_err(got[k], r) for k, r in ref["grads"].items()}
    _report(f"Trainer use_dc={use_dc} (bound {g_bound:.1e}; pyramid {pyr_err:.2e} / {p_bound:.1e}, loss {loss_err:.2e} / {l_bound:.1e})", errs)
    assert pyr_err <= p_bound and loss_err <= l_bound, (pyr_err, loss_err)
    bad = {k: f"{e:.3e}" for k, e in errs.items() if e > g_bound}
    assert not bad, f"relative gradient error above {g_bound:.1e}: {bad}"
    # the flag changes the gradients; two steps give the same bits
    off, _, _ = _trainer_step(ref, use_dc, False)
    assert not torch.equal(off.grads, tn.grads)
    again, _, loss2 = _trainer_step(ref, use_dc, True)
    assert loss2 == loss and torch.equal(again.grads, tn.grads)


def _multiscale_loss_gpu(pyr, gt):
    """losses.py:15-32 in torch ops on the module's outputs (the ground truth is down-sampled on the CPU, it carries no gradient)."""
    from oracle import torch_ref as tr
    loss = 0.0
    for wl, fs in zip(R.LOSS_WEIGHTS, pyr):
        g = tr.resize_nearest(torch.from_numpy(gt) / 20.0, fs.shape[1:3]).cuda()
        loss = loss + wl * torch.linalg.vector_norm(g - fs, ord=2, dim=3).sum(dim=(1, 2)).mean()
    return loss


@pytest.mark.parametrize("use_dc", [False, True])
def test_module_gradients_against_float64_autograd(fn, use_dc):
    """PWCDCNetModule with the multiscale loss written in torch ops: every variable and both images at the bounds
    tests/test_gpu_autograd.py asserts for the un-normalised module at this shape (COTANGENT_BOUNDS)."""
    import pwcnet_amd
    from tests.test_gpu_autograd import COTANGENT_BOUNDS
    g_bound, i_bound = COTANGENT_BOUNDS[(use_dc, R.MODEL_SHAPE)]
    ref = R.model_reference(use_dc)

    def run():
        net = pwcnet_amd.PWCDCNetModule(use_dc=use_dc, normalize_features=True)
        net.load_weights(ref["w"])
        i0, i1 = gpu(ref["im0"]).requires_grad_(True), gpu(ref["im1"]).requires_grad_(True)
        final, pyr = net(i0, i1)
        _multiscale_loss_gpu(pyr, ref["gt"]).backward()
        torch.cuda.synchronize()
        return net, final, i0.grad, i1.grad

    net, final, d0, d1 = run()
    assert float(np.abs(final.detach().cpu().double().numpy() - ref["final"]).max()) <= 1e-3
    errs = {k: _rel_err(net._net._view(net.flat.grad, k), r) for k, r in ref["grads"].items()}
    errs["images_0"], errs["images_1"] = _rel_err(d0, ref["d_im0"]), _rel_err(d1, ref["d_im1"])
    _report(f"PWCDCNetModule use_dc={use_dc} (bounds {g_bound:.1e} / images {i_bound:.1e})", errs)
    bad = {k: f"{e:.3e}" for k, e in errs.items() if e > (i_bound if k.startswith("images") else g_bound)}
    assert not bad, f"relative gradient error above the bounds {g_bound:.1e} / {i_bound:.1e}: {bad}"
    net2, _, e0, e1 = run()
    assert torch.equal(net2.flat.grad, net.flat.grad) and torch.equal(e0, d0) and torch.equal(e1, d1)


# ------------------------------------------------------------------ train.py
@pytest.mark.parametrize("extra", [(), ("--loss", "unsup", "--occlusion", "fb")])
def test_train_cli_with_normalize_features(tmp_path, extra):
    """One synthetic epoch at batch 2, 64 x 128 crops, supervised and label-free: the loss is finite and the same in two runs."""
    lines = []
    for run in range(2):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "--synthetic_pairs", "8", "-e", "1",
                              "-b", "2", "--crop_shape", "64", "128", "--normalize_features", "--model_dir", str(tmp_path / f"m{run}"),
                              *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        ep = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch ")]
        assert len(ep) == 1, out.stdout[-1500:]
        lines.append(ep[0].split("  global_step")[0])
    print("featnorm train.py", extra, lines[0])
    loss = float(lines[0].split()[3])
    assert np.isfinite(loss) and lines[0] == lines[1], lines
