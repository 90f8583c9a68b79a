"""Per-kernel sweeps of the training path's backward ops (pwcnet_amd/grad_ops.py) at the shapes, layouts and modes the
Trainer uses, against torch.autograd on the float64 restatement (oracle/torch_ref.py), or against float64 sums where the op
is a sum.  Same helpers and tolerances as tests/test_gpu_grad.py: 2e-5 of max |ref| for data gradients, 3e-5 for the
convolution gradients, 1e-4 for the flow gradient, 1e-5 / 2e-5 for the channel sums, 1e-6 / 3e-6 for Adam."""
import math

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr
from tests.test_gpu_grad import V, View, close, gpu, rnd, t64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def go():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import grad_ops
    return grad_ops


def _wide(t, cs, off):
    """t (N,H,W,C) copied into channels off .. off+C of a zero (N,H,W,cs) buffer: (buffer, View of that slice)."""
    N, H, W, C = t.shape
    buf = torch.zeros((N, H, W, cs), dtype=torch.float32, device="cuda")
    buf[..., off:off + C] = t
    return buf, V(buf[..., off:off + C])


def _outside(buf, off, C):
    """The channels of buf outside off .. off+C (must stay as they were: zero)."""
    return torch.cat([buf[..., :off], buf[..., off + C:]], dim=3)


def _amax(a):
    return float(np.abs(a).max()) or 1.0


# ------------------------------------------------------------------ cost volume
def _cv_case(go, N, H, W, C):
    seed = 7 * C + 131 * H + 17 * W + N
    f0, f1, dcv = rnd((N, H, W, C), seed), rnd((N, H, W, C), seed + 1), rnd((N, H, W, 81), seed + 2)
    a, b = t64(f0), t64(f1)
    cv = tr.cost_volume(a, b)
    (cv * t64(dcv, False)).sum().backward()
    r0, r1 = a.grad.numpy(), b.grad.numpy()
    g0, g1, gcv, gdcv = gpu(f0), gpu(f1), gpu(cv.detach().numpy()), gpu(dcv)
    # cv / dcv: dense 81-float records (scalar path), 16-byte aligned slices of wider records (float4 path), slices at a
    # 4-byte offset (scalar path again) -- every layout gives the same bits
    wc4, vc4 = _wide(gcv, 96, 4)
    wd4, vd4 = _wide(gdcv, 100, 8)
    wc1, vc1 = _wide(gcv, 88, 1)
    wd1, vd1 = _wide(gdcv, 85, 3)
    layouts = {"dense": (V(gcv), V(gdcv)), "float4": (vc4, vd4), "offset": (vc1, vd1)}
    outs = {}
    for name, (vc, vd) in layouts.items():
        df0 = torch.full((N, H, W, C), 3.0, device="cuda")       # accumulate=False overwrites
        df1 = torch.full((N, H, W, C), -3.0, device="cuda")
        go.cost_volume_grad(V(g0), V(g1), vc, vd, V(df0), V(df1))
        torch.cuda.synchronize()
        close(df0, r0)
        close(df1, r1)
        outs[name] = (df0, df1)
    for name in ("float4", "offset"):
        assert torch.equal(outs[name][0], outs["dense"][0]) and torch.equal(outs[name][1], outs["dense"][1]), name
    # features as channel slices of wider buffers, the Trainer's three modes (float4 records, as in the estimator buffer)
    wf0, vf0 = _wide(g0, C + 8, 4)
    wf1, vf1 = _wide(g1, C + 12, 8)
    b0, b1 = rnd((N, H, W, C), seed + 3) * _amax(r0), rnd((N, H, W, C), seed + 4) * _amax(r1)
    # df0 only, accumulating into non-zero memory (dF0 += ...)
    d0, vd0 = _wide(gpu(b0), C + 4, 4)
    go.cost_volume_grad(vf0, vf1, vc4, vd4, vd0, None, accumulate=True)
    close(d0[..., 4:4 + C], b0 + r0)
    assert not torch.any(_outside(d0, 4, C))
    # df1 only, written
    d1 = torch.full((N, H, W, C), 7.0, device="cuda")
    go.cost_volume_grad(vf0, vf1, vc4, vd4, None, V(d1))
    close(d1, r1)
    # both, accumulating
    e0, e1 = gpu(b0), gpu(b1)
    go.cost_volume_grad(vf0, vf1, vc4, vd4, V(e0), V(e1), accumulate=True)
    close(e0, b0 + r0)
    close(e1, b1 + r1)
    # a second run gives the same bits
    df0 = torch.zeros((N, H, W, C), device="cuda")
    df1 = torch.zeros((N, H, W, C), device="cuda")
    go.cost_volume_grad(V(g0), V(g1), V(gcv), V(gdcv), V(df0), V(df1))
    assert torch.equal(df0, outs["dense"][0]) and torch.equal(df1, outs["dense"][1])


@pytest.mark.parametrize("C", [4, 16, 20, 32, 64, 96, 128, 196])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (6, 7), (12, 14), (13, 9), (24, 28)])
def test_cost_volume_grad_sweep(go, H, W, C):
    for N in (1, 3):
        _cv_case(go, N, H, W, C)


@pytest.mark.parametrize("N", [1, 3])
def test_cost_volume_grad_at_96x112(go, N):
    """The finest estimator level of a 384x448 crop (14 x 12 tiles per image)."""
    _cv_case(go, N, 96, 112, 32)


# ------------------------------------------------------------------ bilinear warp
WARP_SCALES = [0.625, 1.25, 2.5, 5.0, 10.0]          # weights.SCALES[1:6]: every level a Trainer can warp at


def _warp_flows(kind, N, H, W, scale, seed):
    """Flows (fp32) whose product with `scale` is: sub-pixel ('subpixel'); up to +-50 px, with pixels whose corners
    straddle a border -- one corner inside, one clamped -- ('far'); exactly an integer or a half ('exact')."""
    rs = np.random.RandomState(seed)
    if kind == "subpixel":
        return (rs.uniform(-0.95, 0.95, (N, H, W, 2)) / scale).astype(np.float32)
    if kind == "far":
        f = rs.uniform(-50.0, 50.0, (N, H, W, 2))
        m = rs.uniform(size=(N, H, W)) < 0.2
        f[m] = rs.choice([-50.0, 50.0], size=(int(m.sum()), 2))
        gy, gx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        edge = rs.randint(0, 6, size=(N, H, W))
        frac = rs.uniform(0.05, 0.95, (N, H, W))
        sub = rs.uniform(-0.9, 0.9, (N, H, W))
        # edge 0 / 1: x lands between -1 (clamped) and 0, or between W-1 and W (clamped); edge 2 / 3 the same in y
        f[..., 0] = np.where(edge == 0, frac - 1 - gx, np.where(edge == 1, W - 1 + frac - gx, np.where(edge < 4, sub, f[..., 0])))
        f[..., 1] = np.where(edge == 2, frac - 1 - gy, np.where(edge == 3, H - 1 + frac - gy, np.where(edge < 4, sub, f[..., 1])))
        return (f / scale).astype(np.float32)
    assert kind == "exact"
    # scale = 0.625 * 2^i and flow = q * 2^(2 - i): the fp32 product is exactly 2.5 q (q even: integer, q odd: half)
    i = int(round(math.log2(scale / 0.625)))
    assert 0.625 * 2.0 ** i == scale
    return (rs.randint(-6, 7, (N, H, W, 2)) * 2.0 ** (2 - i)).astype(np.float32)


def _warp_ref(x, flow, scale, dy):
    """(dx, dflow) of sum(dy * warp(x, flow * scale)) in float64, the scaled flow rounded to fp32 as the kernel rounds it
    (so that floor() agrees with pwc_mul_rounded)."""
    fs = np.float32(flow) * np.float32(scale)
    assert fs.dtype == np.float32
    xt, ft = t64(x), t64(fs)
    (tr.bilinear_warp(xt, ft) * t64(dy, False)).sum().backward()
    return xt.grad.numpy(), scale * ft.grad.numpy()


def _warp_case(go, N, H, W, C, scale, kind, seed, repeat=False):
    x, dy = rnd((N, H, W, C), seed), rnd((N, H, W, C), seed + 1)
    flow = _warp_flows(kind, N, H, W, scale, seed + 2)
    rdx, rdf = _warp_ref(x, flow, scale, dy)
    gx, gdy = gpu(x), gpu(dy)
    wfl, vfl = _wide(gpu(flow), 10, 6)                        # flow: a 2-channel slice of a wider record
    base = rnd((2 * N, H, W, C), seed + 3) * _amax(rdx)
    fbase = rnd((N, H, W, 2), seed + 4) * _amax(rdf)
    for det in (True, False):
        for acc in (False, True):
            dX = gpu(base)                                        # dx: the second half of a stacked 2N tensor (dF1)
            dxv = View(dX.data_ptr() + 4 * N * H * W * C, C, N, H, W, C)
            wdf, vdf = _wide(gpu(fbase), 12, 3)                   # dflow: a slice of a wider record
            go.warp_grad(V(gx), vfl, scale, V(gdy), dxv, vdf, dflow_accumulate=acc, deterministic=det)
            torch.cuda.synchronize()
            tag = f"{kind} scale {scale} N {N} C {C} deterministic {det} accumulate {acc}"
            assert torch.equal(dX[:N], gpu(base[:N])), tag
            close(dX[N:], base[N:] + rdx)
            close(wdf[..., 3:5], (fbase if acc else 0.0) + rdf, rel=1e-4)
            assert not torch.any(_outside(wdf, 3, 2)), tag
            if det and repeat:
                for _ in range(2):
                    again = gpu(base)
                    av = View(again.data_ptr() + 4 * N * H * W * C, C, N, H, W, C)
                    go.warp_grad(V(gx), vfl, scale, V(gdy), av, None, deterministic=True)
                    torch.cuda.synchronize()
                    assert torch.equal(again, dX), f"fixed-point warp gradient not bit-identical: {tag}"


@pytest.mark.parametrize("C", [4, 16, 32, 64, 96, 128, 196])
@pytest.mark.parametrize("scale", WARP_SCALES)
def test_warp_grad_sweep(go, scale, C):
    for N in (1, 3):
        for j, kind in enumerate(("subpixel", "far", "exact")):
            _warp_case(go, N, 9, 13, C, scale, kind, seed=100 * C + 10 * N + j, repeat=C == 196)


@pytest.mark.parametrize("kind", ["subpixel", "far"])
def test_warp_grad_many_blocks(go, kind):
    """8 x 96 x 112 x 64 (the finest level of a batch of 8 at 384x448: 2688 blocks)."""
    _warp_case(go, 8, 96, 112, 64, 5.0, kind, seed=5 if kind == "far" else 6)


# ------------------------------------------------------------------ legacy bilinear resize
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [2, 3, 32, 34])
def test_resize_grad_sweep(go, k, C):
    for H, W in [(1, 1), (1, 2), (3, 5), (6, 7)]:
        for N in (1, 3):
            seed = 1000 * k + 10 * C + H + W + N
            x, dy = rnd((N, H, W, C), seed), rnd((N, k * H, k * W, C), seed + 1)
            xt = t64(x)
            (tr.resize_legacy(xt, (k * H, k * W)) * t64(dy, False)).sum().backward()
            r = xt.grad.numpy()
            gdy = gpu(dy)
            dx = torch.full((N, H, W, C), 5.0, device="cuda")
            go.resize_grad(V(gdy), V(dx))
            close(dx, r)
            # dy as the feat_up slice of an estimator record, dx as a slice of a wider buffer, accumulate with mul != 1
            wdy, vdy = _wide(gdy, C + 7, 5)
            b = rnd((N, H, W, C), seed + 2) * _amax(r)
            wdx, vdx = _wide(gpu(b), C + 3, 2)
            go.resize_grad(vdy, vdx, mul=-0.75, accumulate=True)
            close(wdx[..., 2:2 + C], b - 0.75 * r)
            assert not torch.any(_outside(wdx, 2, C))


def test_resize_grad_grid_stride(go):
    """4 x 48 x 56 x 196 = 2 107 392 dx elements: more than the 8192 blocks x 256 threads of one pass."""
    N, H, W, C = 4, 48, 56, 196
    x, dy = rnd((N, H, W, C), 41), rnd((N, 2 * H, 2 * W, C), 42)
    assert N * H * W * C > 8192 * 256
    xt = t64(x)
    (tr.resize_legacy(xt, (2 * H, 2 * W)) * t64(dy, False)).sum().backward()
    r = xt.grad.numpy()
    gdy = gpu(dy)
    dx = torch.full((N, H, W, C), 5.0, device="cuda")
    go.resize_grad(V(gdy), V(dx))
    close(dx, r)
    go.resize_grad(V(gdy), V(dx), mul=0.5, accumulate=True)
    close(dx, 1.5 * r)


def test_resize_grad_refuses_unsupported_factors(go):
    from pwcnet_amd._lib import PwcHipError
    dx = torch.zeros((1, 4, 4, 8), device="cuda")
    for oh, ow in [(8, 12), (20, 20), (6, 6), (8, 6)]:         # unequal factors, k = 5, ratio 1.5, unequal again
        dy = torch.zeros((1, oh, ow, 8), device="cuda")
        with pytest.raises(PwcHipError):
            go.resize_grad(V(dy), V(dx))
        torch.cuda.synchronize()
    assert not torch.any(dx)


# ------------------------------------------------------------------ loss gradient
_PYRAMID = {(64, 128): [(1, 2), (2, 4), (4, 8), (8, 16), (16, 32)],
            (384, 448): [(6, 7), (12, 14), (24, 28), (48, 56), (96, 112)]}


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("gt_hw", [(64, 128), (384, 448)])
def test_flow_norm_grad_sweep(go, order, gt_hw):
    """pred at the five pyramid sizes of the gt, as strided records; gt values of 2.5 k, so that gt / 20 = k / 8 is exact in
    fp32 and float64.  Where pred equals gt / 20 in both components the gradient is 0 (the kernel's documented value, and
    torch.linalg.vector_norm's); where it equals it in one, that component is 0."""
    N, (GH, GW) = 2, gt_hw
    rs = np.random.RandomState(GH + order)
    gt = (rs.randint(-60, 61, (N, GH, GW, 2)) * 2.5).astype(np.float32)
    wgt, vgt = _wide(gpu(gt), 4, 1)
    scale = 0.32 / N
    for h, w in _PYRAMID[gt_hw]:
        gtd = tr.resize_nearest(torch.from_numpy(gt.astype(np.float64)) / 20.0, (h, w)).numpy()
        pred = gtd + rs.uniform(-0.5, 0.5, (N, h, w, 2))
        sel = rs.randint(0, 4, (N, h, w))
        pred[sel == 0] = gtd[sel == 0]                           # both components equal
        pred[sel == 1, 0] = gtd[sel == 1, 0]                     # x only
        pred[sel == 2, 1] = gtd[sel == 2, 1]                     # y only
        pred = pred.astype(np.float32)
        pt = t64(pred)
        (scale * torch.linalg.vector_norm(pt - torch.from_numpy(gtd), ord=order, dim=3).sum()).backward()
        r = pt.grad.numpy()
        wp, vp = _wide(gpu(pred), 6, 2)
        out, vo = _wide(torch.full((N, h, w, 2), 9.0, device="cuda"), 8, 4)
        go.flow_norm_grad(vp, vgt, vo, gt_div=20.0, ord=order, scale=scale)
        got = out[..., 4:6]
        close(got, r)
        g = got.cpu().numpy()
        assert np.all(g[sel == 0] == 0.0) and np.all(g[sel == 1, 0] == 0.0) and np.all(g[sel == 2, 1] == 0.0), (h, w)
        assert np.all(out[..., :4].cpu().numpy() == 0.0) and np.all(out[..., 6:].cpu().numpy() == 0.0)
        b = rnd((N, h, w, 2), h + w) * scale
        acc, va = _wide(gpu(b), 2, 0)
        go.flow_norm_grad(vp, vgt, va, gt_div=20.0, ord=order, scale=scale, accumulate=True)
        close(acc, b + r)


# ------------------------------------------------------------------ bias gradient / fused leaky-relu gradient
# every channel count at 1, 255 and 524 289 pixels (past 524 288 the partial count saturates at 2048 parts); 917 504
# pixels for the narrow ones; the widest at fewer pixels (what the float64 reference holds in host memory)
_CS_CASES = ([(p, c) for p in (1, 255, 524289, 917504) for c in (2, 16, 32)] +
             [(p, 301) for p in (1, 255, 65537)] + [(p, 1028) for p in (1, 255, 8193)])


@pytest.mark.parametrize("npix,C", _CS_CASES)
def test_channel_sums_sweep(go, npix, C):
    """C = 301: scalar lanes, two 256-lane channel blocks; C = 1028: float4 lanes, 257 of them (two blocks); y and dy as
    slices of wider records (y_cs > C); accumulate; the same bits on a second run."""
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(npix + C)
    y = torch.rand((1, 1, npix, C), generator=gen, device=dev) - 0.5
    d = torch.rand((1, 1, npix, C), generator=gen, device=dev) * 2 - 1
    wy, vy = _wide(y, C + 4, 0)
    wd, vd = _wide(d, C + 8, 4)
    # plain sums
    exp = d.cpu().double().reshape(npix, C).sum(0)
    out = torch.full((C,), 11.0, device=dev)
    go.channel_sums(vd, out, dev)
    close(out, exp, rel=1e-5)
    again = torch.zeros((C,), device=dev)
    go.channel_sums(vd, again, dev)
    assert torch.equal(again, out)
    base = torch.rand((C,), generator=gen, device=dev) * float(exp.abs().max())
    acc = base.clone()
    go.channel_sums(vd, acc, dev, accumulate=True)
    close(acc, base.cpu().double() + exp, rel=1e-5)
    assert torch.equal(wd[..., 4:4 + C], d) and not torch.any(_outside(wd, 4, C))
    # fused: dy *= (y > 0 ? 1 : slope) in place, and its sums
    masked = torch.where(y > 0, d, d * 0.1)
    out = torch.zeros((C,), device=dev)
    go.lrelu_grad_channel_sums_(vy, vd, out, dev)
    torch.cuda.synchronize()
    assert torch.equal(wd[..., 4:4 + C], masked)
    expm = masked.cpu().double().reshape(npix, C).sum(0)
    close(out, expm, rel=2e-5)
    wd[..., 4:4 + C] = d
    acc = base.clone()
    go.lrelu_grad_channel_sums_(vy, vd, acc, dev, accumulate=True)
    assert torch.equal(wd[..., 4:4 + C], masked)
    close(acc, base.cpu().double() + expm, rel=2e-5)
    wd[..., 4:4 + C] = d
    again = torch.zeros((C,), device=dev)
    go.lrelu_grad_channel_sums_(vy, vd, again, dev)
    assert torch.equal(again, out)


# ------------------------------------------------------------------ Adam
@pytest.mark.parametrize("n", [1, 257, 2097153, 5000003])
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_step_sweep(go, n, step):
    """grad_scale 1/2 (two data-parallel ranks), the L2 term folded in, the first step (zero moments) and step 1000;
    n above 8192 x 256 runs the grid-stride loop.  The reference takes beta1, beta2 and eps as the fp32 values the kernel
    receives (TF's Adam computes in the variable's fp32 as well): 1 - fp32(0.999) is 1.29e-5 below 0.001, which is the
    whole of v's first-step value."""
    p, g = rnd((n,), n % 1000 + 1), rnd((n,), n % 1000 + 2)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m, v = rnd((n,), 3) * 0.1, np.abs(rnd((n,), 4)) * 0.01
    gp, gg, gm, gv = gpu(p), gpu(g), gpu(m), gpu(v)
    lr, gamma, gs = 1e-4, 4e-4, 0.5
    lr_t = lr * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
    go.adam_step_(gp, gg, gm, gv, lr_t, l2_gamma=gamma, grad_scale=gs)
    p64 = t64(p, False)
    f32 = lambda a: float(np.float32(a))
    pt, mt, vt = tr.adam_step(p64, gs * t64(g, False) + gamma * p64, t64(m, False), t64(v, False), step, lr,
                              beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))
    close(gp, pt, rel=1e-6)
    close(gm, mt, rel=1e-6)
    close(gv, vt, rel=3e-6)
    assert torch.equal(gg, gpu(g))


# ------------------------------------------------------------------ convolution weight / data gradients
def _conv_case(go, N, H, W, cin, cout, stride, dil, seed):
    x, k, dy = rnd((N, H, W, cin), seed), rnd((3, 3, cin, cout), seed + 1) * 0.2, None
    Ho, Wo = -(-H // stride), -(-W // stride)
    dy = rnd((N, Ho, Wo, cout), seed + 2)
    xt, kt = t64(x), t64(k)
    (tr.conv3x3_same(xt, kt, None, stride, dil) * t64(dy, False)).sum().backward()
    rw = kt.grad.numpy()
    gx, gdy = gpu(x), gpu(dy)
    dw = torch.full((3, 3, cin, cout), 7.0, device="cuda")
    go.conv3x3_wgrad(V(gx), V(gdy), dw, cin, stride, dil)
    close(dw, rw, rel=3e-5)
    base = rnd((3, 3, cin, cout), seed + 3) * _amax(rw)
    acc = gpu(base)
    go.conv3x3_wgrad(V(gx), V(gdy), acc, cin, stride, dil, accumulate=True)
    close(acc, base + rw, rel=3e-5)
    if cin % 4 == 0:
        dx = torch.full((N, H, W, cin), 7.0, device="cuda")
        go.conv3x3_dgrad(V(gdy), gpu(k), V(dx), stride, dil, keep=[], dy_tensor=gdy)
        torch.cuda.synchronize()
        close(dx, xt.grad, rel=3e-5)


@pytest.mark.parametrize("H,W,cin,cout", [(384, 448, 3, 16), (192, 224, 16, 32), (96, 112, 32, 64), (48, 56, 64, 96),
                                          (24, 28, 96, 128), (12, 14, 128, 196)])
def test_conv_grads_extractor_stride2_at_384x448(go, H, W, cin, cout):
    """The extractor's stride-2 layers at the sizes a 384x448 crop gives them, batch 4 (8 images: both frames)."""
    _conv_case(go, 8, H, W, cin, cout, 2, 1, seed=cin + cout)


@pytest.mark.parametrize("cin,cout,dil", [(34, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16),
                                          (64, 32, 1), (32, 2, 1)])
def test_conv_grads_context_at_96x112(go, cin, cout, dil):
    """The dilated context network at the output level of a 384x448 crop."""
    _conv_case(go, 2, 96, 112, cin, cout, 1, dil, seed=cin + cout + dil)


def test_conv_dgrad_stride2_refuses_odd_sizes(go):
    """TF SAME at stride 2 pads an odd size differently; the data gradient is written for even sizes only and says so."""
    N, H, W, cin, cout = 1, 13, 14, 16, 32
    dy = torch.zeros((N, 7, 7, cout), device="cuda")
    dx = torch.zeros((N, H, W, cin), device="cuda")
    k = torch.zeros((3, 3, cin, cout), device="cuda")
    with pytest.raises(AssertionError, match="even input sizes"):
        go.conv3x3_dgrad(V(dy), k, V(dx), 2, 1, keep=[], dy_tensor=dy)
