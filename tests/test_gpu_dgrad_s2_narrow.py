"""pwc_conv3x3_dgrad_s2_narrow_f32 (the gradient of the images through the first extractor conv) against torch.autograd
on the float64 restatement of the stride-2 TF 'SAME' convolution (oracle/torch_ref.py), and against the zero-stuffed
route of grad_ops.conv3x3_dgrad.

Errors are relative to the reference's largest magnitude.  DGRAD_BOUND is 10x the worst error measured on an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

# measured worst: 2.23e-7 ((2, 12, 20), Cy 32 -> Cx 4; 1.9e-7 at 16 x 448 x 1024, Cy 16 -> Cx 3)
DGRAD_BOUND = 2.3e-6
# against the zero-stuffed fp32 route (same products, another summation order); measured worst 3.95e-7 (Cx 3)
ZERO_STUFFED_BOUND = 4e-6


@pytest.fixture(scope="module")
def go():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import grad_ops
    return grad_ops


def View(*a):
    from pwcnet_amd.modules import View as _V
    return _V(*a)


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, size=shape).astype(np.float32)


def ref_dx(dy, w):
    """float64 autograd of conv3x3_same(x, w, stride=2) w.r.t. x, for the gradient dy."""
    N, Ho, Wo, _ = dy.shape
    torch.set_num_threads(min(16, torch.get_num_threads()))
    x = torch.zeros((N, 2 * Ho, 2 * Wo, w.shape[2]), dtype=torch.float64, requires_grad=True)
    y = tr.conv3x3_same(x, torch.from_numpy(w).double(), None, 2, 1)
    y.backward(torch.from_numpy(dy).double())
    return x.grad.numpy()


def rel_err(got, ref):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


@pytest.mark.parametrize("N,H,W,Cx,Cy", [
    (2, 64, 128, 3, 16), (16, 448, 1024, 3, 16), (3, 6, 10, 3, 16), (1, 2, 2, 3, 16),
    (2, 12, 20, 1, 16), (2, 12, 20, 2, 8), (2, 12, 20, 4, 32), (1, 10, 6, 3, 4)])
def test_dgrad_s2_narrow_vs_float64(go, N, H, W, Cx, Cy):
    dy, w = rnd((N, H // 2, W // 2, Cy), 1 + Cx), rnd((3, 3, Cx, Cy), 2 + Cy) * 0.3
    ref = ref_dx(dy, w)
    gdy, gw = torch.from_numpy(dy).cuda(), torch.from_numpy(w).cuda()
    dx = torch.full((N, H, W, Cx), 7.0, device="cuda")
    go.conv3x3_dgrad_s2_narrow(View(gdy.data_ptr(), Cy, N, H // 2, W // 2, Cy), gw, View(dx.data_ptr(), Cx, N, H, W, Cx))
    err = rel_err(dx, ref)
    # dy as a channel slice of a wider buffer (dy_cs > Cy), dx accumulated onto a base with a wider channel stride
    wide = torch.zeros((N, H // 2, W // 2, Cy + 8), device="cuda")
    wide[..., 4:4 + Cy] = gdy
    base = torch.from_numpy(rnd((N, H, W, Cx + 1), 3)).cuda()
    acc = base.clone()
    go.conv3x3_dgrad_s2_narrow(View(wide.data_ptr() + 16, Cy + 8, N, H // 2, W // 2, Cy), gw,
                               View(acc.data_ptr(), Cx + 1, N, H, W, Cx), accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(acc[..., Cx], base[..., Cx]), "wrote outside its channels"
    err_acc = float(np.abs((acc[..., :Cx] - base[..., :Cx]).double().cpu().numpy() - ref).max()) / float(np.abs(ref).max())
    print(f"\n({N},{H},{W}) Cy {Cy} -> Cx {Cx}: relative error {err:.2e}, strided + accumulate {err_acc:.2e}")
    assert err <= DGRAD_BOUND, err
    assert err_acc <= DGRAD_BOUND, err_acc


@pytest.mark.parametrize("N,H,W,Cx", [(2, 64, 128, 4), (2, 64, 128, 3)])
def test_dgrad_s2_narrow_vs_zero_stuffed_route(go, N, H, W, Cx):
    Cy = 16
    dy, w = rnd((N, H // 2, W // 2, Cy), 11), rnd((3, 3, Cx, Cy), 12) * 0.3
    gdy, gw = torch.from_numpy(dy).cuda(), torch.from_numpy(w).cuda()
    a = torch.zeros((N, H, W, Cx), device="cuda")
    b = torch.zeros((N, H, W, Cx), device="cuda")
    vdy = View(gdy.data_ptr(), Cy, N, H // 2, W // 2, Cy)
    go.conv3x3_dgrad_s2_narrow(vdy, gw, View(a.data_ptr(), Cx, N, H, W, Cx))
    go.conv3x3_dgrad(vdy, gw, View(b.data_ptr(), Cx, N, H, W, Cx), 2, 1, keep=[], dy_tensor=gdy)
    torch.cuda.synchronize()
    err = rel_err(a, b.double().cpu().numpy())
    print(f"\nnarrow vs zero-stuffed route, Cx {Cx}: {err:.2e}")
    assert err <= ZERO_STUFFED_BOUND, err


def test_dgrad_s2_narrow_refuses_bad_arguments_and_writes_nothing(go):
    from pwcnet_amd import _lib
    L = _lib.lib()
    s = _lib.current_stream()
    N, H, W, Cx, Cy = 1, 8, 8, 3, 16
    dy = torch.ones((N, H // 2, W // 2, Cy), device="cuda")
    w = torch.ones((3, 3, 4, Cy), device="cuda")
    dx = torch.full((N, H + 1, W + 1, 5), 3.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = L.pwc_conv3x3_dgrad_s2_narrow_f32
    cases = [
        ((None, Cy, p(w), p(dx), Cx, N, H, W, Cx, Cy, 0, s), -1),           # null dy
        ((p(dy), Cy, p(w), None, Cx, N, H, W, Cx, Cy, 0, s), -1),           # null dx
        ((p(dy), Cy, p(w), p(dx), Cx, N, H + 1, W, Cx, Cy, 0, s), -4),      # odd H
        ((p(dy), Cy, p(w), p(dx), Cx, N, H, W + 1, Cx, Cy, 0, s), -4),      # odd W
        ((p(dy), Cy, p(w), p(dx), 5, N, H, W, 5, Cy, 0, s), -4),            # Cx 5
        ((p(dy), Cy, p(w), p(dx), Cx, N, H, W, Cx, 6, 0, s), -4),           # Cy not a multiple of 4
        ((p(dy), 12, p(w), p(dx), Cx, N, H, W, Cx, Cy, 0, s), -1),          # dy_cs < Cy
        ((p(dy), Cy, p(w), p(dx), 2, N, H, W, Cx, Cy, 0, s), -1),           # dx_cs < Cx
        ((ctypes.c_void_p(dy.data_ptr() + 4), Cy, p(w), p(dx), Cx, N, H, W, Cx, Cy, 0, s), -2),   # misaligned dy
    ]
    for args, rc in cases:
        assert f(*args) == rc, (args, rc)
    torch.cuda.synchronize()
    assert bool((dx == 3.0).all()), "a refused call wrote into dx"
