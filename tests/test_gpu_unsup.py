"""GPU tests of the self-supervised losses (csrc/pwc_unsup.hip, pwcnet_amd/unsup.py) against the float64 restatements of
tests/unsup_ref.py (validated on the CPU by tests/test_host_unsup.py) on its cases: 23 x 37 (odd sizes, tail lanes) and 272 x 256
(more than 256 partials per image: the grid-stride loop and the capped partition), C in {1, 3, 4}, wide-stride views,
flow_scale in {1, 20 / 4}, (eps, q) in {(1e-3, 0.5), (1e-2, 0.45)}, a ~70 % mask with NaN behind it, an image that contributes
nothing.

Bounds.  Counts: exact.  Sums: 1e-5 of the largest reference sum (what tests/test_gpu_masked_loss.py holds the sum kernels to).
Gradients: max-abs error over the largest reference element, at most max(4 x the error of the SAME formulas run in float32 torch
ops on the same inputs, 2e-5) -- rho' magnifies an fp32 rounding of the difference by up to 1 / eps, the float32 run measures what
that costs a straightforward composition, 4 allows for another order of operations, 2e-5 is `close`'s default.  Every test prints
its figures before it asserts.  (Not yet run on an MI355X when committed: DESIGN.md section 7 has no measured HIP errors.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import unsup_ref as ur
from tests.test_gpu_grad import _rel_err, close, gpu
from tests.test_gpu_grad_ops import _wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(ur.CASES)


@pytest.fixture(scope="module")
def us():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import unsup
    return unsup


def _inputs(case, poisoned=True):
    """The case on the GPU as channel slices of wider buffers (`_wide`): images_0, images_1, flows, mask."""
    k = "_nan" if poisoned else ""
    C = case["C"]
    im0 = _wide(gpu(case["im0" + k]), C + 3, 2)[0][..., 2:2 + C]
    im1 = _wide(gpu(case["im1" + k]), C + 1, 1)[0][..., 1:1 + C]
    flow = _wide(gpu(case["flow" + k]), 6, 3)[0][..., 3:5]
    valid = None if case["valid"] is None else torch.from_numpy(case["valid"]).cuda()
    return im0, im1, flow, valid


def _up():
    return torch.tensor(ur.UPSTREAM, dtype=torch.float32, device="cuda")


def _grad_bound(err32):
    return max(4.0 * err32, 2e-5)


# ------------------------------------------------------------------ photometric term
@pytest.mark.parametrize("name", NAMES)
def test_photometric_sums_and_counts_vs_float64(us, name):
    ref = ur.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    s64, c64, _ = ref["photo64"]
    im0, im1, flow, valid = _inputs(case)
    sums, counts = us.photometric_sums(im0, im1, flow, case["flow_scale"], valid, eps, q)
    again, cagain = us.photometric_sums(im0, im1, flow, case["flow_scale"], valid, eps, q)
    torch.cuda.synchronize()
    print(f"{name}: sums {sums.tolist()} ref {s64.tolist()} counts {counts.tolist()} ref {c64.tolist()} "
          f"rel err {_rel_err(sums, s64):.3e} (float32 torch {_rel_err(ref['photo32'][0], s64):.3e})")
    assert counts.dtype == torch.int32 and counts.cpu().tolist() == c64.tolist()
    assert bool(torch.isfinite(sums).all())
    close(sums, s64, rel=1e-5)
    assert torch.equal(sums, again) and torch.equal(counts, cagain)
    if valid is not None:                      # a uint8 mask with other non-zero values is the same mask
        s8, c8 = us.photometric_sums(im0, im1, flow, case["flow_scale"], valid.to(torch.uint8) * 7, eps, q)
        assert torch.equal(s8, sums) and torch.equal(c8, counts)
    if case["empty"] is not None:
        assert float(sums[case["empty"]]) == 0.0 and int(counts[case["empty"]]) == 0
    loss = us.photometric_loss(im0, im1, flow, case["flow_scale"], valid, eps, q)
    want = float(s64.sum()) / (case["C"] * max(int(c64.sum()), 1))
    assert loss.dim() == 0 and abs(float(loss) - want) <= 1e-5 * want


@pytest.mark.parametrize("name", NAMES)
def test_photometric_gradient_vs_float64_autograd(us, name):
    ref = ur.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    g64, g32 = ref["photo64"][2], ref["photo32"][2]
    im0, im1, flow, valid = _inputs(case)
    grads = []
    for _ in range(2):
        fl = flow.detach().requires_grad_(True)
        sums, _ = us.photometric_sums(im0, im1, fl, case["flow_scale"], valid, eps, q)
        (sums * _up()).sum().backward()
        grads.append(fl.grad)
    torch.cuda.synchronize()
    err, err32 = _rel_err(grads[0], g64), _rel_err(g32, g64)
    print(f"{name}: photometric gradient rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}, "
          f"max |ref| {float(g64.abs().max()):.3e}")
    assert grads[0].shape == flow.shape and bool(torch.isfinite(grads[0]).all())
    assert err <= _grad_bound(err32)
    assert torch.equal(grads[0], grads[1])
    quiet = torch.from_numpy(~case["contributing"]).cuda()
    assert not bool(grads[0][quiet].any())                 # a pixel that does not contribute: exactly 0
    # accumulate: added onto a pre-filled wide buffer, pixels that do not contribute (and the other channels) untouched
    base = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, (case["N"], case["H"], case["W"], 5)).astype(np.float32)).cuda()
    buf = base.clone()
    us.photometric_grad(im0, im1, flow, _up(), buf[..., 1:3], case["flow_scale"], valid, eps, q, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(buf[..., 1:3][quiet], base[..., 1:3][quiet])
    assert torch.equal(buf[..., :1], base[..., :1]) and torch.equal(buf[..., 3:], base[..., 3:])
    assert torch.equal(buf[..., 1:3][~quiet], (base[..., 1:3] + grads[0])[~quiet])
    buf = base.clone()                                      # without it: overwritten, zeros where nothing contributes
    us.photometric_grad(im0, im1, flow, _up(), buf[..., 1:3], case["flow_scale"], valid, eps, q)
    assert torch.equal(buf[..., 1:3], grads[0]) and torch.equal(buf[..., 3:], base[..., 3:])


@pytest.mark.parametrize("C", [1, 3, 4])
def test_zero_flow_is_the_direct_charbonnier_sum(us, C):
    N, H, W, eps, q = 2, 23, 37, 1e-3, 0.5
    rs = np.random.RandomState(20 + C)
    im0, im1 = (rs.uniform(0, 1, (N, H, W, C)).astype(np.float32) for _ in range(2))
    want = ur.rho(torch.from_numpy(im0).double() - torch.from_numpy(im1).double(), eps, q).sum(dim=(1, 2, 3))
    sums, counts = us.photometric_sums(gpu(im0), gpu(im1), torch.zeros((N, H, W, 2), device="cuda"), eps=eps, q=q)
    print(f"C {C}: sums {sums.tolist()} direct {want.tolist()} rel err {_rel_err(sums, want):.3e}")
    assert counts.cpu().tolist() == [H * W] * N
    close(sums, want, rel=1e-5)


# ------------------------------------------------------------------ smoothness term
@pytest.mark.parametrize("name", NAMES)
def test_smoothness_sums_and_gradient_vs_float64(us, name):
    ref = ur.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    im0, _, flow, _ = _inputs(case, poisoned=False)
    for key, image in (("smooth", im0), ("smooth_noimg", None)):
        (s64, g64), (s32, g32) = ref[key + "64"], ref[key + "32"]
        outs = []
        for _ in range(2):
            fl = flow.detach().requires_grad_(True)
            sums = us.smoothness_sums(fl, image, ur.ALPHA, eps, q)
            (sums * _up()).sum().backward()
            outs.append((sums.detach(), fl.grad))
        torch.cuda.synchronize()
        (sums, grad), err32 = outs[0], _rel_err(g32, g64)
        err = _rel_err(grad, g64)
        print(f"{name} {key}: sums {sums.tolist()} ref {s64.tolist()} rel err {_rel_err(sums, s64):.3e}; gradient rel err HIP "
              f"{err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}, max |ref| {float(g64.abs().max()):.3e}")
        close(sums, s64, rel=1e-5)
        assert bool(torch.isfinite(grad).all()) and err <= _grad_bound(err32)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        loss = us.smoothness_loss(flow, image, ur.ALPHA, eps, q)
        want = float(s64.sum()) / (case["N"] * case["H"] * case["W"])
        assert loss.dim() == 0 and abs(float(loss) - want) <= 1e-5 * want
        base = torch.from_numpy(np.random.RandomState(8).uniform(-1, 1, tuple(flow.shape[:3]) + (4,)).astype(np.float32)).cuda()
        buf = base.clone()
        us.smoothness_grad(flow, _up(), buf[..., 2:4], image, ur.ALPHA, eps, q, accumulate=True)
        assert torch.equal(buf[..., 2:4], base[..., 2:4] + grad) and torch.equal(buf[..., :2], base[..., :2])


@pytest.mark.parametrize("name", ["23x37_c3_s1", "272x256_c4_s5"])
def test_smoothness_without_an_image_is_a_constant_image(us, name):
    ref = ur.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    flow = gpu(case["flow"])
    const = torch.full((case["N"], case["H"], case["W"], case["C"]), 0.375, device="cuda")
    res = []
    for image in (None, const):
        fl = flow.detach().requires_grad_(True)
        sums = us.smoothness_sums(fl, image, ur.ALPHA, eps, q)
        sums.sum().backward()
        res.append((sums.detach(), fl.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------ end to end
def test_losses_train_the_module_bit_reproducibly(us):
    """N = 1, 64 x 128: PWCDCNetModule forward, photometric + 0.1 smoothness on flows_final, backward; twice."""
    from pwcnet_amd import PWCDCNetModule
    from tests import util
    im0, im1 = (gpu(a) for a in util.smooth_images(1, 64, 128))
    runs = []
    for _ in range(2):
        model = PWCDCNetModule(seed=3)
        final, _ = model(im0, im1)
        loss = us.photometric_loss(im0, im1, final) + 0.1 * us.smoothness_loss(final, im0)
        loss.backward()
        runs.append((loss.detach().clone(), model.flat.grad.clone()))
    torch.cuda.synchronize()
    (loss, grad), (loss2, grad2) = runs
    print(f"loss {float(loss):.6f}, |grad| max {float(grad.abs().max()):.3e}, non-zero {int((grad != 0).sum())} of {grad.numel()}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_train_cli_label_free_mode(tmp_path):
    from pwcnet_amd import PWCDCNet, ckpt
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                          "64", "128", "--synthetic_pairs", "4", "--loss", "unsup", "--model_dir", str(tmp_path)],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    steps = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 1, steps                       # 4 pairs: 1 for validation, 3 to train on, batch 2, drop_last
    for ln in steps:
        assert np.isfinite(float(ln.split("loss/unsup")[1].split()[0])), ln
    assert "EPE/val" in out.stdout
    PWCDCNet().load_weights(ckpt.load_weights(str(tmp_path / "model_1.ckpt")))
