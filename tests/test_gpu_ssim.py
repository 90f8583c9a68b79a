"""GPU tests of the SSIM term (csrc/pwc_ssim.hip, pwcnet_amd/unsup.py ssim_*) against the float64 restatement of
tests/ssim_ref.py (validated on the CPU by tests/test_host_ssim.py) on its cases: 23 x 37 (odd sizes, seams of the 32 x 8 tiles in
both directions) at radius 1, 2 and 3, 272 x 256 (272 tiles for 256 parts: the strided partition) at radius 1 and 3, 5 x 9 at
radius 3 (no interior), C in {1, 3, 4}, flow_scale in {1, 5}, a ~70 % mask and none, an image that contributes nothing, a
low-contrast pair in which c2 dominates the variances, every input a channel slice of a wider buffer.

Bounds.  Counts: exact.  Sums: 1e-5 of the largest reference sum.  Gradients: max-abs error over the largest reference element, at
most max(4 x the error of the SAME formulas run in float32 torch ops on the same inputs, 2e-5) -- tests/test_gpu_unsup.py's rule,
for its reason: the fp32 sample coordinate and the window statistics magnify roundings, the float32 run measures what that costs
a straightforward composition (1e-6 .. 1.8e-5 on these cases), 4 allows for another order of operations, 2e-5 is `close`'s
default.  Every test prints its figures before it asserts; DESIGN.md section 7 records them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ssim_ref as sr
from tests import unsup_ref as ur
from tests.test_gpu_grad import _rel_err, close, gpu
from tests.test_gpu_grad_ops import _wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(sr.CASES)


@pytest.fixture(scope="module")
def us():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import unsup
    return unsup


def _inputs(case, flow=None):
    """The case on the GPU as channel slices of wider buffers (`_wide`): images_0, images_1, flows, mask."""
    C = case["C"]
    im0 = _wide(gpu(case["im0"]), C + 3, 2)[0][..., 2:2 + C]
    im1 = _wide(gpu(case["im1"]), C + 1, 1)[0][..., 1:1 + C]
    fl = _wide(gpu(case["flow"] if flow is None else flow), 6, 3)[0][..., 3:5]
    valid = None if case["valid"] is None else torch.from_numpy(case["valid"]).cuda()
    return im0, im1, fl, valid


def _up():
    return torch.tensor(ur.UPSTREAM, dtype=torch.float32, device="cuda")


def _grad_bound(err32):
    return max(4.0 * err32, 2e-5)


# ------------------------------------------------------------------ against the float64 restatement
@pytest.mark.parametrize("name", NAMES)
def test_ssim_sums_and_counts_vs_float64(us, name):
    ref = sr.reference(name)
    case, r = ref["case"], ref["radius"]
    s64, c64, _, _ = ref["run64"]
    im0, im1, flow, valid = _inputs(case)
    sums, counts = us.ssim_sums(im0, im1, flow, case["flow_scale"], valid, radius=r)
    again, cagain = us.ssim_sums(im0, im1, flow, case["flow_scale"], valid, radius=r)
    loss = us.ssim_loss(im0, im1, flow, case["flow_scale"], valid, radius=r)
    torch.cuda.synchronize()
    want = float(s64.sum()) / (case["C"] * max(int(c64.sum()), 1))
    print(f"{name}: sums {sums.tolist()} ref {s64.tolist()} counts {counts.tolist()} ref {c64.tolist()} "
          f"rel err {_rel_err(sums, s64):.3e} (float32 torch {_rel_err(ref['run32'][0], s64):.3e}); loss {float(loss):.8f} ref {want:.8f}")
    assert counts.dtype == torch.int32 and counts.cpu().tolist() == c64.tolist()
    assert bool(torch.isfinite(sums).all())
    close(sums, s64, rel=1e-5)
    assert torch.equal(sums, again) and torch.equal(counts, cagain)
    if valid is not None:                      # a uint8 mask with other non-zero values is the same mask
        s8, c8 = us.ssim_sums(im0, im1, flow, case["flow_scale"], valid.to(torch.uint8) * 7, radius=r)
        assert torch.equal(s8, sums) and torch.equal(c8, counts)
    if case["empty"] is not None:
        assert float(sums[case["empty"]]) == 0.0 and int(counts[case["empty"]]) == 0
    if name.startswith("5x9"):
        assert not bool(sums.any()) and not bool(counts.any())
    assert loss.dim() == 0 and abs(float(loss) - want) <= 1e-5 * want


@pytest.mark.parametrize("name", NAMES)
def test_ssim_gradient_vs_float64_autograd(us, name):
    ref = sr.reference(name)
    case, r = ref["case"], ref["radius"]
    _, _, g64, contributing = ref["run64"]
    g32 = ref["run32"][2]
    im0, im1, flow, valid = _inputs(case)
    grads = []
    for _ in range(2):
        fl = flow.detach().requires_grad_(True)
        sums, _ = us.ssim_sums(im0, im1, fl, case["flow_scale"], valid, radius=r)
        (sums * _up()).sum().backward()
        grads.append(fl.grad)
    torch.cuda.synchronize()
    err, err32 = _rel_err(grads[0], g64), _rel_err(g32, g64)
    print(f"{name}: ssim gradient rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}, "
          f"max |ref| {float(g64.abs().max()):.3e}")
    assert grads[0].shape == flow.shape and bool(torch.isfinite(grads[0]).all())
    assert err <= _grad_bound(err32)
    assert torch.equal(grads[0], grads[1])
    # exactly 0 out of frame and where no contributing centre lies within the radius
    quiet = (~ref["inside"] | ~sr.near(contributing, r)).cuda()
    assert bool(quiet.any()) and not bool(grads[0][quiet].any())
    if name.startswith("5x9"):
        assert not bool(grads[0].any())
    # accumulate: added onto a pre-filled wide buffer, quiet pixels and the other channels untouched
    base = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, (case["N"], case["H"], case["W"], 5)).astype(np.float32)).cuda()
    buf = base.clone()
    us.ssim_grad(im0, im1, flow, _up(), buf[..., 1:3], case["flow_scale"], valid, radius=r, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(buf[..., 1:3][quiet], base[..., 1:3][quiet])
    assert torch.equal(buf[..., :1], base[..., :1]) and torch.equal(buf[..., 3:], base[..., 3:])
    assert torch.equal(buf[..., 1:3], base[..., 1:3] + grads[0])
    buf = base.clone()                                      # without it: overwritten, zeros where nothing contributes
    us.ssim_grad(im0, im1, flow, _up(), buf[..., 1:3], case["flow_scale"], valid, radius=r)
    assert torch.equal(buf[..., 1:3], grads[0]) and torch.equal(buf[..., 3:], base[..., 3:]) and torch.equal(buf[..., :1], base[..., :1])


@pytest.mark.parametrize("name", ["23x37_r1_c3_s1", "272x256_r3_c4_s5"])
def test_non_finite_flows_are_out_of_frame(us, name):
    """NaN, +Inf and -Inf at ~6 % of the pixels: each switches off the windows it belongs to, sums and gradient are finite and
    the reference's, and the gradient is exactly 0 at the bad pixels."""
    ref = sr.reference(name)
    case, r = ref["case"], ref["radius"]
    bad_flow = sr.nonfinite_flow(case)
    s64, c64, g64, _ = sr.run(case, r, torch.float64, bad_flow)
    g32 = sr.run(case, r, torch.float32, bad_flow)[2]
    im0, im1, flow, valid = _inputs(case, bad_flow)
    fl = flow.detach().requires_grad_(True)
    sums, counts = us.ssim_sums(im0, im1, fl, case["flow_scale"], valid, radius=r)
    (sums * _up()).sum().backward()
    torch.cuda.synchronize()
    err, err32 = _rel_err(fl.grad, g64), _rel_err(g32, g64)
    print(f"{name} non-finite: counts {counts.tolist()} ref {c64.tolist()}, sums rel err {_rel_err(sums, s64):.3e}, gradient rel err "
          f"HIP {err:.3e}, float32 torch {err32:.3e}")
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(fl.grad).all())
    assert int(c64.sum()) > 0 and counts.cpu().tolist() == c64.tolist()
    close(sums, s64, rel=1e-5)
    assert err <= _grad_bound(err32)
    assert not bool(fl.grad[torch.from_numpy(~np.isfinite(bad_flow).all(axis=3)).cuda()].any())


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("radius,C", [(1, 1), (2, 3), (3, 4)])
def test_identical_images_and_zero_flow(us, radius, C):
    """SSIM = 1 in every window: |sums| <= 1e-6 C counts, every interior centre counts, and the gradient vanishes."""
    N, H, W = 2, 23, 37
    im = gpu(np.random.RandomState(40 + C).uniform(0, 1, (N, H, W, C)).astype(np.float32))
    fl = torch.zeros((N, H, W, 2), device="cuda", requires_grad=True)
    sums, counts = us.ssim_sums(im, im, fl, radius=radius)
    sums.sum().backward()
    interior = (H - 2 * radius) * (W - 2 * radius)
    print(f"radius {radius} C {C}: sums {sums.tolist()} counts {counts.tolist()} max |grad| {float(fl.grad.abs().max()):.3e}")
    assert counts.cpu().tolist() == [interior] * N
    assert float(sums.detach().abs().max()) <= 1e-6 * C * interior
    assert float(fl.grad.abs().max()) <= 1e-6


@pytest.mark.parametrize("radius,a,b", [(1, 0.25, 0.75), (3, 0.6, 0.1)])
def test_constant_images_have_the_luminance_term_alone(us, radius, a, b):
    """x = a, y = b everywhere at zero flow: the variances are 0, SSIM = (2ab + c1) / (a^2 + b^2 + c1), and the sample has no
    slope, so the gradient is exactly 0."""
    N, H, W, C = 2, 23, 37, 3
    im0 = torch.full((N, H, W, C), a, device="cuda")
    im1 = torch.full((N, H, W, C), b, device="cuda")
    fl = torch.zeros((N, H, W, 2), device="cuda", requires_grad=True)
    sums, counts = us.ssim_sums(im0, im1, fl, radius=radius)
    sums.sum().backward()
    interior = (H - 2 * radius) * (W - 2 * radius)
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    want = C * interior * (1 - (2 * a32 * b32 + sr.C1) / (a32 * a32 + b32 * b32 + sr.C1)) / 2
    print(f"radius {radius} a {a} b {b}: sums {sums.tolist()} want {want} counts {counts.tolist()}")
    assert counts.cpu().tolist() == [interior] * N
    close(sums, np.full((N,), want), rel=1e-5)
    assert not bool(fl.grad.any())


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_an_out_of_frame_block_removes_the_centres_within_the_radius(us, radius):
    """Zero flow but for one 8 x 8 block (rows 8..15, columns 16..23 of image 0) thrown out of frame: exactly the (8 + 2r)^2
    centres within r of it leave the counts; image 1 keeps its whole interior."""
    N, H, W, C = 2, 23, 37, 3
    rs = np.random.RandomState(50)
    im0, im1 = (gpu(rs.uniform(0, 1, (N, H, W, C)).astype(np.float32)) for _ in range(2))
    fl = torch.zeros((N, H, W, 2), device="cuda")
    fl[0, 8:16, 16:24, 0] = W + 2
    _, counts = us.ssim_sums(im0, im1, fl, radius=radius)
    _, plain = us.ssim_sums(im0, im1, torch.zeros_like(fl), radius=radius)
    interior = (H - 2 * radius) * (W - 2 * radius)
    print(f"radius {radius}: counts {counts.tolist()} without the block {plain.tolist()}")
    assert plain.cpu().tolist() == [interior] * N
    assert counts.cpu().tolist() == [interior - (8 + 2 * radius) ** 2, interior]


# ------------------------------------------------------------------ end to end
def test_ssim_trains_the_module_bit_reproducibly(us):
    """N = 1, 64 x 128: PWCDCNetModule forward, 0.15 photometric + 0.85 ssim + 0.1 smoothness on flows_final, backward; twice."""
    from pwcnet_amd import PWCDCNetModule
    from tests import util
    im0, im1 = (gpu(a) for a in util.smooth_images(1, 64, 128))
    runs = []
    for _ in range(2):
        model = PWCDCNetModule(seed=3)
        final, _ = model(im0, im1)
        loss = 0.15 * us.photometric_loss(im0, im1, final) + 0.85 * us.ssim_loss(im0, im1, final) + 0.1 * us.smoothness_loss(final, im0)
        loss.backward()
        runs.append((loss.detach().clone(), model.flat.grad.clone()))
    torch.cuda.synchronize()
    (loss, grad), (loss2, grad2) = runs
    print(f"loss {float(loss):.6f}, |grad| max {float(grad.abs().max()):.3e}, non-zero {int((grad != 0).sum())} of {grad.numel()}")
    assert bool(torch.isfinite(loss)) and float(loss) != 0.0 and bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def _train(tmp_path, *extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                          "64", "128", "--synthetic_pairs", "4", "--loss", "unsup", "--model_dir", str(tmp_path), *extra],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    return [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]


def test_train_cli_ssim_weight(tmp_path):
    """ARFlow's first-stage data term, 0.15 Charbonnier + 0.85 SSIM: the step line carries both, in that order."""
    from pwcnet_amd import PWCDCNet, ckpt
    steps = _train(tmp_path, "--ssim_weight", "0.85")
    assert len(steps) == 1, steps                       # 4 pairs: 1 for validation, 3 to train on, batch 2, drop_last
    for key in ("loss/unsup", "photometric", "ssim", "smoothness"):
        assert np.isfinite(float(steps[0].split(" " + key + " ")[1].split()[0])), steps[0]
    assert steps[0].index(" photometric ") < steps[0].index(" ssim ") < steps[0].index(" smoothness ")
    PWCDCNet().load_weights(ckpt.load_weights(str(tmp_path / "model_1.ckpt")))


def test_train_cli_ssim_alone_has_no_base_term(tmp_path):
    steps = _train(tmp_path, "--ssim_weight", "1", "--ssim_radius", "2")
    assert len(steps) == 1, steps
    assert " ssim " in steps[0] and "photometric" not in steps[0] and "census" not in steps[0]
    for key in ("loss/unsup", "ssim", "smoothness"):
        assert np.isfinite(float(steps[0].split(" " + key + " ")[1].split()[0])), steps[0]


def test_train_cli_weight_zero_is_the_run_as_it_was(tmp_path):
    """Without --ssim_weight and with --ssim_weight 0 the step lines are the same, and neither names the SSIM term."""
    default, zero = _train(tmp_path / "a"), _train(tmp_path / "b", "--ssim_weight", "0")
    assert len(default) == 1 and default == zero
    assert " photometric " in default[0] and "ssim" not in default[0]
