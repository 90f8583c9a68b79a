"""GPU tests of the soft census term (csrc/pwc_census.hip, pwcnet_amd/unsup.py census_*) against the float64 restatement of
tests/census_ref.py (validated on the CPU by tests/test_host_census.py) on its cases: 23 x 37 (odd sizes, seams of the 32 x 8
tiles in both directions), 272 x 256 (272 tiles for 256 parts: the strided partition) and 5 x 9 at radius 3 (no interior), radius
in {1, 2, 3}, C in {1, 3, 4}, scale in {255, 8}, flow_scale in {1, 5}, a ~70 % mask and none, an image that contributes nothing,
every input a channel slice of a wider buffer.

Bounds.  Counts: exact.  Sums: 1e-5 of the largest reference sum.  Gradients: max-abs error over the largest reference element, at
most max(4 x the error of the SAME formulas run in float32 torch ops on the same inputs, 2e-5) -- tests/test_gpu_unsup.py's rule,
for its reason: rho' and the fp32 sample coordinate magnify roundings, the float32 run measures what that costs a straightforward
composition (2e-5 .. 6e-3 on these cases), 4 allows for another order of operations, 2e-5 is `close`'s default.  Every test prints
its figures before it asserts; DESIGN.md section 7 records them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import census_ref as cr
from tests import unsup_ref as ur
from tests.test_gpu_grad import _rel_err, close, gpu
from tests.test_gpu_grad_ops import _wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(cr.CASES)


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


def _near(contributing, radius):
    """Pixels with a contributing centre within `radius` (themselves included)."""
    return torch.nn.functional.max_pool2d(contributing[:, None].double(), 2 * radius + 1, 1, radius)[:, 0] > 0


# ------------------------------------------------------------------ against the float64 restatement
@pytest.mark.parametrize("name", NAMES)
def test_census_sums_and_counts_vs_float64(us, name):
    ref = cr.reference(name)
    case, kw = ref["case"], dict(ref["kw"], **cr.CONSTS)
    s64, c64, _, _ = ref["run64"]
    im0, im1, flow, valid = _inputs(case)
    sums, counts = us.census_sums(im0, im1, flow, case["flow_scale"], valid, **kw)
    again, cagain = us.census_sums(im0, im1, flow, case["flow_scale"], valid, **kw)
    torch.cuda.synchronize()
    print(f"{name}: sums {sums.tolist()} ref {s64.tolist()} counts {counts.tolist()} ref {c64.tolist()} "
          f"rel err {_rel_err(sums, s64):.3e} (float32 torch {_rel_err(ref['run32'][0], s64):.3e})")
    assert counts.dtype == torch.int32 and counts.cpu().tolist() == c64.tolist()
    assert bool(torch.isfinite(sums).all())
    close(sums, s64, rel=1e-5)
    assert torch.equal(sums, again) and torch.equal(counts, cagain)
    if valid is not None:                      # a uint8 mask with other non-zero values is the same mask
        s8, c8 = us.census_sums(im0, im1, flow, case["flow_scale"], valid.to(torch.uint8) * 7, **kw)
        assert torch.equal(s8, sums) and torch.equal(c8, counts)
    if case["empty"] is not None:
        assert float(sums[case["empty"]]) == 0.0 and int(counts[case["empty"]]) == 0
    if name.startswith("5x9"):
        assert not bool(sums.any()) and not bool(counts.any())
    loss = us.census_loss(im0, im1, flow, case["flow_scale"], valid, **kw)
    want = float(s64.sum()) / max(int(c64.sum()), 1)
    assert loss.dim() == 0 and abs(float(loss) - want) <= 1e-5 * want


@pytest.mark.parametrize("name", NAMES)
def test_census_gradient_vs_float64_autograd(us, name):
    ref = cr.reference(name)
    case, kw = ref["case"], dict(ref["kw"], **cr.CONSTS)
    _, _, g64, contributing = ref["run64"]
    g32 = ref["run32"][2]
    im0, im1, flow, valid = _inputs(case)
    grads = []
    for _ in range(2):
        fl = flow.detach().requires_grad_(True)
        sums, _ = us.census_sums(im0, im1, fl, case["flow_scale"], valid, **kw)
        (sums * _up()).sum().backward()
        grads.append(fl.grad)
    torch.cuda.synchronize()
    err, err32 = _rel_err(grads[0], g64), _rel_err(g32, g64)
    print(f"{name}: census gradient rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}, "
          f"max |ref| {float(g64.abs().max()):.3e}")
    assert grads[0].shape == flow.shape and bool(torch.isfinite(grads[0]).all())
    assert err <= _grad_bound(err32)
    assert torch.equal(grads[0], grads[1])
    # exactly 0 out of frame and where no contributing centre lies within the radius
    quiet = (~ref["inside"] | ~_near(contributing, kw["radius"])).cuda()
    assert bool(quiet.any()) and not bool(grads[0][quiet].any())
    if name.startswith("5x9"):
        assert not bool(grads[0].any())
    # accumulate: added onto a pre-filled wide buffer, quiet pixels and the other channels untouched
    base = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, (case["N"], case["H"], case["W"], 5)).astype(np.float32)).cuda()
    buf = base.clone()
    us.census_grad(im0, im1, flow, _up(), buf[..., 1:3], case["flow_scale"], valid, accumulate=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(buf[..., 1:3][quiet], base[..., 1:3][quiet])
    assert torch.equal(buf[..., :1], base[..., :1]) and torch.equal(buf[..., 3:], base[..., 3:])
    assert torch.equal(buf[..., 1:3], base[..., 1:3] + grads[0])
    buf = base.clone()                                      # without it: overwritten, zeros where nothing contributes
    us.census_grad(im0, im1, flow, _up(), buf[..., 1:3], case["flow_scale"], valid, **kw)
    assert torch.equal(buf[..., 1:3], grads[0]) and torch.equal(buf[..., 3:], base[..., 3:]) and torch.equal(buf[..., :1], base[..., :1])


@pytest.mark.parametrize("name", ["23x37_r3_c3_s1_k255", "272x256_r1_c3_s1_k8_nomask"])
def test_non_finite_flows_are_out_of_frame(us, name):
    """NaN, +Inf and -Inf at ~6 % of the pixels: b is 0 there, sums and gradient are finite and the reference's."""
    ref = cr.reference(name)
    case, kw = ref["case"], dict(ref["kw"], **cr.CONSTS)
    bad_flow = cr.nonfinite_flow(case)
    s64, c64, g64, _ = cr.run(case, ref["kw"], torch.float64, bad_flow)
    g32 = cr.run(case, ref["kw"], torch.float32, bad_flow)[2]
    im0, im1, flow, valid = _inputs(case, bad_flow)
    fl = flow.detach().requires_grad_(True)
    sums, counts = us.census_sums(im0, im1, fl, case["flow_scale"], valid, **kw)
    (sums * _up()).sum().backward()
    torch.cuda.synchronize()
    err, err32 = _rel_err(fl.grad, g64), _rel_err(g32, g64)
    print(f"{name} non-finite: sums rel err {_rel_err(sums, s64):.3e}, gradient rel err HIP {err:.3e}, float32 torch {err32:.3e}")
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(fl.grad).all())
    assert counts.cpu().tolist() == c64.tolist()
    close(sums, s64, rel=1e-5)
    assert err <= _grad_bound(err32)
    assert not bool(fl.grad[torch.from_numpy(~np.isfinite(bad_flow).all(axis=3)).cuda()].any())


# ------------------------------------------------------------------ known answers
def _mixed_images(N=2, H=23, W=37):
    """Smooth structure plus 30 % noise, in [0, 1]: windows with small and with large intensity differences."""
    from tests import util
    smooth, _ = util.smooth_images(N, H, W)
    noise = np.random.RandomState(31).uniform(0, 1, smooth.shape).astype(np.float32)
    return (0.7 * smooth + 0.3 * noise).astype(np.float32)


@pytest.mark.parametrize("radius,C", [(1, 1), (2, 3), (3, 4)])
def test_identical_images_and_zero_flow(us, radius, C):
    """h = 0 everywhere: sums = counts * eps^(2q), and the gradient is exactly 0."""
    N, H, W, eps, q = 2, 23, 37, 1e-2, 0.4
    im = gpu(np.random.RandomState(40 + C).uniform(0, 1, (N, H, W, C)).astype(np.float32))
    fl = torch.zeros((N, H, W, 2), device="cuda", requires_grad=True)
    sums, counts = us.census_sums(im, im, fl, radius=radius, eps=eps, q=q)
    sums.sum().backward()
    want = np.full((N,), (H - 2 * radius) * (W - 2 * radius) * eps ** (2 * q))
    print(f"radius {radius} C {C}: sums {sums.tolist()} want {want.tolist()} counts {counts.tolist()}")
    assert counts.cpu().tolist() == [(H - 2 * radius) * (W - 2 * radius)] * N
    close(sums, want, rel=1e-5)
    assert not bool(fl.grad.any())


@pytest.mark.parametrize("radius", [1, 3])
def test_brightness_changes_barely_move_the_census_term(us, radius):
    """images_1 = images_0 + 0.1 and images_1 = 0.8 * images_0 at zero flow, both terms with eps = 1e-2, q = 0.4.  Additive: the
    census sum stays within 1e-4 relative of the identical-image value.  Multiplicative: its relative rise is at most a tenth of
    the Charbonnier term's (the float64 restatements give 0.05 - 0.11 against 5.4 on these images)."""
    im = _mixed_images()
    N, H, W, C = im.shape
    im0, zero = gpu(im), torch.zeros((N, H, W, 2), device="cuda")
    kw = dict(eps=1e-2, q=0.4)
    res = {}
    for key, im1 in (("same", im0), ("add", gpu(im + np.float32(0.1))), ("mul", gpu(np.float32(0.8) * im))):
        res[key] = (float(us.census_loss(im0, im1, zero, radius=radius, **kw)), float(us.photometric_loss(im0, im1, zero, **kw)))
    rise = {k: tuple((res[k][i] - res["same"][i]) / res["same"][i] for i in range(2)) for k in ("add", "mul")}
    print(f"radius {radius}: (census, charbonnier) identical {res['same']}, +0.1 {res['add']}, x0.8 {res['mul']}; relative rise "
          f"+0.1 {rise['add']}, x0.8 {rise['mul']}")
    assert abs(rise["add"][0]) <= 1e-4
    assert rise["mul"][1] > 1.0 and 0.0 <= rise["mul"][0] <= 0.1 * rise["mul"][1]


# ------------------------------------------------------------------ end to end
def test_census_trains_the_module_bit_reproducibly(us):
    """N = 1, 64 x 128: PWCDCNetModule forward, census + 0.1 smoothness on flows_final, backward; twice."""
    from pwcnet_amd import PWCDCNetModule
    from tests import util
    im0, im1 = (gpu(a) for a in util.smooth_images(1, 64, 128))
    runs = []
    for _ in range(2):
        model = PWCDCNetModule(seed=3)
        final, _ = model(im0, im1)
        loss = us.census_loss(im0, im1, final) + 0.1 * us.smoothness_loss(final, im0)
        loss.backward()
        runs.append((loss.detach().clone(), model.flat.grad.clone()))
    torch.cuda.synchronize()
    (loss, grad), (loss2, grad2) = runs
    print(f"loss {float(loss):.6f}, |grad| max {float(grad.abs().max()):.3e}, non-zero {int((grad != 0).sum())} of {grad.numel()}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def _train(tmp_path, *extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                          "64", "128", "--synthetic_pairs", "4", "--loss", "unsup", "--model_dir", str(tmp_path), *extra],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    return [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]


def test_train_cli_census_mode(tmp_path):
    from pwcnet_amd import PWCDCNet, ckpt
    steps = _train(tmp_path, "--photo", "census")
    assert len(steps) == 1, steps                       # 4 pairs: 1 for validation, 3 to train on, batch 2, drop_last
    assert " census " in steps[0] and "photometric" not in steps[0]
    for key in ("loss/unsup", "census", "smoothness"):
        assert np.isfinite(float(steps[0].split(key)[1].split()[0])), steps[0]
    PWCDCNet().load_weights(ckpt.load_weights(str(tmp_path / "model_1.ckpt")))


def test_train_cli_default_is_the_charbonnier_path(tmp_path):
    """Without --photo the step line is the one `--photo charbonnier` prints: the parent's code path, bit for bit."""
    default, explicit = _train(tmp_path / "a"), _train(tmp_path / "b", "--photo", "charbonnier")
    assert len(default) == 1 and default == explicit
    assert " photometric " in default[0] and "census" not in default[0]
