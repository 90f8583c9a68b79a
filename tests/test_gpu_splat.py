"""GPU tests of forward splatting (csrc/pwc_splat.hip, pwcnet_amd/splat.py) against the float64 restatement of tests/splat_ref.py
(validated on the CPU by tests/test_host_splat.py) on its cases: frames (2, 9, 13) and (2, 24, 40) -- odd sizes, several
workgroups' worth of collisions and holes -- C in {1, 3, 5}, x as a channel slice of a wider buffer and the flow at channel
stride 4 in one case each way.

Bounds, per element.
  sum      |got - ref| <= 2^-24 |ref| + cnt 2^-37 (1 + 2^-20) + 1e-30: one fp32 rounding of the result, and half a fixed-point step
           (2^-36) for each of the cnt contributions the reference counts on that target.
  average  where the reference denominator D is at least 2^-10: got = fl(N' / D') with |N' - N|, |D' - D| <= e = cnt 2^-37
           (1 + 2^-20), so |N' / D' - N / D| <= (e + |ref| e) / (D - e), and with the rounding of the quotient
           |got - ref| <= 2^-24 |ref| + e (1 + |ref|) / (D - e) + 1e-30.
  gradient |got - ref| <= 2^-23 A, A the sum of the absolute values of the element's terms in the reference: the gather forms
           each element in double and rounds once (2^-24 A); the factor two is the issue's.  In the average mode the terms hold
           1 / den and num / den from the fixed-point accumulators, relative error e / den each; the inputs of that test keep every
           positive den above 2^-6 (tests/splat_ref.py mid_cell_flow; asserted on the reference), so that share is below 2^-27 A
           per term at cnt <= 16.
Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import splat_ref as sp
from tests.test_gpu_grad import gpu

pytestmark = pytest.mark.gpu
NAMES = sorted(sp.CASES)
STEP = 2.0 ** -37 * (1 + 2.0 ** -20)
MODES = ("sum", "average")


@pytest.fixture(scope="module")
def sl():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import splat
    return splat


def _slice_of_wider(t, width, at):
    """t (N,H,W,C) as channels at..at+C of a buffer of `width` channels filled with NaN: a read outside the slice shows."""
    buf = torch.full(tuple(t.shape[:3]) + (width,), float("nan"), dtype=torch.float32, device="cuda")
    buf[..., at:at + t.shape[3]] = t
    return buf[..., at:at + t.shape[3]]


def _inputs(name, wide=False, flow_key="flow"):
    c = sp.case(name)
    x, fl, w = c["x"].cuda(), c[flow_key].cuda(), c["w"].cuda()
    if wide:
        x, fl = _slice_of_wider(x, c["C"] + 3, 2), _slice_of_wider(fl, 4, 1)
        assert x.stride(2) > c["C"] and fl.stride(2) == 4
    return c, x, fl, w


# ------------------------------------------------------------------ 1. exact cases
@pytest.mark.parametrize("shape", [(2, 9, 13, 3), (2, 24, 40, 5)])
def test_zero_flow_returns_x_and_coverage_one(sl, shape):
    N, H, W, C = shape
    rs = np.random.RandomState(1)
    x = gpu(rs.randint(-4096, 4097, size=shape).astype(np.float32) / 4096.0)
    for mode in MODES:
        out, cov = sl.forward_splat(x, torch.zeros((N, H, W, 2), device="cuda"), mode=mode)
        assert torch.equal(out, x) and torch.equal(cov, torch.ones((N, H, W), device="cuda"))


def test_integer_flow_shifts_x(sl):
    N, H, W, C = 2, 9, 13, 3
    x = gpu(np.random.RandomState(2).uniform(0, 1, (N, H, W, C)).astype(np.float32))
    flow = torch.zeros((N, H, W, 2), device="cuda")
    flow[..., 0], flow[..., 1] = 2.0, -1.0
    out, cov = sl.forward_splat(x, flow)
    want, want_cov = torch.zeros_like(x), torch.zeros((N, H, W), device="cuda")
    want[:, :H - 1, 2:] = x[:, 1:, :W - 2]
    want_cov[:, :H - 1, 2:] = 1.0
    assert torch.equal(out, want) and torch.equal(cov, want_cov)


def test_a_whole_frame_onto_one_target_counts_exactly(sl):
    H = W = 16
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    flow = torch.stack([5.0 - xs, 9.0 - ys], dim=-1)[None].cuda().contiguous()
    r = sl.range_map(flow)
    want = torch.zeros((1, H, W), device="cuda")
    want[0, 9, 5] = 256.0
    assert torch.equal(r, want)


def test_a_mask_of_zeros_gives_zeros(sl):
    c, x, fl, w = _inputs("9x13_c3")
    for dtype in (torch.bool, torch.uint8):
        out, cov = sl.forward_splat(x, fl, w, valid=torch.zeros((c["N"], c["H"], c["W"]), dtype=dtype, device="cuda"), mode="average")
        assert not bool(out.any()) and not bool(cov.any())


# ------------------------------------------------------------------ 2., 3. against the reference
@pytest.mark.parametrize("name,wide", [(n, False) for n in NAMES] + [("9x13_c3", True), ("24x40_c5", True)])
def test_sum_mode_against_the_reference(sl, name, wide):
    c, x, fl, w = _inputs(name, wide)
    ref, ref_cov, cnt = sp.reference(name, "sum")
    out, cov = sl.forward_splat(x, fl, w)
    for what, got, want, n in (("out", out, ref, cnt[..., None]), ("coverage", cov, ref_cov, cnt)):
        err = (got.double().cpu() - want).abs()
        bound = 2.0 ** -24 * want.abs() + n * STEP + 1e-30
        print(f"{name} wide={wide} {what}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, "
              f"max ref {float(want.abs().max()):.3f}, most contributions {int(cnt.max())}")
        assert bool((err <= bound).all())


@pytest.mark.parametrize("name", NAMES)
def test_average_mode_against_the_reference(sl, name):
    c, x, fl, w = _inputs(name, wide=name == "24x40_c3")
    ref, den, cnt = sp.reference(name, "average")
    covered = den > 0
    small = covered & (den < sp.MIN_DEN)
    share = float(small.sum()) / float(covered.sum())
    print(f"{name}: {int(small.sum())} of {int(covered.sum())} covered targets have a denominator below 2^-10 ({share:.4f})")
    assert share <= 0.02
    out, cov = sl.forward_splat(x, fl, w, mode="average")
    out, cov = out.double().cpu(), cov.double().cpu()
    use = den >= sp.MIN_DEN
    e = (cnt.double() * STEP)[..., None]
    D = torch.where(use, den, torch.ones_like(den))[..., None]
    bound = 2.0 ** -24 * ref.abs() + e * (1 + ref.abs()) / (D - e) + 1e-30
    err = (out - ref).abs()
    sel = use[..., None].expand_as(err)
    print(f"{name}: max err {float(err[sel].max()):.3e}, max err / bound {float((err / bound)[sel].max()):.3f}")
    assert bool((err <= bound)[sel].all())
    assert not bool(out[~covered].any())                                 # nothing lands: 0, not NaN
    assert bool(((cov - den).abs() <= 2.0 ** -24 * den + cnt * STEP + 1e-30).all())


# ------------------------------------------------------------------ 4. edges
def test_non_finite_flows_contribute_nothing(sl):
    """NaN, +Inf and -Inf in either component: the result is, bit for bit, that of the same call with those pixels masked out."""
    c, x, fl, w = _inputs("24x40_c3")
    bad = torch.zeros((c["N"], c["H"], c["W"]), dtype=torch.bool, device="cuda")
    fl = fl.clone()
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"), float("nan"), float("inf"), float("-inf"))):
        n, y, xx = i % 2, 3 + 3 * i, 5 + 6 * i
        fl[n, y, xx, i // 3] = v
        bad[n, y, xx] = True
    clean = torch.where(bad[..., None], torch.zeros_like(fl), fl)
    for mode in MODES:
        out, cov = sl.forward_splat(x, fl, w, mode=mode)
        want, want_cov = sl.forward_splat(x, clean, w, valid=~bad, mode=mode)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, want) and torch.equal(cov, want_cov)


def test_a_point_left_of_the_frame_reaches_column_zero_only(sl):
    N, H, W = 1, 3, 5
    flow = torch.zeros((N, H, W, 2), device="cuda")
    valid = torch.zeros((N, H, W), dtype=torch.bool, device="cuda")
    flow[0, 1, 0, 0], valid[0, 1, 0] = -0.5, True                        # px = -0.5
    flow[0, 2, 1, 0], valid[0, 2, 1] = -1.75, True                       # px = -0.75
    flow[0, 0, 2, 0], valid[0, 0, 2] = -3.0, True                        # px = -1: the open end, contributes nothing
    x = torch.full((N, H, W, 1), 4.0, device="cuda")
    out, cov = sl.forward_splat(x, flow, valid=valid)
    want = torch.zeros((N, H, W), device="cuda")
    want[0, 1, 0], want[0, 2, 0] = 0.5, 0.25
    assert torch.equal(cov, want) and torch.equal(out[..., 0], 4.0 * want)


@pytest.mark.parametrize("shape", [(2, 1, 40), (2, 24, 1), (1, 1, 1)])
def test_frames_of_one_row_or_column(sl, shape):
    N, H, W = shape
    rs = np.random.RandomState(7)
    flow = torch.from_numpy(rs.uniform(-0.9, 0.9, (N, H, W, 2)).astype(np.float32))
    x = torch.from_numpy(rs.uniform(0, 1, (N, H, W, 3)).astype(np.float32))
    ref, ref_cov, cnt = sp.splat_ref(x, flow)
    out, cov = sl.forward_splat(x.cuda(), flow.cuda())
    assert int(cnt.sum()) > 0
    for got, want, n in ((out, ref, cnt[..., None]), (cov, ref_cov, cnt)):
        assert bool(((got.double().cpu() - want).abs() <= 2.0 ** -24 * want.abs() + n * STEP + 1e-30).all())


def test_a_contribution_out_of_range_poisons_the_outputs_and_the_process_goes_on(sl):
    c, x, fl, w = _inputs("9x13_c3")
    huge = w.clone()
    huge[1, 4, 6] = 1e9
    for mode in MODES:
        out, cov = sl.forward_splat(x, fl, huge, mode=mode)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(cov).all())
    out, cov = sl.forward_splat(x, fl, w)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cov).all())


# ------------------------------------------------------------------ 5. bit reproducibility
@pytest.mark.parametrize("mode", ["sum", "average"])
def test_two_calls_and_single_images_give_the_same_bits(sl, mode):
    c, x, fl, w = _inputs("24x40_c5")
    out, cov = sl.forward_splat(x, fl, w, mode=mode)
    out2, cov2 = sl.forward_splat(x, fl, w, mode=mode)
    assert torch.equal(out, out2) and torch.equal(cov, cov2)
    for n in range(c["N"]):
        o, cv = sl.forward_splat(x[n:n + 1], fl[n:n + 1], w[n:n + 1], mode=mode)
        assert torch.equal(o[0], out[n]) and torch.equal(cv[0], cov[n])


# ------------------------------------------------------------------ 6. gradients
@pytest.mark.parametrize("mode", ["sum", "average"])
@pytest.mark.parametrize("name", ["9x13_c1", "9x13_c3", "24x40_c5"])
def test_gradients_against_autograd_of_the_reference(sl, name, mode):
    """x, weights and flows, through autograd (forward_splat + backward) and through splat_grad with accumulate; the reference
    gradients are the explicit float64 formulas that tests/test_host_splat.py holds to torch.autograd on the restatement."""
    flow_key = "flow_mid" if mode == "average" else "flow"
    c, x, fl, w = _inputs(name, wide=name == "24x40_c5", flow_key=flow_key)
    if mode == "average":
        den = sp.splat_ref(None, c["flow_mid"], c["w"])[1]
        assert float(den[den > 0].min()) >= sp.MIN_DEN_GRAD
    (rx, rw, rf), (ax, aw, af), ok = sp.grad_reference(name, mode)
    g_out, g_cov = c["g_out"].cuda(), c["g_cov"].cuda()
    xg, fg, wg = x.detach().clone().requires_grad_(True), fl.detach().clone().requires_grad_(True), w.clone().requires_grad_(True)
    out, cov = sl.forward_splat(xg, fg, wg, mode=mode)
    ((out * g_out).sum() + (cov * g_cov).sum()).backward()
    for what, got, want, A in (("dx", xg.grad, rx, ax), ("dweights", wg.grad, rw, aw), ("dflows", fg.grad, rf, af)):
        err = (got.double().cpu() - want).abs()
        print(f"{name} {mode} {what}: max err {float(err.max()):.3e}, max err / (2^-23 A) "
              f"{float((err / (2.0 ** -23 * A).clamp(min=1e-300)).max()):.3f}, max A {float(A.max()):.3e}")
        assert bool((err <= 2.0 ** -23 * A).all())
        assert not bool(got.cpu()[~ok].any()) and bool((~ok).any())     # a pixel that does not contribute: exact zeros
    # the raw call: the same bits, and accumulate adds exactly what a plain call writes
    dx, dw, df = sl.splat_grad(x, fl, g_out, g_cov, w, mode=mode)
    assert torch.equal(dx, xg.grad) and torch.equal(dw, wg.grad) and torch.equal(df, fg.grad)
    rs = np.random.RandomState(3)
    bx, bw, bf = (gpu(rs.uniform(-1, 1, tuple(t.shape)).astype(np.float32)) for t in (dx, dw, df))
    ax_, aw_, af_ = sl.splat_grad(x, fl, g_out, g_cov, w, mode=mode, dx=bx.clone(), dweights=bw.clone(), dflows=bf.clone(),
                                  accumulate=True)
    assert torch.equal(ax_, bx + dx) and torch.equal(aw_, bw + dw) and torch.equal(af_, bf + df)


# ------------------------------------------------------------------ 7. range_valid
@pytest.mark.parametrize("name", ["9x13_c1", "24x40_c3"])
def test_range_valid_against_the_thresholded_reference(sl, name):
    c = sp.case(name)
    r_fw, r_bw = sp.splat_ref(None, c["flow_bw"])[1], sp.splat_ref(None, c["flow"])[1]      # mask_fw comes from the BACKWARD flow
    near_fw, near_bw = (r_fw - 0.5).abs() <= 1e-6, (r_bw - 0.5).abs() <= 1e-6
    share = max(float(near_fw.double().mean()), float(near_bw.double().mean()))
    print(f"{name}: share of pixels within 1e-6 of min_range {share:.4f}; occluded {1 - float((r_fw >= 0.5).double().mean()):.3f} / "
          f"{1 - float((r_bw >= 0.5).double().mean()):.3f}")
    assert share <= 0.005
    m_fw, m_bw = sl.range_valid(c["flow"].cuda().requires_grad_(True), c["flow_bw"].cuda(), min_range=0.5)
    assert m_fw.dtype == torch.bool and m_fw.is_contiguous() and not m_fw.requires_grad
    for got, ref, near in ((m_fw, r_fw, near_fw), (m_bw, r_bw, near_bw)):
        differ = got.cpu() != (ref >= 0.5)
        assert not bool((differ & ~near).any())
        assert bool(got.any()) and not bool(got.all())
    # range_map itself: the coverage of a splat of ones, bit for bit, and differentiable with respect to the flow
    fl = c["flow"].cuda().requires_grad_(True)
    r = sl.range_map(fl)
    ones = torch.ones((c["N"], c["H"], c["W"], 1), device="cuda")
    out, cov = sl.forward_splat(ones, fl.detach())
    assert torch.equal(r, cov) and torch.equal(out[..., 0], cov)
    g_cov = c["g_cov"].cuda()
    (r * g_cov).sum().backward()
    (_, _, rf), (_, _, af), _ = sp.splat_grads_ref(None, c["flow"], None, None, 1.0, "sum", None, c["g_cov"])
    assert bool(((fl.grad.double().cpu() - rf).abs() <= 2.0 ** -23 * af).all()) and bool(fl.grad.any())


# ------------------------------------------------------------------ 8. under the module
def test_range_map_trains_the_module_bit_reproducibly(sl):
    """One 64 x 64 step: range_map(flows_final).sum().backward() gives a finite model.flat.grad, twice the same bits."""
    from pwcnet_amd import PWCDCNetModule
    from tests import util
    im0, im1 = (gpu(a) for a in util.smooth_images(1, 64, 64))
    runs = []
    for _ in range(2):
        model = PWCDCNetModule(seed=3)
        final, _ = model(im0, im1)
        total = sl.range_map(final).sum()
        total.backward()
        runs.append((total.detach().clone(), model.flat.grad.clone()))
    torch.cuda.synchronize()
    (total, grad), (total2, grad2) = runs
    print(f"range sum {float(total):.4f}, |grad| max {float(grad.abs().max()):.3e}, non-zero {int((grad != 0).sum())} of {grad.numel()}")
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(grad).all())
    assert torch.equal(total, total2) and torch.equal(grad, grad2)
