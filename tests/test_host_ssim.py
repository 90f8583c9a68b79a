"""CPU tests of the SSIM term: the float64 yardstick of tests/ssim_ref.py against central finite differences, the closed form of
dL/dy (the alpha / beta / gamma split that the kernels implement) against autograd of the yardstick, the guarantees of every GPU
case, the C-ABI surface of csrc/pwc_ssim.hip with every return code of its argument checks in the stated order, every refusal
that pwcnet_amd/unsup.py raises before it calls the library, and train.py's flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from tests import ssim_ref as sr
from tests import unsup_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_ssim_workspace_floats", "pwc_ssim_sums_f32", "pwc_ssim_grad_f32")


def _small_case():
    """2 x 11 x 13, C = 3, flow_scale 5, ~70 % mask, a tenth of the 2 x 2 blocks thrown out of frame."""
    return ur.build_case(2, 11, 13, 3, flow_scale=5.0, seed=11, eps=1e-2, block=2, max_off=1, far=0.1)


def _small_planes(radius):
    case = _small_case()
    x, im1, flow = (torch.from_numpy(case[k]).double() for k in ("im0", "im1", "flow"))
    y, inside = sr.warped(im1, flow, 5.0)
    return case, x, y, sr.centres(inside, torch.from_numpy(case["valid"]), radius)


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("radius", [1, 2])
def test_reference_gradient_agrees_with_finite_differences(radius):
    """Autograd through the float64 restatement against central differences, h = 1e-6 (truncation h^2 f''' / 6 ~ 1e-12 times
    derivatives of a rational function whose denominators c2 + s_x + s_y stay above 1e-2 on noise images, rounding 1e-16 * sum /
    h ~ 1e-9 against gradients of ~0.1): every 5th component of the flow one by one, and 6 random directions over all of them.
    Every sample coordinate is 0.1 from a kink of floor, so no difference straddles one."""
    case = _small_case()
    im0, im1 = torch.from_numpy(case["im0"]).double(), torch.from_numpy(case["im1"]).double()
    valid = torch.from_numpy(case["valid"])
    up = torch.tensor(ur.UPSTREAM, dtype=torch.float64)

    def f(fl):
        return (sr.ssim_ref(im0, im1, fl, 5.0, valid, radius)[0] * up).sum()

    flow = torch.from_numpy(case["flow"]).double().requires_grad_(True)
    sums, counts, contributing = sr.ssim_ref(im0, im1, flow, 5.0, valid, radius)
    (sums * up).sum().backward()
    grad = flow.grad
    assert all(int(c) > 0 for c in counts) and float(grad.abs().max()) > 0
    h = 1e-6
    with torch.no_grad():
        x = flow.detach().clone()
        flat = x.reshape(-1)
        worst = 0.0
        for i in range(0, flat.numel(), 5):
            keep = float(flat[i])
            flat[i] = keep + h
            hi = float(f(x))
            flat[i] = keep - h
            lo = float(f(x))
            flat[i] = keep
            worst = max(worst, abs((hi - lo) / (2 * h) - float(grad.reshape(-1)[i])))
        rs = np.random.RandomState(5)
        for _ in range(6):
            v = torch.from_numpy(rs.choice([-1.0, 1.0], size=tuple(x.shape)))
            fd = (float(f(x + h * v)) - float(f(x - h * v))) / (2 * h)
            want = float((grad * v).sum())
            worst = max(worst, abs(fd - want) / np.sqrt(v.numel()))
    err = worst / float(grad.abs().max())
    print(f"radius {radius}: counts {counts.tolist()}, autograd vs central differences, rel err {err:.3e}, "
          f"max |grad| {float(grad.abs().max()):.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_closed_form_of_dLdy_agrees_with_autograd(radius):
    """The kernels' formula (three coefficients per contributing centre, box sums, alpha + beta x_q + gamma y_q) against
    autograd of the restatement with the warped frame y as the variable, in float64: they agree to rounding (the split
    cancels: 1e-10 allows for coefficients ~1e3 times the result)."""
    case, x, y, contributing = _small_planes(radius)
    up = torch.tensor(ur.UPSTREAM, dtype=torch.float64)
    y = y.detach().requires_grad_(True)
    (sr.sums_from_planes(x, y, contributing, radius) * up).sum().backward()
    with torch.no_grad():
        closed = sr.closed_form_dLdy(x, y, contributing, up, radius)
    err = float((closed - y.grad).abs().max()) / float(y.grad.abs().max())
    print(f"radius {radius}: contributing {contributing.sum(dim=(1, 2)).tolist()}, closed form vs autograd, rel err {err:.3e}, "
          f"max |dL/dy| {float(y.grad.abs().max()):.3e}")
    assert bool(contributing.any()) and float(y.grad.abs().max()) > 0 and err <= 1e-10
    # a pixel with no contributing centre within `radius` (itself included) has no gradient
    quiet = ~sr.near(contributing, radius)
    assert bool(quiet.any()) and not bool(closed[quiet].any()) and not bool(y.grad[quiet].any())


def test_one_out_of_frame_pixel_switches_off_every_window_it_belongs_to():
    """The whole-window rule, on the reference: with every other pixel in frame and valid, one out-of-frame pixel removes exactly
    the (2r+1)^2 centres within r of it (those in the interior), and a masked pixel removes only itself."""
    N, H, W, r = 1, 12, 14, 2
    inside = torch.ones((N, H, W), dtype=torch.bool)
    inside[0, 5, 6] = False
    valid = torch.ones((N, H, W), dtype=torch.bool)
    valid[0, 8, 10] = False
    c = sr.centres(inside, valid, r)
    want = torch.zeros((N, H, W), dtype=torch.bool)
    want[:, r:H - r, r:W - r] = True
    want[0, 3:8, 4:9] = False
    want[0, 8, 10] = False
    assert torch.equal(c, want) and int(c.sum()) == (H - 2 * r) * (W - 2 * r) - 25 - 1


def test_reference_ignores_non_finite_flows_and_degenerate_frames():
    case = _small_case()
    flow = sr.nonfinite_flow(case)
    assert np.isnan(flow).any() and np.isposinf(flow).any() and np.isneginf(flow).any()
    sums, counts, grad, contributing = sr.run(case, 1, torch.float64, flow)
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(grad).all())
    bad = torch.from_numpy(~np.isfinite(flow).all(axis=3))
    assert not bool(contributing[sr.near(bad, 1)].any()) and not bool(grad[bad].any())
    # H <= 2 radius: nothing contributes, no error
    short = [torch.from_numpy(case[k][:, :6]).double() for k in ("im0", "im1", "flow")]
    sums, counts, contributing = sr.ssim_ref(*short, radius=3)
    assert not bool(sums.any()) and not bool(counts.any()) and not bool(contributing.any())


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_case_guarantees_hold_for_every_gpu_case(name):
    """reference() asserts the share of the interior that contributes, the share of pixels that carry a gradient and the range
    of the per-pixel terms itself (build_case the 10-40 % out of frame); here every case of the GPU tests is built and what the
    tests rely on besides is checked."""
    ref = sr.reference(name)
    case, r = ref["case"], ref["radius"]
    s64, c64, g64, contributing = ref["run64"]
    s32, c32, g32, _ = ref["run32"]
    err32 = float((g32.double() - g64).abs().max()) / max(float(g64.abs().max()), 1e-300)
    print(f"{name}: counts {c64.tolist()}, interior shares {[round(s, 3) for s in ref['shares']]}, share of pixels with a gradient "
          f"{ref['grad_share']:.3f}, terms in [{ref['term_range'][0]:.3e}, {ref['term_range'][1]:.6f}], float32 torch gradient rel "
          f"err {err32:.3e}, sums rel err {float((s32.double() - s64).abs().max()) / max(float(s64.abs().max()), 1e-300):.3e}")
    assert c32.tolist() == c64.tolist() and bool(torch.isfinite(g64).all())
    assert -1e-9 <= ref["term_range"][0] and ref["term_range"][1] <= 1 + 1e-9
    border = torch.ones((case["H"], case["W"]), dtype=torch.bool)
    if case["H"] > 2 * r and case["W"] > 2 * r:
        border[r:case["H"] - r, r:case["W"] - r] = False
        assert ref["grad_share"] >= 0.05
        for n, share in enumerate(ref["shares"]):
            assert (share == 0.0) if n == case["empty"] else (share >= 0.10)
    assert not bool(contributing[:, border].any())
    # every pixel of a contributing centre's window is in frame
    assert not bool(contributing[sr.near(~ref["inside"], r)].any())
    # the gradient lives in frame and within r of a contributing centre, and that leaves pixels without one
    quiet = ~ref["inside"] | ~sr.near(contributing, r)
    assert bool(quiet.any()) and not bool(g64[quiet].any())
    if case["valid"] is not None:
        assert not bool(contributing[torch.from_numpy(~case["valid"])].any())
    if case["empty"] is not None:
        assert float(s64[case["empty"]]) == 0.0 and not bool(g64[case["empty"]].any())
    if name.startswith("5x9"):
        assert not bool(c64.any()) and not bool(s64.any()) and not bool(g64.any())
    if name.startswith("272x256"):                # more tiles than parts: the strided partition takes a second tile
        assert (272 // 8) * (256 // 32) > 256
    if name.endswith("lowcontrast"):              # c2 dominates the variances
        assert float(np.var(case["im0"])) + float(np.var(case["im1"])) < sr.C2


# ------------------------------------------------------------------ C ABI
def test_header_declares_the_entries_and_they_are_bound():
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int, "size_t": ctypes.c_size_t}
    L = _lib.lib()
    for name in ENTRIES:
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/pwc_hip.h"
        want = []
        for arg in m.group(2).split(","):
            arg = " ".join(arg.split())
            want.append(ctypes.c_void_p if ("*" in arg or arg.startswith("pwc_stream_t")) else ctype[arg.rsplit(" ", 1)[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[m.group(1)] and args == want, name
        assert getattr(L, name).argtypes == want
    assert "pwc_ssim.hip" in _lib.SOURCES
    assert header.index("self-supervised losses") < header.index("pwc_census_grad_f32") < header.index("pwc_ssim_sums_f32")
    assert header.index("pwc_ssim_grad_f32") < header.index("==== occlusion")


def test_workspace_sizes_and_every_return_code():
    """Host-side answers and argument checks: nothing is launched (the pointers are dummies)."""
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert "2 * N * parts + (with_grad ? 9 : 1) * C * N * H * W + (N * H * W + 3) / 4 + (with_grad ? 1 : 0)" in header
    assert "parts = min(256, ceil(W / 32) * ceil(H / 8))" in header

    def formula(N, H, W, C, with_grad):
        parts = min(256, -(-W // 32) * -(-H // 8))
        return 2 * N * parts + (9 if with_grad else 1) * C * N * H * W + (N * H * W + 3) // 4 + (1 if with_grad else 0)

    for shape in ((2, 23, 37, 3), (2, 272, 256, 4), (1, 5, 9, 1), (3, 8, 32, 2), (1, 9, 33, 4)):
        for with_grad in (0, 1):
            assert L.pwc_ssim_workspace_floats(*shape, with_grad) == formula(*shape, with_grad), (shape, with_grad)
    assert L.pwc_ssim_workspace_floats(2, 23, 37, 3, 0) == 2 * 2 * 6 + 3 * 2 * 23 * 37 + (2 * 23 * 37 + 3) // 4
    assert L.pwc_ssim_workspace_floats(0, 4, 4, 3, 0) == 0 and L.pwc_ssim_workspace_floats(1, 4, -1, 3, 1) == 0
    p = ctypes.c_void_p(4096)
    OK_WS = 1 << 20

    def sums(im0=p, im1=p, flow=p, cs=3, flow_cs=2, N=2, H=8, W=8, C=3, r=1, c1=1e-4, c2=9e-4, ws=p, nws=OK_WS, out=p, cnt=p):
        return L.pwc_ssim_sums_f32(im0, cs, im1, cs, flow, flow_cs, 1.0, None, N, H, W, C, r, c1, c2, ws, nws, out, cnt, None)

    EINVAL, ERANGE, EUNSUPPORTED = -1, -3, -4
    for bad in (dict(im0=None), dict(im1=None), dict(flow=None), dict(N=0), dict(H=0), dict(W=-1), dict(cs=2), dict(flow_cs=1),
                dict(c1=0.0), dict(c1=-1e-4), dict(c1=float("nan")), dict(c2=0.0), dict(c2=-0.1), dict(c2=float("nan")),
                dict(ws=None), dict(out=None), dict(cnt=None), dict(nws=L.pwc_ssim_workspace_floats(2, 8, 8, 3, 0) - 1)):
        assert sums(**bad) == EINVAL, bad
    for bad in (dict(C=0), dict(C=5, cs=5), dict(r=0), dict(r=4), dict(r=-1)):
        assert sums(**bad) == EUNSUPPORTED, bad
    for bad in (dict(N=65536), dict(H=1 << 16, W=1 << 15)):
        assert sums(**bad) == ERANGE, bad
    # the order the checks report in: null pointers and sizes, C and radius, strides and constants, the range, the workspace, the
    # outputs
    assert sums(im0=None, C=5) == EINVAL and sums(N=0, r=7) == EINVAL
    assert sums(C=5, cs=2) == EUNSUPPORTED and sums(r=4, c1=0.0) == EUNSUPPORTED
    assert sums(cs=2, N=65536) == EINVAL and sums(c2=0.0, N=65536) == EINVAL
    assert sums(N=65536, nws=0) == ERANGE and sums(N=65536, ws=None) == ERANGE and sums(N=65536, out=None) == ERANGE
    assert sums(nws=0, out=None) == EINVAL

    def grad(dsums=p, dflow=p, dflow_cs=2, C=3, r=1, c1=1e-4, c2=9e-4, N=2, ws=p, nws=OK_WS, cs=3):
        return L.pwc_ssim_grad_f32(p, cs, p, cs, p, 2, 1.0, None, N, 8, 8, C, r, c1, c2, dsums, ws, nws, dflow, dflow_cs, 0, None)

    for bad in (dict(dsums=None), dict(dflow=None), dict(dflow_cs=1), dict(c1=0.0), dict(c2=float("nan")), dict(ws=None), dict(cs=2),
                dict(nws=L.pwc_ssim_workspace_floats(2, 8, 8, 3, 1) - 1), dict(nws=L.pwc_ssim_workspace_floats(2, 8, 8, 3, 0))):
        assert grad(**bad) == EINVAL, bad
    assert grad(C=7, cs=7) == EUNSUPPORTED and grad(r=5) == EUNSUPPORTED and grad(N=70000) == ERANGE
    assert grad(C=7, cs=2) == EUNSUPPORTED and grad(N=70000, dflow=None) == ERANGE
    # an image whose last pixels an int pixel index stepped by up to 65536 cannot pass: the shared range check refuses it
    for wide in ((1 << 31) - 1, (1 << 31) - 65536):
        assert sums(H=1, W=wide) == ERANGE and sums(H=1, W=wide, nws=0) == ERANGE
    assert sums(H=1, W=(1 << 31) - 1 - 65536, nws=0) == EINVAL                       # the largest it takes: on to the workspace
    assert L.pwc_ssim_grad_f32(p, 3, p, 3, p, 2, 1.0, None, 1, 1, (1 << 31) - 1, 3, 1, 1e-4, 9e-4, p, p, OK_WS, p, 2, 0, None) == ERANGE


# ------------------------------------------------------------------ refusals before the library call
def test_python_refusals_come_before_the_library(monkeypatch):
    """Every argument fault is raised before the library is called, and the device is looked at last: on a machine without a GPU
    each call below ends in its own refusal, and a call with nothing else wrong in the refusal of CPU tensors."""
    from pwcnet_amd import unsup

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    N, H, W = 2, 9, 10
    im, fl = torch.zeros((N, H, W, 3)), torch.zeros((N, H, W, 2))
    up = torch.ones((N,))
    # CPU tensors
    with pytest.raises(ValueError, match="GPU only"):
        unsup.ssim_sums(im, im, fl)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.ssim_loss(im, im, fl, flow_scale=5.0, radius=3, c1=1e-3, c2=1e-2)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.ssim_grad(im, im, fl, up)
    # dtype
    with pytest.raises(TypeError, match="float32"):
        unsup.ssim_sums(im.double(), im, fl)
    with pytest.raises(TypeError, match="float32"):
        unsup.ssim_loss(im, im.half(), fl)
    with pytest.raises(TypeError, match="float32"):
        unsup.ssim_grad(im, im, fl.double(), up)
    with pytest.raises(TypeError):
        unsup.ssim_sums(im, im, np.zeros((N, H, W, 2), np.float32))
    # shape
    with pytest.raises(ValueError, match="channels"):
        unsup.ssim_sums(im, im, torch.zeros((N, H, W, 3)))
    with pytest.raises(ValueError, match="channels"):
        unsup.ssim_sums(torch.zeros((N, H, W, 5)), torch.zeros((N, H, W, 5)), fl)
    with pytest.raises(ValueError, match="channels"):
        unsup.ssim_sums(im, torch.zeros((N, H, W, 1)), fl)
    with pytest.raises(ValueError, match=r"\(N,H,W\)"):
        unsup.ssim_sums(torch.zeros((N, H + 1, W, 3)), im, fl)
    with pytest.raises(ValueError, match="NHWC"):
        unsup.ssim_loss(im, im, torch.zeros((H, W, 2)))
    # the mask: grad_ops.mask_ptr's refusals, unchanged
    with pytest.raises(TypeError, match="torch.bool or torch.uint8"):
        unsup.ssim_sums(im, im, fl, valid=torch.ones((N, H, W)))
    with pytest.raises(ValueError, match="expected shape"):
        unsup.ssim_sums(im, im, fl, valid=torch.ones((N, H, W + 1), dtype=torch.bool))
    with pytest.raises(ValueError, match="the mask is on"):
        unsup.ssim_sums(im, im, fl, valid=torch.ones((N, H, W), dtype=torch.bool))
    # images are constants
    for k in range(2):
        ims = [im, im]
        ims[k] = im.clone().requires_grad_(True)
        with pytest.raises(ValueError, match="not implemented"):
            unsup.ssim_sums(ims[0], ims[1], fl)
        with pytest.raises(ValueError, match="not implemented"):
            unsup.ssim_grad(ims[0], ims[1], fl, up)
    # the term's parameters: before the tensors are looked at (a wrong dtype besides does not hide them)
    for bad in (dict(radius=0), dict(radius=4), dict(radius=2.0), dict(radius=True), dict(radius=None), dict(c1=0.0),
                dict(c1=-1.0), dict(c1=float("nan")), dict(c2=0.0), dict(c2=float("nan"))):
        with pytest.raises(ValueError, match="radius|c1|c2"):
            unsup.ssim_sums(im, im, fl, **bad)
        with pytest.raises(ValueError, match="radius|c1|c2"):
            unsup.ssim_loss(im, im, fl, **bad)
        with pytest.raises(ValueError, match="radius|c1|c2"):
            unsup.ssim_grad(im, im, fl, up, **bad)
    # there is no eps and no q: the term is not passed through rho
    with pytest.raises(TypeError):
        unsup.ssim_sums(im, im, fl, eps=1e-3)
    with pytest.raises(TypeError):
        unsup.ssim_loss(im, im, fl, q=0.5)


def test_ssim_is_exported_and_documents_the_window_rule():
    import inspect

    import pwcnet_amd
    for name in ("ssim_sums", "ssim_loss", "ssim_grad"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(pwcnet_amd.unsup, name)
    doc = " ".join(pwcnet_amd.ssim_sums.__doc__.split())
    assert "every pixel of the window must be in frame" in doc and "centres only" in doc
    sig = inspect.signature(pwcnet_amd.ssim_sums)
    assert [(k, v.default) for k, v in sig.parameters.items()][3:] == [("flow_scale", 1.0), ("valid", None), ("radius", 1),
                                                                       ("c1", 1e-4), ("c2", 9e-4)]
    assert list(inspect.signature(pwcnet_amd.ssim_loss).parameters) == list(sig.parameters)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "SSIM term" in text and all(name in text for name in ENTRIES)
    left_out = re.search(r"\*\*Not included:\*\* range-map.*?\n\n", text, flags=re.S)          # section 3.3's list
    assert left_out and "SSIM" not in left_out.group(0)


# ------------------------------------------------------------------ train.py
def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), *args], capture_output=True, text=True, timeout=120,
                          cwd=ROOT)


def test_train_cli_lists_the_ssim_flags_and_refuses_bad_weights():
    out = _cli("--help")
    assert out.returncode == 0, out.stderr
    text = " ".join(out.stdout.split())
    assert "--ssim_weight" in text and re.search(r"--ssim_radius \{1,2,3\}", text), text
    assert re.search(r"--photo \{charbonnier,census\}", text), text          # --photo is as it was
    bad = _cli("--loss", "unsup", "--ssim_weight", "1.5")
    assert bad.returncode != 0 and "--ssim_weight" in bad.stderr
    bad = _cli("--loss", "unsup", "--ssim_weight", "-0.1")
    assert bad.returncode != 0 and "--ssim_weight" in bad.stderr
    bad = _cli("--ssim_weight", "0.5")                                        # the default --loss is supervised
    assert bad.returncode != 0 and "--ssim_weight" in bad.stderr and "--loss unsup" in bad.stderr
    bad = _cli("--loss", "unsup", "--ssim_weight", "0.5", "--ssim_radius", "4")
    assert bad.returncode != 0 and "--ssim_radius" in bad.stderr
