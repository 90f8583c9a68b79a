"""CPU tests of the soft census term: the float64 yardstick of tests/census_ref.py against central finite differences, the closed
form of dL/db that the gather kernel implements against autograd of the yardstick, the guarantees of every GPU case, the C-ABI
surface of csrc/pwc_census.hip with every return code of its argument checks, every refusal that pwcnet_amd/unsup.py raises
before it calls the library, and train.py's flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from tests import census_ref as cr
from tests import unsup_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_census_workspace_floats", "pwc_census_sums_f32", "pwc_census_grad_f32")


def _small_case():
    """2 x 11 x 13, C = 3, flow_scale 5, ~70 % mask: interior 5 x 7 at radius 3."""
    return ur.build_case(2, 11, 13, 3, flow_scale=5.0, seed=11, eps=1e-2, block=2, max_off=1, far=0.1)


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("radius", [1, 3])
def test_reference_gradient_agrees_with_finite_differences(radius):
    """Autograd through the float64 restatement against central differences, h = 1e-6 (truncation h^2 f''' / 6 ~ 1e-12 times
    derivatives that eps = 1e-2 keeps below ~1e5, rounding 1e-16 * sum / h ~ 1e-8 of a sum of ~50 against gradients of ~1):
    every 5th component of the flow one by one, and 6 random directions over all of them.  Every sample coordinate is 0.1 from a
    kink of floor, so no difference straddles one."""
    case = _small_case()
    im0, im1 = torch.from_numpy(case["im0"]).double(), torch.from_numpy(case["im1"]).double()
    valid = torch.from_numpy(case["valid"])
    up = torch.tensor(ur.UPSTREAM, dtype=torch.float64)

    def f(fl):
        return (cr.census_ref(im0, im1, fl, 5.0, valid, radius, 8.0, **cr.CONSTS)[0] * up).sum()

    flow = torch.from_numpy(case["flow"]).double().requires_grad_(True)
    sums, counts, contributing = cr.census_ref(im0, im1, flow, 5.0, valid, radius, 8.0, **cr.CONSTS)
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
    print(f"radius {radius}: autograd vs central differences, rel err {err:.3e}, max |grad| {float(grad.abs().max()):.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_closed_form_of_dLdb_agrees_with_autograd(radius):
    """The gather kernel's formula (G, D, one loop for both roles of a pixel) against autograd of the restatement with the
    warped grey plane b as the variable, in float64: they agree to rounding."""
    case = _small_case()
    im0, im1 = torch.from_numpy(case["im0"]).double(), torch.from_numpy(case["im1"]).double()
    valid = torch.from_numpy(case["valid"])
    up = torch.tensor(ur.UPSTREAM, dtype=torch.float64)
    a, b, inside = cr.grey_planes(im0, im1, torch.from_numpy(case["flow"]).double(), 5.0, 255.0)
    contributing = cr.centres(inside, valid, radius)
    b = b.detach().requires_grad_(True)
    (cr.sums_from_planes(a, b, contributing, radius, **cr.CONSTS) * up).sum().backward()
    with torch.no_grad():
        closed = cr.closed_form_dLdb(a, b, contributing, up, radius, **cr.CONSTS)
    err = float((closed - b.grad).abs().max()) / float(b.grad.abs().max())
    print(f"radius {radius}: closed form vs autograd, rel err {err:.3e}, max |dL/db| {float(b.grad.abs().max()):.3e}")
    assert float(b.grad.abs().max()) > 0 and err <= 1e-12
    # a pixel with no contributing centre within `radius` (itself included) has no gradient
    near = torch.nn.functional.max_pool2d(contributing[:, None].double(), 2 * radius + 1, 1, radius)[:, 0] > 0
    assert not bool(closed[~near].any()) and not bool(b.grad[~near].any())


def test_reference_ignores_non_finite_flows_and_degenerate_frames():
    case = _small_case()
    flow = cr.nonfinite_flow(case)
    assert np.isnan(flow).any() and np.isposinf(flow).any() and np.isneginf(flow).any()
    sums, counts, grad, contributing = cr.run(case, dict(radius=1, scale=255.0), torch.float64, flow)
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(grad).all())
    bad = torch.from_numpy(~np.isfinite(flow).all(axis=3))
    assert not bool(contributing[bad].any()) and not bool(grad[bad].any())
    # H <= 2 radius: nothing contributes, no error
    short = [torch.from_numpy(case[k][:, :6]).double() for k in ("im0", "im1", "flow")]
    sums, counts, contributing = cr.census_ref(*short, radius=3)
    assert not bool(sums.any()) and not bool(counts.any()) and not bool(contributing.any())


@pytest.mark.parametrize("name", sorted(cr.CASES))
def test_case_guarantees_hold_for_every_gpu_case(name):
    """reference() asserts the contributing pixels and the share of pixels that carry a gradient itself (build_case the 10-40 %
    out of frame); here every case of the GPU tests is built and what the tests rely on besides is checked."""
    ref = cr.reference(name)
    case, kw = ref["case"], ref["kw"]
    s64, c64, g64, contributing = ref["run64"]
    s32, c32, g32, _ = ref["run32"]
    r = kw["radius"]
    err32 = float((g32.double() - g64).abs().max()) / max(float(g64.abs().max()), 1e-300)
    print(f"{name}: counts {c64.tolist()}, share of pixels with a gradient {ref['grad_share']:.3f}, float32 torch gradient rel err "
          f"{err32:.3e}, sums rel err {float((s32.double() - s64).abs().max()) / max(float(s64.abs().max()), 1e-300):.3e}")
    assert c32.tolist() == c64.tolist() and bool(torch.isfinite(g64).all())
    border = torch.ones((case["H"], case["W"]), dtype=torch.bool)
    if case["H"] > 2 * r and case["W"] > 2 * r:
        border[r:case["H"] - r, r:case["W"] - r] = False
        assert ref["grad_share"] >= 0.05
    assert not bool(contributing[:, border].any())
    if case["valid"] is not None:
        assert not bool(contributing[torch.from_numpy(~case["valid"])].any())
    if case["empty"] is not None:
        assert float(s64[case["empty"]]) == 0.0 and not bool(g64[case["empty"]].any())
    if name.startswith("5x9"):
        assert not bool(c64.any()) and not bool(s64.any()) and not bool(g64.any())
    if name.startswith("272x256"):                # more tiles than parts: the strided partition takes a second tile
        assert (272 // 8) * (256 // 32) > 256


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
    assert "pwc_census.hip" in _lib.SOURCES
    assert header.index("self-supervised losses") < header.index("pwc_census_sums_f32")


def test_workspace_sizes_and_every_return_code():
    """Host-side answers and argument checks: nothing is launched (the pointers are dummies)."""
    L = _lib.lib()
    # [2][N][parts] partials + 2 (5: with_grad) planes + the in-frame bytes; 32 x 8 tiles, at most 256 parts
    assert L.pwc_census_workspace_floats(2, 23, 37, 0) == 2 * 2 * 6 + 2 * 2 * 23 * 37 + (2 * 23 * 37 + 3) // 4
    assert L.pwc_census_workspace_floats(2, 23, 37, 1) == 2 * 2 * 6 + 5 * 2 * 23 * 37 + (2 * 23 * 37 + 3) // 4
    assert L.pwc_census_workspace_floats(2, 272, 256, 0) == 2 * 2 * 256 + 2 * 2 * 272 * 256 + 2 * 272 * 256 // 4
    assert L.pwc_census_workspace_floats(0, 4, 4, 0) == 0 and L.pwc_census_workspace_floats(1, 4, -1, 1) == 0
    p = ctypes.c_void_p(4096)
    OK_WS = 1 << 20

    def sums(im0=p, im1=p, flow=p, cs=3, flow_cs=2, N=2, H=8, W=8, C=3, r=3, scale=255.0, c1=0.81, c2=0.1, eps=1e-2, q=0.4, ws=p,
             nws=OK_WS, out=p, cnt=p):
        return L.pwc_census_sums_f32(im0, cs, im1, cs, flow, flow_cs, 1.0, None, N, H, W, C, r, scale, c1, c2, eps, q, ws, nws, out,
                                     cnt, None)

    EINVAL, ERANGE, EUNSUPPORTED = -1, -3, -4
    for bad in (dict(im0=None), dict(im1=None), dict(flow=None), dict(N=0), dict(H=0), dict(W=-1), dict(cs=2), dict(flow_cs=1),
                dict(eps=0.0), dict(eps=float("nan")), dict(q=0.0), dict(q=1.5), dict(scale=0.0), dict(scale=-1.0),
                dict(c1=0.0), dict(c1=float("nan")), dict(c2=0.0), dict(c2=-0.1), dict(ws=None), dict(out=None), dict(cnt=None),
                dict(nws=L.pwc_census_workspace_floats(2, 8, 8, 0) - 1)):
        assert sums(**bad) == EINVAL, bad
    for bad in (dict(C=0), dict(C=5, cs=5), dict(r=0), dict(r=4), dict(r=-1)):
        assert sums(**bad) == EUNSUPPORTED, bad
    for bad in (dict(N=65536), dict(H=1 << 16, W=1 << 15)):
        assert sums(**bad) == ERANGE, bad
    assert sums(C=5, cs=2) == EUNSUPPORTED and sums(N=65536, nws=0) == ERANGE       # the order the checks report in

    def grad(dsums=p, dflow=p, dflow_cs=2, C=3, r=3, q=0.4, c2=0.1, N=2, ws=p, nws=OK_WS, cs=3):
        return L.pwc_census_grad_f32(p, cs, p, cs, p, 2, 1.0, None, N, 8, 8, C, r, 255.0, 0.81, c2, 1e-2, q, dsums, ws, nws, dflow,
                                     dflow_cs, 0, None)

    for bad in (dict(dsums=None), dict(dflow=None), dict(dflow_cs=1), dict(q=-0.5), dict(c2=0.0), dict(ws=None), dict(cs=2),
                dict(nws=L.pwc_census_workspace_floats(2, 8, 8, 1) - 1), dict(nws=L.pwc_census_workspace_floats(2, 8, 8, 0))):
        assert grad(**bad) == EINVAL, bad
    assert grad(C=7, cs=7) == EUNSUPPORTED and grad(r=5) == EUNSUPPORTED and grad(N=70000) == ERANGE
    # an image whose last pixels an int pixel index stepped by up to 65536 cannot pass: the shared range check refuses it
    for wide in ((1 << 31) - 1, (1 << 31) - 65536):
        assert sums(H=1, W=wide) == ERANGE and sums(H=1, W=wide, nws=0) == ERANGE
    assert sums(H=1, W=(1 << 31) - 1 - 65536, nws=0) == EINVAL                       # the largest it takes: on to the workspace
    assert L.pwc_census_grad_f32(p, 3, p, 3, p, 2, 1.0, None, 1, 1, (1 << 31) - 1, 3, 3, 255.0, 0.81, 0.1, 1e-2, 0.4, p, p, OK_WS, p, 2, 0,
                                 None) == ERANGE


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
        unsup.census_sums(im, im, fl)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.census_loss(im, im, fl, flow_scale=5.0, radius=1, scale=8.0)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.census_grad(im, im, fl, up)
    # dtype
    with pytest.raises(TypeError, match="float32"):
        unsup.census_sums(im.double(), im, fl)
    with pytest.raises(TypeError, match="float32"):
        unsup.census_loss(im, im.half(), fl)
    with pytest.raises(TypeError, match="float32"):
        unsup.census_grad(im, im, fl.double(), up)
    with pytest.raises(TypeError):
        unsup.census_sums(im, im, np.zeros((N, H, W, 2), np.float32))
    # shape
    with pytest.raises(ValueError, match="channels"):
        unsup.census_sums(im, im, torch.zeros((N, H, W, 3)))
    with pytest.raises(ValueError, match="channels"):
        unsup.census_sums(torch.zeros((N, H, W, 5)), torch.zeros((N, H, W, 5)), fl)
    with pytest.raises(ValueError, match="channels"):
        unsup.census_sums(im, torch.zeros((N, H, W, 1)), fl)
    with pytest.raises(ValueError, match=r"\(N,H,W\)"):
        unsup.census_sums(torch.zeros((N, H + 1, W, 3)), im, fl)
    with pytest.raises(ValueError, match="NHWC"):
        unsup.census_loss(im, im, torch.zeros((H, W, 2)))
    # the mask: grad_ops.mask_ptr's refusals, unchanged
    with pytest.raises(TypeError, match="torch.bool or torch.uint8"):
        unsup.census_sums(im, im, fl, valid=torch.ones((N, H, W)))
    with pytest.raises(ValueError, match="expected shape"):
        unsup.census_sums(im, im, fl, valid=torch.ones((N, H, W + 1), dtype=torch.bool))
    with pytest.raises(ValueError, match="the mask is on"):
        unsup.census_sums(im, im, fl, valid=torch.ones((N, H, W), dtype=torch.bool))
    # images are constants
    for k in range(2):
        ims = [im, im]
        ims[k] = im.clone().requires_grad_(True)
        with pytest.raises(ValueError, match="not implemented"):
            unsup.census_sums(ims[0], ims[1], fl)
    # the term's parameters
    for bad in (dict(eps=0.0), dict(eps=float("nan")), dict(q=0.0), dict(q=1.01), dict(radius=0), dict(radius=4), dict(radius=2.0),
                dict(radius=True), dict(scale=0.0), dict(scale=float("nan")), dict(c1=0.0), dict(c1=-1.0), dict(c2=0.0)):
        with pytest.raises(ValueError, match="eps|q|radius|scale|c1|c2"):
            unsup.census_sums(im, im, fl, **bad)
        with pytest.raises(ValueError, match="eps|q|radius|scale|c1|c2"):
            unsup.census_loss(im, im, fl, **bad)
        with pytest.raises(ValueError, match="eps|q|radius|scale|c1|c2"):
            unsup.census_grad(im, im, fl, up, **bad)


def test_census_is_exported_and_documents_the_centre_rule():
    import pwcnet_amd
    for name in ("census_sums", "census_loss", "census_grad"):
        assert name in pwcnet_amd.__all__ and callable(getattr(pwcnet_amd, name))
    doc = " ".join(pwcnet_amd.census_sums.__doc__.split())
    assert "CENTRES only" in doc and "always read" in doc


# ------------------------------------------------------------------ train.py
def test_train_cli_lists_the_census_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr
    text = " ".join(out.stdout.split())
    assert re.search(r"--photo \{charbonnier,census\}", text), text
    assert "--census_radius" in text
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--photo", "ssim"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert bad.returncode != 0 and "--photo" in bad.stderr
