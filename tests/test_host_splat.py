"""CPU tests of forward splatting: the float64 yardstick of tests/splat_ref.py on hand-computed cases, its explicit gradient formulas
against torch.autograd, the conditions on the inputs that the GPU tests rely on, the C-ABI surface of csrc/pwc_splat.hip with the
return codes of its argument checks, the refusals pwcnet_amd/splat.py raises before it calls the library, and train.py's flags."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from tests import splat_ref as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_splat_workspace_bytes", "pwc_splat_f32", "pwc_splat_grad_f32")


# ------------------------------------------------------------------ the yardstick, by hand
def test_reference_on_a_2x2_frame_with_flow_quarter_half():
    """Every pixel moves by (0.25, 0.5): wx = 0.25, wy = 0.5, the weights are 0.375 (x0) and 0.125 (x0 + 1) on both rows; the
    corners right of column 1 and below row 1 are outside the frame and are dropped one by one."""
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0]]).view(1, 2, 2, 1)
    flow = torch.tensor([0.25, 0.5]).expand(1, 2, 2, 2).contiguous()
    out, cov, cnt = sp.splat_ref(x, flow)
    assert cov.view(2, 2).tolist() == [[0.375, 0.5], [0.75, 1.0]]
    assert out.view(2, 2).tolist() == [[0.375, 0.875], [1.5, 2.75]]
    assert cnt.view(2, 2).tolist() == [[1, 2], [2, 4]]
    avg = sp.splat_ref(x, flow, mode="average")[0]
    assert avg.view(2, 2).tolist() == [[1.0, 1.75], [2.0, 2.75]]
    # weights scale numerator and coverage alike
    w = torch.tensor([[2.0, 1.0], [1.0, 1.0]]).view(1, 2, 2)
    out_w, cov_w, _ = sp.splat_ref(x, flow, w)
    assert cov_w.view(2, 2).tolist() == [[0.75, 0.625], [1.125, 1.125]]
    assert out_w.view(2, 2).tolist() == [[0.75, 1.0], [1.875, 2.875]]


def test_reference_splats_a_point_half_a_pixel_outside_onto_the_border():
    """px = -0.5: x0 = -1 is outside and dropped, column 0 receives the weight 0.5; px = -1 exactly contributes nothing."""
    x = torch.tensor([4.0, 0.0, 0.0]).view(1, 1, 3, 1)
    flow = torch.zeros((1, 1, 3, 2))
    flow[0, 0, 0, 0] = -0.5
    flow[0, 0, 1, 0] = 10.0                       # px = 11: outside
    flow[0, 0, 2, 0] = -3.0                       # px = -1: the open end of (-1, W)
    out, cov, cnt = sp.splat_ref(x, flow)
    assert cov.view(3).tolist() == [0.5, 0.0, 0.0] and out.view(3).tolist() == [2.0, 0.0, 0.0] and cnt.view(3).tolist() == [1, 0, 0]
    assert sp.splat_ref(x, flow, mode="average")[0].view(3).tolist() == [4.0, 0.0, 0.0]


def test_reference_ignores_non_finite_flows_and_masked_pixels():
    x = torch.ones((1, 2, 3, 2))
    flow = torch.zeros((1, 2, 3, 2))
    flow[0, 0, 0, 0] = float("nan")
    flow[0, 0, 1, 1] = float("inf")
    flow[0, 1, 0, 0] = float("-inf")
    valid = torch.ones((1, 2, 3), dtype=torch.bool)
    valid[0, 1, 2] = False
    out, cov, cnt = sp.splat_ref(x, flow, valid=valid)
    want = [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]
    # (cnt counts the in-frame corners, the zero-weight ones of an integer target point included)
    assert cov.view(2, 3).tolist() == want and cnt.view(2, 3).tolist() == [[0, 0, 1], [0, 1, 2]]
    assert out[..., 0].view(2, 3).tolist() == want and bool(torch.isfinite(out).all())
    # ... and their gradients are exact zeros
    dx, dw, df = sp.autograd_grads(x, flow.nan_to_num(0.0, 0.0, 0.0), None, valid, 1.0, "sum", torch.ones_like(x), torch.ones((1, 2, 3)))
    assert not bool(dx[0, 1, 2].any()) and float(dw[0, 1, 2]) == 0.0 and not bool(df[0, 1, 2].any())


def test_flow_scale_enters_as_a_float32():
    flow = torch.full((1, 1, 4, 2), 1.0)
    flow[..., 1] = 0.0
    cov = sp.splat_ref(None, flow, flow_scale=0.3)[1].view(4)
    frac = float(np.float32(0.3))
    assert cov.tolist() == [1 - frac, 1.0, 1.0, 1.0] and frac != 0.3


# ------------------------------------------------------------------ the explicit gradient formulas
@pytest.mark.parametrize("mode", ["sum", "average"])
@pytest.mark.parametrize("name", ["9x13_c3", "24x40_c5"])
def test_explicit_gradients_agree_with_autograd(name, mode):
    """The formulas of include/pwc_hip.h (and, with mode average, the chain rule through num / den) against torch.autograd on the
    restatement, both float64: they agree to rounding, relative to A, the sum of the absolute values of the element's terms."""
    c = sp.case(name)
    flow = c["flow_mid"] if mode == "average" else c["flow"]
    (dx, dw, df), (a_dx, a_dw, a_df), ok = sp.grad_reference(name, mode)
    ex, ew, ef = sp.autograd_grads(c["x"], flow, c["w"], None, sp.FLOW_SCALE, mode, c["g_out"], c["g_cov"])
    for what, got, want, A in (("dx", dx, ex, a_dx), ("dw", dw, ew, a_dw), ("dflow", df, ef, a_df)):
        err = float(((got - want).abs() / A.clamp(min=1e-300)).max())
        print(f"{name} {mode} {what}: max |explicit - autograd| / A = {err:.3e}, max A {float(A.max()):.3e}")
        assert err <= 1e-12 and bool((got.abs() <= A * (1 + 1e-12)).all()) and float(A.max()) > 0
        assert not bool(want[~ok].any()) and not bool(got[~ok].any())          # a pixel that does not contribute: exact zeros
    assert bool((~ok).any())


def test_explicit_gradient_of_a_range_map_agrees_with_autograd():
    """No frame and no weights: the flow's gradient through the coverage alone."""
    c = sp.case("9x13_c1")
    (dx, _, df), (_, _, a_df), ok = sp.splat_grads_ref(None, c["flow"], None, None, 1.0, "sum", None, c["g_cov"])
    _, _, ef = sp.autograd_grads(None, c["flow"], None, None, 1.0, "sum", None, c["g_cov"])
    assert dx is None and float(((df - ef).abs() / a_df.clamp(min=1e-300)).max()) <= 1e-12 and bool(ef.any())
    assert not bool(df[~ok].any()) and bool((~ok).any())


# ------------------------------------------------------------------ what the GPU tests rely on
@pytest.mark.parametrize("name", sorted(sp.CASES))
def test_case_conditions_hold_for_every_gpu_case(name):
    c = sp.case(name)
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    assert (N, H, W) in ((2, 9, 13), (2, 24, 40)) and C in (1, 3, 5)
    assert 0.0 <= float(c["x"].min()) and float(c["x"].max()) <= 1.0
    assert 0.5 <= float(c["w"].min()) and float(c["w"].max()) <= 2.0
    # about a tenth of the pixels leave the frame
    left = sp.left_frame_share(c["flow"])
    out, den, cnt = sp.reference(name, "sum")
    covered = den > 0
    small = covered & (den < sp.MIN_DEN)
    share = float(small.sum()) / float(covered.sum())
    # the average mode's gradient inputs: every positive denominator is well above the fixed point's step
    den_mid = sp.splat_ref(None, c["flow_mid"], c["w"])[1]
    min_mid = float(den_mid[den_mid > 0].min())
    # range_valid: near-ties of the threshold
    near = 0.0
    for f in (c["flow"], c["flow_bw"]):
        r = sp.splat_ref(None, f)[1]
        near = max(near, float(((r - 0.5).abs() <= 1e-6).double().mean()))
    print(f"{name}: {left:.3f} of the pixels leave the frame, most contributions on a target {int(cnt.max())}, covered targets "
          f"{int(covered.sum())}, of them with a denominator below 2^-10 {share:.4f}, smallest positive denominator of the "
          f"mid-cell flow {min_mid:.4f}, share of pixels within 1e-6 of min_range {near:.4f}")
    assert 0.04 <= left <= 0.20
    assert share <= 0.02
    assert min_mid >= sp.MIN_DEN_GRAD
    assert near <= 0.005
    assert int(cnt.max()) >= 3 and bool((cnt == 0).any())             # collisions and holes both occur


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
    assert "pwc_splat.hip" in _lib.SOURCES
    assert header.index("==== occlusion") < header.index("==== forward splatting") < header.index("pwc_splat_f32")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_workspace_size_and_every_return_code():
    """Host-side answers and argument checks: nothing is launched (the pointers are aligned dummies)."""
    L = _lib.lib()
    for N, H, W, C in ((2, 9, 13, 3), (8, 384, 448, 1), (1, 1, 1, 0), (3, 24, 40, 64)):
        assert L.pwc_splat_workspace_bytes(N, H, W, C) == 8 * (N * H * W * (C + 1) + 1)
    assert L.pwc_splat_workspace_bytes(0, 4, 4, 1) == 0 and L.pwc_splat_workspace_bytes(1, 4, 4, -1) == 0
    assert L.pwc_splat_workspace_bytes(1, 4, 4, 65) == 0
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    EINVAL, EALIGN, ERANGE, EUNSUPPORTED = -1, -2, -3, -4
    BIG = 1 << 24

    def fwd(x=p, x_cs=3, flow=p, flow_cs=2, w=None, valid=None, N=2, H=8, W=8, C=3, normalize=0, ws=p, nws=BIG, out=p, out_cs=3,
            cov=p):
        return L.pwc_splat_f32(x, x_cs, flow, flow_cs, 1.0, w, valid, N, H, W, C, normalize, ws, nws, out, out_cs, cov, None)

    need = L.pwc_splat_workspace_bytes(2, 8, 8, 3)
    for bad in (dict(flow=None), dict(x=None), dict(N=0), dict(H=0), dict(W=-1), dict(C=-1), dict(flow_cs=1), dict(x_cs=2),
                dict(cov=None), dict(out=None), dict(out_cs=2), dict(ws=None), dict(nws=need - 1), dict(nws=0)):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(C=65, x_cs=65, out_cs=65) == EUNSUPPORTED
    assert fwd(N=65536) == ERANGE and fwd(H=1 << 16, W=1 << 15) == ERANGE
    assert fwd(ws=odd) == EALIGN
    # the order: sizes, C, strides, the range, the outputs, the workspace
    assert fwd(N=0, C=65) == EINVAL and fwd(C=65, x_cs=2) == EUNSUPPORTED and fwd(flow_cs=1, N=65536) == EINVAL
    assert fwd(N=65536, cov=None) == ERANGE and fwd(cov=None, ws=odd) == EINVAL and fwd(ws=odd, nws=0) == EALIGN

    def grad(x=p, x_cs=3, flow=p, flow_cs=2, N=2, H=8, W=8, C=3, normalize=0, g=p, g_cs=3, gc=p, ws=None, nws=0, dx=p, dx_cs=3, dw=p,
             df=p, df_cs=2):
        return L.pwc_splat_grad_f32(x, x_cs, flow, flow_cs, 1.0, None, None, N, H, W, C, normalize, g, g_cs, gc, ws, nws, dx, dx_cs,
                                    dw, df, df_cs, 0, None)

    for bad in (dict(flow=None), dict(x=None), dict(N=0), dict(C=-2), dict(flow_cs=0), dict(x_cs=1), dict(dx=None, dw=None, df=None),
                dict(g_cs=2), dict(dx_cs=2), dict(df_cs=1), dict(normalize=1), dict(normalize=1, ws=p, nws=need - 1)):
        assert grad(**bad) == EINVAL, bad
    assert grad(C=70, x_cs=70) == EUNSUPPORTED and grad(N=70000) == ERANGE and grad(normalize=1, ws=odd, nws=BIG) == EALIGN
    assert grad(N=70000, dx=None, dw=None, df=None) == ERANGE and grad(g_cs=2, normalize=1) == EINVAL
    # an image whose last pixels an int pixel index stepped by up to 65536 cannot pass: the shared range check refuses it
    for wide in ((1 << 31) - 1, (1 << 31) - 65536):
        assert fwd(N=1, H=1, W=wide) == ERANGE and grad(N=1, H=1, W=wide) == ERANGE
    assert fwd(N=1, H=1, W=(1 << 31) - 1 - 65536, nws=0) == EINVAL                   # the largest it takes: on to the workspace


# ------------------------------------------------------------------ refusals before the library call
def test_python_refusals_come_before_the_library(monkeypatch):
    import pwcnet_amd
    from pwcnet_amd import splat

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    N, H, W = 2, 6, 7
    x, fl, w = torch.zeros((N, H, W, 3)), torch.zeros((N, H, W, 2)), torch.ones((N, H, W))
    mask = torch.ones((N, H, W), dtype=torch.bool)
    # nothing else wrong: CPU tensors are what is refused
    with pytest.raises(ValueError, match="GPU only"):
        splat.forward_splat(x, fl)
    with pytest.raises(ValueError, match="GPU only"):
        splat.forward_splat(x, fl, weights=w, flow_scale=0.5, mode="average")
    with pytest.raises(ValueError, match="GPU only"):
        splat.range_map(fl)
    with pytest.raises(ValueError, match="GPU only"):
        splat.range_valid(fl, fl)
    with pytest.raises(ValueError, match="GPU only"):
        splat.splat_grad(x, fl, x, w)
    # the mode, the threshold
    with pytest.raises(ValueError, match="mode"):
        splat.forward_splat(x, fl, mode="softmax")
    with pytest.raises(ValueError, match="mode"):
        splat.splat_grad(x, fl, x, w, mode="mean")
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="min_range"):
            splat.range_valid(fl, fl, min_range=bad)
    # dtype
    with pytest.raises(TypeError, match="float32"):
        splat.forward_splat(x.double(), fl)
    with pytest.raises(TypeError, match="float32"):
        splat.forward_splat(x, fl.half())
    with pytest.raises(TypeError, match="float32"):
        splat.forward_splat(x, fl, weights=w.double())
    with pytest.raises(TypeError):
        splat.forward_splat(None, fl)
    with pytest.raises(TypeError, match="float32"):
        splat.range_map(fl.double())
    # shape
    with pytest.raises(ValueError, match="channels"):
        splat.forward_splat(x, torch.zeros((N, H, W, 3)))
    with pytest.raises(ValueError, match="channels"):
        splat.forward_splat(torch.zeros((N, H, W, 65)), fl)
    with pytest.raises(ValueError, match=r"\(N,H,W\)"):
        splat.forward_splat(torch.zeros((N, H + 1, W, 3)), fl)
    with pytest.raises(ValueError, match=r"\(N,H,W\)"):
        splat.forward_splat(x, fl, weights=torch.ones((N, H, W, 1)))
    with pytest.raises(ValueError, match=r"\(N,H,W\)"):
        splat.range_valid(fl, torch.zeros((N, H, W + 1, 2)))
    with pytest.raises(ValueError, match="NHWC"):
        splat.range_map(torch.zeros((H, W, 2)))
    # the mask: grad_ops.mask_ptr's refusals
    with pytest.raises(TypeError, match="torch.bool or torch.uint8"):
        splat.forward_splat(x, fl, valid=torch.ones((N, H, W)))
    with pytest.raises(ValueError, match="expected shape"):
        splat.range_map(fl, valid=torch.ones((N, H, W + 1), dtype=torch.bool))
    with pytest.raises(ValueError, match="the mask is on"):
        splat.forward_splat(x, fl, valid=mask)
    # exported, and the docstrings say what the issue asks them to say
    for name in ("forward_splat", "splat_grad", "range_map", "range_valid"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(splat, name)
    doc = " ".join(splat.forward_splat.__doc__.split())
    assert 'weights=torch.exp(alpha * z), mode="average"' in doc and "flow_scale=t" in doc
    assert "nobody has trained with it" in " ".join(splat.range_valid.__doc__.split())
    assert "nobody has trained with it" in " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())


# ------------------------------------------------------------------ train.py
def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), *args], capture_output=True, text=True, timeout=120,
                          cwd=ROOT)


def test_train_cli_takes_occlusion_range():
    out = _cli("--help")
    assert out.returncode == 0, out.stderr
    text = " ".join(out.stdout.split())
    assert "--occ_min_range" in text and re.search(r"--occlusion \{none,fb\}\|range", text), text
    bad = _cli("-d", "synthetic", "--occlusion", "range")                          # the default --loss is supervised
    assert bad.returncode == 2 and "--occlusion range belongs to --loss unsup" in bad.stderr, bad.stderr
    bad = _cli("-d", "synthetic", "--loss", "unsup", "--occlusion", "range", "--occ_min_range", "-1")
    assert bad.returncode == 2 and "--occ_min_range" in bad.stderr, bad.stderr
    bad = _cli("-d", "synthetic", "--loss", "unsup", "--occlusion", "wang")
    assert bad.returncode == 2 and "invalid choice" in bad.stderr, bad.stderr
    bad = _cli("-d", "synthetic", "--loss", "unsup", "--consistency_weight", "0.1")
    assert bad.returncode == 2 and "--consistency_weight needs --occlusion fb or range" in bad.stderr, bad.stderr


def test_train_parser_accepts_range_with_the_consistency_term(monkeypatch):
    """main() parses --occlusion range with --consistency_weight and every ap.error path lets it through: the first thing after
    them is the device, which is where this test stops it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_cli_under_test", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)

    class Reached(Exception):
        pass

    def stop(_device):
        raise Reached()

    monkeypatch.setattr(torch.cuda, "set_device", stop)
    for occlusion in ("range", "fb"):
        monkeypatch.setattr(sys, "argv", ["train.py", "-d", "synthetic", "--loss", "unsup", "--occlusion", occlusion,
                                          "--consistency_weight", "0.2", "--occ_min_range", "0.25"])
        with pytest.raises(Reached):
            train.main()
