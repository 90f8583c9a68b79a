"""CPU tests of second-order smoothness and the forward-backward consistency term: the float64 yardstick of tests/unflow_ref.py
against finite differences, the guarantees of its builders for every GPU case, the C-ABI surface (csrc/pwc_unsup.hip,
csrc/pwc_fbcheck.hip), every refusal pwcnet_amd/unsup.py raises before it calls the library, and train.py's two flags on the
command line."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from tests import unflow_ref as uf
from tests import unsup_ref as ur
from tests.test_host_unsup import _finite_differences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_flow_smoothness2_sums_f32", "pwc_flow_smoothness2_grad_f32", "pwc_fb_consistency_workspace_floats",
           "pwc_fb_consistency_sums_f32", "pwc_fb_consistency_grad_workspace_bytes", "pwc_fb_consistency_grad_f32")


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("eps,q", [(1e-3, 0.5), (1e-2, 0.45)])
def test_reference_gradients_agree_with_finite_differences(eps, q):
    """6 x 7, N = 2: autograd through the float64 restatements against central differences -- tests/test_host_unsup.py's bound
    (1e-6 of the largest element) and step (h = 1e-6); every sample coordinate is 0.1 px from a kink, so no difference straddles
    one.  The consistency term with masks, flow_scale 5, with respect to BOTH flows."""
    case = ur.build_case(2, 6, 7, 3, flow_scale=5.0, seed=11, eps=eps, block=2, max_off=1, far=0.0)
    im0 = torch.from_numpy(case["im0"]).double()
    up = torch.tensor(ur.UPSTREAM, dtype=torch.float64)

    def smooth2(fl):
        return (uf.smoothness2_ref(fl, im0, uf.ALPHA, eps, q) * up).sum()

    flow = torch.from_numpy(case["flow"]).double().requires_grad_(True)
    smooth2(flow).backward()
    with torch.no_grad():
        fd = _finite_differences(smooth2, flow.detach().clone())
    err = float((flow.grad - fd).abs().max()) / float(fd.abs().max())
    print(f"smoothness2 eps {eps} q {q}: autograd vs central differences, rel err {err:.3e}, max |grad| {float(fd.abs().max()):.3e}")
    assert float(fd.abs().max()) > 0 and err <= 1e-6

    cc = uf.build_case(2, 6, 7, flow_scale=5.0, seed=11, block=2, max_off=1, noise=0.3)
    vf, vb = torch.from_numpy(cc["valid_fw"]), torch.from_numpy(cc["valid_bw"])
    ua, ub = (torch.tensor(u, dtype=torch.float64) for u in uf.UPSTREAM)

    def cons(fw, bw):
        out = uf.fb_consistency_ref(fw, bw, 5.0, vf, vb, eps, q)
        return (out[0] * ua).sum() + (out[3] * ub).sum()

    fw = torch.from_numpy(cc["fw"]).double().requires_grad_(True)
    bw = torch.from_numpy(cc["bw"]).double().requires_grad_(True)
    cons(fw, bw).backward()
    with torch.no_grad():
        fd_fw = _finite_differences(lambda x: cons(x, bw.detach()), fw.detach().clone())
        fd_bw = _finite_differences(lambda x: cons(fw.detach(), x), bw.detach().clone())
    for what, g, fd in (("fw", fw.grad, fd_fw), ("bw", bw.grad, fd_bw)):
        err = float((g - fd).abs().max()) / float(fd.abs().max())
        print(f"consistency d/d{what} eps {eps} q {q}: autograd vs central differences, rel err {err:.3e}, "
              f"max |grad| {float(fd.abs().max()):.3e}")
        assert float(fd.abs().max()) > 0 and err <= 1e-6, what
    # NaN behind the masks reaches neither a sum nor a gradient
    fw = torch.from_numpy(cc["fw_nan"]).double().requires_grad_(True)
    bw = torch.from_numpy(cc["bw_nan"]).double().requires_grad_(True)
    out = uf.fb_consistency_ref(fw, bw, 5.0, vf, vb, eps, q)
    (out[0].sum() + out[3].sum()).backward()
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[3]).all())
    assert bool(torch.isfinite(fw.grad).all()) and bool(torch.isfinite(bw.grad).all())


def test_second_order_reference_ignores_a_constant_slope_and_small_frames():
    N, H, W, eps, q = 2, 5, 6, 1e-3, 0.5
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ramp = torch.stack([0.3 * xs - 0.2 * ys, 1.5 + 0.1 * ys], dim=2).expand(N, H, W, 2)
    terms = 2 * ((W - 2) * H + (H - 2) * W)
    want = terms * float(np.float32(eps)) ** (2 * float(np.float32(q)))
    assert torch.allclose(uf.smoothness2_ref(ramp, None, 10.0, eps, q), torch.full((N,), want, dtype=torch.float64), rtol=1e-9)
    fl = torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, (1, 3, 3, 2)))
    assert float(uf.smoothness2_ref(fl[:, :2, :2])) == 0.0                      # 2 x 2: nothing
    row = uf.smoothness2_ref(fl[:, :1])                                          # 1 x 3: the x term of the one centre
    assert torch.allclose(row, ur.rho(fl[0, 0, 0] - 2 * fl[0, 0, 1] + fl[0, 0, 2], float(np.float32(eps)), float(np.float32(q))).sum())


# ------------------------------------------------------------------ the cases of the GPU tests
@pytest.mark.parametrize("name", sorted(uf.CASES) + [uf.CONTENTION])
def test_consistency_builder_guarantees_hold_for_every_gpu_case(name):
    """build_case asserts the distance of every sample coordinate to the integers itself; here: the counts are the contributing
    pixels, both gradients are finite and non-zero, the empty image gives 0, the NaN behind the masks does not move the
    reference, and the float32 run takes the same pixels."""
    ref = uf.reference(name)
    case = ref["case"]
    s_a, c_a, in_a, s_b, c_b, in_b, g_fw, g_bw = ref["run64"]
    print(f"{name}: sums fw {s_a.tolist()} bw {s_b.tolist()}, counts fw {c_a.tolist()} bw {c_b.tolist()} of {case['H'] * case['W']}, "
          f"max |d/dfw| {float(g_fw.abs().max()):.3e}, max |d/dbw| {float(g_bw.abs().max()):.3e}")
    assert c_a.tolist() == in_a.sum(dim=(1, 2)).tolist() and c_b.tolist() == in_b.sum(dim=(1, 2)).tolist()
    for g in (g_fw, g_bw):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    for n in range(case["N"]):
        assert (int(c_a[n]) > 0) == (n != case["empty"]) and (int(c_b[n]) > 0) == (n != case["empty"])
    if case["empty"] is not None:
        e = case["empty"]
        assert float(s_a[e]) == 0.0 and float(s_b[e]) == 0.0 and not bool(g_fw[e].any()) and not bool(g_bw[e].any())
    r32 = ref["run32"]
    assert torch.equal(r32[2], in_a) and torch.equal(r32[5], in_b)
    for own, valid, inside in (("fw", case["valid_fw"], in_a), ("bw", case["valid_bw"], in_b)):
        if valid is not None:
            assert 0.6 < float(valid.mean()) < 0.8
            assert np.isnan(case[own + "_nan"]).any() and np.isfinite(case[own + "_nan"][valid]).all()
            assert not bool(inside[torch.from_numpy(~valid)].any())
    if case["valid_fw"] is not None:
        poisoned = dict(case, fw=case["fw_nan"], bw=case["bw_nan"])
        again = uf.consistency_run(poisoned, ref["eps"], ref["q"], torch.float64)
        for x, y in zip(again, ref["run64"]):
            assert torch.equal(x, y)
    if name == uf.CONTENTION:
        # every forward pixel contributes and reads the same four corners (the builder asserts the cell)
        assert c_a.tolist() == [case["H"] * case["W"]] * case["N"]
        x0, y0 = int(uf.CELL[0]), int(uf.CELL[1])
        assert bool((g_bw[:, y0:y0 + 2, x0:x0 + 2] != 0).all())


@pytest.mark.parametrize("name", sorted(uf.SMOOTH_CASES))
def test_smoothness_builder_guarantees_hold_for_every_gpu_case(name):
    ref = uf.smooth_reference(name)
    for key in ("smooth", "smooth_noimg"):
        s64, g64 = ref[key + "64"]
        assert bool(torch.isfinite(s64).all()) and bool((s64 > 0).all())
        assert bool(torch.isfinite(g64).all()) and float(g64.abs().max()) > 0


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
    # the second-order entries take exactly the first-order entries' parameters
    for kind in ("sums", "grad"):
        assert _lib.SIGNATURES[f"pwc_flow_smoothness2_{kind}_f32"] == _lib.SIGNATURES[f"pwc_flow_smoothness_{kind}_f32"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= exported


def test_workspace_sizes_and_argument_checks_need_no_gpu():
    """Every code is returned before any launch (non-null dummy addresses, no GPU here)."""
    L = _lib.lib()
    einval, erange, eunsupported = -1, -3, -4
    p = ctypes.c_void_p(4096)

    # second order: the first-order entries' checks in their order
    def s2(flow=p, cs=2, image=p, ics=3, C=3, alpha=10.0, eps=1e-3, q=0.5, N=2, H=8, W=8, ws=p, nws=1 << 20, out=p):
        return L.pwc_flow_smoothness2_sums_f32(flow, cs, image, ics, C, alpha, eps, q, N, H, W, ws, nws, out, None)

    def g2(flow=p, cs=2, image=p, ics=3, C=3, alpha=10.0, eps=1e-3, q=0.5, N=2, H=8, W=8, ds=p, df=p, dcs=2):
        return L.pwc_flow_smoothness2_grad_f32(flow, cs, image, ics, C, alpha, eps, q, N, H, W, ds, df, dcs, 0, None)

    for f in (s2, g2):
        assert f(flow=None) == einval and f(N=0) == einval and f(H=0) == einval and f(W=-1) == einval and f(cs=1) == einval
        assert f(C=5) == eunsupported and f(C=0) == eunsupported and f(ics=2) == einval
        assert f(eps=0.0) == einval and f(q=0.0) == einval and f(q=1.5) == einval and f(alpha=-1.0) == einval
        assert f(eps=float("nan")) == einval and f(q=float("nan")) == einval
        assert f(N=65536) == erange and f(H=1 << 16, W=1 << 15) == erange
        assert f(N=0, H=1 << 16, W=1 << 15) == einval
    assert s2(nws=1) == einval and s2(ws=None) == einval and s2(out=None) == einval
    assert s2(N=65536, nws=0) == erange                     # the range is reported before the workspace
    # an image whose last pixels the sums loop's int pixel index cannot step over (it advances by up to 65536 past them)
    assert s2(H=1, W=(1 << 31) - 1) == erange and s2(H=1, W=(1 << 31) - 65536, nws=0) == erange
    assert g2(H=1, W=(1 << 31) - 1) == erange
    assert s2(H=1, W=(1 << 31) - 1 - 65536, nws=0) == einval        # the largest it can: on to the workspace check
    assert g2(ds=None) == einval and g2(df=None) == einval and g2(dcs=1) == einval

    # consistency term
    assert L.pwc_fb_consistency_workspace_floats(2, 23, 37) == 2 * (2 * 2 * 4)
    assert L.pwc_fb_consistency_workspace_floats(8, 448, 1024) == 2 * (2 * 8 * 256)
    assert L.pwc_fb_consistency_workspace_floats(0, 4, 4) == 0
    assert L.pwc_fb_consistency_grad_workspace_bytes(2, 23, 37) == 2 * (2 * 23 * 37 * 2 + 1) * 8
    assert L.pwc_fb_consistency_grad_workspace_bytes(2, 0, 37) == 0

    def cs(fa=p, a_cs=2, fb=p, b_cs=2, N=2, H=8, W=8, eps=1e-3, q=0.5, ws=p, nws=1 << 20, sa=p, ca=p, sb=p, cb=p):
        return L.pwc_fb_consistency_sums_f32(fa, a_cs, fb, b_cs, 1.0, None, None, N, H, W, eps, q, ws, nws, sa, ca, sb, cb, None)

    def cg(fa=p, a_cs=2, fb=p, b_cs=2, N=2, H=8, W=8, eps=1e-3, q=0.5, da=p, db=p, ws=p, nws=1 << 20, oa=p, oa_cs=2, ob=p, ob_cs=2):
        return L.pwc_fb_consistency_grad_f32(fa, a_cs, fb, b_cs, 1.0, None, None, N, H, W, eps, q, da, db, ws, nws, oa, oa_cs, ob,
                                             ob_cs, 0, None)

    for f in (cs, cg):
        assert f(fa=None) == einval and f(fb=None) == einval
        assert f(N=0) == einval and f(H=0) == einval and f(W=-1) == einval
        assert f(a_cs=1) == einval and f(b_cs=0) == einval
        assert f(eps=0.0) == einval and f(eps=-1e-3) == einval and f(eps=float("nan")) == einval
        assert f(q=0.0) == einval and f(q=1.0001) == einval and f(q=float("nan")) == einval
        assert f(N=65536) == erange and f(H=1 << 16, W=1 << 15) == erange
        assert f(N=65536, nws=0) == erange                  # the range is reported before the workspace
        assert f(N=0, H=1 << 16, W=1 << 15) == einval       # ... and the sizes before the range
        assert f(ws=None) == einval and f(nws=3) == einval
        assert f(H=1, W=(1 << 31) - 1) == erange and f(H=1, W=(1 << 31) - 65536, nws=0) == erange       # (as s2 above)
        assert f(H=1, W=(1 << 31) - 1 - 65536, nws=0) == einval
    for key in ("sa", "ca", "sb", "cb"):
        assert cs(**{key: None}) == einval
    for key in ("da", "db", "oa", "ob"):
        assert cg(**{key: None}) == einval
    assert cg(oa_cs=1) == einval and cg(ob_cs=0) == einval
    assert cg(ws=ctypes.c_void_p(4100)) == einval           # the fixed-point accumulators are 64-bit words
    assert cg(nws=L.pwc_fb_consistency_grad_workspace_bytes(2, 8, 8) - 1) == einval
    assert cs(nws=L.pwc_fb_consistency_workspace_floats(2, 8, 8) - 1) == einval


# ------------------------------------------------------------------ refusals before the library call
def test_python_refusals_come_before_the_library_and_the_device_last(monkeypatch):
    from pwcnet_amd import unsup

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    N, H, W = 2, 6, 7
    fl = torch.zeros((N, H, W, 2))
    img = torch.zeros((N, H, W, 3))
    up = torch.zeros((N,))
    ok_mask = torch.ones((N, H, W), dtype=torch.bool)
    # the order of the smoothness term
    for bad in (0, 3, -1, 1.5, "2", None, True):
        for call in (lambda o: unsup.smoothness_sums(fl, img, order=o), lambda o: unsup.smoothness_loss(fl, order=o),
                     lambda o: unsup.smoothness_grad(fl, up, order=o)):
            with pytest.raises(ValueError, match="order"):
                call(bad)
    # order 2 with nothing else wrong: CPU tensors are what is refused -- frames below 3 x 3 are no fault
    for order in (1, 2):
        with pytest.raises(ValueError, match="GPU only"):
            unsup.smoothness_sums(fl, img, order=order)
    for shape in ((1, 1, 37, 2), (1, 2, 5, 2), (1, 2, 2, 2), (1, 1, 1, 2)):
        with pytest.raises(ValueError, match="GPU only"):
            unsup.smoothness_loss(torch.zeros(shape), order=2)
    with pytest.raises(ValueError, match="eps"):
        unsup.smoothness_sums(fl, order=2, eps=0.0)
    with pytest.raises(TypeError, match="float32"):
        unsup.smoothness_sums(fl.double(), order=2)

    # the consistency term
    calls = (unsup.fb_consistency_sums, unsup.fb_consistency_loss, lambda a, b, **kw: unsup.fb_consistency_grad(a, b, up, up, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="GPU only"):
            call(fl, fl)
        with pytest.raises(ValueError, match="GPU only"):
            call(fl, fl.clone().requires_grad_(True), flow_scale=5.0, eps=1e-2, q=0.45)
        with pytest.raises(TypeError, match="float32"):
            call(fl.double(), fl)
        with pytest.raises(TypeError, match="float32"):
            call(fl, fl.half())
        with pytest.raises(TypeError):
            call(fl, np.zeros((N, H, W, 2), np.float32))
        with pytest.raises(ValueError, match="channels"):
            call(torch.zeros((N, H, W, 3)), fl)
        with pytest.raises(ValueError, match="NHWC"):
            call(fl, torch.zeros((H, W, 2)))
        for other in (torch.zeros((N, H + 1, W, 2)), torch.zeros((N, H, W - 1, 2)), torch.zeros((N + 1, H, W, 2))):
            with pytest.raises(ValueError, match=r"\(N,H,W\)"):
                call(fl, other)
        for bad in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan"))):
            with pytest.raises(ValueError, match="eps"):
                call(fl, fl, **bad)
        for bad in (dict(q=0.0), dict(q=1.5), dict(q=float("nan"))):
            with pytest.raises(ValueError, match="q must"):
                call(fl, fl, **bad)
        for key in ("valid_fw", "valid_bw"):
            with pytest.raises(TypeError, match="torch.bool or torch.uint8"):
                call(fl, fl, **{key: torch.ones((N, H, W))})
            with pytest.raises(ValueError, match="expected shape"):
                call(fl, fl, **{key: torch.ones((N, H, W + 1), dtype=torch.bool)})
            with pytest.raises(ValueError, match="contiguous"):
                call(fl, fl, **{key: torch.ones((N, W, H), dtype=torch.bool).transpose(1, 2)})
            with pytest.raises(ValueError, match="the mask is on"):
                call(fl, fl, **{key: ok_mask})
        # a fault of another kind wins over the device
        with pytest.raises(ValueError, match="eps"):
            call(fl, fl, eps=-1.0, valid_fw=ok_mask)


def test_new_functions_are_exported():
    import inspect
    import pwcnet_amd
    for name in ("fb_consistency_sums", "fb_consistency_loss", "fb_consistency_grad"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(pwcnet_amd.unsup, name)
    for name in ("smoothness_sums", "smoothness_loss", "smoothness_grad"):
        params = list(inspect.signature(getattr(pwcnet_amd.unsup, name)).parameters.values())
        assert params[-1].name == "order" and params[-1].default == 1, name


# ------------------------------------------------------------------ train.py
def test_train_cli_lists_both_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr
    text = " ".join(out.stdout.split())
    assert re.search(r"--smooth_order \{1,2\}", text), text
    assert "--consistency_weight" in text, text


def test_train_cli_refuses_the_consistency_term_without_the_backward_flow():
    for extra in ((), ("--loss", "unsup")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "--consistency_weight", "0.1", *extra],
                             capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert out.returncode == 2, (out.returncode, out.stderr)
        assert "--consistency_weight needs --occlusion fb" in out.stderr, out.stderr
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "--loss", "unsup", "--smooth_order", "3"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--smooth_order" in out.stderr, out.stderr
