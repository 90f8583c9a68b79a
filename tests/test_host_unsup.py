"""CPU tests of the self-supervised losses: the float64 yardstick of tests/unsup_ref.py against finite differences, the
guarantees of its input builder for every GPU case, the C-ABI surface of csrc/pwc_unsup.hip, every refusal that
pwcnet_amd/unsup.py raises before it calls the library, and train.py's label-free mode on the command line."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from tests import unsup_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_photometric_workspace_floats", "pwc_photometric_sums_f32", "pwc_photometric_grad_f32",
           "pwc_flow_smoothness_workspace_floats", "pwc_flow_smoothness_sums_f32", "pwc_flow_smoothness_grad_f32")


# ------------------------------------------------------------------ the yardstick
def _finite_differences(f, x, h=1e-6):
    g = torch.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + h
        up = float(f(x))
        flat[i] = keep - h
        down = float(f(x))
        flat[i] = keep
        gf[i] = (up - down) / (2 * h)
    return g


@pytest.mark.parametrize("eps,q", [(1e-3, 0.5), (1e-2, 0.45)])
def test_reference_gradients_agree_with_finite_differences(eps, q):
    """6 x 7, N = 2, masked: autograd through the float64 restatements against central differences (h = 1e-6: the truncation
    error is h^2 rho''' ~ 1e-12 / eps^2 relative, rounding 1e-16 / h = 1e-10 of a sum of ~50; every sample coordinate is 0.1
    from a kink, so no difference straddles one)."""
    case = ur.build_case(2, 6, 7, 3, flow_scale=5.0, seed=11, eps=eps, block=2, max_off=1, far=0.0)
    im0, im1 = torch.from_numpy(case["im0"]).double(), torch.from_numpy(case["im1"]).double()
    valid = torch.from_numpy(case["valid"])
    up = torch.tensor(ur.UPSTREAM, dtype=torch.float64)

    def photo(fl):
        return (ur.photometric_ref(im0, im1, fl, 5.0, valid, eps, q)[0] * up).sum()

    def smooth(fl):
        return (ur.smoothness_ref(fl, im0, ur.ALPHA, eps, q) * up).sum()

    for name, f in (("photometric", photo), ("smoothness", smooth)):
        flow = torch.from_numpy(case["flow"]).double().requires_grad_(True)
        f(flow).backward()
        with torch.no_grad():
            fd = _finite_differences(f, flow.detach().clone())
        err = float((flow.grad - fd).abs().max()) / float(fd.abs().max())
        print(f"{name} eps {eps} q {q}: autograd vs central differences, rel err {err:.3e}, max |grad| {float(fd.abs().max()):.3e}")
        assert float(fd.abs().max()) > 0
        assert err <= 1e-6, name
    # a masked pixel has no gradient, whatever its flow holds
    flow = torch.from_numpy(case["flow_nan"]).double().requires_grad_(True)
    sums, counts, inside = ur.photometric_ref(torch.from_numpy(case["im0_nan"]).double(), torch.from_numpy(case["im1_nan"]).double(),
                                              flow, 5.0, valid, eps, q)
    sums.sum().backward()
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(flow.grad).all())
    assert bool((flow.grad[~inside] == 0).all()) and counts.tolist() == case["contributing"].sum(axis=(1, 2)).tolist()


@pytest.mark.parametrize("name", sorted(ur.CASES))
def test_builder_guarantees_hold_for_every_gpu_case(name):
    """build_case asserts the distance to the integers, the out-of-frame share and the contributing pixels itself; here every
    case of the GPU tests is built, and what the tests rely on besides is checked."""
    kw, (eps, q) = ur.CASES[name]
    case = ur.build_case(**kw)
    N, H, W = case["N"], case["H"], case["W"]
    px = np.arange(W)[None, None, :] + np.float64(np.float32(case["flow_scale"])) * case["flow"][..., 0]
    assert float(np.abs(px - np.round(px)).min()) >= 0.1
    oof = ~case["contributing"] if case["valid"] is None else ~case["contributing"] & case["valid"]
    print(f"{name}: out of frame (of the valid pixels) {float(oof.mean()):.3f}, contributing per image "
          f"{case['contributing'].sum(axis=(1, 2)).tolist()}")
    if case["valid"] is not None:
        assert 0.6 < float(case["valid"].mean()) < 0.8
        assert np.isnan(case["flow_nan"][~case["valid"]]).all() and np.isnan(case["im0_nan"][~case["valid"]]).all()
        assert np.isfinite(case["flow_nan"][case["valid"]]).all()
    if case["empty"] is not None:
        assert not case["contributing"][case["empty"]].any()
    ref = ur.reference(name)
    s64, c64, g64 = ref["photo64"]
    assert c64.tolist() == case["contributing"].sum(axis=(1, 2)).tolist()
    assert bool(torch.isfinite(g64).all()) and float(g64.abs().max()) > 0
    if case["empty"] is not None:
        assert float(s64[case["empty"]]) == 0.0 and not bool(g64[case["empty"]].any())


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
    assert "pwc_unsup.hip" in _lib.SOURCES
    # host-side answers and argument checks: nothing is launched
    assert L.pwc_photometric_workspace_floats(2, 23, 37) == 2 * 2 * 4
    assert L.pwc_photometric_workspace_floats(8, 448, 1024) == 2 * 8 * 256
    assert L.pwc_flow_smoothness_workspace_floats(2, 272, 256) == 2 * 256
    assert L.pwc_flow_smoothness_workspace_floats(0, 4, 4) == 0
    p = ctypes.c_void_p(4096)

    def sums(im0=p, cs=3, flow_cs=2, N=2, H=8, W=8, C=3, eps=1e-3, q=0.5, ws=p, nws=1 << 20):
        return L.pwc_photometric_sums_f32(im0, cs, p, cs, p, flow_cs, 1.0, None, N, H, W, C, eps, q, ws, nws, p, p, None)

    assert sums(im0=None) == -1 and sums(ws=None) == -1 and sums(N=0) == -1 and sums(cs=2) == -1 and sums(flow_cs=1) == -1
    assert sums(eps=0.0) == -1 and sums(q=0.0) == -1 and sums(q=1.5) == -1 and sums(eps=float("nan")) == -1 and sums(nws=3) == -1
    assert sums(C=0) == -4 and sums(C=5, cs=5) == -4
    assert sums(N=65536) == -3 and sums(H=1 << 16, W=1 << 15) == -3

    def grad(dsums=p, dflow=p, dflow_cs=2, C=3, q=0.5):
        return L.pwc_photometric_grad_f32(p, 3, p, 3, p, 2, 1.0, None, 2, 8, 8, C, 1e-3, q, dsums, dflow, dflow_cs, 0, None)

    assert grad(dsums=None) == -1 and grad(dflow=None) == -1 and grad(dflow_cs=1) == -1 and grad(q=-0.5) == -1 and grad(C=7) == -4

    def smooth(flow=p, image=p, image_cs=3, C=3, alpha=10.0, eps=1e-3, q=0.5, N=2, H=8, W=8, nws=1 << 20):
        return L.pwc_flow_smoothness_sums_f32(flow, 2, image, image_cs, C, alpha, eps, q, N, H, W, p, nws, p, None)

    assert smooth(flow=None) == -1 and smooth(alpha=-1.0) == -1 and smooth(eps=-1.0) == -1 and smooth(q=2.0) == -1
    assert smooth(image_cs=2) == -1 and smooth(nws=1) == -1 and smooth(C=5, image_cs=5) == -4 and smooth(N=70000) == -3
    # an image whose last pixels the int pixel index of the sums loops cannot step over (it advances by up to 65536 past them):
    # refused; the largest it can is let through to the workspace check
    for f in (sums, smooth):
        assert f(H=1, W=(1 << 31) - 1) == -3 and f(H=1, W=(1 << 31) - 65536) == -3 and f(H=1, W=(1 << 31) - 1, nws=0) == -3
        assert f(H=1, W=(1 << 31) - 1 - 65536, nws=0) == -1

    def sgrad(dsums=p, dflow=p, dflow_cs=2, alpha=10.0):
        return L.pwc_flow_smoothness_grad_f32(p, 2, None, 0, 0, alpha, 1e-3, 0.5, 2, 8, 8, dsums, dflow, dflow_cs, 0, None)

    assert sgrad(dsums=None) == -1 and sgrad(dflow=None) == -1 and sgrad(dflow_cs=0) == -1 and sgrad(alpha=float("nan")) == -1


# ------------------------------------------------------------------ refusals before the library call
def test_python_refusals_need_no(monkeypatch):
    """Every argument fault is raised before the library is called, and the device is looked at last: on a machine without a GPU
    each call below ends in its own refusal, and a call with nothing else wrong in the refusal of CPU tensors."""
    from pwcnet_amd import unsup

    
    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    N, H, W = 2, 6, 7
    im, fl = torch.zeros((N, H, W, 3)), torch.zeros((N, H, W, 2))
    ok_mask = torch.ones((N, H, W), dtype=torch.bool)
    # CPU tensors
    with pytest.raises(ValueError, match="GPU only"):
        unsup.photometric_sums(im, im, fl)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.photometric_loss(im, im, fl, flow_scale=5.0, eps=1e-2, q=0.45)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.smoothness_sums(fl)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.smoothness_loss(fl, im)
    # dtype
    with pytest.raises(TypeError, match="float32"):
        unsup.photometric_sums(im.double(), im, fl)
    with pytest.raises(TypeError, match="float32"):
        unsup.photometric_loss(im, im, fl.half())
    with pytest.raises(TypeError, match="float32"):
        unsup.smoothness_sums(fl, im.to(torch.int32))
    with pytest.raises(TypeError):
        unsup.smoothness_sums(np.zeros((N, H, W, 2), np.float32))
    # shape
    with pytest.raises(ValueError, match="channels"):
        unsup.photometric_sums(im, im, torch.zeros((N, H, W, 3)))
    with pytest.raises(ValueError, match="channels"):
        unsup.photometric_sums(torch.zeros((N, H, W, 5)), torch.zeros((N, H, W, 5)), fl)
    with pytest.raises(ValueError, match="channels"):
        unsup.photometric_sums(im, torch.zeros((N, H, W, 1)), fl)
    with pytest.raises(ValueError, match=r"\(N,H,W\)"):
        unsup.photometric_sums(torch.zeros((N, H + 1, W, 3)), im, fl)
    with pytest.raises(ValueError, match=r"\(N,H,W\)"):
        unsup.smoothness_sums(fl, torch.zeros((N, H, W - 1, 3)))
    with pytest.raises(ValueError, match="NHWC"):
        unsup.smoothness_sums(torch.zeros((H, W, 2)))
    # the mask: grad_ops.mask_ptr's refusals, unchanged
    with pytest.raises(TypeError, match="torch.bool or torch.uint8"):
        unsup.photometric_sums(im, im, fl, valid=torch.ones((N, H, W)))
    with pytest.raises(ValueError, match="expected shape"):
        unsup.photometric_sums(im, im, fl, valid=torch.ones((N, H, W + 1), dtype=torch.bool))
    with pytest.raises(ValueError, match="contiguous"):
        unsup.photometric_sums(im, im, fl, valid=torch.ones((N, W, H), dtype=torch.bool).transpose(1, 2))
    with pytest.raises(ValueError, match="the mask is on"):
        unsup.photometric_sums(im, im, fl, valid=ok_mask)
    # images are constants
    for k in range(2):
        ims = [im, im]
        ims[k] = im.clone().requires_grad_(True)
        with pytest.raises(ValueError, match="not implemented"):
            unsup.photometric_sums(ims[0], ims[1], fl)
    with pytest.raises(ValueError, match="not implemented"):
        unsup.smoothness_sums(fl, im.clone().requires_grad_(True))
    # the robust function's parameters
    for bad in (dict(eps=0.0), dict(eps=-1e-3), dict(eps=float("nan")), dict(q=0.0), dict(q=1.01), dict(q=float("nan"))):
        with pytest.raises(ValueError, match="eps|q"):
            unsup.photometric_sums(im, im, fl, **bad)
        with pytest.raises(ValueError, match="eps|q"):
            unsup.smoothness_loss(fl, **bad)
    with pytest.raises(ValueError, match="alpha"):
        unsup.smoothness_sums(fl, alpha=-1.0)


def test_losses_are_exported():
    import pwcnet_amd
    for name in ("photometric_sums", "photometric_loss", "smoothness_sums", "smoothness_loss"):
        assert name in pwcnet_amd.__all__ and callable(getattr(pwcnet_amd, name))


# ------------------------------------------------------------------ train.py
def test_train_cli_lists_the_label_free_mode():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr
    text = " ".join(out.stdout.split())
    assert re.search(r"--loss \{[^}]*unsup[^}]*\}", text), text
    for flag in ("--smooth_weight", "--photo_eps", "--photo_q", "--edge_alpha"):
        assert flag in text, flag


def test_train_cli_refuses_a_multi_rank_label_free_launch():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "--loss", "unsup"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode != 0
    assert "single process" in out.stderr, out.stderr
