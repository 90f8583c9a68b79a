"""Cost-volume feature normalisation without a GPU: the float64 restatement the GPU tests compare against (tests/featnorm_ref.py),
the C ABI's host-side answers and argument checks, the kwargs' way into the four model classes, the CLIs' flags, and the
conditions the GPU model tests rest on."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from tests import featnorm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_feature_norm_workspace_bytes", "pwc_feature_norm_parts", "pwc_feature_norm_f32", "pwc_feature_norm_grad_f32")


# ------------------------------------------------------------------ the restatement
def test_restatement_is_layer_norm_over_the_concatenated_pair():
    f0, f1 = (torch.from_numpy(a).double() for a in R.lrelu_maps((3, 5, 7, 6), 1))
    for eps in (1e-16, 1e-5):
        y0, y1, mean, rstd = R.feature_norm(f0, f1, eps)
        x = torch.stack([f0, f1], dim=1)                                     # (N, 2, h, w, C): one norm over everything but N
        want = torch.nn.functional.layer_norm(x, x.shape[1:], eps=eps)
        assert float((y0 - want[:, 0]).abs().max()) <= 1e-13 and float((y1 - want[:, 1]).abs().max()) <= 1e-13
        assert float((mean - x.reshape(3, -1).mean(1)).abs().max()) <= 1e-15
        assert float((rstd - 1.0 / torch.sqrt(x.reshape(3, -1).var(1, unbiased=False) + eps)).abs().max()) <= 1e-13


def test_restatement_by_hand_on_a_1x1x2_pair():
    """f0 = (1, 2), f1 = (3, 6): M = 4, mean 3, var (4 + 1 + 0 + 9) / 4 = 3.5."""
    f0 = torch.tensor([[[[1.0, 2.0]]]], dtype=torch.float64)
    f1 = torch.tensor([[[[3.0, 6.0]]]], dtype=torch.float64)
    y0, y1, mean, rstd = R.feature_norm(f0, f1, eps=0.0)
    s = 3.5 ** 0.5
    assert float(mean) == 3.0 and abs(float(rstd) - 1.0 / s) <= 1e-16
    assert np.allclose(y0.numpy().ravel(), [-2.0 / s, -1.0 / s], rtol=0, atol=1e-15)
    assert np.allclose(y1.numpy().ravel(), [0.0, 3.0 / s], rtol=0, atol=1e-15)


def test_restatement_of_a_constant_pair_is_exactly_zero():
    for c in (0.1, -3.7, 1e-3, 65000.0):
        v = float(np.float32(c))
        f = torch.full((2, 3, 5, 4), v, dtype=torch.float64)
        y0, y1, mean, rstd = R.feature_norm(f, f.clone())
        assert not bool(y0.any()) and not bool(y1.any()) and float(mean[0]) == v and float(rstd[0]) == 1e8


def test_explicit_gradient_formula_is_autograds():
    """dx = rstd (g - a - xh b), the formula the kernel evaluates, against autograd through the two-pass restatement."""
    f0, f1 = R.lrelu_maps((2, 3, 5, 4), 2)
    g0, g1 = R.lrelu_maps((2, 3, 5, 4), 3, shift=-0.4)
    d0, d1, A0, A1 = R.feature_norm_grads(f0, f1, g0, g1)
    y0, y1, mean, rstd = R.feature_norm_np(f0, f1)
    M = 2 * f0[0].size
    for n in range(2):
        a = (g0[n].astype(np.float64).sum() + g1[n].astype(np.float64).sum()) / M
        b = ((g0[n] * y0[n]).sum() + (g1[n] * y1[n]).sum()) / M
        for g, y, d, A in ((g0, y0, d0, A0), (g1, y1, d1, A1)):
            want = rstd[n] * (g[n] - a - y[n] * b)
            assert np.abs(want - d[n]).max() <= 1e-13 * A[n].max() and bool((np.abs(d[n]) <= A[n] * (1 + 1e-12)).all())


# ------------------------------------------------------------------ C ABI
def test_header_declares_the_entries_and_they_are_bound():
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
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
    assert "pwc_featnorm.hip" in _lib.SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_partition_is_a_function_of_the_level_only():
    L = _lib.lib()
    # at most 1024 groups of four per frame: one part, no workspace
    for H, W, C in ((1, 2, 192), (5, 7, 16), (3, 5, 3), (1, 1, 1), (4, 8, 128)):
        assert L.pwc_feature_norm_parts(H, W, C) == 1 and L.pwc_feature_norm_workspace_bytes(7, H, W, C) == 0
    for (H, W, C), parts in (((16, 32, 32), 16), ((28, 64, 32), 56), ((9, 31, 15), 5), ((4, 8, 129), 5), ((112, 256, 32), 256)):
        assert L.pwc_feature_norm_parts(H, W, C) == parts == min(256, -(-(-(-H * W * C // 4)) // 256))
        for N in (1, 2, 9):
            assert L.pwc_feature_norm_workspace_bytes(N, H, W, C) == 16 * N * parts
    assert L.pwc_feature_norm_parts(0, 4, 4) == 0 and L.pwc_feature_norm_parts(1 << 16, 1 << 15, 1) == 0
    assert L.pwc_feature_norm_workspace_bytes(0, 16, 32, 32) == 0 and L.pwc_feature_norm_workspace_bytes(1, 16, 32, -1) == 0


def test_every_return_code():
    """Argument checks only: nothing is launched (the pointers are aligned dummies)."""
    L = _lib.lib()
    p, odd4, odd1 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    EINVAL, EALIGN, ERANGE = -1, -2, -3
    BIG = 1 << 24
    need = L.pwc_feature_norm_workspace_bytes(2, 16, 32, 32)

    def fwd(f0=p, f0_cs=32, f1=p, f1_cs=32, N=2, H=16, W=32, C=32, eps=1e-16, ws=p, nws=BIG, y0=p, y0_cs=32, y1=p, y1_cs=32, stats=p):
        return L.pwc_feature_norm_f32(f0, f0_cs, f1, f1_cs, N, H, W, C, eps, ws, nws, y0, y0_cs, y1, y1_cs, stats, None)

    for bad in (dict(f0=None), dict(f1=None), dict(y0=None), dict(y1=None), dict(stats=None), dict(N=0), dict(H=0), dict(W=-1),
                dict(C=0), dict(f0_cs=31), dict(f1_cs=8), dict(y0_cs=31), dict(y1_cs=0), dict(eps=-1e-16), dict(eps=float("nan")),
                dict(ws=None), dict(nws=need - 1), dict(nws=0)):
        assert fwd(**bad) == EINVAL, bad
    for bad in (dict(f0=odd1), dict(f1=odd1), dict(y0=odd1), dict(y1=odd1), dict(stats=odd4), dict(ws=odd4)):
        assert fwd(**bad) == EALIGN, bad
    assert fwd(N=65536) == ERANGE and fwd(H=1 << 16, W=1 << 15, C=1, f0_cs=1, f1_cs=1, y0_cs=1, y1_cs=1) == ERANGE
    # the order: nulls and sizes, strides and eps, float alignment, the range, stats, the workspace
    assert fwd(N=0, f0_cs=1) == EINVAL and fwd(f0_cs=1, f0=odd1) == EINVAL and fwd(f0=odd1, N=65536) == EALIGN
    assert fwd(N=65536, stats=odd4) == ERANGE and fwd(stats=odd4, ws=None) == EALIGN and fwd(ws=odd4, nws=0) == EALIGN

    def grad(f0=p, f0_cs=32, f1=p, f1_cs=32, g0=p, g0_cs=32, g1=p, g1_cs=32, stats=p, N=2, H=16, W=32, C=32, ws=p, nws=BIG, d0=p,
             d0_cs=32, d1=p, d1_cs=32, acc=0):
        return L.pwc_feature_norm_grad_f32(f0, f0_cs, f1, f1_cs, g0, g0_cs, g1, g1_cs, stats, N, H, W, C, ws, nws, d0, d0_cs, d1,
                                           d1_cs, acc, None)

    for bad in (dict(f0=None), dict(f1=None), dict(g0=None), dict(g1=None), dict(d0=None), dict(d1=None), dict(stats=None),
                dict(N=-1), dict(H=0), dict(W=0), dict(C=0), dict(f0_cs=31), dict(f1_cs=31), dict(g0_cs=31), dict(g1_cs=31),
                dict(d0_cs=31), dict(d1_cs=31), dict(ws=None), dict(nws=need - 1)):
        assert grad(**bad) == EINVAL, bad
    for bad in (dict(f0=odd1), dict(g1=odd1), dict(d0=odd1), dict(stats=odd4), dict(ws=odd4)):
        assert grad(**bad) == EALIGN, bad
    assert grad(N=70000) == ERANGE and grad(N=70000, ws=None) == ERANGE and grad(g0_cs=1, N=70000) == EINVAL


def test_cpu_tensors_and_bad_eps_are_refused_in_python():
    import pwcnet_amd
    from pwcnet_amd.modules import FeatureNormLayer
    assert pwcnet_amd.FeatureNormLayer is FeatureNormLayer and "FeatureNormLayer" in pwcnet_amd.__all__
    f = torch.zeros((1, 2, 3, 4))
    with pytest.raises(_lib.PwcHipError, match="GPU only"):
        FeatureNormLayer()(f, f)
    with pytest.raises(TypeError):
        FeatureNormLayer()(None, f)
    with pytest.raises(_lib.PwcHipError, match="GPU only"):
        FeatureNormLayer()(f, f, with_stats=True)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            FeatureNormLayer(bad)
        with pytest.raises(ValueError, match="eps"):
            pwcnet_amd.PWCDCNet(normalize_features=True, norm_eps=bad)
    assert FeatureNormLayer().eps == 1e-16 and FeatureNormLayer(0).eps == 0.0


# ------------------------------------------------------------------ the kwargs
def test_kwargs_reach_the_four_model_classes():
    import pwcnet_amd
    from pwcnet_amd.train import Trainer
    net = pwcnet_amd.PWCDCNet()
    assert net.normalize_features is False and net.norm_layer.eps == 1e-16               # default off
    net = pwcnet_amd.PWCDCNet(normalize_features=True, norm_eps=1e-6)
    assert net.normalize_features is True and net.norm_layer.eps == 1e-6
    tn = Trainer(device="cpu")
    assert tn.normalize_features is False
    tn = Trainer(device="cpu", normalize_features=True, norm_eps=1e-8)
    assert tn.normalize_features is True and tn.norm_layer.eps == 1e-8
    mod = pwcnet_amd.PWCDCNetModule(device="cpu")
    assert mod._net.normalize_features is False
    mod = pwcnet_amd.PWCDCNetModule(device="cpu", normalize_features=True, norm_eps=1e-7)
    assert mod._net.normalize_features is True and mod._net.norm_layer.eps == 1e-7
    pipe = pwcnet_amd.ForwardPipeline(depth=2, device="cpu", normalize_features=True, norm_eps=1e-9)
    assert len(pipe.nets) == 2 and all(n.normalize_features and n.norm_layer.eps == 1e-9 for n in pipe.nets)
    assert not any(n.normalize_features for n in pwcnet_amd.ForwardPipeline(depth=2, device="cpu").nets)


@pytest.mark.parametrize("script", ["train.py", "infer.py", "infer_continuous.py", "evaluate.py"])
def test_cli_flags(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    text = " ".join(out.stdout.split())
    assert "--normalize_features" in text and "--norm_eps NORM_EPS" in text
    assert "checkpoint carries no marker" in text and "trained with" in text


def test_docs_say_what_the_variant_is():
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    assert "Feature normalisation" in design and "per pair" in design
    assert "nobody has trained with either variant" in design.lower().replace("*", "")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "normalize_features" in readme and "--normalize_features" in readme


# ------------------------------------------------------------------ what the GPU model tests rest on
@pytest.mark.parametrize("use_dc", [False, True])
def test_model_inputs_keep_every_level_away_from_a_vanishing_variance(use_dc):
    """The model tests hold the normalised model to the bounds of the un-normalised one: fair while 1 / std does not amplify the
    features' own rounding, i.e. while std / |mean| >= 2^-4 at every level and pair of the float64 model."""
    ref = R.model_reference(use_dc)
    assert len(ref["level_stats"]) == 5
    ratios = [r for _, _, r in ref["level_stats"]]
    print(f"use_dc={use_dc}: std / |mean| per level (minimum over the pairs): {[round(r, 3) for r in ratios]}")
    assert min(ratios) >= 2.0 ** -4, ratios
    assert np.isfinite(ref["loss"]) and all(bool(torch.isfinite(g).all()) for g in ref["grads"].values())
    # the flag changes the function: the plain model's flows differ
    from tests import util
    plain, _ = util.float64_flows(ref["w"], use_dc, ref["im0"], ref["im1"])
    assert float(np.abs(plain - ref["final"]).max()) > 1e-3
