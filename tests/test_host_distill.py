"""CPU tests of the self-supervision (flow distillation) feature: the float64 restatement tests/distill_ref.py against hand values
and its closed-form gradient, every refusal pwcnet_amd.unsup.flow_distill_* raises before it calls the library, the library's own
argument checks (they return before any launch), UnsupObjective's selfsup_mask modes and train.py's --selfsup_* flags."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import distill_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def _hand_case():
    """A 2 x 2 student inside a 3 x 4 teacher at (1, 2).  Window pixels: (0,0) d = (3, -4); (0,1) teacher_valid 0; (1,0)
    excluded; (1,1) d = (0, 0)."""
    teacher = torch.zeros((1, 3, 4, 2), dtype=torch.float32)
    teacher[0, 1, 2] = torch.tensor([1.0, 6.0])
    teacher[0, 1, 3] = torch.tensor([5.0, 5.0])
    teacher[0, 2, 2] = torch.tensor([7.0, 7.0])
    teacher[0, 2, 3] = torch.tensor([-2.0, 0.5])
    teacher[0, 0, 0] = float("nan")                                       # outside the window: never read
    student = torch.tensor([[[[4.0, 2.0], [9.0, 9.0]], [[1.0, 1.0], [-2.0, 0.5]]]], dtype=torch.float32)
    teacher_valid = torch.ones((1, 3, 4), dtype=torch.uint8)
    teacher_valid[0, 1, 3] = 0
    exclude = torch.zeros((1, 2, 2), dtype=torch.uint8)
    exclude[0, 1, 0] = 1
    return student, teacher, teacher_valid, exclude


def test_restatement_against_hand_values():
    student, teacher, tv, ex = _hand_case()
    eps = 0.5
    # q = 1: rho(d) = d^2 + eps^2
    sums, counts = R.distill_sums(student, teacher, (1, 2), tv, ex, eps=eps, q=1.0)
    assert int(counts[0]) == 2
    assert float(sums[0]) == (9.0 + 0.25) + (16.0 + 0.25) + 0.25 + 0.25
    # q = 0.5: sqrt(d^2 + eps^2)
    sums, _ = R.distill_sums(student, teacher, (1, 2), tv, ex, eps=eps, q=0.5)
    assert abs(float(sums[0]) - (np.sqrt(9.25) + np.sqrt(16.25) + 0.5 + 0.5)) <= 1e-14
    assert abs(float(R.distill_loss(student, teacher, (1, 2), tv, ex, eps=eps, q=0.5)) - float(sums[0]) / 4.0) <= 1e-15
    # no masks: all four pixels
    sums, counts = R.distill_sums(student, teacher, (1, 2), eps=eps, q=1.0)
    assert int(counts[0]) == 4
    assert float(sums[0]) == 25.5 + (16.0 + 16.0 + 0.5) + (36.0 + 36.0 + 0.5) + 0.5
    # the closed-form gradient, by hand: 2 q d (d^2 + eps^2)^(q - 1) with q = 1 is 2 d
    g = R.distill_grad(student, teacher, torch.tensor([3.0]), (1, 2), tv, ex, eps=eps, q=1.0)
    assert g[0, 0, 0].tolist() == [18.0, -24.0] and g[0, 0, 1].tolist() == [0.0, 0.0]
    assert g[0, 1, 0].tolist() == [0.0, 0.0] and g[0, 1, 1].tolist() == [0.0, 0.0]


def test_restatement_leaves_unknown_and_non_finite_pixels_out():
    student, teacher, _, _ = _hand_case()
    teacher[0, 1, 2, 0] = 1e10                                            # the .flo sentinel
    teacher[0, 1, 3, 1] = float("inf")
    teacher[0, 2, 2, 0] = float("nan")
    student[0, 1, 1, 1] = float("nan")
    sums, counts = R.distill_sums(student, teacher, (1, 2), eps=0.5, q=0.5)
    assert int(counts[0]) == 0 and float(sums[0]) == 0.0
    assert float(R.distill_loss(student, teacher, (1, 2), eps=0.5, q=0.5)) == 0.0
    teacher[0, 1, 2, 0] = 1e9                                             # at the threshold: known
    sums, counts = R.distill_sums(student, teacher, (1, 2), eps=0.5, q=0.5)
    assert int(counts[0]) == 1 and bool(torch.isfinite(sums).all())
    s = student.clone().requires_grad_(True)
    R.distill_sums(s, teacher, (1, 2), eps=0.5, q=0.5)[0].sum().backward()
    assert bool(torch.isfinite(s.grad).all()) and int((s.grad != 0).sum()) == 2


@pytest.mark.parametrize("q,eps", [(0.5, 1e-3), (0.4, 1e-2), (1.0, 0.5)])
def test_restatement_autograd_equals_the_closed_form(q, eps):
    student, teacher, tv, ex = R.random_case(3, 5, 7, 9, 13, seed=11)
    student[1, 2, 3, 0] = float("nan")
    dsums = torch.tensor([0.5, -2.0, 3.0], dtype=torch.float64)
    for kw in (dict(), dict(teacher_valid=tv), dict(exclude=ex), dict(teacher_valid=tv, exclude=ex)):
        s = student.double().requires_grad_(True)
        sums, counts = R.distill_sums(s, teacher, (2, 3), eps=eps, q=q, **kw)
        (sums * dsums).sum().backward()
        ref = R.distill_grad(student, teacher, dsums, (2, 3), eps=eps, q=q, **kw)
        assert bool(torch.isfinite(s.grad).all())
        assert float((s.grad - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
        share = counts.double() / 35.0
        assert 0.1 <= float(share.min()) and float(share.max()) <= 0.9, (kw.keys(), share)


# ------------------------------------------------------------------ pwcnet_amd.unsup: refusals before any library call
def test_python_functions_refuse_bad_arguments_on_the_cpu():
    import pwcnet_amd as P
    s = torch.zeros((2, 5, 7, 2))
    t = torch.zeros((2, 9, 13, 2))
    for fn in (P.flow_distill_sums, P.flow_distill_loss):
        with pytest.raises(ValueError, match="eps must be positive"):
            fn(s, t, eps=0.0)
        with pytest.raises(ValueError, match=r"q must be in \(0, 1\]"):
            fn(s, t, q=1.5)
        with pytest.raises(TypeError, match="student"):
            fn(s.double(), t)
        with pytest.raises(TypeError, match="teacher"):
            fn(s, t.half())
        with pytest.raises(ValueError, match="student"):
            fn(torch.zeros((2, 5, 7, 3)), t)
        with pytest.raises(ValueError, match="teacher"):
            fn(s, torch.zeros((2, 9, 13)))
        with pytest.raises(ValueError, match="student: empty"):
            fn(torch.zeros((2, 0, 7, 2)), t)
        with pytest.raises(ValueError, match="teacher: expected a batch of 2"):
            fn(s, torch.zeros((3, 9, 13, 2)))
        for offset in ((5, 0), (0, 7), (-1, 0), (0, -1)):
            with pytest.raises(ValueError, match="offset: the 5 x 7 student"):
                fn(s, t, offset)
        for offset in (3, (1, 2, 3), (1.0, 2), (True, 0), None):
            with pytest.raises(ValueError, match="offset: expected a pair"):
                fn(s, t, offset)
        with pytest.raises(TypeError, match="teacher_valid"):
            fn(s, t, teacher_valid=torch.zeros((2, 9, 13)))
        with pytest.raises(ValueError, match="teacher_valid: expected shape"):
            fn(s, t, teacher_valid=torch.zeros((2, 5, 7), dtype=torch.bool))
        with pytest.raises(TypeError, match="exclude"):
            fn(s, t, exclude=torch.zeros((2, 5, 7), dtype=torch.int32))
        with pytest.raises(ValueError, match="exclude: expected shape"):
            fn(s, t, exclude=torch.zeros((2, 9, 13), dtype=torch.uint8))
        with pytest.raises(ValueError, match="exclude: the mask must be contiguous"):
            fn(s, t, exclude=torch.zeros((2, 7, 5), dtype=torch.uint8).transpose(1, 2))
        # everything else in order: the device is what is left (no fallback to the CPU)
        with pytest.raises(ValueError, match="student: the tensor is on cpu"):
            fn(s, t, (4, 6), torch.ones((2, 9, 13), dtype=torch.bool), torch.zeros((2, 5, 7), dtype=torch.uint8))
    with pytest.raises(ValueError, match="flow_distill_grad: eps"):
        P.flow_distill_grad(s, t, torch.ones(2), eps=-1.0)
    with pytest.raises(ValueError, match="offset"):
        P.flow_distill_grad(s, t, torch.ones(2), offset=(5, 7))
    with pytest.raises(ValueError, match="student: the tensor is on cpu"):
        P.flow_distill_grad(s, t, torch.ones(2))


def test_library_refuses_before_any_launch():
    from pwcnet_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN, ERANGE = -1, -2, -3
    p, odd, half = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    assert L.pwc_flow_distill_workspace_bytes(3, 5, 7) == 3 * 1 * 12
    assert L.pwc_flow_distill_workspace_bytes(2, 16, 17) == 2 * 2 * 12            # 272 pixels: two parts
    assert L.pwc_flow_distill_workspace_bytes(1, 1024, 1024) == 256 * 12          # at most 256 parts
    assert L.pwc_flow_distill_workspace_bytes(0, 5, 7) == 0 and L.pwc_flow_distill_workspace_bytes(1, 0, 7) == 0

    def sums(student=p, s_cs=2, teacher=p, t_cs=2, N=2, h=5, w=7, H=9, W=13, y0=2, x0=3, eps=1e-3, q=0.5, out=p, counts=p, ws=p,
             ws_bytes=1 << 20):
        return L.pwc_flow_distill_sums_f32(student, s_cs, teacher, t_cs, N, h, w, H, W, y0, x0, None, None, eps, q, out, counts, ws,
                                           ws_bytes, None)

    def grad(student=p, s_cs=2, teacher=p, t_cs=2, N=2, h=5, w=7, H=9, W=13, y0=2, x0=3, eps=1e-3, q=0.5, dsums=p, d=p, d_cs=2):
        return L.pwc_flow_distill_grad_f32(student, s_cs, teacher, t_cs, N, h, w, H, W, y0, x0, None, None, eps, q, dsums, d, d_cs, 0,
                                           None)

    shared = (dict(student=None), dict(teacher=None), dict(N=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(s_cs=1),
              dict(t_cs=1), dict(y0=-1), dict(x0=-1), dict(y0=5), dict(x0=7), dict(h=10), dict(w=14), dict(y0=2 ** 31 - 1),
              dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(q=0.0), dict(q=1.5), dict(q=float("nan")))
    for fn in (sums, grad):
        for bad in shared:
            assert fn(**bad) == EINVAL, (fn.__name__, bad)
        assert fn(N=65536) == ERANGE
        assert fn(N=1, h=1 << 16, w=1 << 15, H=1 << 16, W=1 << 15, y0=0, x0=0) == ERANGE
        assert fn(N=1, H=1 << 16, W=1 << 15) == ERANGE                             # the teacher alone is too large
        # a row whose last pixels the sums loop's int pixel index cannot step over (it advances by up to 65536 past them)
        for wide in ((1 << 31) - 1, (1 << 31) - 65536):
            assert fn(N=1, h=1, w=wide, H=1, W=wide, y0=0, x0=0) == ERANGE
            assert fn(N=1, h=1, w=7, H=1, W=wide, y0=0, x0=0) == ERANGE
        assert fn(student=odd) == EALIGN and fn(teacher=odd) == EALIGN
    most = (1 << 31) - 1 - 65536                                                   # the largest it can: on to the workspace check
    assert sums(N=1, h=1, w=most, H=1, W=most, y0=0, x0=0, ws_bytes=0) == EINVAL
    assert L.pwc_flow_distill_workspace_bytes(1, 1, (1 << 31) - 1) == 0 and L.pwc_flow_distill_workspace_bytes(1, 1, most) == 256 * 12
    for bad in (dict(out=None), dict(counts=None), dict(ws=None), dict(ws_bytes=2 * 12 - 1)):
        assert sums(**bad) == EINVAL, bad
    assert sums(ws=half) == EALIGN                                                 # off an 8-byte boundary
    for bad in (dict(dsums=None), dict(d=None), dict(d_cs=1)):
        assert grad(**bad) == EINVAL, bad
    assert grad(d=odd) == EALIGN and grad(dsums=odd) == EALIGN


# ------------------------------------------------------------------ UnsupObjective
def test_objective_selfsup_mask_modes():
    from pwcnet_amd import UnsupObjective
    assert UnsupObjective().selfsup_mask == "all"
    assert UnsupObjective(occlusion="fb").selfsup_mask == "occluded"
    assert UnsupObjective(occlusion="range").selfsup_mask == "occluded"
    for occlusion in ("fb", "range"):
        for mode in ("occluded", "teacher", "all"):
            assert UnsupObjective(occlusion=occlusion, selfsup_mask=mode).selfsup_mask == mode
    assert UnsupObjective(selfsup_mask="all").selfsup_mask == "all"
    for mode in ("occluded", "teacher"):
        with pytest.raises(ValueError, match="needs occlusion"):
            UnsupObjective(selfsup_mask=mode)
    with pytest.raises(ValueError, match="selfsup_mask must be"):
        UnsupObjective(occlusion="fb", selfsup_mask="soft")
    # the masks a mode reads must be there: refused before any tensor is looked at
    s, t = torch.zeros((4, 5, 7, 2)), torch.zeros((4, 9, 13, 2))
    m = (torch.ones((2, 9, 13), dtype=torch.bool),) * 2
    with pytest.raises(ValueError, match="needs teacher_masks"):
        UnsupObjective(occlusion="fb").selfsup_term(s, t, (2, 3))
    with pytest.raises(ValueError, match="needs student_masks"):
        UnsupObjective(occlusion="fb").selfsup_term(s, t, (2, 3), teacher_masks=m)
    with pytest.raises(ValueError, match="needs teacher_masks"):
        UnsupObjective(occlusion="range", selfsup_mask="teacher").selfsup_term(s, t, (2, 3))
    # "all" reads no mask and goes straight to the term, which refuses CPU tensors
    with pytest.raises(ValueError, match="student: the tensor is on cpu"):
        UnsupObjective(occlusion="fb", selfsup_mask="all").selfsup_term(s, t, (2, 3))


# ------------------------------------------------------------------ train.py
def test_train_parser_selfsup_flags(monkeypatch, capsys):
    """main() lets the good combinations through all its ap.error checks -- the first thing after them is the device, which is
    where this test stops it -- and refuses each bad one with exit status 2 and a message that names the flag."""
    spec = importlib.util.spec_from_file_location("train_cli_under_test", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)

    class Reached(Exception):
        pass

    def stop(_device):
        raise Reached()

    monkeypatch.setattr(torch.cuda, "set_device", stop)
    base = ["train.py", "-d", "synthetic", "--loss", "unsup"]
    on = ["--selfsup_weight", "0.3"]
    for extra in ([], on, on + ["--occlusion", "fb"], on + ["--occlusion", "range", "--selfsup_mask", "teacher"],
                  on + ["--selfsup_mask", "all", "--selfsup_after", "100"],
                  on + ["--crop_shape", "128", "192", "--selfsup_crop", "32", "--occlusion", "fb"],
                  ["--crop_shape", "128", "192"],                        # flag off: the default crop of 64 is not looked at
                  ["--selfsup_weight", "0", "--crop_shape", "64", "128"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(Reached):
            train.main()
    for argv, message in ((["train.py", "-d", "synthetic"] + on, "--selfsup_weight belongs to --loss unsup"),
                          (base + ["--selfsup_weight", "-0.1"], "--selfsup_weight must be non-negative"),
                          (base + on + ["--selfsup_crop", "0"], "--selfsup_crop must be positive"),
                          (base + on + ["--selfsup_crop", "-32"], "--selfsup_crop must be positive"),
                          (base + on + ["--crop_shape", "128", "192"], "positive multiple of 64"),          # 0 x 64
                          (base + on + ["--selfsup_crop", "48"], "positive multiple of 64"),                # 288 x 352
                          (base + on + ["--crop_shape", "384", "192", "--selfsup_crop", "96"], "positive multiple of 64"),
                          (base + on + ["--selfsup_mask", "occluded"], "needs --occlusion fb or range"),
                          (base + on + ["--selfsup_mask", "teacher"], "needs --occlusion fb or range"),
                          (base + on + ["--selfsup_mask", "soft"], "invalid choice"),
                          (base + on + ["--selfsup_after", "-1"], "--selfsup_after must be non-negative")):
        monkeypatch.setattr(sys, "argv", argv)
        with pytest.raises(SystemExit) as exit_info:
            train.main()
        err = capsys.readouterr().err
        assert exit_info.value.code == 2 and message in err, (argv, err)
    doc = " ".join(train.__doc__.split())
    assert "--selfsup_weight W" in doc and "--selfsup_crop C" in doc and "--selfsup_after K" in doc
