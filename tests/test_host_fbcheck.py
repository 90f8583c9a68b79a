"""CPU tests of the forward-backward occlusion masks: the float64 yardstick of tests/fb_ref.py on a scene whose occlusions are
known, the guarantees of its seeded cases (among them the near-tie cap that lets the GPU tests leave near-ties out), the C-ABI
surface of csrc/pwc_fbcheck.hip, every refusal pwcnet_amd.unsup.fb_valid raises before it calls the library, and train.py's
--occlusion flag on the command line."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from tests import fb_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_fb_workspace_floats", "pwc_fb_valid_u8")


# ------------------------------------------------------------------ the yardstick on an analytic scene
def _scene(top, left, H=40, W=48, h=10, w=12, dx=5, dy=3):
    """An h x w foreground rectangle at (top, left) of frame 0 moves by the integer shift (dx, dy) over a static background:
    the ground-truth flows of both directions, per layer, and the rectangle in frame 0 / in frame 1 (clipped to the frame)."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r0 = (ys >= top) & (ys < top + h) & (xs >= left) & (xs < left + w)
    r1 = (ys >= top + dy) & (ys < top + dy + h) & (xs >= left + dx) & (xs < left + dx + w)
    fw, bw = np.zeros((1, H, W, 2), np.float32), np.zeros((1, H, W, 2), np.float32)
    fw[0, r0] = (dx, dy)
    bw[0, r1] = (-dx, -dy)
    exits = r0 & ((xs + dx > W - 1) | (ys + dy > H - 1))
    return torch.from_numpy(fw), torch.from_numpy(bw), r0, r1, exits


def test_reference_marks_exactly_the_occluded_pixels_of_a_moving_rectangle():
    fw, bw, r0, r1, exits = _scene(12, 14)
    assert not exits.any() and int(r0.sum()) == int(r1.sum()) == 120
    a, b = fr.fb_ref(fw, bw)
    covered, uncovered = r1 & ~r0, r0 & ~r1          # background the rectangle covers in frame 1 / background it uncovered
    assert covered.any() and uncovered.any()
    assert np.array_equal(~a.mask[0].numpy(), covered)
    assert np.array_equal(~b.mask[0].numpy(), uncovered)
    assert a.counts.tolist() == [40 * 48 - int(covered.sum())] and b.counts.tolist() == [40 * 48 - int(uncovered.sum())]
    # the same flows stored as px / 5 with flow_scale 5: the same masks
    a5, b5 = fr.fb_ref(fw / 5, bw / 5, flow_scale=5.0)
    assert torch.equal(a5.mask, a.mask) and torch.equal(b5.mask, b.mask)


def test_reference_marks_the_pixels_that_leave_the_frame():
    fw, bw, r0, r1, exits = _scene(12, 34)           # columns 34 .. 45 move to 39 .. 50 of 48: x >= 43 exits
    assert int(exits.sum()) == 10 * 3
    a, b = fr.fb_ref(fw, bw)
    assert np.array_equal(~a.mask[0].numpy(), (r1 & ~r0) | exits)
    assert np.array_equal(~b.mask[0].numpy(), r0 & ~r1)
    assert bool((a.margin[0][torch.from_numpy(exits)] == -float("inf")).all())


def test_reference_zero_flows_are_valid_everywhere():
    z = torch.zeros((2, 40, 48, 2))
    for alphas in ((0.01, 0.5), (0.0, 0.25), (0.0, 0.0)):
        a, b = fr.fb_ref(z, z, 1.0, *alphas)
        assert bool(a.mask.all()) and bool(b.mask.all()) and a.counts.tolist() == [40 * 48] * 2


# ------------------------------------------------------------------ the cases of the GPU tests
@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_case_guarantees_and_near_tie_cap(name):
    """What tests/test_gpu_fbcheck.py relies on.  The cap: at most 0.1 % of the candidates (in frame, unmasked) lie within
    1e-9 * max(1, bound) of the threshold -- a condition on the INPUTS, met by the reference alone; it is what allows the GPU test
    to leave near-ties out without hiding a failure."""
    ref = fr.reference(name)
    case = ref["case"]
    keep = [n for n in range(case["N"]) if n != case["empty"]]
    for key, d in (("a", ref["a"]), ("b", ref["b"])):
        cand = int(d.candidate.sum())
        ties = int(fr.near_ties(d).sum())
        share = float(d.mask[keep].sum()) / int(d.candidate[keep].sum())
        print(f"{name} {key}: candidates {cand} of {d.mask.numel()}, valid share of them {share:.3f}, counts {d.counts.tolist()}, "
              f"near-ties {ties}")
        assert cand > 0 and ties <= 1e-3 * cand
        assert 0.3 <= share <= 0.7
        assert d.counts.tolist() == d.mask.sum(dim=(1, 2)).tolist()
        assert bool((d.margin[~d.candidate] == -float("inf")).all())
        if case["empty"] is not None:
            assert int(d.counts[case["empty"]]) == 0 and not bool(d.candidate[case["empty"]].any())
    for own, key, valid in (("fw", "a", case["valid_fw"]), ("bw", "b", case["valid_bw"])):
        if valid is not None:
            assert 0.6 < float(valid.mean()) < 0.8
            assert np.isnan(case[own + "_nan"]).any() and np.isfinite(case[own + "_nan"][valid]).all()
            assert not bool(ref[key].mask[torch.from_numpy(~valid)].any())
        if case["nonfinite"]:
            bad = torch.from_numpy(~np.isfinite(case[own]).all(axis=3))
            assert int(bad.sum()) >= 5 and not bool(ref[key].mask[bad].any()) and not bool(ref[key].candidate[bad].any())
    if case["valid_fw"] is not None:
        # the NaN behind the masks is where no candidate reads: the reference does not move
        a, b = fr.fb_ref(torch.from_numpy(case["fw_nan"]), torch.from_numpy(case["bw_nan"]), case["flow_scale"], *case["alphas"],
                         torch.from_numpy(case["valid_fw"]), torch.from_numpy(case["valid_bw"]))
        assert torch.equal(a.mask, ref["a"].mask) and torch.equal(b.mask, ref["b"].mask)
        assert torch.equal(a.margin, ref["a"].margin) and torch.equal(b.margin, ref["b"].margin)


# ------------------------------------------------------------------ C ABI
def test_header_declares_the_entries_and_they_are_bound():
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert "occlusion" in header
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
    assert "pwc_fbcheck.hip" in _lib.SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= exported


def test_workspace_sizes_and_argument_checks_need_no_gpu():
    """Per direction a float and an int32 per part of every image, and N floats for the final sum; every code is returned before
    any launch (null or tiny arguments, no GPU here)."""
    L = _lib.lib()
    assert L.pwc_fb_workspace_floats(2, 23, 37) == 2 * (2 * 2 * 4 + 2)
    assert L.pwc_fb_workspace_floats(8, 448, 1024) == 2 * (2 * 8 * 256 + 8)
    assert L.pwc_fb_workspace_floats(0, 4, 4) == 0
    p = ctypes.c_void_p(4096)

    def call(fa=p, a_cs=2, fb=p, b_cs=2, N=2, H=8, W=8, a1=0.01, a2=0.5, va=p, vb=p, ca=p, cb=p, ws=p, nws=1 << 20):
        return L.pwc_fb_valid_u8(fa, a_cs, fb, b_cs, 1.0, None, None, N, H, W, a1, a2, va, vb, ca, cb, ws, nws, None)

    einval, erange = -1, -3
    assert call(fa=None) == einval and call(fb=None) == einval and call(va=None) == einval
    assert call(N=0) == einval and call(H=0) == einval and call(W=-1) == einval
    assert call(a_cs=1) == einval and call(b_cs=0) == einval
    assert call(a1=-0.01) == einval and call(a2=-0.5) == einval
    assert call(a1=float("nan")) == einval and call(a2=float("nan")) == einval
    assert call(nws=3) == einval and call(ws=None) == einval and call(ca=None, nws=3) == einval and call(cb=None, nws=3) == einval
    assert call(vb=None) == einval                      # counts of a direction that is not computed
    assert call(N=65536) == erange and call(H=1 << 16, W=1 << 15) == erange
    assert call(N=65536, nws=0) == erange               # the range is reported before the workspace
    assert call(N=0, H=1 << 16, W=1 << 15) == einval    # ... and the sizes before the range
    # an image whose last pixels the int pixel index cannot step over (it advances by up to 65536 past them)
    assert call(H=1, W=(1 << 31) - 1) == erange and call(H=1, W=(1 << 31) - 65536, nws=0) == erange
    assert call(H=1, W=(1 << 31) - 1 - 65536, nws=0) == einval      # the largest it can: on to the workspace check


# ------------------------------------------------------------------ refusals before the library call
def test_python_refusals_come_before_the_library_and_the_device_last(monkeypatch):
    from pwcnet_amd import unsup

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    N, H, W = 2, 6, 7
    fl = torch.zeros((N, H, W, 2))
    ok_mask = torch.ones((N, H, W), dtype=torch.bool)
    # nothing else wrong: CPU tensors are what is refused
    with pytest.raises(ValueError, match="GPU only"):
        unsup.fb_valid(fl, fl)
    with pytest.raises(ValueError, match="GPU only"):
        unsup.fb_valid(fl, fl.clone().requires_grad_(True), flow_scale=5.0, alpha1=0.0, alpha2=0.25, return_counts=True)
    # dtype
    with pytest.raises(TypeError, match="float32"):
        unsup.fb_valid(fl.double(), fl)
    with pytest.raises(TypeError, match="float32"):
        unsup.fb_valid(fl, fl.half())
    with pytest.raises(TypeError):
        unsup.fb_valid(fl, np.zeros((N, H, W, 2), np.float32))
    # shape
    with pytest.raises(ValueError, match="channels"):
        unsup.fb_valid(torch.zeros((N, H, W, 3)), fl)
    with pytest.raises(ValueError, match="NHWC"):
        unsup.fb_valid(fl, torch.zeros((H, W, 2)))
    for other in (torch.zeros((N, H + 1, W, 2)), torch.zeros((N, H, W - 1, 2)), torch.zeros((N + 1, H, W, 2))):
        with pytest.raises(ValueError, match=r"\(N,H,W\)"):
            unsup.fb_valid(fl, other)
    # the alphas
    for bad in (dict(alpha1=-0.01), dict(alpha2=-0.5), dict(alpha1=float("nan")), dict(alpha2=float("nan"))):
        with pytest.raises(ValueError, match="alpha"):
            unsup.fb_valid(fl, fl, **bad)
    # the masks: grad_ops.mask_ptr's refusals
    for key in ("valid_fw", "valid_bw"):
        with pytest.raises(TypeError, match="torch.bool or torch.uint8"):
            unsup.fb_valid(fl, fl, **{key: torch.ones((N, H, W))})
        with pytest.raises(ValueError, match="expected shape"):
            unsup.fb_valid(fl, fl, **{key: torch.ones((N, H, W + 1), dtype=torch.bool)})
        with pytest.raises(ValueError, match="contiguous"):
            unsup.fb_valid(fl, fl, **{key: torch.ones((N, W, H), dtype=torch.bool).transpose(1, 2)})
        with pytest.raises(ValueError, match="the mask is on"):
            unsup.fb_valid(fl, fl, **{key: ok_mask})
    # a fault of another kind wins over the device
    with pytest.raises(ValueError, match="alpha"):
        unsup.fb_valid(fl, fl, alpha2=-1.0, valid_fw=ok_mask)


def test_fb_valid_is_exported():
    import pwcnet_amd
    assert "fb_valid" in pwcnet_amd.__all__ and callable(pwcnet_amd.fb_valid)
    assert pwcnet_amd.fb_valid is pwcnet_amd.unsup.fb_valid


# ------------------------------------------------------------------ train.py
def test_train_cli_lists_the_occlusion_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr
    text = " ".join(out.stdout.split())
    assert re.search(r"--occlusion \{none,fb\}", text), text
    for flag in ("--occ_alpha1", "--occ_alpha2"):
        assert flag in text, flag


def test_train_cli_refuses_occlusion_without_the_label_free_loss():
    for loss in ((), ("--loss", "robust")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "--occlusion", "fb", *loss],
                             capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert out.returncode == 2, (out.returncode, out.stderr)
        assert "--occlusion fb belongs to --loss unsup" in out.stderr, out.stderr
