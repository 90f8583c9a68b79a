"""CPU tests of the pyramids: the reference of tests/pyramid_ref.py against hand-computed cases and avg_pool2d in float64, the
order independence of byte sums (what the GPU tests' bit-equality rests on), the `need` arithmetic, every argument check of
pwcnet_amd/pyramid.py on CPU tensors, the C ABI surface and train.py's --level_weights."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pwcnet_amd
from pwcnet_amd import _lib, pyramid
from tests import pyramid_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pwc_frame_pyramid_f32", "pwc_mask_pyramid_u8")


# ------------------------------------------------------------------ the reference
def test_reference_on_hand_computed_cases():
    x = torch.arange(16, dtype=torch.float32).reshape(1, 4, 4, 1)
    p2, p4 = pr.frame_pyramid_ref(x, (2, 4))
    assert p2.dtype == torch.float32 and tuple(p2.shape) == (1, 2, 2, 1) and tuple(p4.shape) == (1, 1, 1, 1)
    assert p2.flatten().tolist() == [2.5, 4.5, 10.5, 12.5] and p4.flatten().tolist() == [7.5]
    b = torch.tensor([[0, 255, 255, 255], [255, 0, 255, 255], [51, 51, 0, 0], [51, 51, 0, 255]], dtype=torch.uint8).reshape(1, 4, 4, 1)
    p2, p4 = pr.frame_pyramid_ref(b, (2, 4))
    fifth = float(np.float32(51.0 / 255.0))
    want4 = (7.0 + 4.0 * fifth) / 16.0
    assert p2.flatten().tolist() == [0.5, 1.0, float(np.float32(fifth)), 0.25]
    assert p4.flatten().tolist() == [float(np.float32(want4))]
    # two channels stay apart, the outputs come in the order asked
    two = torch.stack([x[..., 0], 2 * x[..., 0]], dim=-1)
    q4, q2 = pr.frame_pyramid_ref(two, (4, 2))
    assert q4.flatten().tolist() == [7.5, 15.0] and torch.equal(q2[..., 0], p2_of(x)) and torch.equal(q2[..., 1], 2 * p2_of(x))
    m = torch.tensor([[1, 0, 0, 0], [1, 7, 0, 0], [0, 0, 1, 1], [0, 0, 1, 255]], dtype=torch.uint8).reshape(1, 4, 4)
    masks, counts = pr.mask_pyramid_ref(m, (2, 4), 1.0)
    assert counts[0].flatten().tolist() == [3, 0, 0, 4] and counts[1].flatten().tolist() == [7]
    assert masks[0].flatten().tolist() == [False, False, False, True] and masks[1].flatten().tolist() == [False]
    masks, _ = pr.mask_pyramid_ref(m, (2, 4), 0.4)                    # need 2 of 4, 7 of 16
    assert masks[0].flatten().tolist() == [True, False, False, True] and masks[1].flatten().tolist() == [True]


def p2_of(x):
    return pr.frame_pyramid_ref(x, (2,))[0][..., 0]


def test_reference_is_avg_pool2d_in_float64():
    for name in ("n2_64x128x3", "128x64x4"):
        for frames in (pr.byte_frames(name), pr.signed_frames(name)):
            x = pr.to_float(frames).double().permute(0, 3, 1, 2)
            for f, got in zip(pr.DEFAULT, pr.frame_pyramid_ref(frames, pr.DEFAULT)):
                want = torch.nn.functional.avg_pool2d(x, f).permute(0, 2, 3, 1)
                # (two float64 orders of the same sum: a few ulps of float64 apart before the one rounding to float32)
                assert float((got.double() - want).abs().max()) <= float(np.spacing(np.float32(want.abs().max()))), (name, f)
    # the byte conversion is the float32 nearest v / 255, for all 256 values
    v = torch.arange(256, dtype=torch.uint8)
    assert np.array_equal(pr.to_float(v).numpy(), (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32))


def test_byte_sums_do_not_depend_on_the_order():
    """Every summand float32(v / 255) is a multiple of 2^-31 and at most 1; a 64 x 64 block sums to at most 4096: 43 bits, under
    double's 53.  So every partial sum is exact and any order gives the same double."""
    vals = pr.to_float(torch.arange(256, dtype=torch.uint8)).double().numpy()
    scaled = vals * 2.0 ** 31
    assert np.array_equal(scaled, np.rint(scaled)) and vals.max() == 1.0
    rs = np.random.RandomState(5)
    block = vals[rs.randint(0, 256, size=4096)]
    total = np.sum(np.rint(block * 2.0 ** 31).astype(np.int64))        # the exact sum, in integers
    for order in (np.arange(4096), np.arange(4096)[::-1], rs.permutation(4096), np.argsort(block), np.argsort(-block)):
        acc = 0.0
        for t in block[order]:
            acc += t
        assert acc * 2.0 ** 31 == float(total)
    frames = pr.byte_frames("n2_64x128x3")
    perm = torch.from_numpy(rs.permutation(64))
    for f, ref in zip(pr.DEFAULT, pr.byte_ref("n2_64x128x3")):
        x = pr.to_float(frames).double()
        N, H, W, C = x.shape
        blocks = x.reshape(N, H // f, f, W // f, f, C)
        shuffled = blocks[:, :, perm[perm < f]][:, :, :, :, perm[perm < f]]
        seq = torch.zeros((N, H // f, W // f, C), dtype=torch.float64)
        for i in range(f):
            for j in range(f):
                seq += shuffled[:, :, i, :, j]
        assert torch.equal((seq / (f * f)).float().view(torch.int32), ref.view(torch.int32)), f


def test_need_arithmetic():
    fs = (2, 4, 8, 16, 32, 64)
    assert pyramid.need_counts(fs, 1.0) == [f * f for f in fs]
    assert pyramid.need_counts(fs, 0.5) == [f * f // 2 for f in fs]
    assert pyramid.need_counts(fs, 1.0 / 4096) == [1, 1, 1, 1, 1, 1]
    assert pyramid.need_counts(fs, 0.3) == [2, 5, 20, 77, 308, 1229]
    for f in fs:
        for frac in (1.0, 0.5, 1.0 / 4096, 0.3):
            assert pyramid.need_counts((f,), frac) == [pr.need_ref(f, frac)]
    for bad in (0.0, 1.5, -0.25, float("nan")):
        with pytest.raises(ValueError, match="min_fraction"):
            pyramid.need_counts(fs, bad)


# ------------------------------------------------------------------ argument checks, on CPU tensors
def test_argument_checks_come_before_the_device_and_the_library():
    fr = torch.zeros((1, 64, 128, 3), dtype=torch.uint8)
    va = torch.ones((1, 64, 128), dtype=torch.bool)
    with pytest.raises(TypeError, match="float64"):
        pyramid.frame_pyramid(fr.double())
    with pytest.raises(TypeError, match="ndarray"):
        pyramid.frame_pyramid(fr.numpy())
    with pytest.raises(TypeError, match="float32"):
        pyramid.mask_pyramid(va.float())
    with pytest.raises(ValueError, match=r"\(1, 64, 128, 5\)"):
        pyramid.frame_pyramid(torch.zeros((1, 64, 128, 5)))
    with pytest.raises(ValueError, match=r"\(64, 128, 3\)"):
        pyramid.frame_pyramid(fr[0])
    with pytest.raises(ValueError, match=r"\(1, 64, 128, 3\)"):
        pyramid.mask_pyramid(fr)
    for call, t in ((pyramid.frame_pyramid, fr), (pyramid.mask_pyramid, va)):
        with pytest.raises(ValueError, match="factor 3 "):
            call(t, (4, 3))
        with pytest.raises(ValueError, match="factor 128 "):
            call(t, (128,))
        with pytest.raises(ValueError, match="twice"):
            call(t, (8, 4, 8))
        with pytest.raises(ValueError, match="1 to 6 factors"):
            call(t, ())
        with pytest.raises(TypeError, match="4.0"):
            call(t, (4.0,))
        with pytest.raises(ValueError, match="largest factor 64, got 96 x 128"):
            call(torch.zeros((1, 96, 128) + tuple(t.shape[3:]), dtype=t.dtype))
        with pytest.raises(ValueError, match="largest factor 16, got 64 x 24"):
            call(torch.zeros((1, 64, 24) + tuple(t.shape[3:]), dtype=t.dtype), (16, 2))
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match=f"min_fraction must lie in .* got {bad}"):
            pyramid.mask_pyramid(va, min_fraction=bad)
    with pytest.raises(ValueError, match="contiguous"):
        pyramid.frame_pyramid(torch.zeros((1, 64, 128, 6), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="contiguous"):
        pyramid.mask_pyramid(torch.ones((1, 128, 64), dtype=torch.bool).transpose(1, 2))
    with pytest.raises(ValueError, match="no gradient"):
        pyramid.frame_pyramid(torch.zeros((1, 64, 128, 3), requires_grad=True))
    # the device, last of all: a CPU tensor that passes everything else
    with pytest.raises(ValueError, match="is on cpu"):
        pyramid.frame_pyramid(fr)
    with pytest.raises(ValueError, match="is on cpu"):
        pyramid.mask_pyramid(va, (8, 2), min_fraction=0.5, return_counts=True)
    assert pyramid.level_flow_scale(torch.zeros((2, 6, 7, 2)), (384, 448)) == 20.0 / 64
    assert pyramid.level_flow_scale(torch.zeros((2, 16, 32, 2)), (64, 128)) == 5.0
    for name in ("frame_pyramid", "mask_pyramid", "level_flow_scale"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(pyramid, name)
    assert "No autograd" in pyramid.frame_pyramid.__doc__ and "No autograd" in pyramid.__doc__
    assert "nobody has trained with it" in " ".join(pyramid.mask_pyramid.__doc__.split())


# ------------------------------------------------------------------ C ABI
def test_header_declares_the_entries_and_they_are_bound():
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/pwc_hip.h"
        want = [ctypes.c_void_p if ("*" in arg or arg.strip().startswith("pwc_stream_t")) else ctypes.c_int for arg in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == want, name
        assert getattr(L, name).argtypes == want
    assert "pwc_pyramid.hip" in _lib.SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_every_return_code():
    """Host-side argument checks: nothing is launched (the pointers are aligned dummies, every call is refused)."""
    L = _lib.lib()
    EINVAL, EALIGN, ERANGE, EUNSUPPORTED = -1, -2, -3, -4
    p, odd = 4096, 4098

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*v)

    def frames(x=p, u8=1, N=1, H=64, W=64, C=3, factors=(64, 4), outs=(p, p), n=None):
        return L.pwc_frame_pyramid_f32(x, u8, N, H, W, C, ints(*factors) if factors else None, ptrs(*outs) if outs else None,
                                       len(factors) if n is None else n, None)

    for bad in (dict(x=None), dict(outs=None), dict(N=0), dict(H=0), dict(W=-64), dict(factors=None, n=2), dict(n=0), dict(n=7),
                dict(factors=(4, 4)), dict(H=96), dict(W=32), dict(outs=(p, None))):
        assert frames(**bad) == EINVAL, bad
    for bad in (dict(C=0), dict(C=5), dict(factors=(3, 4)), dict(factors=(128, 4)), dict(factors=(0, 4)), dict(factors=(1, 4))):
        assert frames(**bad) == EUNSUPPORTED, bad
    assert frames(x=odd, u8=0) == EALIGN and frames(outs=(p, odd)) == EALIGN
    assert frames(N=1 << 8, H=1 << 12, W=1 << 12, C=1) == ERANGE
    # the order: sizes, C, the factors, divisibility, alignment, the range
    assert frames(N=0, C=5) == EINVAL and frames(C=5, factors=(4, 4)) == EUNSUPPORTED and frames(factors=(3, 3), H=96) == EUNSUPPORTED
    assert frames(H=96, x=odd, u8=0) == EINVAL and frames(x=odd, u8=0, N=1 << 8, H=1 << 12, W=1 << 12, C=1) == EALIGN

    def masks(v=p, N=1, H=64, W=64, factors=(64, 4), need=(4096, 8), outs=(p, p), counts=None):
        return L.pwc_mask_pyramid_u8(v, N, H, W, ints(*factors), ints(*need) if need else None, ptrs(*outs) if outs else None,
                                     ptrs(*counts) if counts else None, len(factors), None)

    for bad in (dict(v=None), dict(outs=None), dict(need=None), dict(N=0), dict(H=32), dict(factors=(4, 4)), dict(need=(4097, 8)),
                dict(need=(4096, 0)), dict(outs=(None, p))):
        assert masks(**bad) == EINVAL, bad
    assert masks(factors=(5, 4)) == EUNSUPPORTED
    assert masks(counts=(p, odd)) == EALIGN
    assert masks(N=1 << 8, H=1 << 12, W=1 << 12) == ERANGE


# ------------------------------------------------------------------ train.py
def test_train_parser_takes_five_level_weights(monkeypatch):
    """main() parses --level_weights with five values and every ap.error path lets it through: the first thing after them is the
    device, which is where this test stops it.  Four values, a negative one and the supervised losses are refused."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_cli_under_test", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)

    class Reached(Exception):
        pass

    def stop(_device):
        raise Reached()

    monkeypatch.setattr(torch.cuda, "set_device", stop)
    base = ["train.py", "-d", "synthetic", "--loss", "unsup"]
    five = ["--level_weights", "0.32", "0.08", "0.02", "0.01", "0.005"]
    for extra in ([], ["--occlusion", "range", "--occ_pool", "1.0"], ["--photo", "census", "--occlusion", "fb"]):
        monkeypatch.setattr(sys, "argv", base + five + extra)
        with pytest.raises(Reached):
            train.main()
    for argv, message in ((base + five[:-1], "expected 5 arguments"),
                          (base + ["--level_weights", "1", "1", "1", "1", "-1"], "--level_weights must be non-negative"),
                          (["train.py", "-d", "synthetic"] + five, "--level_weights belongs to --loss unsup"),
                          (base + five + ["--output_level", "5"], "--output_level 4"),
                          (base + five + ["--occ_pool", "0"], "--occ_pool must be in")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, *argv[:1]), *argv[1:]], capture_output=True, text=True, timeout=120,
                             cwd=ROOT)
        assert out.returncode == 2 and message in out.stderr, (argv, out.stderr)
    doc = " ".join(train.__doc__.split())
    assert "--level_weights W0 W1 W2 W3 W4" in doc and "nobody has trained with it yet" in doc
