"""GPU tests of the frame and mask pyramids (csrc/pwc_pyramid.hip, pwcnet_amd/pyramid.py) against the float64 restatement of
tests/pyramid_ref.py (validated on the CPU by tests/test_host_pyramid.py), on its cases: the smallest shapes at which the
indexing can still go wrong.

Bounds.  Byte frames and float32 frames that are multiples of 2^-16: BIT-EQUAL to the reference -- every partial sum is exact in
double, so any order gives the correctly rounded mean (a float32 accumulator does not, and fails here).  Arbitrary non-negative
float32: within one float32 spacing at |ref| (two single roundings of double sums that differ by at most 2^-40 * mean|x|).
Signed: spacing(ref) + 2^-40 * mean|x| of the block (cancellation can leave a mean far below its summands).  Masks and counts:
equal to the integer reference."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pyramid_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(pr.FRAME_CASES)


@pytest.fixture(scope="module")
def py():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import pyramid
    return pyramid


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _same_bits(got, ref, what):
    assert len(got) == len(ref), what
    for f, g, r in zip(what[1], got, ref):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(r.shape) and g.is_contiguous(), (what, f)
        differ = _bits(g) != r.view(torch.int32)
        assert not bool(differ.any()), (what, f, int(differ.sum()), float((g.cpu() - r).abs().max()))


# ------------------------------------------------------------------ frames
@pytest.mark.parametrize("name", NAMES)
def test_byte_frames_are_bit_equal_to_the_reference(py, name):
    factors = pr.FRAME_CASES[name][1]
    frames = pr.byte_frames(name)
    ref = pr.byte_ref(name)
    got = py.frame_pyramid(frames.cuda(), factors)
    _same_bits(got, ref, (name, factors, "uint8"))
    # the float32 path fed the same values (the division on the host: the float32 nearest v / 255)
    got32 = py.frame_pyramid(pr.to_float(frames).cuda(), factors)
    _same_bits(got32, ref, (name, factors, "float32"))


@pytest.mark.parametrize("name", NAMES)
def test_dyadic_float_frames_are_bit_equal_to_the_reference(py, name):
    factors = pr.FRAME_CASES[name][1]
    frames = pr.dyadic_frames(name)
    _same_bits(py.frame_pyramid(frames.cuda(), factors), pr.frame_pyramid_ref(frames, factors), (name, factors, "dyadic"))


@pytest.mark.parametrize("name", ["n2_64x128x3", "128x64x4", "16x24_f8_2"])
def test_arbitrary_float_frames_are_within_one_rounding(py, name):
    factors = pr.FRAME_CASES[name][1]
    for kind, frames in (("positive", pr.positive_frames(name)), ("signed", pr.signed_frames(name))):
        ref = pr.frame_pyramid_ref(frames, factors)
        mean_abs = pr.frame_pyramid_ref(frames.abs(), factors)
        got = py.frame_pyramid(frames.cuda(), factors)
        for f, g, r, m in zip(factors, got, ref, mean_abs):
            err = (g.cpu().double() - r.double()).abs()
            bound = torch.from_numpy(np.spacing(r.abs().numpy())).double()
            if kind == "signed":
                bound = bound + 2.0 ** -40 * m.double()
            print(f"{name} {kind} f={f}: max err / bound {float((err / bound).max()):.3f}, exact {float((err == 0).double().mean()):.4f}")
            assert bool((err <= bound).all()), (name, kind, f)


def test_non_finite_inputs_stay_in_their_cells(py):
    name = "n2_64x128x3"
    factors = pr.FRAME_CASES[name][1]
    clean = pr.dyadic_frames(name)
    frames = clean.clone()
    frames[0, 5, 70, 1] = float("nan")
    frames[1, 63, 0, 2] = float("inf")
    frames[1, 0, 127, 0] = float("-inf")
    bad = torch.zeros_like(frames)
    bad[~torch.isfinite(frames)] = 1.0
    ref = pr.frame_pyramid_ref(frames, factors)
    got = py.frame_pyramid(frames.cuda(), factors)
    for f, g, r in zip(factors, got, ref):
        g = g.cpu()
        hit = pr.block_sums(bad.double(), f) > 0
        assert int(hit.sum()) == 3 and torch.equal(~torch.isfinite(g), hit) and torch.equal(~torch.isfinite(r), hit), f
        assert torch.equal(_bits(g)[~hit], r.view(torch.int32)[~hit]), f
    _same_bits(py.frame_pyramid(clean.cuda(), factors), pr.frame_pyramid_ref(clean, factors), (name, factors, "clean again"))


def test_two_calls_and_batching_give_the_same_bits(py):
    name = "n2_64x128x3"
    for frames in (pr.byte_frames(name), pr.signed_frames(name)):
        x = frames.cuda()
        a, b = py.frame_pyramid(x), py.frame_pyramid(x)
        singles = [py.frame_pyramid(x[n:n + 1].contiguous()) for n in range(x.shape[0])]
        for l in range(len(a)):
            assert torch.equal(_bits(a[l]), _bits(b[l]))
            assert torch.equal(_bits(a[l]), _bits(torch.cat([s[l] for s in singles])))


# ------------------------------------------------------------------ masks
def _check_masks(py, valid, factors, what):
    for frac in pr.MIN_FRACTIONS:
        want_m, want_c = pr.mask_pyramid_ref(valid, factors, frac)
        masks, counts = py.mask_pyramid(valid.cuda(), factors, min_fraction=frac, return_counts=True)
        only = py.mask_pyramid(valid.cuda(), factors, min_fraction=frac)
        for f, m, c, o, wm, wc in zip(factors, masks, counts, only, want_m, want_c):
            assert m.dtype == torch.bool and c.dtype == torch.int32 and m.is_contiguous() and tuple(m.shape) == tuple(wm.shape)
            assert torch.equal(c.cpu(), wc), (what, frac, f)
            assert torch.equal(m.cpu(), wm) and torch.equal(o.cpu(), wm), (what, frac, f)
            assert int(m.view(torch.uint8).max()) <= 1


@pytest.mark.parametrize("name", NAMES)
def test_masks_and_counts_equal_the_integer_reference(py, name):
    (N, H, W, _), factors = pr.FRAME_CASES[name]
    for density in pr.DENSITIES:
        _check_masks(py, pr.random_mask(name, density), factors, (name, density))


def test_constant_masks_and_bytes_other_than_0_and_1(py):
    name = "n2_64x128x3"
    (N, H, W, _), factors = pr.FRAME_CASES[name]
    _check_masks(py, torch.ones((N, H, W), dtype=torch.bool), factors, "ones")
    _check_masks(py, torch.zeros((N, H, W), dtype=torch.bool), factors, "zeros")
    m = pr.random_mask(name, 0.5)
    values = torch.from_numpy(np.random.RandomState(9).randint(1, 256, size=(N, H, W)).astype(np.uint8))
    as_bytes = values * m.to(torch.uint8)
    assert int(as_bytes.max()) > 1 and torch.equal(as_bytes != 0, m)
    _check_masks(py, as_bytes, factors, "uint8 values")
    want = pr.mask_pyramid_ref(m, factors, 0.5)[0]
    for g, w in zip(py.mask_pyramid(as_bytes.cuda(), factors, min_fraction=0.5), want):
        assert torch.equal(g.cpu(), w)


# ------------------------------------------------------------------ with the existing terms
def test_level_losses_train_the_module_bit_reproducibly(py):
    """(2, 64, 128, 3) frames: photometric_loss on every pyramid level under pooled masks, weights (1, 1, 1, 1, 1), backward.
    The gradient is finite, is not the final-only gradient, and is the same bits on a second run."""
    from pwcnet_amd import PWCDCNetModule, unsup
    from tests import util
    im0, im1 = (torch.from_numpy(a).cuda() for a in util.smooth_images(2, 64, 128))
    valid = pr.random_mask("n2_64x128x3", 0.9).cuda()
    pyr0, pyr1 = py.frame_pyramid(im0), py.frame_pyramid(im1)
    mpyr = py.mask_pyramid(valid, min_fraction=0.5)
    runs = []
    for levels in (True, True, False):
        model = PWCDCNetModule(seed=3)
        final, flows_pyramid = model(im0, im1)
        assert [tuple(f.shape[1:3]) for f in flows_pyramid] == [tuple(p.shape[1:3]) for p in pyr0]
        loss = unsup.photometric_loss(im0, im1, final, valid=valid)
        if levels:
            for l, fl in enumerate(flows_pyramid):
                loss = loss + unsup.photometric_loss(pyr0[l], pyr1[l], fl, flow_scale=py.level_flow_scale(fl, (64, 128)),
                                                     valid=mpyr[l])
        loss.backward()
        runs.append((loss.detach().clone(), model.flat.grad.clone()))
    torch.cuda.synchronize()
    (loss, grad), (loss2, grad2), (loss_f, grad_f) = runs
    print(f"loss {float(loss):.6f} (final only {float(loss_f):.6f}), |grad| max {float(grad.abs().max()):.3e}, "
          f"|grad - final only| max {float((grad - grad_f).abs().max()):.3e}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    assert not torch.equal(grad, grad_f)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


# ------------------------------------------------------------------ train.py
def _train(tmp_path, *flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                          "64", "128", "--synthetic_pairs", "6", "--loss", "unsup", *flags, "--model_dir", str(tmp_path)],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    steps = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 2, steps                       # 6 pairs: 1 for validation, 5 to train on, batch 2, drop_last
    return steps


def test_train_cli_zero_level_weights_are_the_run_as_it_was(tmp_path):
    plain = _train(tmp_path / "a")
    zeros = _train(tmp_path / "b", "--level_weights", "0", "0", "0", "0", "0")
    assert plain == zeros and not any("levels" in ln for ln in plain)


def test_train_cli_level_weights(tmp_path):
    flags = ("--photo", "census", "--occlusion", "range", "--level_weights", "0.32", "0.08", "0.02", "0.01", "0.005")
    first, second = _train(tmp_path / "a", *flags), _train(tmp_path / "b", *flags)
    for ln in first:
        m = re.search(r"loss/unsup (\S+)  census (\S+)  smoothness (\S+)  occluded (\S+)  levels (\S+) (\S+) (\S+) (\S+) (\S+)$", ln)
        assert m, ln
        assert all(np.isfinite(float(v)) for v in m.groups()[:3]), ln
        levels = [float(v) for v in m.groups()[4:]]
        # --census_radius 3: the 1 x 2, 2 x 4 and 4 x 8 levels hold no window (nan, nothing added), 8 x 16 and 16 x 32 do
        assert all(np.isnan(v) for v in levels[:3]) and all(np.isfinite(v) and v > 0 for v in levels[3:]), ln
    assert first == second
