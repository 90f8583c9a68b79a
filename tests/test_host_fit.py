"""The frame fit and the flow refit without a GPU: the float64 reference of tests/fit_ref.py (the yardstick of
tests/test_gpu_fit.py) checked against the properties the arithmetic promises, the geometry record of pwcnet_amd.fit, the
library's argument checks (they return before any launch) and the command lines' --fit option.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pwcnet_amd import _lib, fit  # noqa: E402
from tests import fit_ref as R  # noqa: E402
from tests import util  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_uint8_conversion_is_what_the_command_lines_do():
    """float(double(v) / 255.0) is numpy's v.astype(float32) / 255.0 for all 256 values, and so is the kernel's spelling
    float(double(v) * (1.0 / 255.0))."""
    v = np.arange(256, dtype=np.uint8)
    want = bits(v.astype(np.float32) / 255.0)
    assert np.array_equal(bits(R.to_float32(v)), want)
    assert np.array_equal(bits((v.astype(np.float64) * (1.0 / 255.0)).astype(np.float32)), want)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 100, 436, 1242])
def test_axis_that_fits_is_a_copy(n):
    i0, i1, f = R.taps(n, n)
    assert np.array_equal(i0, np.arange(n)) and np.array_equal(f, np.zeros(n)) and f.dtype == np.float64
    assert np.array_equal(i1, np.minimum(np.arange(n) + 1, n - 1))


@pytest.mark.parametrize("inn,out", [(1, 64), (65, 128), (67, 128), (100, 128), (436, 448), (375, 384), (1242, 1280), (128, 65)])
def test_taps_stay_in_the_source(inn, out):
    i0, i1, f = R.taps(inn, out)
    assert i0.min() >= 0 and i1.max() <= inn - 1 and np.all(i1 - i0 <= 1) and np.all(i1 >= i0)
    assert np.all(f >= 0) and np.all(f < 1)
    assert i0[0] == 0 and i1[-1] == inn - 1
    if out >= inn:                                                  # the outermost sample centres lie outside the source's: clamped
        assert f[0] == 0 and i0[-1] == inn - 1 and f[-1] == 0
    assert np.all(np.diff(i0 + f) >= 0)                             # monotone


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_frame_that_fits_is_unchanged(mode, dtype):
    rng = np.random.RandomState(5)
    x = rng.randint(0, 256, size=(2, 64, 128, 3)).astype(np.uint8)
    x = x if dtype == np.uint8 else R.to_float32(x)
    v, S = R.fit_frames(x, mode)
    assert v.shape == x.shape and np.array_equal(v, R.to_float32(x).astype(np.float64))
    flow = util.flow_field(2, 64, 128)
    v, _ = R.refit_flow(flow, 64, 128, mode)
    assert np.array_equal(v, flow.astype(np.float64))


def test_linear_ramp_is_reproduced_at_the_sample_positions():
    """Bilinear interpolation is exact on a + b x + c y inside the frame; outside the outermost sample centres it holds the
    edge value.  32 -> 64: the sample positions are quarters, every product is exact, the equality is bitwise.  65 x 67 ->
    128 x 128: the positions are not representable, the equality holds to the double rounding of four products."""
    def ramp(H, W):
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        return np.stack([3.0 + 2.0 * xs - 5.0 * ys, 7.0 * xs, -1.0 * ys], axis=-1)[None].astype(np.float32)

    def positions(inn, out):
        d = np.arange(out, dtype=np.float64)
        return np.clip(((2 * d + 1) * inn - out) / (2.0 * out), 0, inn - 1)

    for (H, W, OH, OW), tol in (((32, 32, 64, 64), 0.0), ((65, 67, 128, 128), 2.0 ** -52 * 1000.0)):
        v, _ = R.resize(ramp(H, W), OH, OW)
        sy, sx = np.meshgrid(positions(H, OH), positions(W, OW), indexing="ij")
        want = np.stack([3.0 + 2.0 * sx - 5.0 * sy, 7.0 * sx, -1.0 * sy], axis=-1)[None]
        assert float(np.abs(v - want).max()) <= tol, (H, W, float(np.abs(v - want).max()))


@pytest.mark.parametrize("H,W", [(65, 67), (100, 150), (436, 1024)])
def test_constant_flow_refits_to_the_scaled_constant(H, W):
    FH, FW = R.ceil_to(H), R.ceil_to(W)
    a, b = np.float32(3.25), np.float32(-7.1)
    flow = np.empty((1, FH, FW, 2), np.float32)
    flow[..., 0], flow[..., 1] = a, b
    v, S = R.refit_flow(flow, H, W, "resize")
    assert v.shape == (1, H, W, 2)
    want = np.array([float(a) * W / FW, float(b) * H / FH])
    assert float((np.abs(v - want) / np.abs(want)).max()) <= 4 * 2.0 ** -53          # (1 - f) a + f a, three roundings and the scale's
    assert np.array_equal(S, np.broadcast_to(np.abs(np.array([float(a) * (W / FW), float(b) * (H / FH)])), S.shape))
    v, _ = R.refit_flow(flow, H, W, "pad")
    assert v.shape == (1, H, W, 2) and np.array_equal(v, flow[:, :H, :W].astype(np.float64))


@pytest.mark.parametrize("mode", R.MODES)
def test_fitted_image_stays_within_the_source_range(mode):
    rng = np.random.RandomState(11)
    x = rng.randint(37, 201, size=(2, 65, 67, 3)).astype(np.uint8)
    v, S = R.fit_frames(x, mode)
    y = v.astype(np.float32)                                         # the once-rounded value: rounding is monotone
    lo, hi = R.to_float32(x).min(), R.to_float32(x).max()
    assert y.shape == (2, 128, 128, 3) and y.min() >= lo and y.max() <= hi
    assert float(R.ratio(y, v, S).max()) <= 1.0
    if mode == "pad":
        assert np.array_equal(y[:, :65, :67], R.to_float32(x)) and np.array_equal(y[:, 65:, 70], y[:, 64:65, 66].repeat(63, 1))


@pytest.mark.parametrize("H,W,FH,FW", [(1, 1, 64, 64), (63, 130, 64, 192), (64, 100, 64, 128), (436, 1024, 448, 1024),
                                       (375, 1242, 384, 1280)])
def test_info_geometry(H, W, FH, FW):
    for mode in R.MODES:
        info = fit.fit_info(H, W, mode)
        assert info == (mode, H, W, FH, FW) and (info.mode, info.H, info.W, info.FH, info.FW) == (mode, H, W, FH, FW)
        with pytest.raises(AttributeError):
            info.H = 3                                               # immutable
    assert (R.ceil_to(H), R.ceil_to(W)) == (FH, FW)
    with pytest.raises(ValueError):
        fit.fit_info(H, W, "crop")


def test_python_layer_rejects_what_the_kernels_cannot_take():
    """CPU tensors, other dtypes, other shapes and non-contiguous tensors raise ValueError with the reason, before the library
    is asked anything."""
    with pytest.raises(ValueError, match="CUDA"):
        fit.fit_frames(torch.zeros((1, 8, 8, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        fit.refit_flow(torch.zeros((1, 64, 64, 2)), fit.fit_info(8, 8))
    with pytest.raises(ValueError, match="torch tensor"):
        fit.fit_frames(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="unknown mode"):
        fit.fit_info(8, 8, "stretch")


def test_planted_fault_is_caught_at_the_bound():
    """The same arithmetic in float32 (coordinate, weights, blend) misses the bound the kernels are held to: the bound tells
    'formed in double, rounded once' from a float32 composition.  The float64 value rounded once meets it."""
    rng = np.random.RandomState(2)
    x = rng.uniform(0, 1, size=(2, 65, 67, 3)).astype(np.float32)
    ref, S = R.fit_frames(x, "resize")
    good = float(R.ratio(ref.astype(np.float32), ref, S).max())
    bad = float(R.ratio(R.fit_frames(x, "resize", dtype=np.float32)[0], ref, S).max())
    print(f"fit 65x67 -> 128x128: once-rounded float64 r = {good:.4f}, float32 arithmetic r = {bad:.3f}")
    assert good <= 1.0 < bad
    flow = util.flow_field(2, 128, 128)
    ref, S = R.refit_flow(flow, 65, 67, "resize")
    good = float(R.ratio(ref.astype(np.float32), ref, S).max())
    bad = float(R.ratio(R.refit_flow(flow, 65, 67, "resize", dtype=np.float32)[0], ref, S).max())
    print(f"refit 128x128 -> 65x67: once-rounded float64 r = {good:.4f}, float32 arithmetic r = {bad:.3f}")
    assert good <= 1.0 < bad


def test_library_argument_checks_return_before_any_launch():
    """Bad arguments come back as the library's error codes; nothing is launched (there is no GPU here)."""
    L = _lib.lib()
    al = ctypes.c_void_p(4096)          # an aligned non-null address: argument checks only
    fitf, refit = L.pwc_fit_frames_f32, L.pwc_refit_flow_f32
    RS, PAD = _lib.FIT_RESIZE, _lib.FIT_PAD
    assert fitf(None, 1, al, 1, 8, 8, 64, 64, RS, None) == -1
    assert fitf(al, 1, None, 1, 8, 8, 64, 64, RS, None) == -1
    assert fitf(al, 1, al, 1, 65, 8, 64, 64, RS, None) == -1                  # OH < H
    assert fitf(al, 0, al, 1, 8, 65, 64, 64, PAD, None) == -1                 # OW < W
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert fitf(al, 1, al, *bad, 64, 64, RS, None) == -1
    assert fitf(al, 1, al, 1, 8, 8, 64, 64, 2, None) == -1 and fitf(al, 1, al, 1, 8, 8, 64, 64, -1, None) == -1
    assert fitf(al, 1, ctypes.c_void_p(4104), 1, 8, 8, 64, 64, RS, None) == -2      # y off a 16-byte boundary
    assert fitf(ctypes.c_void_p(4097), 0, al, 1, 8, 8, 64, 64, RS, None) == -2      # float32 x off a 4-byte boundary
    assert fitf(al, 1, al, 1 << 10, 1 << 10, 1 << 10, 1 << 11, 1 << 10, RS, None) == -3
    assert refit(None, al, 1, 64, 64, 8, 8, RS, None) == -1 and refit(al, None, 1, 64, 64, 8, 8, RS, None) == -1
    for bad in ((0, 64, 64, 8, 8), (1, 0, 64, 8, 8), (1, 64, 0, 8, 8), (1, 64, 64, 0, 8), (1, 64, 64, 8, -2)):
        assert refit(al, al, *bad, RS, None) == -1
    assert refit(al, al, 1, 64, 64, 8, 8, 3, None) == -1
    assert refit(al, al, 1, 64, 64, 65, 8, PAD, None) == -1                   # PAD cannot crop to more than there is
    assert refit(al, al, 1, 64, 64, 8, 65, PAD, None) == -1
    assert refit(ctypes.c_void_p(4100), al, 1, 64, 64, 8, 8, RS, None) == -2
    assert refit(al, ctypes.c_void_p(4100), 1, 64, 64, 8, 8, RS, None) == -2
    assert refit(al, al, 1 << 10, 1 << 11, 1 << 10, 8, 8, RS, None) == -3


@pytest.mark.parametrize("script,argv", [("infer", ["--input_images", "a.png", "b.png"]),
                                         ("infer_continuous", ["-i", "a.png", "b.png"]),
                                         ("evaluate", ["--list", "pairs.txt"])])
def test_command_lines_take_fit_and_default_to_crop(script, argv):
    import importlib
    ap = importlib.import_module(script).build_parser()
    assert ap.parse_args(argv).fit == "crop"
    for mode in ("crop", "resize", "pad"):
        assert ap.parse_args(argv + ["--fit", mode]).fit == mode
    with pytest.raises(SystemExit):
        ap.parse_args(argv + ["--fit", "stretch"])
