"""The frame fit and the flow refit on the GPU (pwcnet_amd/fit.py over csrc/pwc_fit.hip) against the float64 reference of
tests/fit_ref.py, and flow_any_size end to end.

Bounds.  Mode "pad" moves values: bitwise, both directions.  Mode "resize" forms every value in double and rounds it to float32
once, so per element r = |y - ref| / (2^-24 S) <= 1 against the UNROUNDED float64 reference, S the largest magnitude among the
element's four corners (times the refit scale): half an ulp of a value no larger than S; 1 + 1e-6 allows for the reference's
own double rounding.  tests/test_host_fit.py shows the same arithmetic in float32 measures 2.5 (fit) and above 100 (refit).
Every test prints its worst r before it asserts (profiles/fit_gpu_test_figures.txt).  End to end the project's 1e-3 px forward
tolerance against the CPU oracle carries over: the refit scales are at most 1.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import fit_ref as R  # noqa: E402
from tests import util  # noqa: E402

pytestmark = pytest.mark.gpu

GEOM_IDS = [f"{n}x{h}x{w}" for n, h, w, _, _ in R.GEOMETRIES]


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    torch.cuda.set_device(0)
    return pwcnet_amd


def bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else t
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def frames_u8(g):
    n, h, w, _, _ = R.GEOMETRIES[g]
    return np.random.RandomState(100 + g).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def fit_reference(g, mode):
    return R.fit_frames(frames_u8(g), mode)


@functools.lru_cache(maxsize=None)
def flow_in(g):
    n, _, _, oh, ow = R.GEOMETRIES[g]
    return util.flow_field(n, oh, ow, seed=30 + g)


@functools.lru_cache(maxsize=None)
def refit_reference(g, mode):
    _, h, w, _, _ = R.GEOMETRIES[g]
    return R.refit_flow(flow_in(g), h, w, mode)


def judge(tag, y, ref, S, mode):
    """pad: bitwise; resize: worst r printed, then held to the bound."""
    y = y.cpu().numpy()
    assert y.shape == ref.shape and y.dtype == np.float32, (tag, y.shape, ref.shape)
    if mode == "pad":
        assert np.array_equal(bits(y), bits(ref.astype(np.float32))), tag
        print(f"{tag}: bitwise")
        return
    r = float(R.ratio(y, ref, S).max())
    print(f"{tag}: worst r = {r:.6f} (bound {R.BOUND})")
    assert r <= R.BOUND, (tag, r)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("g", range(len(R.GEOMETRIES)), ids=GEOM_IDS)
def test_fit_frames(pa, g, mode):
    n, h, w, oh, ow = R.GEOMETRIES[g]
    u8 = frames_u8(g)
    ref, S = fit_reference(g, mode)
    xu = torch.from_numpy(u8).cuda()
    xf = torch.from_numpy(R.to_float32(u8)).cuda()
    yu, info = pa.fit_frames(xu, mode)
    yf, info_f = pa.fit_frames(xf, mode)
    assert info == info_f == (mode, h, w, oh, ow) and tuple(yu.shape) == (n, oh, ow, 3) and yu.dtype == torch.float32
    judge(f"fit {mode} {GEOM_IDS[g]} -> {oh}x{ow} uint8", yu, ref, S, mode)
    judge(f"fit {mode} {GEOM_IDS[g]} -> {oh}x{ow} float32", yf, ref, S, mode)
    assert np.array_equal(bits(yu), bits(yf))                              # uint8 against the float32 that holds v / 255
    assert np.array_equal(bits(pa.fit_frames(xu, mode)[0]), bits(yu))      # two calls, the same bits
    if (h, w) == (oh, ow):
        assert yf is xf                                                    # nothing to do: the input object itself
        assert yu is not xu and np.array_equal(bits(yu), bits(xf))         # uint8 is still converted
    if mode == "resize" and h == oh and w != ow:
        # the exact-copy axis: every weight down H is 0, so a row is the one-dimensional resize of its own source row --
        # (1 - fx) a + fx b in double, rounded once -- to the bit
        x0, x1, fx = R.taps(w, ow)
        src = R.to_float32(u8).astype(np.float64)
        fx = fx.reshape(1, 1, ow, 1)
        rows = ((1.0 - fx) * src[:, :, x0] + fx * src[:, :, x1]).astype(np.float32)
        assert np.array_equal(bits(yu), bits(rows))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("g", range(len(R.GEOMETRIES)), ids=GEOM_IDS)
def test_refit_flow(pa, g, mode):
    n, h, w, oh, ow = R.GEOMETRIES[g]
    ref, S = refit_reference(g, mode)
    f = torch.from_numpy(flow_in(g)).cuda()
    info = pa.fit_info(h, w, mode)
    y = pa.refit_flow(f, info)
    assert tuple(y.shape) == (n, h, w, 2)
    judge(f"refit {mode} {oh}x{ow} -> {GEOM_IDS[g]}", y, ref, S, mode)
    assert np.array_equal(bits(pa.refit_flow(f, info)), bits(y))
    if (h, w) == (oh, ow):
        assert y is f


def test_entry_points_on_odd_sizes_and_tails(pa):
    """The C entries take any OH >= H, OW >= W.  5 x 7 -> 6 x 9 (54 pixels: a tail of two behind the groups of four; groups that
    run over row ends), a refit to 5 x 7 (35 pixels: a tail of one behind the pairs) into a destination that is 16-byte
    aligned and into one that is only 8-byte aligned.  Guard words behind every destination stay untouched."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    rng = np.random.RandomState(9)
    u8 = rng.randint(0, 256, size=(1, 5, 7, 3)).astype(np.uint8)
    guard = 12345.0
    for mode, code in (("resize", _lib.FIT_RESIZE), ("pad", _lib.FIT_PAD)):
        if mode == "resize":
            ref, S = R.resize(R.to_float32(u8), 6, 9)
        else:
            ref = R.to_float32(u8)[:, np.minimum(np.arange(6), 4)][:, :, np.minimum(np.arange(9), 6)].astype(np.float64)
            S = np.abs(ref)
        for x in (torch.from_numpy(u8).cuda(), torch.from_numpy(R.to_float32(u8)).cuda()):
            buf = torch.full((6 * 9 * 3 + 64,), guard, device="cuda")
            _lib.check(L.pwc_fit_frames_f32(ctypes.c_void_p(x.data_ptr()), int(x.dtype == torch.uint8), ctypes.c_void_p(buf.data_ptr()),
                                            1, 5, 7, 6, 9, code, _lib.current_stream()))
            assert bool((buf[6 * 9 * 3:] == guard).all())
            judge(f"fit {mode} 1x5x7 -> 6x9 {x.dtype}", buf[:6 * 9 * 3].reshape(1, 6, 9, 3), ref, S, mode)
        flow = util.flow_field(1, 6, 9, seed=4)
        ref, S = R.refit_flow(flow, 5, 7, mode)
        f = torch.from_numpy(flow).cuda()
        for off in (0, 2):                                                  # floats: 16-byte aligned, then 8-byte aligned only
            buf = torch.full((4 + 5 * 7 * 2 + 64,), guard, device="cuda")
            _lib.check(L.pwc_refit_flow_f32(ctypes.c_void_p(f.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 4 * off), 1, 6, 9, 5, 7, code,
                                            _lib.current_stream()))
            assert bool((buf[:off] == guard).all()) and bool((buf[off + 70:] == guard).all())
            judge(f"refit {mode} 6x9 -> 1x5x7 offset {off}", buf[off:off + 70].reshape(1, 5, 7, 2), ref, S, mode)


def test_argument_checks_return_errors_without_launching(pa):
    from pwcnet_amd import _lib
    L = _lib.lib()
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    y = torch.full((1, 64, 64, 3), 7.0, device="cuda")
    f = torch.full((1, 64, 64, 2), 7.0, device="cuda")
    o = torch.full((1, 8, 8, 2), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = _lib.current_stream()
    RS, PAD = _lib.FIT_RESIZE, _lib.FIT_PAD
    assert L.pwc_fit_frames_f32(None, 1, p(y), 1, 8, 8, 64, 64, RS, s) == -1
    assert L.pwc_fit_frames_f32(p(x), 1, None, 1, 8, 8, 64, 64, RS, s) == -1
    assert L.pwc_fit_frames_f32(p(x), 1, p(y), 1, 8, 8, 7, 64, RS, s) == -1            # OH < H
    assert L.pwc_fit_frames_f32(p(x), 1, p(y), 1, 8, 8, 64, 7, PAD, s) == -1           # OW < W
    assert L.pwc_fit_frames_f32(p(x), 1, p(y), 0, 8, 8, 64, 64, RS, s) == -1
    assert L.pwc_fit_frames_f32(p(x), 1, p(y), 1, 8, 8, 64, 64, 2, s) == -1            # no such mode
    assert L.pwc_refit_flow_f32(None, p(o), 1, 64, 64, 8, 8, RS, s) == -1
    assert L.pwc_refit_flow_f32(p(f), None, 1, 64, 64, 8, 8, RS, s) == -1
    assert L.pwc_refit_flow_f32(p(f), p(o), 1, 64, 64, 8, 0, RS, s) == -1
    assert L.pwc_refit_flow_f32(p(f), p(o), 1, 64, 64, 8, 8, 5, s) == -1
    assert L.pwc_refit_flow_f32(p(o), p(f), 1, 8, 8, 64, 64, PAD, s) == -1             # PAD with FH < H
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((o == 7.0).all()) and bool((f == 7.0).all())          # nothing was launched
    # the Python layer says why
    with pytest.raises(ValueError, match="contiguous"):
        pa.fit_frames(torch.zeros((1, 8, 3, 8), device="cuda").permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="dtype"):
        pa.fit_frames(torch.zeros((1, 8, 8, 3), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="dtype"):
        pa.refit_flow(torch.zeros((1, 64, 64, 2), dtype=torch.float64, device="cuda"), pa.fit_info(8, 8))
    with pytest.raises(ValueError, match="shape"):
        pa.fit_frames(torch.zeros((1, 8, 8, 4), device="cuda"))
    with pytest.raises(ValueError, match="the fit was to"):
        pa.refit_flow(torch.zeros((1, 64, 128, 2), device="cuda"), pa.fit_info(8, 8))
    with pytest.raises(ValueError, match="CUDA"):
        pa.fit_frames(torch.zeros((1, 8, 8, 3)))


# ---------------------------------------------------------------------------------------------- end to end
E2E_H, E2E_W = 100, 150          # network geometry 128 x 192


@pytest.fixture(scope="module")
def e2e(pa):
    w = util.model_weights(False)
    net = pa.PWCDCNet(use_dc=False)
    net.load_weights(w)
    im0, im1 = (np.ascontiguousarray(im[:, :E2E_H, :E2E_W]) for im in util.smooth_images(1, 104, 152))   # (its sizes: multiples of 8)
    assert im0.shape == im1.shape == (1, E2E_H, E2E_W, 3)
    return {"w": w, "net": net, "im0": im0, "im1": im1, "x0": torch.from_numpy(im0).cuda(), "x1": torch.from_numpy(im1).cuda()}


@pytest.mark.parametrize("mode", R.MODES)
def test_flow_any_size_is_fit_forward_refit(pa, e2e, mode):
    """flow_any_size = the three steps; the same through a ForwardPipeline(depth=2); both to the bit.  The pyramid stays at the
    network's geometry."""
    net = e2e["net"]
    final, pyr = pa.flow_any_size(net, e2e["x0"], e2e["x1"], mode)
    assert tuple(final.shape) == (1, E2E_H, E2E_W, 2) and tuple(pyr[-1].shape) == (1, 32, 48, 2)
    a, info = pa.fit_frames(e2e["x0"], mode)
    b, _ = pa.fit_frames(e2e["x1"], mode)
    assert info == (mode, E2E_H, E2E_W, 128, 192)
    steps = pa.refit_flow(net(a, b)[0], info)
    assert np.array_equal(bits(final), bits(steps))
    pipe = pa.ForwardPipeline(depth=2, use_dc=False)
    pipe.load_weights(e2e["w"])
    tickets = [pipe.submit(a, b) for _ in range(2)]                       # one forward per lane
    pipe.synchronize()
    for t in tickets:
        assert np.array_equal(bits(pa.refit_flow(t.result()[0], info)), bits(final))


@pytest.mark.parametrize("mode", R.MODES)
def test_flow_any_size_against_the_oracle(pa, e2e, mode):
    """The CPU oracle on the reference-fitted frames, reference-refitted: within the forward's 1e-3 px."""
    from oracle import oracle as orc
    a = R.fit_frames(e2e["im0"], mode)[0].astype(np.float32)
    b = R.fit_frames(e2e["im1"], mode)[0].astype(np.float32)
    e_final, _ = orc.OraclePWCDCNet(e2e["w"], use_dc=False)(a, b)
    assert float(np.abs(e_final).max()) > 0.5                             # the comparison is not vacuous
    want, _ = R.refit_flow(np.ascontiguousarray(e_final, np.float32), E2E_H, E2E_W, mode)
    final, _ = pa.flow_any_size(e2e["net"], e2e["x0"], e2e["x1"], mode)
    err = float(np.abs(final.cpu().numpy() - want).max())
    print(f"flow_any_size {mode} {E2E_H}x{E2E_W}: max |flow| {float(np.abs(want).max()):.3f} px, max abs err vs oracle {err:.3e} px")
    assert err <= 1e-3, (mode, err)


@pytest.mark.parametrize("mode", R.MODES)
def test_frames_that_fit_take_the_plain_call(pa, e2e, mode):
    im0, im1 = util.smooth_images(1, 128, 192)
    x0, x1 = torch.from_numpy(im0).cuda(), torch.from_numpy(im1).cuda()
    plain, plain_pyr = e2e["net"](x0, x1)
    final, pyr = pa.flow_any_size(e2e["net"], x0, x1, mode)
    assert np.array_equal(bits(final), bits(plain))
    for p, q in zip(pyr, plain_pyr):
        assert np.array_equal(bits(p), bits(q))
