"""The strided tile kernel (pwcnet_amd/csrc/conv3x3_s2.hip: stride 2, a workgroup owns 4 x 32 output pixels and all output
channels) behind pwc_conv3x3_sk_f32 and pwc_conv3x3_h2_stride2_f32, forced through pwc_conv3x3_sk_variant_f32 (tile 50), against
float64 with the reference and metric of tests/test_gpu_forward_f64.py: r = max |y - y64| / (2^-24 S), bound B = 16 (the sk_s2
family's: the same arithmetic), B = 28 on the h2 entry point, B_TOP = 160 with a planted 65503 / 65519.

Shapes (N, H, W, Cin, Cout) at the 4 x 32 tile: output 10 x 36 of two images (ragged rows and columns), 4 x 32 (exactly one tile
row), 9 x 65 (three column tiles, the last one pixel wide; 96 input channels: a 64- and a 32-channel patch), 3 x 5 (less than one
tile, 128 input channels: two 64-channel patches).
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_forward_f64 import B_TOP, SLOPE, ULP, conv_f64, magnitudes, out_hw, ratio, reference
from tests.test_gpu_ops import _p, gpu

pytestmark = pytest.mark.gpu

TILE = 50
B_SK_S2 = 16
B_H2 = 28
SHAPES = [(2, 20, 72, 64, 96), (1, 8, 64, 32, 64), (2, 18, 130, 96, 128), (1, 6, 10, 128, 64)]
FIRST = SHAPES[0]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def case(shape, seed=401):
    """(x, k, b, ref, S) of a shape: operands built like operands() of test_gpu_forward_f64, the float64 reference once."""
    N, H, W, cin, cout = shape
    x, k, b = (magnitudes((N, H, W, cin), seed, 1.0), magnitudes((3, 3, cin, cout), seed + 1, 1.0 / np.sqrt(9 * cin)),
               magnitudes((cout,), seed + 2, 0.1))
    ref, S, _ = reference(x, k, b, 1, 2)
    for a in (ref, S):
        a.setflags(write=False)
    return x, k, b, ref, S


def pack_sk(L, k):
    from pwcnet_amd import _lib
    cin, cout = k.shape[2], k.shape[3]
    packed = torch.empty(L.pwc_conv3x3_sk_packed_floats(cin, cout), device="cuda")
    _lib.check(L.pwc_conv3x3_sk_pack_f32(_p(gpu(k)), None, cin, cin, cout, _p(packed), None))
    return packed


def run_sk(L, x, k, b, tile=TILE, x_slack=0, y_slack=0, act=1, packed=None):
    """One stride-2 launch (tile 0: pwc_conv3x3_sk_f32, the library's choice).  Slack channels of x hold NaN, of y -7."""
    from pwcnet_amd import _lib
    N, H, W, cin = x.shape
    cout = k.shape[3]
    Ho, Wo = out_hw(H, W, 2)
    xs = np.full((N, H, W, cin + x_slack), np.nan, np.float32)
    xs[..., :cin] = x
    xg, bg = gpu(xs), gpu(b)
    packed = pack_sk(L, k) if packed is None else packed
    y = torch.full((N, Ho, Wo, cout + y_slack), -7.0, device="cuda")
    head = (_p(xg), cin + x_slack, _p(packed), _p(bg), _p(y), cout + y_slack, N, H, W, cin, cout, 2, 1, act, SLOPE)
    if tile:
        _lib.check(L.pwc_conv3x3_sk_variant_f32(*head, tile, None))
    else:
        _lib.check(L.pwc_conv3x3_sk_f32(*head, None))
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_s2_tile_shapes_vs_float64(L, shape):
    x, k, b, ref, S = case(shape)
    y = run_sk(L, x, k, b)
    r, _ = ratio(y, ref, S)
    print(f"MEASURED s2_tile {shape} {r:.4g}")
    assert r <= B_SK_S2, (shape, r)


def test_s2_tile_strided_views(L):
    """x_cs = Cin + 16 with NaN in the slack, y_cs = Cout + 4 with a sentinel in the slack."""
    x, k, b, ref, S = case(FIRST)
    cout = k.shape[3]
    y = run_sk(L, x, k, b, x_slack=16, y_slack=4)
    assert np.all(y[..., cout:] == -7.0), "the slack of y was written"
    r, _ = ratio(y[..., :cout], ref, S)             # (ratio fails on a non-finite output: the slack of x reached one)
    print(f"MEASURED s2_tile views {r:.4g}")
    assert r <= B_SK_S2, r
    assert np.array_equal(y[..., :cout], run_sk(L, x, k, b)), "the strides of the views changed a sum"


@pytest.mark.parametrize("H", [20, 19])
def test_s2_tile_same_padding_corners(L, H):
    """'SAME' at stride 2 pads bottom and right only for even sizes, one line on each side for odd ones."""
    N, W, cin, cout = 1, 72, 64, 96
    x = np.zeros((N, H, W, cin), np.float32)
    x[0, 0, 0] = 1.0
    x[0, H - 1, W - 1] = 1.0
    k, b = np.ones((3, 3, cin, cout), np.float32), np.zeros(cout, np.float32)
    y = run_sk(L, x, k, b, act=0)
    exp = conv_f64(x.astype(np.float64), k.astype(np.float64), 1, 2)
    Ho, Wo = out_hw(H, W, 2)
    assert np.all(exp[0, 0, 0] == cin) and np.all(exp[0, Ho - 1, Wo - 1] == cin)
    assert np.all(exp[0, 0, Wo - 1] == 0) and np.all(exp[0, Ho - 1, 0] == 0)
    for oy, ox in ((0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1)):
        assert np.array_equal(y[0, oy, ox], exp[0, oy, ox].astype(np.float32)), (oy, ox, y[0, oy, ox, :4])
    assert np.array_equal(y, exp.astype(np.float32))


def test_s2_tile_fp16_top_edge(L):
    N, H, W, cin, cout = FIRST
    x1, k1, b1, _, _ = case(FIRST)
    py, px, ci, co = 9, 33, 3, 5
    hot = np.zeros((N, H, W, cin))
    hot[0, py, px, ci] = 1.0
    reads_x = conv_f64(hot, np.ones((3, 3, cin, cout)), 1, 2) > 0
    reads_w = np.zeros(reads_x.shape, bool)
    reads_w[..., co] = True
    for which in ("x", "w"):
        for val in (65503.0, 65519.0, 65520.0, -65520.0):
            x, k = x1.copy(), k1.copy()
            if which == "x":
                x[0, py, px, ci] = val
            else:
                k[1, 1, ci, co] = val
            reads = reads_x if which == "x" else reads_w
            ref, S, _ = reference(x, k, b1, 1, 2)
            y = run_sk(L, x, k, b1)
            nan = np.isnan(y)
            assert not np.any(nan & ~reads), (which, val, "NaN outside the outputs that read the operand")
            assert not np.any(np.isinf(y)), (which, val)
            if abs(val) >= 65520.0:
                assert nan[reads].all(), (which, val, int((~nan[reads]).sum()))
            else:
                assert not nan.any(), (which, val)
            ok = ~nan
            r = float((np.abs(y[ok].astype(np.float64) - ref[ok]) / (ULP * S[ok])).max())
            print(f"MEASURED s2_tile top {which}={val:.0f} {r:.4g} nan={int(nan.sum())}")
            assert r <= B_TOP, (which, val, r)


def test_s2_tile_repeats_bitwise(L):
    x, k, b, _, _ = case(FIRST)
    packed = pack_sk(L, k)
    first = run_sk(L, x, k, b, packed=packed)
    for _ in range(9):
        assert np.array_equal(first, run_sk(L, x, k, b, packed=packed))


def test_s2_tile_and_library_choice_vs_float64(L):
    shape = (2, 28, 64, 64, 96)
    x, k, b, ref, S = case(shape)
    for tile in (0, TILE):
        r, _ = ratio(run_sk(L, x, k, b, tile=tile), ref, S)
        print(f"MEASURED s2_tile old/new tile={tile} {r:.4g}")
        assert r <= B_SK_S2, (tile, r)


def test_s2_tile_behind_h2_stride2_entry_point(L):
    """fp_extractor/conv2d_6's form (32 -> 64): pwc_conv3x3_h2_stride2_f32 routes 32 input channels to the strided tile kernel,
    which reads the second image of pwc_conv3x3_h2_stride2_pack_f32 -- the same bits as the forced kernel on the sk pack."""
    from pwcnet_amd import _lib
    shape = (2, 16, 64, 32, 64)
    N, H, W, cin, cout = shape
    x, k, b, ref, S = case(shape)
    xg, kg, bg = gpu(x), gpu(k), gpu(b)
    packed = torch.empty(L.pwc_conv3x3_h2_stride2_packed_floats(cin, cout), device="cuda")
    _lib.check(L.pwc_conv3x3_h2_stride2_pack_f32(_p(kg), None, cin, cin, cout, _p(packed), None))
    n_ws = L.pwc_conv3x3_h2_stride2_workspace_floats(N, H, W, cin, cout)
    ws = torch.full((max(n_ws, 4),), float("nan"), device="cuda").view(torch.int32).fill_(-1).view(torch.float32)
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    y = torch.full((N, H // 2, W // 2, cout), -7.0, device="cuda")
    _lib.check(L.pwc_conv3x3_h2_stride2_f32(_p(xg), cin, _p(packed), _p(bg), _p(y), cout, N, H, W, cin, cout, 1, SLOPE,
                                            _p(ws) if n_ws else None, n_ws, _p(status), None))
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    r, _ = ratio(y, ref, S)
    print(f"MEASURED s2_tile h2_stride2 {r:.4g}")
    assert r <= B_H2, r
    assert int(status.abs().sum()) == 0
    assert bool((ws.view(torch.int32) == -1).all()), "the stream-K workspace must stay all ones"
    assert np.array_equal(y, run_sk(L, x, k, b)), "pwc_conv3x3_h2_stride2_f32 did not run the strided tile kernel"
