"""The F16-pipe convolutions (pwc_conv3x3_h2_f32 in every tile variant, pwc_conv3x3_sk_f32 at stride 1 and 2, pwc_conv3x3_t32_f32,
pwc_conv3x3_w32_f32) against float64 at the edges of their operand split, at production layer shapes.

These kernels use every fp32 operand as x = h + 2^-11 m' with h = fp16(x), m' = fp16((x - h) 2^11) (pwcnet_amd/csrc/pwc_common.h,
pwc_split2) and form three of the four cross products in fp32 accumulators.  Error metric, per output element (not against
max |y|): err_i = |y_i - ref_i| with ref the float64 convolution + bias, leaky-relu'd, and S_i the same evaluation on absolute
values (sum |x||w| + |b|, times the slope where ref's pre-activation is negative); r = max_i err_i / (2^-24 S_i).

  * Operands of scale 2^k (magnitudes in [2^(k-1), 2^k]), activations and weights scaled separately.  Where every operand is
    at least 2^-14 the split holds 22 bits and r must stay within the family's bound B (B_FAMILY: max(10 x the worst r
    measured on an MI355X at those scales, 16)).  Below 2^-14, h and m' reach fp16's subnormals and an operand keeps an
    ABSOLUTE precision of 2^-36 (half of m's spacing 2^-24, times 2^-11): every output must stay within
    B 2^-24 S + 2^-35 (sum |w| + sum |x|) over its taps, and r within 3 x what was measured at that scale (SMALL_R: the
    launches are bit-deterministic).
  * Weights spread like a trained layer's: magnitudes log-uniform over [2^-24, 2^-10] (largest 2^-10, most of them below
    2^-14): r within B.  The large weights dominate S, the subnormal ones add at most 2^-36 |x| each.
  * Fp16's top edge: |x| < 65520 rounds h to a finite value (65504 at most) and the split stays exact; from 65520 on h is inf
    and every output that reads the operand is NaN (inf - inf), which the model's range check turns into an fp32 repeat.  A
    single operand of 65503, 65519 and +-65520 is planted in the activations and, separately, in the weights: NaN exactly on
    the outputs that read +-65520, and r <= B_TOP on every finite output (no finite wrong number).  A planted 65519 dominates
    S and the fp32 accumulators round at its product's magnitude: h2 measured r = 15.4 there (a dropped or saturated m' of
    65519 would be off by 15 |w|: r = 2^12).
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_ops import H2_COUTS, _p, gpu, run_conv_h2

pytestmark = pytest.mark.gpu

SLOPE = 0.1
ULP = 2.0 ** -24
SUB = 2.0 ** -35          # twice the absolute precision of a split operand below 2^-14
SCALES = (-24, -20, -16, -14, -8, 0, 8, 14)
# family -> (N, H, W, cin, cout, stride, dilation): production layer shapes (batch cut for the float64 reference)
FAMILIES = {
    "h2": (2, 28, 64, 64, 128, 1, 1),           # the estimators' 64 -> 128 form, 8-16-row tiles
    "h2_dil2": (1, 28, 64, 48, 96, 1, 2),       # context/conv2d_1 style dilation, the 96-cout variant
    "sk": (2, 14, 32, 128, 96, 1, 1),           # optflow_1/conv2d_2 of a batch of 8 at 14 x 32
    "sk_s2": (2, 28, 64, 64, 96, 2, 1),         # fp_extractor/conv2d_9 (64 -> 96, stride 2)
    "t32": (1, 56, 128, 32, 32, 1, 1),          # fp_extractor/conv2d_4 (32 -> 32)
    "t32_s2": (1, 60, 128, 16, 32, 2, 1),       # fp_extractor/conv2d_3 (16 -> 32, stride 2)
    "w32": (1, 56, 128, 64, 32, 1, 1),          # optflow_l/conv2d_4 (64 -> 32)
}
B_FAMILY = {                                    # max(10 x the worst r at scales >= 2^-14 or with spread weights, 16)
    "h2": 28,           # measured 2.78
    "h2_dil2": 29,      # measured 2.87
    "sk": 16,           # measured 0.847
    "sk_s2": 16,        # measured 1.09
    "t32": 30,          # measured 2.95
    "t32_s2": 23,       # measured 2.25
    "w32": 18,          # measured 1.72
}
B_TOP = 160.0             # r on the finite outputs with a planted 65503 / 65519: 10 x h2's measured 15.4
# (family, "x" | "w", k) -> worst r measured below 2^-14 (every variant of the family)
SMALL_R = {
    **{("h2", "x", k): r for k, r in {-24: 2259, -20: 142.8, -16: 3.082, -14: 1.404, -8: 1.314}.items()},
    **{("h2", "w", k): r for k, r in {-24: 1.172e+05, -20: 3169, -16: 168.1, -14: 17.95, -8: 1.314}.items()},
    **{("h2_dil2", "x", k): r for k, r in {-24: 1367, -20: 55.17, -16: 3.285, -14: 1.708, -8: 1.114}.items()},
    **{("h2_dil2", "w", k): r for k, r in {-24: 7.791e+04, -20: 2988, -16: 67.74, -14: 17.08, -8: 1.369}.items()},
    **{("sk", "x", k): r for k, r in {-24: 509.6, -20: 32.87, -16: 1.98, -14: 0.511, -8: 0.3946}.items()},
    **{("sk", "w", k): r for k, r in {-24: 9.741e+04, -20: 3409, -16: 66.78, -14: 18.73, -8: 0.4714}.items()},
    **{("sk_s2", "x", k): r for k, r in {-24: 1476, -20: 42.32, -16: 2.865, -14: 0.8835, -8: 0.5959}.items()},
    **{("sk_s2", "w", k): r for k, r in {-24: 6.554e+04, -20: 3036, -16: 65.44, -14: 15.75, -8: 0.5959}.items()},
    **{("t32", "x", k): r for k, r in {-24: 3135, -20: 60.23, -16: 3.804, -14: 1.553, -8: 1.381}.items()},
    **{("t32", "w", k): r for k, r in {-24: 8.638e+04, -20: 3023, -16: 61.69, -14: 17.51, -8: 1.381}.items()},
    **{("t32_s2", "x", k): r for k, r in {-24: 2034, -20: 85.06, -16: 5.725, -14: 1.705, -8: 1.352}.items()},
    **{("t32_s2", "w", k): r for k, r in {-24: 5.987e+04, -20: 1777, -16: 62.19, -14: 15.92, -8: 1.352}.items()},
    **{("w32", "x", k): r for k, r in {-24: 2835, -20: 44.33, -16: 2.904, -14: 1.013, -8: 0.7378}.items()},
    **{("w32", "w", k): r for k, r in {-24: 1.006e+05, -20: 3749, -16: 197.7, -14: 17.46, -8: 0.7677}.items()},
}


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    return pwcnet_amd


def out_hw(H, W, stride):
    return -(-H // stride), -(-W // stride)


def conv_f64(x, k, dil, stride=1):
    """TF 'SAME' 3x3 convolution in float64: nine shifted (strided) matmuls."""
    N, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, stride)
    ph, pw = max((Ho - 1) * stride + 2 * dil + 1 - H, 0), max((Wo - 1) * stride + 2 * dil + 1 - W, 0)
    xp = np.zeros((N, H + ph, W + pw, C))
    xp[:, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W] = x
    y = np.zeros((N * Ho * Wo, k.shape[3]))
    for dy in range(3):
        for dx in range(3):
            tap = xp[:, dy * dil:dy * dil + (Ho - 1) * stride + 1:stride, dx * dil:dx * dil + (Wo - 1) * stride + 1:stride]
            y += tap.reshape(-1, C) @ k[dy, dx].astype(np.float64)
    return y.reshape(N, Ho, Wo, -1)


def reference(x, k, b, dil, stride=1):
    """(ref, S, T): the leaky-relu'd float64 convolution, its evaluation on absolute values, and sum |w| + sum |x| over the
    taps each output reads (the subnormal floor's weight), all slope-scaled where ref's pre-activation is negative."""
    x, k, b = x.astype(np.float64), k.astype(np.float64), b.astype(np.float64)
    ref = conv_f64(x, k, dil, stride) + b
    S = conv_f64(np.abs(x), np.abs(k), dil, stride) + np.abs(b)
    T = conv_f64(np.ones_like(x), np.abs(k), dil, stride) + conv_f64(np.abs(x), np.ones_like(k), dil, stride)
    neg = ref < 0
    for a in (ref, S, T):
        a[neg] *= SLOPE
    return ref, S, T


def _launch(fam, v, x, k, b):
    """One launch of family `fam` (tile variant v where the family has them) with leaky-relu; the output as numpy."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    N, H, W, cin, cout, stride, dil = FAMILIES[fam]
    if fam.startswith("h2"):
        return run_conv_h2(x, k, b, SLOPE, dil=dil, variant=v).cpu().numpy()
    xg, kg, bg = gpu(x), gpu(k), gpu(b)
    Ho, Wo = out_hw(H, W, stride)
    y = torch.full((N, Ho, Wo, cout), -7.0, device="cuda")
    if fam.startswith("sk"):
        packed = torch.empty(L.pwc_conv3x3_sk_packed_floats(cin, cout), device="cuda")
        _lib.check(L.pwc_conv3x3_sk_pack_f32(_p(kg), None, cin, cin, cout, _p(packed), None))
        _lib.check(L.pwc_conv3x3_sk_f32(_p(xg), cin, _p(packed), _p(bg), _p(y), cout, N, H, W, cin, cout, stride, dil, 1, SLOPE,
                                        None))
    elif fam.startswith("t32"):
        packed = torch.empty(L.pwc_conv3x3_t32_packed_floats(cin), device="cuda")
        _lib.check(L.pwc_conv3x3_t32_pack_f32(_p(kg), None, cin, cin, _p(packed), None))
        _lib.check(L.pwc_conv3x3_t32_f32(_p(xg), cin, _p(packed), _p(bg), _p(y), cout, N, H, W, cin, cout, stride, 1, SLOPE, None))
    else:
        packed = torch.empty(L.pwc_conv3x3_w32_packed_floats(cin), device="cuda")
        _lib.check(L.pwc_conv3x3_w32_pack_f32(_p(kg), None, cin, cin, _p(packed), None))
        _lib.check(L.pwc_conv3x3_w32_f32(_p(xg), cin, _p(packed), _p(bg), _p(y), cout, N, H, W, cin, cout, 1, SLOPE, None))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def magnitudes(shape, seed, scale):
    rs = np.random.RandomState(seed)
    return (rs.uniform(0.5, 1.0, size=shape) * rs.choice([-1.0, 1.0], size=shape) * scale).astype(np.float32)


def variants(fam):
    """The tile variants a family's launch is checked in (h2: every one whose couts divide Cout; the others: the library's)."""
    if not fam.startswith("h2"):
        return [0]
    cout = FAMILIES[fam][4]
    return [v for v in range(6) if v == 0 or cout % H2_COUTS[v] == 0]


def ratio(y, ref, S):
    err = np.abs(y.astype(np.float64) - ref)
    assert np.all(np.isfinite(err)), "non-finite output"
    zero = S == 0
    assert not np.any(err[zero]), "an output with S = 0 must be an exact 0"
    return float((err[~zero] / (ULP * S[~zero])).max()), err


def operands(fam, seed):
    N, H, W, cin, cout, stride, dil = FAMILIES[fam]
    return (magnitudes((N, H, W, cin), seed, 1.0), magnitudes((3, 3, cin, cout), seed + 1, 1.0 / np.sqrt(9 * cin)),
            magnitudes((cout,), seed + 2, 0.1))


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_f16_pipe_conv_operand_scales_vs_float64(pa, fam):
    N, H, W, cin, cout, stride, dil = FAMILIES[fam]
    B = B_FAMILY[fam]
    x1, k1, b1 = operands(fam, 301)
    for which in ("x", "w"):
        for kexp in SCALES:
            s = 2.0 ** kexp
            x = (x1 * s).astype(np.float32) if which == "x" else x1
            k = (k1 * s).astype(np.float32) if which == "w" else k1
            b = (b1 * s).astype(np.float32)
            assert max(float(np.abs(x).max()), float(np.abs(k).max())) < 65504.0
            ref, S, T = reference(x, k, b, dil, stride)
            small = min(float(np.abs(x).min()), float(np.abs(k).min())) < 2.0 ** -14
            worst = 0.0
            for v in variants(fam):
                r, err = ratio(_launch(fam, v, x, k, b), ref, S)
                worst = max(worst, r)
                if not small:
                    assert r <= B, (fam, which, kexp, v, r, B)
                else:
                    excess = float((err - (B * ULP * S + SUB * T)).max())
                    assert excess <= 0.0, (fam, which, kexp, v, r, excess)
            print(f"MEASURED {fam} {which} {kexp} {worst:.4g}")
            if small:
                assert worst <= 3.0 * SMALL_R[(fam, which, kexp)], (fam, which, kexp, worst, SMALL_R[(fam, which, kexp)])


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_f16_pipe_conv_trained_weight_spread_vs_float64(pa, fam):
    """Weights log-uniform in magnitude over [2^-24, 2^-10], random signs: the largest |w| a trained layer can have at the low
    end of the claim, most weights in fp16's subnormal range.  The family must still meet B."""
    N, H, W, cin, cout, stride, dil = FAMILIES[fam]
    x, _, b = operands(fam, 321)
    rs = np.random.RandomState(324)
    k = (2.0 ** rs.uniform(-24.0, -10.0, size=(3, 3, cin, cout)) * rs.choice([-1.0, 1.0], size=(3, 3, cin, cout)))
    k = k.astype(np.float32)
    b = (b * 2.0 ** -10).astype(np.float32)
    ref, S, _ = reference(x, k, b, dil, stride)
    for v in variants(fam):
        r, _ = ratio(_launch(fam, v, x, k, b), ref, S)
        print(f"MEASURED {fam} spread {v} {r:.4g}")
        assert r <= B_FAMILY[fam], (fam, v, r)


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_f16_pipe_conv_fp16_top_edge(pa, fam):
    N, H, W, cin, cout, stride, dil = FAMILIES[fam]
    x1, k1, b1 = operands(fam, 311)
    py, px, ci, co = 10, 20, 3, 5
    hot = np.zeros((N, H, W, cin))
    hot[0, py, px, ci] = 1.0
    reads_x = conv_f64(hot, np.ones((3, 3, cin, cout)), dil, stride) > 0   # the outputs whose window holds activation (0, py, px, ci)
    Ho, Wo = out_hw(H, W, stride)
    reads_w = np.zeros((N, Ho, Wo, cout), bool)               # the centre tap of (ci, co) is read by every output of co
    reads_w[..., co] = True
    for which in ("x", "w"):
        for val in (65503.0, 65519.0, 65520.0, -65520.0):
            x, k = x1.copy(), k1.copy()
            if which == "x":
                x[0, py, px, ci] = val
            else:
                k[1, 1, ci, co] = val
            reads = reads_x if which == "x" else reads_w
            ref, S, _ = reference(x, k, b1, dil, stride)
            for v in variants(fam):
                y = _launch(fam, v, x, k, b1)
                nan = np.isnan(y)
                assert not np.any(nan & ~reads), (fam, which, val, v, "NaN outside the outputs that read the operand")
                assert not np.any(np.isinf(y)), (fam, which, val, v)
                if abs(val) >= 65520.0:
                    assert nan[reads].all(), (fam, which, val, v, int((~nan[reads]).sum()))
                else:
                    assert not nan.any(), (fam, which, val, v)
                ok = ~nan
                r = float((np.abs(y[ok].astype(np.float64) - ref[ok]) / (ULP * S[ok])).max())
                print(f"MEASURED {fam} top {which}={val:.0f} {v} {r:.4g} nan={int(nan.sum())}")
                assert r <= B_TOP, (fam, which, val, v, r)
