"""Float64 references, a numpy emulation of the two-term operand split, and the inputs of tests/test_gpu_f16_pipe_f64.py (the
fused extractor pairs pwc_conv3x3_c16pair_f32 / pwc_conv3x3_c3c16pair_f32 and the F16-pipe correlations
pwc_warp_cost_volume_concat_h2_f32 / pwc_warp_cost_volume_concat_blk_f32), shared with tests/test_host_f16_pipe_ref.py, which checks
on the CPU every condition the GPU tests rely on.  Host-side numpy only.

Metric (tests/test_gpu_forward_f64.py): r = max_i |y_i - ref_i| / (2^-24 S_i), S the evaluation on absolute values.

Conv chains.  S is PROPAGATED: S_1 = conv(|x|, |k_1|) + |b_1|, S_l = conv(S_(l-1), |k_l|) + |b_l|, slope-scaled only at the last
layer where ref's pre-activation is negative.  Leaky-relu is 1-Lipschitz and S_l >= |mid_l|, so a first-layer error of
B 2^-24 S_1 reaches the output as at most B 2^-24 S_2, and L layers of bound B each give L B on the propagated S.  Below 2^-14 an
operand keeps an absolute precision of 2^-36 (SUB = 2^-35 with the factor 2 of test_gpu_forward_f64); its weight T propagates
the same way: T_1 = sum |k_1| + sum |x| over the taps, T_l = conv(T_(l-1), |k_l|) + sum |k_l| + sum S_(l-1).
An INTERMEDIATE below 2^-14 has the same absolute floor 2^-36 |w| per tap although the inputs are not small; where S_(l-1) >= 2^-8
at every pixel (asserted on the CPU for every case that is judged by r <= B) that is at most 2^-4 of 2^-24 S_l: inside B's room.

Correlation.  S is the same sum with |f0| and the blend of |f1| (the bilinear weights are not negative), T = (1/C)(sum |f0| + sum
blend |f1|) over the channels; both are 0 where the displaced pixel lies outside the frame (the output is an exact 0 there).  The
fp32 blend (one multiply, three fused multiply-adds, each rounded at no more than the blend of |f1|) adds 4 to the bound B of a
launch with a flow.

Bounds: B = 16 per layer and for the correlation without a flow (the project's floor for this split: every pinned family meets it
with 5 x room at a longer K), 2 B = 32 for the pair, 3 B = 48 for the three-layer launch, B + 4 = 20 for the correlation behind a
warp, B_TOP = 160 with a planted 65503 / 65519.  None of them is measured on these kernels.
"""
import functools

import numpy as np

from tests.test_gpu_forward_f64 import B_TOP, SCALES, SLOPE, SUB, ULP, conv_f64, magnitudes, out_hw

B = 16
B_PAIR, B_C3, B_CV, B_CV_WARP = 2 * B, 3 * B, B, B + 4
B_EMU = 8.0                   # the exact-arithmetic emulation: the split's 22 bits of two operands plus the dropped m'm' term
TOP_VALUES = (65503.0, 65519.0, 65520.0, -65520.0)
FLOW_SCALE = 4.0
R = 4                         # search range

# (N, H, W) of the 16-channel input; tiles are 16 x 32 pixels: ragged rows and columns, exactly one tile, last tiles one pixel wide
PAIR_SHAPES = [(2, 20, 40), (1, 16, 32), (1, 33, 65)]
# (Na, Nb, H0, W0) of the raw frames: Nb = 0; odd height ('SAME' pads the top row only for odd sizes); ragged level-1 tiles
C3_SHAPES = [(1, 1, 40, 80), (2, 0, 33, 64), (1, 2, 66, 132)]
# (N, H, W, C): five block rows (the ring of three Q-row images wraps), W % 16 != 0, H % 4 != 0, every C
CVH_SHAPES = [(2, 18, 37, 32), (1, 18, 21, 64), (1, 10, 16, 96)]
# (N, H, W, C): the first three have fewer than 256 blocks (one window row per workgroup), the last exactly 4 * 8 * 8 = 256 (whole window)
CVB_SHAPES = [(2, 7, 16, 192), (1, 9, 21, 128), (1, 6, 9, 64), (4, 29, 32, 96)]


def lrelu(a):
    return np.maximum(a, SLOPE * a)


# ------------------------------------------------------------------ conv chains
def chain_reference(x, layers, full=False):
    """(ref, S, T) of 2 or 3 chained leaky-relu'd 3x3 'SAME' convolutions `layers` = [(k, b, stride), ...] in float64: the chain,
    the propagated evaluation on absolute values and the propagated weight of the subnormal floor (module docstring), S and T
    slope-scaled at the last layer where ref's pre-activation is negative.  full: also the lists of the intermediates mid_l (the
    last one is ref) and of the unscaled S_l."""
    assert len(layers) in (2, 3)
    mid = x.astype(np.float64)
    S = np.abs(mid)
    T = None
    mids, Ss = [], []
    for k, b, stride in layers:
        k, b = k.astype(np.float64), b.astype(np.float64)
        ak = np.abs(k)
        pre = conv_f64(mid, k, 1, stride) + b
        Tn = conv_f64(np.ones_like(S), ak, 1, stride) + conv_f64(S, np.ones_like(k), 1, stride)
        if T is not None:
            Tn += conv_f64(T, ak, 1, stride)
        S = conv_f64(S, ak, 1, stride) + np.abs(b)
        T = Tn
        mid = lrelu(pre)
        mids.append(mid)
        Ss.append(S)
    neg = pre < 0
    ref, S, T = mid.copy(), S.copy(), T.copy()
    S[neg] *= SLOPE
    T[neg] *= SLOPE
    return (ref, S, T, mids, Ss) if full else (ref, S, T)


def reach(hot, layers):
    """The outputs of the chain `layers` whose receptive set holds a True of the boolean tensor `hot`."""
    m = hot.astype(np.float64)
    for k, _, stride in layers:
        m = (conv_f64(m, np.ones(k.shape), 1, stride) > 0).astype(np.float64)
    return m > 0


# ------------------------------------------------------------------ correlation
def warp_f64(f1, flow, flow_scale):
    """bilinear_warp (reference modules.py:99-137) of f1 in float64: weights from the un-clipped floors, the four corner indices
    clipped independently.  The displacement alone is fp32: the first statement restates
        const float fx = pwc_mul_rounded(f0v, a.flow_scale), fy = pwc_mul_rounded(f1v, a.flow_scale);
    of the corner tables (cost_volume_h2.hip, table_write; cost_volume_blk.hip, the table block; pwc_mul_rounded in pwc_common.h:
    the product is an fp32 operation of its own, floor and fraction come from the ROUNDED value).  Everything behind it is
    float64; the GPU tests' flows make the fp32 weights of pwc_bilinear_corners exact."""
    d = (flow.astype(np.float32) * np.float32(flow_scale)).astype(np.float32).astype(np.float64)
    f1 = f1.astype(np.float64)
    N, H, W, _ = f1.shape
    fx, fy = d[..., 0], d[..., 1]
    fx0, fy0 = np.floor(fx), np.floor(fy)
    gy, gx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    y0 = np.clip(gy + fy0, 0, H - 1).astype(np.int64)
    y1 = np.clip(gy + fy0 + 1, 0, H - 1).astype(np.int64)
    x0 = np.clip(gx + fx0, 0, W - 1).astype(np.int64)
    x1 = np.clip(gx + fx0 + 1, 0, W - 1).astype(np.int64)
    wy1, wx1 = fy - fy0, fx - fx0
    wy0, wx0 = (fy0 + 1) - fy, (fx0 + 1) - fx
    n = np.arange(N)[:, None, None]
    return ((wy0 * wx0)[..., None] * f1[n, y0, x0] + (wy0 * wx1)[..., None] * f1[n, y0, x1] +
            (wy1 * wx0)[..., None] * f1[n, y1, x0] + (wy1 * wx1)[..., None] * f1[n, y1, x1])


def corr_sum(a, b):
    """sum_c a[n, y, x, c] b[n, y + v, x + h, c] for the 81 displacements, channel (v + 4) 9 + (h + 4); b is zero outside."""
    N, H, W, C = a.shape
    pad = np.zeros((N, H + 2 * R, W + 2 * R, C))
    pad[:, R:R + H, R:R + W] = b
    return np.stack([np.einsum("nyxc,nyxc->nyx", a, pad[:, R + v:R + v + H, R + h:R + h + W])
                     for v in range(-R, R + 1) for h in range(-R, R + 1)], axis=3)


def cv_reference(f0, f1, flow=None, flow_scale=1.0):
    """(ref, S, T) of warp + cost volume + leaky-relu 0.1 in float64 (the displacement fx alone in fp32: warp_f64)."""
    C = f0.shape[3]
    f0 = f0.astype(np.float64)
    f1 = f1.astype(np.float64)
    f1w = f1 if flow is None else warp_f64(f1, flow, flow_scale)
    a1 = np.abs(f1) if flow is None else warp_f64(np.abs(f1), flow, flow_scale)
    pre = corr_sum(f0, f1w) / C
    S = corr_sum(np.abs(f0), a1) / C
    inside = corr_sum(np.ones_like(f0[..., :1]), np.ones_like(f0[..., :1])) > 0
    T = (np.abs(f0).sum(axis=3, keepdims=True) * inside + corr_sum(np.ones_like(f0), a1)) / C
    neg = pre < 0
    ref = lrelu(pre)
    S[neg] *= SLOPE
    T[neg] *= SLOPE
    return ref, S, T


# ------------------------------------------------------------------ the arithmetic, emulated
def split(x, scaled=True):
    """h = float16(x), m' = float16((x - h) 2^11) of fp32 values (pwc_split2), as float64.  scaled=False: the fault 'm' left
    unscaled' (m' = float16(x - h), still used as 2^-11 m')."""
    x = x.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        d = x - h.astype(np.float32)
        m = (d * np.float32(2048.0 if scaled else 1.0)).astype(np.float16)
    return h.astype(np.float64), m.astype(np.float64)


def _three(prod, u, v, fault):
    """uh vh + 2^-11 (uh vm' + um' vh) with exact (float64) products and sums; fault 'drop': no um' vh, 'unscaled': see split."""
    uh, um = split(u, fault != "unscaled")
    vh, vm = split(v, fault != "unscaled")
    cross = prod(uh, vm)
    if fault != "drop":
        cross = cross + prod(um, vh)
    return prod(uh, vh) + cross / 2048.0


def emulate_chain(x, layers, fault=None):
    """The chain as the kernels compute it, except that sums are exact: u = weights, v = activations, the intermediate rounded to
    fp32 and split again."""
    mid = x.astype(np.float32)
    for k, b, stride in layers:
        pre = _three(lambda u, v: conv_f64(v, u, 1, stride), k, mid, fault)
        pre = pre + b.astype(np.float64)
        mid = lrelu(pre).astype(np.float32)
    return mid


def blend_f32(f1, flow, flow_scale):
    """pwc_blend_corners: c00 x00, then three fused multiply-adds, every step rounded to fp32 (the products of two fp32 values are
    exact in float64)."""
    d = (flow.astype(np.float32) * np.float32(flow_scale)).astype(np.float32).astype(np.float64)
    N, H, W, _ = f1.shape
    fx, fy = d[..., 0], d[..., 1]
    fx0, fy0 = np.floor(fx), np.floor(fy)
    gy, gx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ys = [np.clip(gy + fy0 + i, 0, H - 1).astype(np.int64) for i in (0, 1)]
    xs = [np.clip(gx + fx0 + i, 0, W - 1).astype(np.int64) for i in (0, 1)]
    wy = [(fy0 + 1) - fy, fy - fy0]
    wx = [(fx0 + 1) - fx, fx - fx0]
    n = np.arange(N)[:, None, None]
    f1 = f1.astype(np.float64)
    v = np.zeros(f1.shape)
    for i in (0, 1):
        for j in (0, 1):
            w = (wy[i].astype(np.float32) * wx[j].astype(np.float32)).astype(np.float64)[..., None]
            v = (w * f1[n, ys[i], xs[j]] + v).astype(np.float32).astype(np.float64)
    return v.astype(np.float32)


def emulate_cv(f0, f1, flow=None, flow_scale=1.0, fault=None):
    C = f0.shape[3]
    f1w = f1.astype(np.float32) if flow is None else blend_f32(f1, flow, flow_scale)
    return lrelu(_three(corr_sum, f0, f1w, fault) / C)


def worst_ratio(y, ref, S):
    """r over the outputs with S != 0 (the others must be exact zeros)."""
    err = np.abs(y.astype(np.float64) - ref)
    zero = S == 0
    assert not np.any(err[zero])
    return float((err[~zero] / (ULP * S[~zero])).max())


# ------------------------------------------------------------------ inputs of the GPU tests: conv chains
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pair_operands(shape):
    """(x, layers) of pwc_conv3x3_c16pair_f32 at `shape` = (N, H, W): operands built like operands() of test_gpu_forward_f64."""
    N, H, W = shape
    x, k1, k2, b1, b2 = _frozen(magnitudes((N, H, W, 16), 501, 1.0), magnitudes((3, 3, 16, 16), 502, 1.0 / 12.0),
                                magnitudes((3, 3, 16, 16), 503, 1.0 / 12.0), magnitudes((16,), 504, 0.1), magnitudes((16,), 505, 0.1))
    return x, ((k1, b1, 1), (k2, b2, 1))


@functools.lru_cache(maxsize=None)
def c3_operands(shape):
    """(x, layers) of pwc_conv3x3_c3c16pair_f32 at `shape` = (Na, Nb, H0, W0): x holds the Na frames of x_a, then the Nb of x_b."""
    Na, Nb, H0, W0 = shape
    x, k0, k1, k2, b0, b1, b2 = _frozen(
        magnitudes((Na + Nb, H0, W0, 3), 511, 1.0), magnitudes((3, 3, 3, 16), 512, 1.0 / np.sqrt(27.0)),
        magnitudes((3, 3, 16, 16), 513, 1.0 / 12.0), magnitudes((3, 3, 16, 16), 514, 1.0 / 12.0), magnitudes((16,), 515, 0.1),
        magnitudes((16,), 516, 0.1), magnitudes((16,), 517, 0.1))
    return x, ((k0, b0, 2), (k1, b1, 1), (k2, b2, 1))


def _scaled(x, layers, sx=1.0, first=None, s=1.0):
    """x * sx; the weights of layer `first` * s; the biases of every layer that the scaled operand reaches * (sx * s) -- the chain is
    homogeneous in each, so every intermediate behind the scaled operand scales with it."""
    out = []
    for l, (k, b, stride) in enumerate(layers):
        sk = s if l == first else 1.0
        sb = sx * (s if first is not None and l >= first else 1.0)
        out.append(((k * sk).astype(np.float32), (b * sb).astype(np.float32), stride))
    return (x * sx).astype(np.float32), out


def chain_scale_cases(x, layers):
    """(tag, x, layers, small): the activations, and each layer's weights, at the scales 2^k of test_gpu_forward_f64; small: an
    operand below 2^-14."""
    for which in ["x"] + [f"w{l}" for l in range(len(layers))]:
        for kexp in SCALES:
            s = 2.0 ** kexp
            xs, ls = _scaled(x, layers, sx=s) if which == "x" else _scaled(x, layers, first=int(which[1]), s=s)
            small = min([float(np.abs(xs).min())] + [float(np.abs(k).min()) for k, _, _ in ls]) < 2.0 ** -14
            yield f"{which} {kexp}", xs, ls, small


def chain_spread_cases(x, layers):
    """(tag, x, layers): each layer's weights in turn log-uniform in magnitude over [2^-10, 2^6], random signs, per weight (one
    layer at a time: two spread layers in a row would take the intermediate behind them out of fp16's range)."""
    for l, (k, b, stride) in enumerate(layers):
        rs = np.random.RandomState(520 + l)
        kk = (2.0 ** rs.uniform(-10.0, 6.0, size=k.shape) * rs.choice([-1.0, 1.0], size=k.shape)).astype(np.float32)
        ls = list(layers)
        ls[l] = (kk, b, stride)
        yield f"spread w{l}", x, ls


def chain_site(x, layers):
    """The planted activation (n, y, x, c) and weight (dy, dx, ci, co): an interior pixel off the tile origin, the centre tap."""
    _, H, W, _ = x.shape
    return (0, H // 2 + 1, W // 2 + 3, 1), (1, 1, 1, 5)


def chain_top_cases(x, layers):
    """(tag, val, x, layers, reads): one operand of 65503 / 65519 / +-65520 planted in the activations and in each layer's weights;
    reads = the outputs that depend on it.  For a weight in front of the last layer the activations (and biases) are scaled by
    2^-4, which keeps the float64 intermediates below 65504 (tests/test_host_f16_pipe_ref.py)."""
    sx, sw = chain_site(x, layers)
    L = len(layers)
    hot = np.zeros(x.shape, bool)
    hot[sx] = True
    reads_x = reach(hot, layers)
    for which in ["x"] + [f"w{l}" for l in range(L)]:
        for val in TOP_VALUES:
            if which == "x":
                xs, ls = x.copy(), list(layers)
                xs[sx] = val
                reads = reads_x
            else:
                l = int(which[1])
                xs, ls = _scaled(x, layers, sx=2.0 ** -4) if l < L - 1 else (x, list(layers))
                k = ls[l][0].copy()
                k[sw] = val
                ls[l] = (k, ls[l][1], ls[l][2])
                N, H, W, _ = x.shape
                for _, _, stride in layers[:l + 1]:
                    H, W = out_hw(H, W, stride)
                hot_l = np.zeros((N, H, W, 16), bool)
                hot_l[..., sw[3]] = True                      # every pixel has its centre tap inside the image
                reads = reach(hot_l, layers[l + 1:]) if l < L - 1 else hot_l
            yield f"top {which}={val:.0f}", val, xs, ls, reads


def chain_overflow_cases(x, layers):
    """(tag, x, layers, site, reads): finite, in-range inputs whose layer-l output (l in front of the last layer) is positive and
    above 65520 at ONE (pixel, channel) `site`: an activation of 60000 under a centre tap of 2 (l = 0), or -- three layers, l = 1
    -- an activation of 60000 under a centre tap of 0.5 and then one of 4.  reads = the outputs behind that intermediate."""
    L = len(layers)
    N, H0, W0, _ = x.shape
    stride = layers[0][2]
    H, W = out_hw(H0, W0, stride)
    oy, ox, ci, co = H // 2 + 1, W // 2 + 3, 1, 5
    # the input pixel under the centre tap of output (oy, ox): 'SAME' pads in front by (total padding) // 2
    pt = max((H - 1) * stride + 3 - H0, 0) // 2
    pl = max((W - 1) * stride + 3 - W0, 0) // 2
    iy, ix = oy * stride + 1 - pt, ox * stride + 1 - pl
    for l in range(L - 1):
        xs = x.copy()
        xs[0, iy, ix, ci] = 60000.0
        ls = [(k.copy(), b, s) for k, b, s in layers]
        if l == 0:
            ls[0][0][1, 1, ci, co] = 2.0
            site = (0, oy, ox, co)
        else:
            ls[0][0][1, 1, ci, co] = 0.5
            ls[1][0][1, 1, co, co] = 4.0
            site = (0, oy, ox, co)
        hot = np.zeros((N, H, W, 16), bool)
        hot[site] = True
        yield f"overflow mid{l}", xs, ls, (l, site), reach(hot, layers[l + 1:])


# ------------------------------------------------------------------ inputs of the GPU tests: correlation
@functools.lru_cache(maxsize=None)
def cv_operands(shape):
    N, H, W, C = shape
    return _frozen(magnitudes((N, H, W, C), 531, 1.0), magnitudes((N, H, W, C), 532, 1.0))


@functools.lru_cache(maxsize=None)
def cv_flow(shape):
    """A flow (N, H, W, 2) whose displacement FLOW_SCALE * flow is a multiple of 1/8 px in [-6, 6] (the flow itself a multiple of
    1/32: the product is exact), with a few far outliers that point outside the frame: fx, the bilinear weights and 1 - w are
    exact in fp32, only the blend's own roundings remain."""
    N, H, W, _ = shape
    rs = np.random.RandomState(533)
    d = rs.randint(-48, 49, size=(N, H, W, 2)) / 8.0
    far = rs.uniform(size=(N, H, W)) < 0.04
    d[far] = rs.choice([-50.0, 50.0, -37.5, 23.125, 0.0], size=(int(far.sum()), 2))
    flow = (d / FLOW_SCALE).astype(np.float32)
    assert np.array_equal(flow.astype(np.float64) * FLOW_SCALE, d)
    flow.setflags(write=False)
    return flow


@functools.lru_cache(maxsize=None)
def cv_integer_flow(shape):
    """A whole-pixel displacement (+2, -1) everywhere: the blend returns f1's values exactly (weights 1, 0, 0, 0)."""
    N, H, W, _ = shape
    flow = np.empty((N, H, W, 2), np.float32)
    flow[..., 0], flow[..., 1] = 2.0 / FLOW_SCALE, -1.0 / FLOW_SCALE
    flow.setflags(write=False)
    return flow


def cv_scale_cases(f0, f1):
    """(tag, f0, f1, small): f0 and f1 separately at the scales 2^k."""
    for which in ("f0", "f1"):
        for kexp in SCALES:
            s = 2.0 ** kexp
            a = (f0 * s).astype(np.float32) if which == "f0" else f0
            b = (f1 * s).astype(np.float32) if which == "f1" else f1
            yield f"{which} {kexp}", a, b, min(float(np.abs(a).min()), float(np.abs(b).min())) < 2.0 ** -14


def cv_mixed_case(f0, f1):
    """Channel magnitudes log-uniform over [2^-10, 2^6], drawn per channel and per operand."""
    C = f0.shape[3]
    rs = np.random.RandomState(534)
    return ((f0 * 2.0 ** rs.uniform(-10.0, 6.0, size=C)).astype(np.float32),
            (f1 * 2.0 ** rs.uniform(-10.0, 6.0, size=C)).astype(np.float32))


def cv_site(shape):
    """The planted element (n, y, x, c): an interior pixel off the block origin, a channel in the last 32-channel group."""
    N, H, W, C = shape
    return N - 1, H // 2 + 1, W // 2 + 2, C - 7


def cv_top_cases(f0, f1, flow):
    """(tag, val, f0, f1, reads): one 65503 / 65519 / +-65520 in f0, then in f1.  reads: for f0 the 81 outputs of its pixel (those
    whose displaced pixel is outside the frame multiply it by the zero that stands for f1 there: inf x 0); for f1 the (pixel,
    displacement) pairs whose warped pixel is the planted one (flow: None or whole pixels)."""
    site = cv_site(f0.shape)
    reads0 = np.zeros(f0.shape[:3] + (81,), bool)
    reads0[site[:3]] = True
    hot = np.zeros(f1.shape)
    hot[site] = 1.0
    hotw = hot if flow is None else warp_f64(hot, flow, FLOW_SCALE)
    reads1 = corr_sum(np.ones(f0.shape), hotw) > 0
    for which in ("f0", "f1"):
        for val in TOP_VALUES:
            a, b = f0.copy(), f1.copy()
            (a if which == "f0" else b)[site] = val
            yield f"top {which}={val:.0f}", val, a, b, reads0 if which == "f0" else reads1
