"""The four F16-pipe launches that were only held to the fp32 oracle's whole-tensor tolerance -- pwc_conv3x3_c16pair_f32 (16 -> 16 ->
16, the intermediate in LDS), pwc_conv3x3_c3c16pair_f32 (pyramid level 1 from the raw frames, 3 -> 16 -> 16 -> 16),
pwc_warp_cost_volume_concat_h2_f32 and pwc_warp_cost_volume_concat_blk_f32 -- against float64 per output element, through their C
entry points, with the metric of tests/test_gpu_forward_f64.py: r = max_i |y_i - ref_i| / (2^-24 S_i).

References, inputs, bounds and their derivation: tests/f16_pipe_ref.py (chains are judged on the PROPAGATED S: 2 x 16 for the
pair, 3 x 16 for the three-layer launch; the correlation 16, behind a warp 16 + 4; B_TOP = 160 with a planted 65503 / 65519).
tests/test_host_f16_pipe_ref.py checks on the CPU that the references agree with the oracle, that every case's preconditions hold
and what a dropped product or an unscaled m' would measure on these inputs.

  * operand scales 2^k, activations and each layer's weights (f0 and f1) separately: r <= B where every operand is at least
    2^-14, |y - ref| <= B 2^-24 S + 2^-35 T per element below that;
  * mixed magnitudes, log-uniform over [2^-10, 2^6] per weight / per channel: r <= B per element;
  * a single 65503, 65519, +65520, -65520 in the activations and in each layer's weights (in f0 and in f1, without a flow and
    with a whole-pixel one): NaN on exactly the outputs that read +-65520, no inf, no NaN for 65503 / 65519, r <= B_TOP on every
    finite output;
  * conv chains: an intermediate above 65520 from finite in-range inputs: NaN on every output behind it, r <= B on all others;
  * five launches return the same bits.

Shapes are the smallest that reach every tile edge and both launch forms of the block kernel (f16_pipe_ref).  The correlation's
flows have displacements flow_scale * flow that are multiples of 1/8 px in [-6, 6] with a few far outliers that leave the frame, at
flow_scale = 4: the displacement, the bilinear weights and 1 - w are exact in fp32.  Measured on an MI355X:
profiles/f16pipe_f64_gpu_test_figures.txt.
"""
import numpy as np
import pytest
import torch

from tests import f16_pipe_ref as F
from tests.test_gpu_forward_f64 import B_TOP, SLOPE, SUB, ULP, ratio
from tests.test_gpu_ops import _p, gpu as _gpu

pytestmark = pytest.mark.gpu

CHAINS = [("pair", s) for s in F.PAIR_SHAPES] + [("c3", s) for s in F.C3_SHAPES]
CVS = [("h2", s) for s in F.CVH_SHAPES] + [("blk", s) for s in F.CVB_SHAPES]
B_CHAIN = {"pair": F.B_PAIR, "c3": F.B_C3}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ launches
def gpu(a):
    return _gpu(np.array(a, np.float32))            # (a copy: the shared operands are read-only)


def run_pair(L, x, layers, x_slack=0, y_slack=0):
    """One pwc_conv3x3_c16pair_f32 launch.  Slack channels of x hold NaN, of y -7 (returned with the slack)."""
    from pwcnet_amd import _lib
    N, H, W, _ = x.shape
    (k1, b1, _), (k2, b2, _) = layers
    xs = np.full((N, H, W, 16 + x_slack), np.nan, np.float32)
    xs[..., :16] = x
    xg, k1g, k2g, b1g, b2g = gpu(xs), gpu(k1), gpu(k2), gpu(b1), gpu(b2)
    packed = torch.empty(L.pwc_conv3x3_c16pair_packed_floats(), device="cuda")
    _lib.check(L.pwc_conv3x3_c16pair_pack_f32(_p(k1g), _p(k2g), _p(packed), None))
    y = torch.full((N, H, W, 16 + y_slack), -7.0, device="cuda")
    _lib.check(L.pwc_conv3x3_c16pair_f32(_p(xg), 16 + x_slack, _p(packed), _p(b1g), _p(b2g), _p(y), 16 + y_slack, N, H, W, SLOPE,
                                         None))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def run_c3(L, shape, x, layers):
    """One pwc_conv3x3_c3c16pair_f32 launch: the first Na images of x as x_a, the others as x_b."""
    from pwcnet_amd import _lib
    Na, Nb, H0, W0 = shape
    (k0, b0, _), (k1, b1, _), (k2, b2, _) = layers
    xag, xbg = gpu(x[:Na]), (gpu(x[Na:]) if Nb else None)
    k0g, k1g, k2g, b0g, b1g, b2g = gpu(k0), gpu(k1), gpu(k2), gpu(b0), gpu(b1), gpu(b2)
    packed = torch.empty(L.pwc_conv3x3_c3c16pair_packed_floats(), device="cuda")
    _lib.check(L.pwc_conv3x3_c3c16pair_pack_f32(_p(k0g), _p(k1g), _p(k2g), _p(packed), None))
    y = torch.full((Na + Nb, (H0 + 1) // 2, W0 // 2, 16), -7.0, device="cuda")
    _lib.check(L.pwc_conv3x3_c3c16pair_f32(_p(xag), Na, _p(xbg) if Nb else None, Nb, _p(packed), _p(b0g), _p(b1g), _p(b2g), _p(y),
                                           16, H0, W0, SLOPE, None))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def run_chain(L, kind, shape, x, layers):
    return run_pair(L, x, layers) if kind == "pair" else run_c3(L, shape, x, layers)


def chain_operands(kind, shape):
    return F.pair_operands(shape) if kind == "pair" else F.c3_operands(shape)


def run_cv(L, kind, f0, f1, flow):
    """One launch of the kernel's own entry point (h2: pwc_warp_cost_volume_concat_h2_f32, blk: pwc_warp_cost_volume_concat_blk_f32)
    into dense 84-channel records whose padding channels are the kernel's to zero; the 81 correlation channels."""
    from pwcnet_amd import _lib
    N, H, W, C = f0.shape
    fn = L.pwc_warp_cost_volume_concat_h2_f32 if kind == "h2" else L.pwc_warp_cost_volume_concat_blk_f32
    g0, g1 = gpu(f0), gpu(f1)
    fl = gpu(flow) if flow is not None else None
    out = torch.full((N, H, W, 84), -7.0, device="cuda")
    _lib.check(fn(_p(g0), C, _p(g1), C, _p(fl) if fl is not None else None, 2 if fl is not None else 0, F.FLOW_SCALE, _p(out), 84, 1,
                  None, 0, N, H, W, C, 4, SLOPE, None))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[..., 81:] == 0.0), "padding channels 81..83 are zeroed"
    return out[..., :81]


# ------------------------------------------------------------------ checks
def judge(tag, y, ref, S, T, small, B):
    """r of one launch, printed; r <= B (every operand at least 2^-14) or the absolute-floor formula per element."""
    r, err = ratio(y, ref, S)
    print(f"MEASURED {tag} {r:.4g}")
    if small:
        excess = float((err - (B * ULP * S + SUB * T)).max())
        assert excess <= 0.0, (tag, r, excess)
    else:
        assert r <= B, (tag, r, B)
    return r


def judge_where(tag, y, ref, S, ok, B):
    """r over the outputs `ok` (all finite there), printed and held to B; an output with S = 0 must be an exact 0."""
    assert np.all(np.isfinite(y[ok])), (tag, "a non-finite output outside the expected set")
    err = np.abs(y.astype(np.float64) - ref)
    zero = ok & (S == 0)
    assert not np.any(err[zero]), (tag, "an output with S = 0 must be an exact 0")
    sel = ok & (S != 0)
    r = float((err[sel] / (ULP * S[sel])).max()) if sel.any() else 0.0      # (a weight in front of the last layer: every output reads it)
    print(f"MEASURED {tag} {r:.4g} nan={int(np.isnan(y).sum())}")
    assert r <= B, (tag, r, B)


def judge_planted(tag, val, y, ref, S, reads):
    nan = np.isnan(y)
    assert not np.any(np.isinf(y)), (tag, "inf")
    assert not np.any(nan & ~reads), (tag, "NaN outside the outputs that read the operand", int((nan & ~reads).sum()))
    if abs(val) >= 65520.0:
        assert nan[reads].all(), (tag, "a finite output that reads the operand", int((~nan[reads]).sum()))
    else:
        assert not nan.any(), (tag, int(nan.sum()))
    judge_where(tag, y, ref, S, ~nan, B_TOP)


# ------------------------------------------------------------------ conv chains
@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_operand_scales_vs_float64(L, kind, shape):
    x, layers = chain_operands(kind, shape)
    for tag, xs, ls, small in F.chain_scale_cases(x, layers):
        ref, S, T = F.chain_reference(xs, ls)
        judge(f"{kind} {shape} {tag}", run_chain(L, kind, shape, xs, ls), ref, S, T, small, B_CHAIN[kind])


@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_mixed_magnitude_weights_vs_float64(L, kind, shape):
    x, layers = chain_operands(kind, shape)
    for tag, xs, ls in F.chain_spread_cases(x, layers):
        ref, S, T = F.chain_reference(xs, ls)
        judge(f"{kind} {shape} {tag}", run_chain(L, kind, shape, xs, ls), ref, S, T, False, B_CHAIN[kind])


@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_fp16_top_edge(L, kind, shape):
    x, layers = chain_operands(kind, shape)
    for tag, val, xs, ls, reads in F.chain_top_cases(x, layers):
        ref, S, _ = F.chain_reference(xs, ls)
        judge_planted(f"{kind} {shape} {tag}", val, run_chain(L, kind, shape, xs, ls), ref, S, reads)


@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_intermediate_beyond_fp16_range_is_nan(L, kind, shape):
    """Finite in-range inputs, one intermediate above 65520 that the caller never sees: NaN on every output behind it (never a
    finite wrong number), every other output finite and within B."""
    x, layers = chain_operands(kind, shape)
    for tag, xs, ls, _, reads in F.chain_overflow_cases(x, layers):
        ref, S, _ = F.chain_reference(xs, ls)
        y = run_chain(L, kind, shape, xs, ls)
        nan = np.isnan(y)
        assert not np.any(np.isinf(y)), (tag, "inf")
        assert nan[reads].all(), (kind, shape, tag, "a finite output behind the intermediate", int((~nan[reads]).sum()))
        assert not np.any(nan & ~reads), (kind, shape, tag, int((nan & ~reads).sum()))
        judge_where(f"{kind} {shape} {tag}", y, ref, S, ~reads, B_CHAIN[kind])


def test_pair_strided_views(L):
    """x_cs = 20 with NaN in the slack, y_cs = 24 with a sentinel in the slack."""
    shape = F.PAIR_SHAPES[0]
    x, layers = F.pair_operands(shape)
    ref, S, T = F.chain_reference(x, layers)
    y = run_pair(L, x, layers, x_slack=4, y_slack=8)
    assert np.all(y[..., 16:] == -7.0), "the slack of y was written"
    judge(f"pair {shape} views", y[..., :16], ref, S, T, False, F.B_PAIR)      # (ratio fails on a non-finite output: x's slack)
    assert np.array_equal(y[..., :16], run_pair(L, x, layers)), "the strides of the views changed a sum"


@pytest.mark.parametrize("kind,shape", [CHAINS[0], CHAINS[5]])
def test_chain_repeats_bitwise(L, kind, shape):
    x, layers = chain_operands(kind, shape)
    first = run_chain(L, kind, shape, x, layers)
    for _ in range(4):
        assert np.array_equal(first, run_chain(L, kind, shape, x, layers))


# ------------------------------------------------------------------ correlation
def cv_flows(shape):
    return (("noflow", None, F.B_CV), ("flow", F.cv_flow(shape), F.B_CV_WARP))


@pytest.mark.parametrize("kind,shape", CVS)
def test_cv_operand_scales_vs_float64(L, kind, shape):
    f0, f1 = F.cv_operands(shape)
    for name, flow, B in cv_flows(shape):
        for tag, a, b, small in F.cv_scale_cases(f0, f1):
            ref, S, T = F.cv_reference(a, b, flow, F.FLOW_SCALE)
            judge(f"cv_{kind} {shape} {name} {tag}", run_cv(L, kind, a, b, flow), ref, S, T, small, B)


@pytest.mark.parametrize("kind,shape", CVS)
def test_cv_mixed_channel_magnitudes_vs_float64(L, kind, shape):
    a, b = F.cv_mixed_case(*F.cv_operands(shape))
    for name, flow, B in cv_flows(shape):
        ref, S, T = F.cv_reference(a, b, flow, F.FLOW_SCALE)
        judge(f"cv_{kind} {shape} {name} mixed", run_cv(L, kind, a, b, flow), ref, S, T, False, B)


@pytest.mark.parametrize("kind,shape", CVS)
def test_cv_fp16_top_edge(L, kind, shape):
    f0, f1 = F.cv_operands(shape)
    for name, flow in (("noflow", None), ("whole", F.cv_integer_flow(shape))):
        for tag, val, a, b, reads in F.cv_top_cases(f0, f1, flow):
            ref, S, _ = F.cv_reference(a, b, flow, F.FLOW_SCALE)
            judge_planted(f"cv_{kind} {shape} {name} {tag}", val, run_cv(L, kind, a, b, flow), ref, S, reads)


@pytest.mark.parametrize("kind,shape", [CVS[0], CVS[3], CVS[6]])
def test_cv_repeats_bitwise(L, kind, shape):
    """The correlation kernels run producer and consumer waves (h2) and three workgroups per record (blk, fewer than 256 blocks):
    five launches, the same bits."""
    f0, f1 = F.cv_operands(shape)
    flow = F.cv_flow(shape)
    first = run_cv(L, kind, f0, f1, flow)
    for _ in range(4):
        assert np.array_equal(first, run_cv(L, kind, f0, f1, flow))
