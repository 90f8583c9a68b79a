"""What tests/test_gpu_f16_pipe_f64.py relies on, checked without a GPU on that module's own inputs (tests/f16_pipe_ref.py):

  * the float64 references agree with the fp32 oracle within its rounding (close() defaults);
  * the preconditions of every case: operands and float64 intermediates inside fp16's range where the case must stay finite, no
    output with S = 0 that is not an out-of-frame displacement, S_(l-1) >= 2^-8 where a chain is judged by r <= B (the floor of a
    small intermediate, f16_pipe_ref's docstring), the planted intermediate of the overflow cases above 65520, positive and alone,
    'reads' masks that are neither empty nor everything;
  * the bounds have teeth: a numpy emulation of the arithmetic (h = float16(x), m' = float16((x - h) 2^11), three products, exact
    sums) stays within r <= 8 on the same inputs, and the same emulation with the um' vh product dropped, or with m' left
    unscaled, exceeds the bounds of the GPU tests (test_chain_emulation_and_faults says where, and names the one place where it
    does not: the three-layer launch at uniform operand scales).
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import f16_pipe_ref as F
from tests.test_gpu_forward_f64 import B_TOP, SLOPE, SUB, ULP, reference
from tests.test_gpu_ops import close

CHAINS = [("pair", s) for s in F.PAIR_SHAPES] + [("c3", s) for s in F.C3_SHAPES]
CVS = [("h2", s) for s in F.CVH_SHAPES] + [("blk", s) for s in F.CVB_SHAPES]
FP16_MAX = 65504.0


def chain_operands(kind, shape):
    return F.pair_operands(shape) if kind == "pair" else F.c3_operands(shape)


def oracle_chain(x, layers):
    y = x
    for k, b, stride in layers:
        y = orc.conv3x3(y, k, b, stride, 1, SLOPE)
    return y


def cv_flows(shape):
    return {"none": None, "flow": F.cv_flow(shape), "whole": F.cv_integer_flow(shape)}


# ------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_reference_matches_oracle(kind, shape):
    x, layers = chain_operands(kind, shape)
    ref, S, T, mids, Ss = F.chain_reference(x, layers, full=True)
    close(ref.astype(np.float32), oracle_chain(x, layers))
    assert np.all(S > 0) and np.all(T > 0) and np.all(S >= np.abs(ref))
    for mid, Sl in zip(mids[:-1], Ss[:-1]):
        assert np.all(Sl >= np.abs(mid))
    # one layer of the chain is the single-layer reference of test_gpu_forward_f64
    k, b, stride = layers[0]
    ref1, _, _ = reference(x, k, b, 1, stride)
    assert np.array_equal(ref1, mids[0])
    for tag, xs, ls in F.chain_spread_cases(x, layers):
        close(F.chain_reference(xs, ls)[0].astype(np.float32), oracle_chain(xs, ls))


@pytest.mark.parametrize("kind,shape", CVS)
def test_cv_reference_matches_oracle(kind, shape):
    f0, f1 = F.cv_operands(shape)
    for a, b in ((f0, f1), F.cv_mixed_case(f0, f1)):
        for name, flow in cv_flows(shape).items():
            f1w = b if flow is None else orc.warp(b, flow, "bilinear", flow_scale=F.FLOW_SCALE)
            ref, S, T = F.cv_reference(a, b, flow, F.FLOW_SCALE)
            close(ref.astype(np.float32), orc.cost_volume(a, f1w, 4))
            assert np.all(S >= np.abs(ref)) and np.all((S == 0) == (T == 0))
    # a whole-pixel flow returns f1's own values
    w = F.warp_f64(f1, F.cv_integer_flow(shape), F.FLOW_SCALE)
    assert np.all(np.isin(w[0, :, :, 0], f1[0, :, :, 0]))


# ------------------------------------------------------------------ preconditions of the GPU cases
def _intermediates_in_range(x, layers, not_small):
    assert max([float(np.abs(x).max())] + [float(np.abs(k).max()) for k, _, _ in layers]) < FP16_MAX
    ref, S, T, mids, Ss = F.chain_reference(x, layers, full=True)
    assert max(float(np.abs(m).max()) for m in mids[:-1]) < FP16_MAX
    assert np.all(S > 0)
    if not_small:
        assert min(float(Sl.min()) for Sl in Ss[:-1]) >= 2.0 ** -8


@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_case_preconditions(kind, shape):
    x, layers = chain_operands(kind, shape)
    n_small = 0
    for tag, xs, ls, small in F.chain_scale_cases(x, layers):
        _intermediates_in_range(xs, ls, not small)
        n_small += small
    assert 0 < n_small < 8 * (1 + len(layers))
    for tag, xs, ls in F.chain_spread_cases(x, layers):
        assert min(float(np.abs(k).min()) for k, _, _ in ls) >= 2.0 ** -14
        _intermediates_in_range(xs, ls, True)
    L = len(layers)
    for tag, val, xs, ls, reads in F.chain_top_cases(x, layers):
        ref, S, T, mids, Ss = F.chain_reference(xs, ls, full=True)
        assert reads.shape == ref.shape and reads.any()
        # a weight in front of the last layer feeds every output; every other planted operand leaves outputs that do not read it
        everything = tag.startswith("top w") and int(tag[5]) < L - 1
        assert reads.all() == everything, tag
        if abs(val) < 65520.0:
            assert max(float(np.abs(m).max()) for m in mids[:-1]) < FP16_MAX, tag
            assert np.all(S > 0)
    for tag, xs, ls, (l, site), reads in F.chain_overflow_cases(x, layers):
        assert max([float(np.abs(xs).max())] + [float(np.abs(k).max()) for k, _, _ in ls]) < FP16_MAX
        ref, S, T, mids, Ss = F.chain_reference(xs, ls, full=True)
        assert mids[l][site] > 65520.0, (tag, mids[l][site])
        for j, m in enumerate(mids[:-1]):
            over = np.abs(m) >= FP16_MAX
            assert int(over.sum()) == (1 if j == l else 0), (tag, j, int(over.sum()))
        assert reads.any() and not reads.all() and np.all(S > 0)
        # the outputs behind one intermediate pixel: 3 x 3 pixels a layer, every channel
        side = 2 * (L - 1 - l) + 1
        assert int(reads.sum()) == side * side * 16, (tag, int(reads.sum()))
    cases = [t for t, *_ in F.chain_overflow_cases(x, layers)]
    assert cases == [f"overflow mid{l}" for l in range(L - 1)]


@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_receptive_sets(kind, shape):
    """The outputs that read the planted activation: 5 x 5 pixels behind the pair; behind the three-layer launch the stride-2
    layer's outputs that hold the raw pixel in their window, grown by two pixels."""
    x, layers = chain_operands(kind, shape)
    sx, _ = F.chain_site(x, layers)
    tag, val, xs, ls, reads = next(iter(F.chain_top_cases(x, layers)))
    assert not reads[1:].any()
    ys, xcols = np.nonzero(reads[0].all(axis=2))
    assert np.array_equal(reads[0].any(axis=2), reads[0].all(axis=2))
    if kind == "pair":
        assert (ys.min(), ys.max(), xcols.min(), xcols.max()) == (sx[1] - 2, sx[1] + 2, sx[2] - 2, sx[2] + 2)
        assert len(ys) == 25
    else:
        H0, W0 = x.shape[1:3]
        pt = H0 & 1                                    # 'SAME', stride 2: odd sizes pad one line in front, even ones none
        first = [o for o in range((H0 + 1) // 2) if 2 * o - pt <= sx[1] <= 2 * o - pt + 2]
        firstx = [o for o in range(W0 // 2) if 2 * o <= sx[2] <= 2 * o + 2]
        assert (ys.min(), ys.max()) == (first[0] - 2, first[-1] + 2) and (xcols.min(), xcols.max()) == (firstx[0] - 2, firstx[-1] + 2)
        assert len(ys) == (len(first) + 4) * (len(firstx) + 4)


@pytest.mark.parametrize("kind,shape", CVS)
def test_cv_case_preconditions(kind, shape):
    N, H, W, C = shape
    f0, f1 = F.cv_operands(shape)
    inside = F.corr_sum(np.ones((N, H, W, 1)), np.ones((N, H, W, 1))) > 0
    assert inside.any() and not inside.all()
    flows = cv_flows(shape)
    d = flows["flow"].astype(np.float64) * F.FLOW_SCALE
    assert np.array_equal(d * 8, np.round(d * 8)) and (np.abs(d) > 6).any() and (np.abs(d) <= 6).mean() > 0.9
    gx = np.arange(W)[None, None, :] + d[..., 0]
    assert ((gx < -1) | (gx > W)).any(), "no outlier points outside the frame"
    for name, flow in flows.items():
        n_small = 0
        for tag, a, b, small in F.cv_scale_cases(f0, f1):
            assert max(float(np.abs(a).max()), float(np.abs(b).max())) < FP16_MAX
            ref, S, T = F.cv_reference(a, b, flow, F.FLOW_SCALE)
            assert np.array_equal(S == 0, ~inside), (name, tag)        # S = 0 only where the displaced pixel is outside the frame
            n_small += small
        assert 0 < n_small < 16
        a, b = F.cv_mixed_case(f0, f1)
        assert min(float(np.abs(a).min()), float(np.abs(b).min())) >= 2.0 ** -14
        assert max(float(np.abs(a).max()), float(np.abs(b).max())) < FP16_MAX
        assert np.array_equal(F.cv_reference(a, b, flow, F.FLOW_SCALE)[1] == 0, ~inside)
    n, sy, sx, sc = F.cv_site(shape)
    assert 0 < sy < H - 1 and 0 < sx < W - 1
    for name, flow in (("none", None), ("whole", flows["whole"])):
        dy, dx = (0, 0) if flow is None else (-1, 2)
        wy, wx = sy - dy, sx - dx                       # the warped pixel that holds the planted one
        assert 0 <= wy < H and 0 <= wx < W              # (clipped corners repeat only border pixels of f1: the site is none)
        pairs = sum(1 for y in range(H) if abs(y - wy) <= 4) * sum(1 for xx in range(W) if abs(xx - wx) <= 4)
        for tag, val, a, b, reads in F.cv_top_cases(f0, f1, flow):
            assert reads.any() and not reads.all()
            if "f0" in tag:
                assert int(reads.sum()) == 81 and reads[n, sy, sx].all()
                assert a[n, sy, sx, sc] == val and np.array_equal(b, f1)
            else:
                assert int(reads.sum()) == pairs <= 81, (name, tag, int(reads.sum()), pairs)
                assert not reads[:n].any()
                assert b[n, sy, sx, sc] == val and np.array_equal(a, f0)
                if flow is not None:
                    assert F.warp_f64(b, flow, F.FLOW_SCALE)[n, wy, wx, sc] == val       # the blend returns the planted value


# ------------------------------------------------------------------ the bounds have teeth
def _teeth(tag, emu, ref, S, T, small, bound):
    """The exact-sum emulation within B_EMU (below 2^-14: the absolute-floor formula); bound is not None: both faults beyond it."""
    r = {}
    for fault in (None, "drop", "unscaled"):
        y = emu(fault)
        assert np.all(np.isfinite(y)), (tag, fault)
        err = np.abs(y.astype(np.float64) - ref)
        assert not np.any(err[S == 0])
        if small:
            r[fault] = float((err - (F.B_EMU * ULP * S + SUB * T)).max())
        else:
            r[fault] = F.worst_ratio(y, ref, S)
    if small:
        assert r[None] <= 0.0, (tag, r)
        return
    assert r[None] <= F.B_EMU, (tag, r)
    if bound is not None:
        assert r["drop"] > bound and r["unscaled"] > bound, (tag, r, bound)


@pytest.mark.parametrize("kind,shape", CHAINS)
def test_chain_emulation_and_faults(kind, shape):
    """Both faults exceed the chain's bound on every spread-weight case and B_TOP on every finite top-edge case, at every shape;
    at uniform operand scales they exceed the pair's 32 (r = 111 .. 181), but the three-layer launch's propagated S has grown so far
    past |ref| there that the dropped product reaches r = 26 .. 56 against 48: those cases alone would let it pass on two of the
    three shapes, the spread-weight (68 .. 169) and top-edge cases (202 and more against 160) do not."""
    x, layers = chain_operands(kind, shape)
    bound = F.B_PAIR if kind == "pair" else F.B_C3
    for tag, xs, ls, small in F.chain_scale_cases(x, layers):
        ref, S, T = F.chain_reference(xs, ls)
        _teeth((kind, shape, tag), lambda fault: F.emulate_chain(xs, ls, fault), ref, S, T, small, bound if kind == "pair" else None)
    for tag, xs, ls in F.chain_spread_cases(x, layers):
        ref, S, T = F.chain_reference(xs, ls)
        _teeth((kind, shape, tag), lambda fault: F.emulate_chain(xs, ls, fault), ref, S, T, False, bound)
    for tag, val, xs, ls, reads in F.chain_top_cases(x, layers):
        if abs(val) < 65520.0:
            ref, S, T = F.chain_reference(xs, ls)
            _teeth((kind, shape, tag), lambda fault: F.emulate_chain(xs, ls, fault), ref, S, T, False, B_TOP)


@pytest.mark.parametrize("kind,shape", CVS)
def test_cv_emulation_and_faults(kind, shape):
    """On the first image of every case (the images of a launch are independent): both faults beyond B_TOP, the largest bound."""
    f0, f1 = F.cv_operands(shape)
    for name, flow in (("none", None), ("flow", F.cv_flow(shape))):
        fl = None if flow is None else flow[:1]
        cases = [(t, a, b, small) for t, a, b, small in F.cv_scale_cases(f0, f1)] + [("mixed",) + F.cv_mixed_case(f0, f1) + (False,)]
        for tag, a, b, small in cases:
            a, b = a[:1], b[:1]
            ref, S, T = F.cv_reference(a, b, fl, F.FLOW_SCALE)
            _teeth((kind, shape, name, tag), lambda fault: F.emulate_cv(a, b, fl, F.FLOW_SCALE, fault), ref, S, T, small, B_TOP)
    n = F.cv_site(shape)[0]
    for name, flow in (("none", None), ("whole", F.cv_integer_flow(shape))):
        fl = None if flow is None else flow[:1]
        for tag, val, a, b, reads in F.cv_top_cases(f0, f1, flow):
            if abs(val) < 65520.0:
                a, b = a[n:n + 1], b[n:n + 1]
                ref, S, T = F.cv_reference(a, b, fl, F.FLOW_SCALE)
                _teeth((kind, shape, name, tag), lambda fault: F.emulate_cv(a, b, fl, F.FLOW_SCALE, fault), ref, S, T, False, B_TOP)


def test_top_edge_emulation():
    """The split at fp16's top edge, emulated: 65503 and 65519 round h to a finite value and stay exact to 22 bits, +-65520 round
    h to infinity -- the band the GPU tests plant."""
    h, m = F.split(np.array([65503.0, 65519.0, 65520.0, -65520.0], np.float32))
    assert np.all(np.isfinite(h[:2])) and np.all(np.isinf(h[2:]))
    assert np.array_equal(h[:2] + m[:2] / 2048.0, [65503.0, 65519.0])
