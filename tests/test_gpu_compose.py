"""Flow composition on the GPU (pwc_compose.hip, pwcnet_amd.compose, infer_continuous.py --chain) against the float64 restatement
of tests/compose_ref.py (checked on the CPU by tests/test_host_compose.py).

Forward: valid_ac exact; an invalid pixel exactly (1e10f, 1e10f); a valid one |got - ref| <= 2^-24 |ref| + 2^-50 A,
  A = |f_k| + sum b_c |flow_bc[c,k]|: the ONE rounding to float32, and a few double ulps of either side's evaluation order.
dflow_ab: |got - ref| <= 2^-23 A', A' the sum of the magnitudes of the exact terms (the splat tests' rule): the value is formed in
  double and rounded once.  Exact zeros at invalid pixels.
dflow_bc: |got - ref| <= 2^-23 |ref| + K_t 2^-36 m_n: each of the K_t contributions to a cell is rounded to the fixed-point step at
  the image's scale 2^e_n < 2 m_n, which costs at most 2^-37 2^e_n; the sum of the integers is exact and is rounded to float32
  once.
Measured figures: profiles/compose_gpu_test_figures.txt."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import compose as C  # the feature: without it nothing here can be collected
from tests import compose_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, H, W): one pixel (every corner clamps); 35 pixels; 135 pixels (two wavefronts and a tail); 257 pixels in a row, the
# smallest image of more than one workgroup (and of more than one part of the per-image maximum); 851 pixels
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 9, 15), (2, 1, 257), (2, 23, 37)]
# the masks given, and "slices": both masks, every flow and gradient a channel slice at an odd offset of a 5-channel buffer
# (pointers off the 8-byte boundary, odd channel stride: the 4-byte path)
VARIANTS = R.MODES + ("slices",)
INTEGER = ((3, 9, 15), True)                         # integer-valued flow_ab (zero weights), the last image all unknown


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.compose_flows is C.compose_flows and pwcnet_amd.chain_flows is C.chain_flows
    return pwcnet_amd


@functools.lru_cache(maxsize=None)
def _case(shape, integer=False):
    """The seeded inputs of a shape (numpy, never written to) and the restatement's forward and gradient per mask mode."""
    N, H, W = shape
    ab, bc, vab, vbc, g = R.random_case(N, H, W, seed=1000 + 10 * H + W, integer=integer)
    ref = {}
    for mode in R.MODES:
        ma, mb = R.masks_of(mode, vab, vbc)
        ref[mode] = (R.compose(ab, bc, ma, mb)[:3], R.compose_grad(ab, bc, g, ma, mb))
    return ab, bc, vab, vbc, g, ref


def _sliced(a):
    """The array on the GPU as channels 1:3 of a 5-channel buffer."""
    wide = torch.full(tuple(a.shape[:3]) + (5,), float("nan"), dtype=torch.float32, device="cuda")
    wide[..., 1:3] = torch.from_numpy(a).cuda()
    return wide[..., 1:3]


def _inputs(case, variant):
    ab, bc, vab, vbc, g, ref = case
    mode = "both" if variant == "slices" else variant
    ma, mb = R.masks_of(mode, vab, vbc)
    up = _sliced if variant == "slices" else (lambda a: torch.from_numpy(a).cuda())
    return (up(ab), up(bc), up(g), None if ma is None else torch.from_numpy(ma).cuda(), None if mb is None else torch.from_numpy(mb).cuda(),
            ref[mode])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_forward(tag, out, valid, ref):
    ref_out, ref_valid, A = ref
    assert out.dtype == torch.float32 and valid.dtype == torch.bool and valid.is_contiguous()
    assert np.array_equal(valid.cpu().numpy(), ref_valid), tag
    o = out.cpu().numpy()
    assert bool((o[~ref_valid] == np.float32(1e10)).all()), tag
    err = np.abs(o.astype(np.float64) - ref_out)[ref_valid]
    tol = (2.0 ** -24 * np.abs(ref_out) + 2.0 ** -50 * A)[ref_valid]
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f"compose forward {tag}: valid {int(ref_valid.sum())} of {ref_valid.size}, worst error / bound {worst:.3f}")
    assert bool((err <= tol).all()), (tag, float(err.max()))


def _check_grad(tag, dab, dbc, ref, scale=1.0):
    """scale: the power of two the upstream gradient was multiplied by (the bounds are linear in it)."""
    da, db = dab.cpu().numpy().astype(np.float64), dbc.cpu().numpy().astype(np.float64)
    assert bool((da[~ref["valid"]] == 0).all()), tag
    err_a, tol_a = np.abs(da - scale * ref["dab"]), 2.0 ** -23 * scale * ref["dab_mag"]
    tol_b = 2.0 ** -23 * scale * np.abs(ref["dbc"]) + (ref["K"] * 2.0 ** -36 * scale * ref["m"][:, None, None])[..., None]
    err_b = np.abs(db - scale * ref["dbc"])
    worst_a = float((err_a / np.maximum(tol_a, 1e-300)).max())
    worst_b = float((err_b / np.maximum(tol_b, 1e-300)).max())
    print(f"compose grad {tag}: dflow_ab worst error / bound {worst_a:.3f}, dflow_bc {worst_b:.3f} (K_t up to {int(ref['K'].max())})")
    assert bool((err_a <= tol_a).all()), (tag, float(err_a.max()))
    assert bool((err_b <= tol_b).all()), (tag, float(err_b.max()))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape,integer", [(s, False) for s in SHAPES] + [INTEGER])
def test_forward_and_gradient_against_float64(P, shape, integer, variant):
    ab, bc, g, ma, mb, (ref_fwd, ref_grad) = _inputs(_case(shape, integer), variant)
    tag = f"{shape}{' integer' if integer else ''} {variant}"
    out, valid = P.compose_flows(ab, bc, ma, mb)
    _check_forward(tag, out, valid, ref_fwd)
    if integer:
        assert not bool(valid[-1].any()) and float(ref_grad["m"][-1]) == 0.0
    dab, dbc = P.compose_grad(ab, bc, g, ma, mb)
    _check_grad(tag, dab, dbc, ref_grad)
    if integer:
        assert bool((dbc[-1] == 0).all())                                      # m_n = 0: exact zeros
    # g times 2^-20: the same bits times 2^-20 (a fixed, unscaled step would lose them)
    s = 2.0 ** -20
    small = (g * s) if variant != "slices" else _sliced((g * s).cpu().numpy())
    dab_s, dbc_s = P.compose_grad(ab, bc, small, ma, mb)
    _check_grad(tag + " g x 2^-20", dab_s, dbc_s, ref_grad, scale=s)
    assert _same_bits(dab_s, dab * s) and _same_bits(dbc_s, dbc * s), tag
    # two calls: the same bits
    out2, valid2 = P.compose_flows(ab, bc, ma, mb)
    dab2, dbc2 = P.compose_grad(ab, bc, g, ma, mb)
    assert _same_bits(out2, out) and torch.equal(valid2, valid) and _same_bits(dab2, dab) and _same_bits(dbc2, dbc), tag
    # into the caller's tensors (for "slices": channel slices), and accumulate adds exactly what a plain call writes
    base = torch.from_numpy(np.random.RandomState(5).uniform(0.5, 2.0, size=(2,) + tuple(dab.shape)).astype(np.float32)).cuda()
    ta, tb = (_sliced(base[i].cpu().numpy()) if variant == "slices" else base[i].clone() for i in range(2))
    ra, rb = P.compose_grad(ab, bc, g, ma, mb, dflow_ab=ta, dflow_bc=tb, accumulate=True)
    assert ra is ta and rb is tb
    assert _same_bits(ta, base[0] + dab) and _same_bits(tb, base[1] + dbc), tag
    ra, rb = P.compose_grad(ab, bc, g, ma, mb, dflow_ab=ta, dflow_bc=tb)
    assert _same_bits(ta, dab) and _same_bits(tb, dbc), tag
    # through autograd
    a, b = ab.clone().requires_grad_(True), bc.clone().requires_grad_(True)
    o, v = P.compose_flows(a, b, ma, mb)
    assert not v.requires_grad
    o.backward(g)
    assert _same_bits(a.grad, dab) and _same_bits(b.grad, dbc), tag


@pytest.mark.parametrize("shape", [(3, 9, 15), (2, 1, 257)])
def test_an_image_alone_gives_the_bits_it_gives_in_the_batch(P, shape):
    for variant in ("none", "both"):
        ab, bc, g, ma, mb, _ = _inputs(_case(shape), variant)
        out, valid = P.compose_flows(ab, bc, ma, mb)
        dab, dbc = P.compose_grad(ab, bc, g, ma, mb)
        for n in range(shape[0]):
            one = slice(n, n + 1)
            m1, m2 = (None if m is None else m[one] for m in (ma, mb))
            o1, v1 = P.compose_flows(ab[one], bc[one], m1, m2)
            a1, b1 = P.compose_grad(ab[one], bc[one], g[one], m1, m2)
            assert _same_bits(o1, out[one]) and torch.equal(v1, valid[one]) and _same_bits(a1, dab[one]) and _same_bits(b1, dbc[one])


def test_non_finite_values_the_rule_excludes_change_no_bit(P):
    shape = (2, 23, 37)
    ab, bc, vab, vbc, g, ref = _case(shape)
    ref_valid = ref["both"][0][1]
    t = lambda a: torch.from_numpy(a).cuda()                                   # noqa: E731
    ma, mb = t(vab), t(vbc)
    out, valid = P.compose_flows(t(ab), t(bc), ma, mb)
    dab, dbc = P.compose_grad(t(ab), t(bc), t(g), ma, mb)
    ab2, bc2, g2 = ab.copy(), bc.copy(), g.copy()
    own, masked = vab == 0, vbc == 0
    assert own.sum() >= 8 and masked.sum() >= 8 and (~ref_valid).sum() >= 8
    ab2[own] = np.array([np.nan, np.inf], np.float32)                          # pixels valid_ab rules out read no flow
    bc2[masked] = np.array([-np.inf, np.nan], np.float32)                      # a masked corner's flow decides nothing
    g2[~ref_valid] = np.array([np.nan, -np.inf], np.float32)                   # g at an invalid pixel is not read
    out2, valid2 = P.compose_flows(t(ab2), t(bc2), ma, mb)
    dab2, dbc2 = P.compose_grad(t(ab2), t(bc2), t(g2), ma, mb)
    assert torch.equal(valid2, valid) and _same_bits(out2, out) and _same_bits(dab2, dab) and _same_bits(dbc2, dbc)
    assert bool(torch.isfinite(dab2).all()) and bool(torch.isfinite(dbc2).all())


def test_a_nan_gradient_poisons_its_own_image_only(P):
    shape = (2, 5, 7)
    ab, bc, g, ma, mb, (ref_fwd, _) = _inputs(_case(shape), "both")
    dab, dbc = P.compose_grad(ab, bc, g, ma, mb)
    y, x = (int(i[0]) for i in np.nonzero(ref_fwd[1][0]))                      # a valid pixel of image 0
    bad = g.clone()
    bad[0, y, x, 1] = float("nan")
    base = torch.ones_like(dbc)
    for accumulate in (False, True):
        ta, tb = base.clone(), base.clone()
        P.compose_grad(ab, bc, bad, ma, mb, dflow_ab=ta, dflow_bc=tb, accumulate=accumulate)
        assert bool(torch.isnan(tb[0]).all())                                  # a flag, not a fault: every element
        want = base[1] + dbc[1] if accumulate else dbc[1]
        assert _same_bits(tb[1], want) and bool(torch.isfinite(tb[1]).all())
        assert bool(torch.isnan(ta[0, y, x]).any())                            # plain arithmetic
        rest = torch.ones_like(ta, dtype=torch.bool)
        rest[0, y, x] = False
        want = base + dab if accumulate else dab
        assert torch.equal(ta[rest], want[rest])
    inf = g.clone()
    inf[0, y, x, 0] = float("inf")
    assert bool(torch.isnan(P.compose_grad(ab, bc, inf, ma, mb)[1][0]).all())


def test_chain_flows_is_the_explicit_fold(P):
    T, H, W = 4, 9, 15
    ab, _, vab, _, _ = R.random_case(T, H, W, seed=2105)
    flows, valids = torch.from_numpy(ab).cuda(), torch.from_numpy(vab).cuda()
    for masks in (None, valids):
        got, mask = P.chain_flows(flows, masks, span=3)
        assert tuple(got.shape) == (2, H, W, 2) and mask.dtype == torch.bool and tuple(mask.shape) == (2, H, W)
        for i in range(2):
            m = [None] * 3 if masks is None else [masks[j:j + 1] for j in range(i, i + 3)]
            acc, am = P.compose_flows(flows[i:i + 1], flows[i + 1:i + 2], m[0], m[1])
            acc, am = P.compose_flows(acc, flows[i + 2:i + 3], am, m[2])
            assert _same_bits(got[i:i + 1], acc) and torch.equal(mask[i:i + 1], am)
            lst, lm = P.chain_flows([flows[j:j + 1] for j in range(i, i + 3)], None if masks is None else m)
            assert _same_bits(lst, acc) and torch.equal(lm, am)
            want, want_mask = R.chain([ab[j:j + 1] for j in range(i, i + 3)], None if masks is None else [vab[j:j + 1] for j in range(i, i + 3)])
            assert 0.05 <= float(want_mask.mean()) <= 0.95
            # the restatement rounds each step to float32 as the kernel does: the masks agree but at a near tie of a floor
            assert float((am.cpu().numpy() != want_mask).mean()) <= 0.02
    # differentiable with respect to every flow of the chain
    f = flows.clone().requires_grad_(True)
    out, mask = P.chain_flows(f, span=3)
    out[mask].sum().backward()
    assert bool(torch.isfinite(f.grad).all()) and bool((f.grad[0] != 0).any()) and bool((f.grad[3] != 0).any())


def test_infer_continuous_chain_cli(P, tmp_path):
    """The CLI in a fresh child process: four 64 x 64 frames, un-learned weights, --chain 2 --batch 2 (the chain of frame 1
    crosses the batch boundary).  Each _plus2.flo is compose_flows of the two consecutive .flo files, bit for bit."""
    from PIL import Image
    from pwcnet_amd import flow_io
    rng = np.random.RandomState(3)
    base = rng.uniform(0, 255, size=(64, 64, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(4):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o"), "--chain", "2", "--batch", "2"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    out = tmp_path / "o" / "seq"
    flo = [torch.from_numpy(flow_io.read_flo(str(out / f"frame_{i:02d}.flo")).astype(np.float32))[None].cuda() for i in range(3)]
    for i in range(2):
        got = torch.from_numpy(flow_io.read_flo(str(out / f"frame_{i:02d}_plus2.flo")).astype(np.float32))[None].cuda()
        want, _ = P.compose_flows(flo[i], flo[i + 1])
        assert tuple(got.shape) == (1, 64, 64, 2) and _same_bits(got, want), i
    assert sorted(p.name for p in out.glob("*_plus*")) == ["frame_00_plus2.flo", "frame_01_plus2.flo"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "plain"), "--batch", "2"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert not list((tmp_path / "plain" / "seq").glob("*_plus*")) and len(list((tmp_path / "plain" / "seq").glob("*.flo"))) == 3
    for i in range(3):                                                         # and the flag changes nothing else
        assert (tmp_path / "plain" / "seq" / f"frame_{i:02d}.flo").read_bytes() == (out / f"frame_{i:02d}.flo").read_bytes()
