"""GPU tests of second-order smoothness (csrc/pwc_unsup.hip) and the forward-backward consistency term (csrc/pwc_fbcheck.hip)
through pwcnet_amd/unsup.py, against the float64 restatements of tests/unflow_ref.py (validated on the CPU by
tests/test_host_unflow.py) on its cases: N = 2 at 23 x 37 (odd sizes, tail lanes) and 272 x 256 (more than 256 parts per image: the
grid-stride loop and the capped partition), wide-stride views, flow_scale in {1, 5}, (eps, q) in {(1e-3, 0.5), (1e-2, 0.45)}, ~70 %
masks with NaN behind them, an image that is out of frame everywhere, and a case whose every forward pixel points into one cell.

Bounds, those of tests/test_gpu_unsup.py.  Counts: exact.  Sums: 1e-5 of the largest reference sum.  Gradients: max-abs error
over the largest reference element, at most max(4 x the error of the SAME formulas run in float32 torch ops on the same inputs,
2e-5).  Bit reproducibility, the accumulate semantics and the exact zeros are torch.equal.  Every test prints its figures before
it asserts.  Measured on an MI355X (profiles/unflow_gpu_test_figures.txt): second-order sums 1.0e-8 ... 4.4e-7 off, gradients
8.8e-8 ... 2.0e-7 (float32 torch 1.6e-7 ... 1.0e-5); consistency sums 1.3e-8 ... 2.5e-7, counts equal, gradients with respect to
both flows 7.5e-8 ... 1.8e-7 (float32 torch 5.9e-6 ... 3.8e-3); the contention case's corners 1.5e-7."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fb_ref as fr
from tests import unflow_ref as uf
from tests import unsup_ref as ur
from tests.test_gpu_grad import _rel_err, close, gpu
from tests.test_gpu_grad_ops import _wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH_NAMES = sorted(uf.SMOOTH_CASES)
NAMES = sorted(uf.CASES)


@pytest.fixture(scope="module")
def us():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import unsup
    return unsup


def _grad_bound(err32):
    return max(4.0 * err32, 2e-5)


def _t(values):
    return torch.tensor(values, dtype=torch.float32, device="cuda")


def _base(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, shape).astype(np.float32)).cuda()


# ------------------------------------------------------------------ second-order smoothness
def _smooth_inputs(case):
    C = case["C"]
    im0 = _wide(gpu(case["im0"]), C + 3, 2)[0][..., 2:2 + C]
    flow = _wide(gpu(case["flow"]), 6, 3)[0][..., 3:5]
    return im0, flow


@pytest.mark.parametrize("name", SMOOTH_NAMES)
def test_second_order_sums_and_gradient_vs_float64(us, name):
    ref = uf.smooth_reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    im0, flow = _smooth_inputs(case)
    up = _t(ur.UPSTREAM)
    for key, image in (("smooth", im0), ("smooth_noimg", None)):
        (s64, g64), (s32, g32) = ref[key + "64"], ref[key + "32"]
        outs = []
        for _ in range(2):
            fl = flow.detach().requires_grad_(True)
            sums = us.smoothness_sums(fl, image, uf.ALPHA, eps, q, order=2)
            (sums * up).sum().backward()
            outs.append((sums.detach(), fl.grad))
        torch.cuda.synchronize()
        (sums, grad), err32 = outs[0], _rel_err(g32, g64)
        err = _rel_err(grad, g64)
        print(f"{name} {key} order 2: sums {sums.tolist()} ref {s64.tolist()} rel err {_rel_err(sums, s64):.3e} (float32 torch "
              f"{_rel_err(s32, s64):.3e}); gradient rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}, "
              f"max |ref| {float(g64.abs().max()):.3e}")
        close(sums, s64, rel=1e-5)
        assert bool(torch.isfinite(grad).all()) and err <= _grad_bound(err32)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        loss = us.smoothness_loss(flow, image, uf.ALPHA, eps, q, order=2)
        want = float(s64.sum()) / (case["N"] * case["H"] * case["W"])
        assert loss.dim() == 0 and abs(float(loss) - want) <= 1e-5 * want
        base = _base(tuple(flow.shape[:3]) + (4,), 8)
        buf = base.clone()
        us.smoothness_grad(flow, up, buf[..., 2:4], image, uf.ALPHA, eps, q, accumulate=True, order=2)
        assert torch.equal(buf[..., 2:4], base[..., 2:4] + grad) and torch.equal(buf[..., :2], base[..., :2])
        buf = base.clone()
        us.smoothness_grad(flow, up, buf[..., 2:4], image, uf.ALPHA, eps, q, order=2)
        assert torch.equal(buf[..., 2:4], grad) and torch.equal(buf[..., :2], base[..., :2])


@pytest.mark.parametrize("name", ["23x37_c3_s1", "272x256_c4_s5"])
def test_second_order_without_an_image_is_a_constant_image(us, name):
    ref = uf.smooth_reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    flow = gpu(case["flow"])
    const = torch.full((case["N"], case["H"], case["W"], case["C"]), 0.375, device="cuda")
    res = []
    for image in (None, const):
        fl = flow.detach().requires_grad_(True)
        sums = us.smoothness_sums(fl, image, uf.ALPHA, eps, q, order=2)
        sums.sum().backward()
        res.append((sums.detach(), fl.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("H,W", [(1, 37), (2, 5), (3, 3)])
def test_second_order_on_frames_with_an_axis_below_three(us, H, W):
    """1 x 37: the x terms only; 2 x 5: the x terms of both rows (the y axis' share is 0); 3 x 3: one centre row and one centre
    column.  A crop with no centre on either axis gives exactly 0."""
    N, eps, q = 2, 1e-3, 0.5
    rs = np.random.RandomState(100 * H + W)
    fl_np = rs.uniform(-2, 2, (N, H, W, 2)).astype(np.float32)
    im_np = rs.uniform(0, 1, (N, H, W, 3)).astype(np.float32)
    runs = {}
    for dt in (torch.float64, torch.float32):
        fl = torch.from_numpy(fl_np).to(dt).requires_grad_(True)
        sums = uf.smoothness2_ref(fl, torch.from_numpy(im_np).to(dt), uf.ALPHA, eps, q)
        (sums * torch.tensor(ur.UPSTREAM, dtype=dt)).sum().backward()
        runs[dt] = (sums.detach(), fl.grad)
    (s64, g64), (_, g32) = runs[torch.float64], runs[torch.float32]
    # the surviving axis only: the same rows / columns taken alone give the same sum
    if H < 3:
        rows = sum(uf.smoothness2_ref(torch.from_numpy(fl_np[:, y:y + 1]).double(), torch.from_numpy(im_np[:, y:y + 1]).double(),
                                      uf.ALPHA, eps, q) for y in range(H))
        assert torch.allclose(rows, s64, rtol=1e-12)
    flow = _wide(gpu(fl_np), 5, 2)[0][..., 2:4].detach().requires_grad_(True)
    sums = us.smoothness_sums(flow, gpu(im_np), uf.ALPHA, eps, q, order=2)
    (sums * _t(ur.UPSTREAM)).sum().backward()
    torch.cuda.synchronize()
    err, err32 = _rel_err(flow.grad, g64), _rel_err(g32, g64)
    print(f"{H}x{W} order 2: sums {sums.tolist()} ref {s64.tolist()}; gradient rel err HIP {err:.3e}, float32 torch {err32:.3e}, "
          f"bound {_grad_bound(err32):.3e}")
    close(sums, s64, rel=1e-5)
    assert bool(torch.isfinite(flow.grad).all()) and err <= _grad_bound(err32)
    # no centre on either axis: 0, and a zero gradient
    tiny = torch.from_numpy(fl_np[:, :min(H, 2), :2].copy()).cuda().requires_grad_(True)
    s0 = us.smoothness_sums(tiny, order=2)
    s0.sum().backward()
    assert s0.tolist() == [0.0] * N and not bool(tiny.grad.any())


def test_order_one_is_the_call_without_the_keyword(us):
    ref = uf.smooth_reference("23x37_c3_s1")
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    im0, flow = _smooth_inputs(case)
    res = []
    for kw in ({}, {"order": 1}):
        fl = flow.detach().requires_grad_(True)
        sums = us.smoothness_sums(fl, im0, uf.ALPHA, eps, q, **kw)
        (sums * _t(ur.UPSTREAM)).sum().backward()
        res.append((sums.detach(), fl.grad, us.smoothness_loss(flow, im0, uf.ALPHA, eps, q, **kw),
                    us.smoothness_grad(flow, _t(ur.UPSTREAM), None, im0, uf.ALPHA, eps, q, **kw)))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    s2 = us.smoothness_sums(flow, im0, uf.ALPHA, eps, q, order=2)
    assert not torch.equal(s2, res[0][0])


# ------------------------------------------------------------------ consistency term
def _inputs(case, poisoned=True):
    """The case on the GPU: the flows as channel slices of wider buffers (`_wide`), NaN behind the masks, and the masks."""
    k = "_nan" if poisoned else ""
    fw = _wide(gpu(case["fw" + k]), 6, 3)[0][..., 3:5]
    bw = _wide(gpu(case["bw" + k]), 3, 1)[0][..., 1:3]
    vf = None if case["valid_fw"] is None else torch.from_numpy(case["valid_fw"]).cuda()
    vb = None if case["valid_bw"] is None else torch.from_numpy(case["valid_bw"]).cuda()
    return fw, bw, vf, vb


def _consistency_grads(us, case, eps, q, fw, bw, vf, vb):
    a, b = fw.detach().requires_grad_(True), bw.detach().requires_grad_(True)
    s_fw, c_fw, s_bw, c_bw = us.fb_consistency_sums(a, b, case["flow_scale"], vf, vb, eps, q)
    ((s_fw * _t(uf.UPSTREAM[0])).sum() + (s_bw * _t(uf.UPSTREAM[1])).sum()).backward()
    return s_fw.detach(), c_fw, s_bw.detach(), c_bw, a.grad, b.grad


@pytest.mark.parametrize("name", NAMES)
def test_consistency_sums_and_counts_vs_float64(us, name):
    ref = uf.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    s_a, c_a, _, s_b, c_b, _, _, _ = ref["run64"]
    fw, bw, vf, vb = _inputs(case)
    out = us.fb_consistency_sums(fw, bw, case["flow_scale"], vf, vb, eps, q)
    again = us.fb_consistency_sums(fw, bw, case["flow_scale"], vf, vb, eps, q)
    torch.cuda.synchronize()
    s_fw, c_fw, s_bw, c_bw = out
    top = max(float(s_a.max()), float(s_b.max()))
    e_fw, e_bw = float((s_fw.cpu().double() - s_a).abs().max()) / top, float((s_bw.cpu().double() - s_b).abs().max()) / top
    print(f"{name}: sums fw {s_fw.tolist()} ref {s_a.tolist()}, bw {s_bw.tolist()} ref {s_b.tolist()}; counts fw {c_fw.tolist()} "
          f"ref {c_a.tolist()}, bw {c_bw.tolist()} ref {c_b.tolist()}; err over the largest sum fw {e_fw:.3e} bw {e_bw:.3e} "
          f"(float32 torch {_rel_err(ref['run32'][0], s_a):.3e} / {_rel_err(ref['run32'][3], s_b):.3e})")
    assert c_fw.dtype == torch.int32 and c_bw.dtype == torch.int32 and not c_fw.requires_grad
    assert c_fw.cpu().tolist() == c_a.tolist() and c_bw.cpu().tolist() == c_b.tolist()
    assert bool(torch.isfinite(s_fw).all()) and bool(torch.isfinite(s_bw).all())
    assert e_fw <= 1e-5 and e_bw <= 1e-5
    for x, y in zip(out, again):
        assert torch.equal(x, y)
    if vf is not None:                          # a uint8 mask with other non-zero values is the same mask
        m8 = us.fb_consistency_sums(fw, bw, case["flow_scale"], vf.to(torch.uint8) * 7, vb.to(torch.uint8) * 7, eps, q)
        for x, y in zip(out, m8):
            assert torch.equal(x, y)
    if case["empty"] is not None:
        e = case["empty"]
        assert float(s_fw[e]) == 0.0 and float(s_bw[e]) == 0.0 and int(c_fw[e]) == 0 and int(c_bw[e]) == 0
    loss = us.fb_consistency_loss(fw, bw, case["flow_scale"], vf, vb, eps, q)
    want = uf.consistency_loss_ref(s_a, c_a, s_b, c_b)
    assert loss.dim() == 0 and abs(float(loss) - want) <= 1e-5 * want


@pytest.mark.parametrize("name", NAMES)
def test_consistency_gradients_vs_float64_autograd(us, name):
    ref = uf.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    g64, g32 = ref["run64"][6:], ref["run32"][6:]
    fw, bw, vf, vb = _inputs(case)
    runs = [_consistency_grads(us, case, eps, q, fw, bw, vf, vb) for _ in range(2)]
    torch.cuda.synchronize()
    grads = runs[0][4:]
    for what, g, r64, r32 in zip(("d/dflows_fw", "d/dflows_bw"), grads, g64, g32):
        err, err32 = _rel_err(g, r64), _rel_err(r32, r64)
        print(f"{name} {what}: rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}, "
              f"max |ref| {float(r64.abs().max()):.3e}")
    for g, r64, r32 in zip(grads, g64, g32):
        assert g.shape == r64.shape and bool(torch.isfinite(g).all())
        assert _rel_err(g, r64) <= _grad_bound(_rel_err(r32, r64))
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(x, y)
    # exact 0 where neither the pixel's own direction nor a corner read of the other direction reaches
    in_a, in_b = ref["run64"][2].numpy(), ref["run64"][5].numpy()
    s = np.float64(np.float32(case["flow_scale"]))
    quiet_fw = ~in_a & ~fr._sampled(s * case["bw"].astype(np.float64), in_b)
    quiet_bw = ~in_b & ~fr._sampled(s * case["fw"].astype(np.float64), in_a)
    print(f"{name}: pixels nothing reaches fw {int(quiet_fw.sum())} bw {int(quiet_bw.sum())} of {quiet_fw.size}")
    if vf is not None:
        assert quiet_fw.any() and quiet_bw.any()
    assert not bool(grads[0][torch.from_numpy(quiet_fw).cuda()].any()) and not bool(grads[1][torch.from_numpy(quiet_bw).cuda()].any())
    if case["empty"] is not None:
        assert not bool(grads[0][case["empty"]].any()) and not bool(grads[1][case["empty"]].any())
    # accumulate: added onto pre-filled wide buffers, the other channels untouched; without it: every pixel written
    N, H, W = case["N"], case["H"], case["W"]
    base_fw, base_bw = _base((N, H, W, 5), 9), _base((N, H, W, 4), 10)
    ups = (_t(uf.UPSTREAM[0]), _t(uf.UPSTREAM[1]))
    buf_fw, buf_bw = base_fw.clone(), base_bw.clone()
    us.fb_consistency_grad(fw, bw, *ups, buf_fw[..., 1:3], buf_bw[..., 2:4], case["flow_scale"], vf, vb, eps, q, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(buf_fw[..., 1:3], base_fw[..., 1:3] + grads[0]) and torch.equal(buf_bw[..., 2:4], base_bw[..., 2:4] + grads[1])
    assert torch.equal(buf_fw[..., :1], base_fw[..., :1]) and torch.equal(buf_fw[..., 3:], base_fw[..., 3:])
    assert torch.equal(buf_bw[..., :2], base_bw[..., :2])
    buf_fw, buf_bw = base_fw.clone(), base_bw.clone()
    d_fw, d_bw = us.fb_consistency_grad(fw, bw, *ups, buf_fw[..., 1:3], buf_bw[..., 2:4], case["flow_scale"], vf, vb, eps, q)
    torch.cuda.synchronize()
    assert torch.equal(d_fw, grads[0]) and torch.equal(d_bw, grads[1])
    assert torch.equal(buf_fw[..., 1:3], grads[0]) and torch.equal(buf_bw[..., 2:4], grads[1])
    assert torch.equal(buf_fw[..., 3:], base_fw[..., 3:]) and torch.equal(buf_bw[..., :2], base_bw[..., :2])
    if vf is not None:
        m8 = _consistency_grads(us, case, eps, q, fw, bw, vf.to(torch.uint8) * 7, vb.to(torch.uint8) * 7)
        assert torch.equal(m8[4], grads[0]) and torch.equal(m8[5], grads[1])


def test_contention_every_forward_pixel_scatters_onto_one_cell(us):
    """23 x 37, N = 2: all 851 forward pixels of an image add into the same four corners (8 accumulators) of d/dflows_bw -- the
    test of the fixed-point scatter: held against float64 at the gradient bound, five calls give the same bits."""
    ref = uf.reference(uf.CONTENTION)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    g64, g32 = ref["run64"][6:], ref["run32"][6:]
    fw, bw, vf, vb = _inputs(case)
    runs = [_consistency_grads(us, case, eps, q, fw, bw, vf, vb) for _ in range(5)]
    torch.cuda.synchronize()
    x0, y0 = int(uf.CELL[0]), int(uf.CELL[1])
    assert runs[0][1].tolist() == [case["H"] * case["W"]] * case["N"]
    for what, g, r64, r32 in zip(("d/dflows_fw", "d/dflows_bw"), runs[0][4:], g64, g32):
        print(f"contention {what}: rel err HIP {_rel_err(g, r64):.3e}, float32 torch {_rel_err(r32, r64):.3e}, "
              f"bound {_grad_bound(_rel_err(r32, r64)):.3e}, max |ref| {float(r64.abs().max()):.3e}")
    corner, c64, c32 = (g[:, y0:y0 + 2, x0:x0 + 2] for g in (runs[0][5], g64[1], g32[1]))
    err, err32 = _rel_err(corner, c64), _rel_err(c32, c64)
    print(f"contention, the four corners of d/dflows_bw: {corner.flatten().tolist()} ref {c64.flatten().tolist()}; rel err HIP "
          f"{err:.3e}, float32 torch {err32:.3e}")
    for g, r64, r32 in zip(runs[0][4:], g64, g32):
        assert bool(torch.isfinite(g).all()) and _rel_err(g, r64) <= _grad_bound(_rel_err(r32, r64))
    assert err <= _grad_bound(_rel_err(g32[1], g64[1]))
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert torch.equal(x, y)


def test_a_non_finite_upstream_poisons_the_flow_it_scatters_onto(us):
    """6 x 7.  dsums_fw scales what the forward pixels scatter onto d/dflows_bw: with dsums_fw[0] = inf EVERY element of
    d/dflows_bw is NaN -- image 1 too, and although image 0 is out of frame everywhere (0 * inf must not come out finite) --
    while d/dflows_fw, whose scatter part hangs on the finite dsums_bw and whose image 0 contributes nothing, is finite.  With
    the inf on the image that contributes, d/dflows_fw carries it where its own pixels contribute.  The next call is clean."""
    eps, q = 1e-3, 0.5
    case = uf.build_case(2, 6, 7, flow_scale=1.0, seed=21, masked=False, empty=0, block=2, max_off=1, noise=0.3)
    fw, bw, vf, vb = _inputs(case)
    clean = us.fb_consistency_grad(fw, bw, _t(uf.UPSTREAM[0]), _t(uf.UPSTREAM[1]), None, None, 1.0, vf, vb, eps, q)
    d_fw, d_bw = us.fb_consistency_grad(fw, bw, _t([float("inf"), uf.UPSTREAM[0][1]]), _t(uf.UPSTREAM[1]), None, None, 1.0, vf, vb,
                                        eps, q)
    torch.cuda.synchronize()
    print(f"dsums_fw[0] = inf: NaN in d/dflows_bw {int(torch.isnan(d_bw).sum())} of {d_bw.numel()}, non-finite in d/dflows_fw "
          f"{int((~torch.isfinite(d_fw)).sum())}")
    assert bool(torch.isnan(d_bw).all())
    assert bool(torch.isfinite(d_fw).all()) and torch.equal(d_fw, clean[0])
    d_fw, d_bw = us.fb_consistency_grad(fw, bw, _t([uf.UPSTREAM[0][0], float("inf")]), _t(uf.UPSTREAM[1]), None, None, 1.0, vf, vb,
                                        eps, q)
    torch.cuda.synchronize()
    print(f"dsums_fw[1] = inf: NaN in d/dflows_bw {int(torch.isnan(d_bw).sum())} of {d_bw.numel()}, non-finite in d/dflows_fw "
          f"{int((~torch.isfinite(d_fw)).sum())} (image 0: {int((~torch.isfinite(d_fw[0])).sum())})")
    assert bool(torch.isnan(d_bw).all())
    assert bool(torch.isfinite(d_fw[0]).all()) and not bool(torch.isfinite(d_fw[1]).all())
    again = us.fb_consistency_grad(fw, bw, _t(uf.UPSTREAM[0]), _t(uf.UPSTREAM[1]), None, None, 1.0, vf, vb, eps, q)
    assert torch.equal(again[0], clean[0]) and torch.equal(again[1], clean[1]) and bool(torch.isfinite(again[1]).all())


@pytest.mark.parametrize("name", ["23x37_s1_a", "272x256_s5_a"])
def test_c_entries_write_inside_their_outputs_and_workspaces(us, name):
    """Through ctypes: sums, counts, both dflows and both workspaces -- each exactly the reported size -- lie between guard bands
    of sentinels that are intact afterwards."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    ref = uf.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    N, H, W = case["N"], case["H"], case["W"]
    fw, bw, vf, vb = _inputs(case)
    want = _consistency_grads(us, case, eps, q, fw, bw, vf, vb)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    G = 64

    def fenced(n, dtype, sentinel):
        return torch.full((G + n + G,), sentinel, dtype=dtype, device="cuda")

    def intact(buf, n, sentinel):
        return bool((buf[:G] == sentinel).all()) and bool((buf[G + n:] == sentinel).all())

    nws = L.pwc_fb_consistency_workspace_floats(N, H, W)
    ws = fenced(nws, torch.float32, -7.0)
    sums = [fenced(N, torch.float32, -7.0) for _ in range(2)]
    counts = [fenced(N, torch.int32, -7) for _ in range(2)]
    args = (p(fw), fw.stride(2), p(bw), bw.stride(2), case["flow_scale"], p(vf), p(vb), N, H, W, eps, q)
    rc = L.pwc_fb_consistency_sums_f32(*args, p(ws[G:]), nws, p(sums[0][G:]), p(counts[0][G:]), p(sums[1][G:]), p(counts[1][G:]),
                                       _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert intact(ws, nws, -7.0)
    for buf, cnt, s, c in zip(sums, counts, (want[0], want[2]), (want[1], want[3])):
        assert intact(buf, N, -7.0) and intact(cnt, N, -7)
        assert torch.equal(buf[G:G + N], s) and torch.equal(cnt[G:G + N], c)

    nbytes = L.pwc_fb_consistency_grad_workspace_bytes(N, H, W)
    assert nbytes % 8 == 0
    gws = fenced(nbytes // 8, torch.int64, -7)
    dflows = [fenced(N * H * W * 2, torch.float32, -7.0) for _ in range(2)]
    ups = (_t(uf.UPSTREAM[0]), _t(uf.UPSTREAM[1]))
    rc = L.pwc_fb_consistency_grad_f32(*args, p(ups[0]), p(ups[1]), p(gws[G:]), nbytes, p(dflows[0][G:]), 2, p(dflows[1][G:]), 2, 0,
                                       _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert intact(gws, nbytes // 8, -7)
    for buf, g in zip(dflows, want[4:]):
        assert intact(buf, N * H * W * 2, -7.0)
        assert torch.equal(buf[G:G + N * H * W * 2].view(N, H, W, 2), g)


# ------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", ["23x37_s1_a", "272x256_s5_a"])
def test_fb_valid_masks_feed_the_consistency_loss(us, name):
    """fb_valid's masks go in as returned; the loss equals the float64 restatement run with the same masks."""
    ref = uf.reference(name)
    case, eps, q = ref["case"], ref["eps"], ref["q"]
    fw, bw, vf, vb = _inputs(case, poisoned=False)
    m_fw, m_bw = us.fb_valid(fw, bw, case["flow_scale"], 0.01, 0.5, vf, vb)
    a, b = fw.detach().requires_grad_(True), bw.detach().requires_grad_(True)
    loss = us.fb_consistency_loss(a, b, case["flow_scale"], m_fw, m_bw, eps, q)
    loss.backward()
    torch.cuda.synchronize()
    out = uf.fb_consistency_ref(torch.from_numpy(case["fw"]).double(), torch.from_numpy(case["bw"]).double(), case["flow_scale"],
                                m_fw.cpu(), m_bw.cpu(), eps, q)
    want = uf.consistency_loss_ref(out[0], out[1], out[3], out[4])
    got = float(loss.detach())
    print(f"{name}: consistency loss under fb_valid's masks {got:.8f} ref {want:.8f} rel err "
          f"{abs(got - want) / want:.3e}, contributing {int(out[1].sum())} + {int(out[4].sum())} of {2 * m_fw.numel()}")
    assert int(out[1].sum()) > 0 and int(out[4].sum()) > 0 and abs(got - want) <= 1e-5 * want
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all()) and bool(a.grad.any()) and bool(b.grad.any())


def test_unflow_loss_trains_the_module_bit_reproducibly(us):
    """One PWCDCNetModule step at 64 x 128 on the pair in both orders (batch 2): census under fb_valid's masks + second-order
    smoothness + the consistency term; twice from the same state."""
    from pwcnet_amd import PWCDCNetModule
    from tests import util
    im0, im1 = (gpu(a) for a in util.smooth_images(1, 64, 128))
    runs = []
    for _ in range(2):
        model = PWCDCNetModule(seed=3)
        final, _ = model(torch.cat([im0, im1]), torch.cat([im1, im0]))
        fw, bw = final[:1], final[1:]
        with torch.no_grad():
            m_fw, m_bw = us.fb_valid(fw.detach(), bw.detach())
        photo = 0.5 * (us.census_loss(im0, im1, fw, valid=m_fw, radius=1) + us.census_loss(im1, im0, bw, valid=m_bw, radius=1))
        smooth = 0.5 * (us.smoothness_loss(fw, im0, order=2) + us.smoothness_loss(bw, im1, order=2))
        cons = us.fb_consistency_loss(fw, bw, valid_fw=m_fw, valid_bw=m_bw)
        loss = photo + 0.1 * smooth + 0.2 * cons
        loss.backward()
        runs.append((loss.detach().clone(), model.flat.grad.clone(), cons.detach().clone()))
    torch.cuda.synchronize()
    (loss, grad, cons), (loss2, grad2, cons2) = runs
    print(f"loss {float(loss):.6f} (consistency {float(cons):.6f}), |grad| max {float(grad.abs().max()):.3e}, non-zero "
          f"{int((grad != 0).sum())} of {grad.numel()}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(cons, cons2)


def _train(tmp_path, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                           "64", "128", "--synthetic_pairs", "4", "--loss", "unsup", "--occlusion", "fb", *flags,
                           "--model_dir", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_train_cli_second_order_and_consistency(tmp_path):
    out = _train(tmp_path, "--smooth_order", "2", "--consistency_weight", "0.2")
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    steps = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 1, steps                       # 4 pairs: 1 for validation, 3 to train on, batch 2, drop_last
    for ln in steps:
        assert "  occluded " in ln and "  consistency " in ln, ln
        value = float(ln.split("  consistency ")[1].split()[0])
        assert np.isfinite(value) and value > 0, ln
        assert np.isfinite(float(ln.split("loss/unsup")[1].split()[0])), ln


def test_train_cli_defaults_print_no_consistency(tmp_path):
    out = _train(tmp_path)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    steps = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 1 and all("consistency" not in ln for ln in steps), steps
    assert steps[0].rstrip().split()[-2] == "occluded", steps
