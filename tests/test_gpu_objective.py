"""GPU tests of the label-free objective (pwcnet_amd/objective.py: what train.py --loss unsup trains) against the float64
restatement of tests/objective_ref.py (validated on the CPU by tests/test_host_objective.py), and of the single loss kernels at the
geometry --level_weights launches them at: the levels of (2, 64, 128, 3) frames (1 x 2, 2 x 4, 4 x 8, 8 x 16, 16 x 32) and of
(1, 128, 192, 3) frames (2 x 3, 4 x 6, 8 x 12, 16 x 24, 32 x 48: odd coarse widths, N = 1, a level as wide as one 32-pixel tile),
flow scales 0.3125 .. 5, flows that are batch slices of a stacked 2N tensor, windows that barely fit or do not fit.

Bounds, all the project's.  Counts: exact.  Sums: 1e-5 of the largest reference sum (`close`).  Every term and per-level value
of the objective: |got - ref| <= 1e-5 ref; the loss: 2e-5 ref (a positively weighted sum of non-negative terms, each within 1e-5,
formed with fewer than twenty float32 operations of 6e-8 each).  Gradients, per flow tensor: max |got - ref64| / max |ref64| <=
max(4 x the same figure of the restatement run in float32, 2e-5) -- tests/test_gpu_unsup.py's _grad_bound -- and exactly 0 where
the reference gradient is exactly 0 (autograd through torch.where: the pixels no term reads).  Every test prints its figures
before it asserts; profiles/objective_gpu_test_figures.txt holds them."""
import math

import numpy as np
import pytest
import torch

from tests import census_ref as cr
from tests import objective_ref as orf
from tests import ssim_ref as sm
from tests import unflow_ref as uf
from tests import unsup_ref as ur
from tests.test_gpu_grad import _rel_err, close

pytestmark = pytest.mark.gpu
UPSTREAM = {1: (0.75,), 2: ur.UPSTREAM}
LEVELS = [(name, l) for name in orf.FRAMES for l in range(5)]


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    return pwcnet_amd


def _grad_bound(err32):
    return max(4.0 * err32, 2e-5)


def _check_grad(tag, got, g64, g32):
    """The gradient check of one flow tensor; got None (autograd reached nothing) counts as zeros."""
    got = torch.zeros_like(g64, dtype=torch.float32) if got is None else got.detach().cpu()
    assert got.shape == g64.shape and bool(torch.isfinite(got).all()), tag
    quiet = (g64 == 0).all(dim=3)
    assert not bool(got[quiet].any()), f"{tag}: a pixel no term of the reference reads has a gradient"
    top = float(g64.abs().max())
    if top == 0.0:
        print(f"{tag}: nothing reaches this flow; gradient exactly zero")
        return
    err, err32 = _rel_err(got, g64), _rel_err(g32, g64)
    print(f"{tag}: gradient rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}, max |ref| {top:.3e}, "
          f"quiet pixels {int(quiet.sum())}")
    assert err <= _grad_bound(err32), tag


# ------------------------------------------------------------------ C1: term by term at level geometry
@pytest.fixture(scope="module")
def level_inputs(pa):
    """Per frames: the level frames (frame_pyramid of both frames), the pooled masks of two seeded ~80 % masks (mask_pyramid,
    min_fraction 0.5), the level flows of both directions -- computed once, read-only."""
    out = {}
    for name, (N, H, W, C) in orf.FRAMES.items():
        im0, im1 = (t.cuda() for t in orf.frames(name))
        rs = np.random.RandomState(5 + N)
        full = [torch.from_numpy(rs.uniform(size=(N, H, W)) < 0.8).cuda() for _ in range(2)]
        out[name] = dict(pyr=(pa.frame_pyramid(im0, orf.FACTORS), pa.frame_pyramid(im1, orf.FACTORS)),
                         masks=[pa.mask_pyramid(m, orf.FACTORS, min_fraction=0.5) for m in full],
                         flows=orf.flows(name, True)[1])
    return out


def _ref_term(ref, A, B, flow, scale, M, up, dt, **kw):
    fl = flow.to(dt).clone().requires_grad_(True)
    sums, counts, _ = ref(A.to(dt), B.to(dt), fl, scale, M, **kw)
    (sums * torch.tensor(up, dtype=dt)).sum().backward()
    return sums.detach(), counts, torch.zeros_like(fl) if fl.grad is None else fl.grad


def _ref_smooth(order, flow, A, up, dt):
    fl = flow.to(dt).clone().requires_grad_(True)
    ref = ur.smoothness_ref if order == 1 else uf.smoothness2_ref
    sums = ref(fl, None if A is None else A.to(dt), ur.ALPHA, 1e-3, 0.5)
    if sums.requires_grad:                      # order 2 on a level with neither three rows nor three columns: no term at all
        (sums * torch.tensor(up, dtype=dt)).sum().backward()
    return sums.detach(), torch.zeros_like(fl) if fl.grad is None else fl.grad


@pytest.mark.parametrize("name,l", LEVELS)
def test_terms_at_level_geometry_vs_float64(pa, level_inputs, name, l):
    """photometric_sums, census_sums r = 1, 2, 3, ssim_sums r = 1, 2 and smoothness_sums order 1, 2 with and without an image, at
    one level: the flow once dense and once as the batch slice of the stacked 2N tensor (the same bits), against float64."""
    N, H, W, C = orf.FRAMES[name]
    inp = level_inputs[name]
    h, w = orf.level_shapes(name)[l]
    scale = pa.level_flow_scale(inp["flows"][l], (H, W))
    assert scale == orf.level_scale(w, W)
    up = UPSTREAM[N]
    up_gpu = torch.tensor(up, dtype=torch.float32, device="cuda")
    stacked = inp["flows"][l].cuda()
    data_terms = [("photometric", pa.photometric_sums, ur.photometric_ref, dict(eps=1e-3, q=0.5), 0)]
    data_terms += [(f"census r{r}", pa.census_sums, cr.census_ref, dict(radius=r), r) for r in (1, 2, 3)]
    data_terms += [(f"ssim r{r}", pa.ssim_sums, sm.ssim_ref, dict(radius=r), r) for r in (1, 2)]
    for d in range(2):
        A, B = (inp["pyr"][d][l], inp["pyr"][1 - d][l])
        M = inp["masks"][d][l]
        part = stacked[d * N:(d + 1) * N]
        assert part.storage_offset() == d * N * h * w * 2
        flow_cpu = inp["flows"][l][d * N:(d + 1) * N]
        for tag, fn, ref, kw, r in data_terms:
            tag = f"{name} level {l} ({h} x {w}, scale {scale}) direction {d} {tag}"
            runs = []
            for sliced in (False, True):                             # dense, then the slice (a view with a storage offset)
                leaf = (stacked if sliced else part).detach().clone().requires_grad_(True)
                sums, counts = fn(A, B, leaf[d * N:(d + 1) * N] if sliced else leaf, scale, M, **kw)
                (sums * up_gpu).sum().backward()
                if sliced:                                           # nothing leaks into the other half of the stacked tensor
                    assert not bool(leaf.grad[(1 - d) * N:(2 - d) * N].any()), tag
                runs.append((sums.detach(), counts, leaf.grad[d * N:(d + 1) * N] if sliced else leaf.grad))
            (sums, counts, grad), (sums_v, counts_v, grad_v) = runs
            assert torch.equal(sums, sums_v) and torch.equal(counts, counts_v) and torch.equal(grad, grad_v), tag
            s64, c64, g64 = _ref_term(ref, A.cpu(), B.cpu(), flow_cpu, scale, M.cpu(), up, torch.float64, **kw)
            _, _, g32 = _ref_term(ref, A.cpu(), B.cpu(), flow_cpu, scale, M.cpu(), up, torch.float32, **kw)
            print(f"{tag}: sums {sums.tolist()} ref {s64.tolist()} counts {counts.tolist()} ref {c64.tolist()}")
            assert counts.cpu().tolist() == c64.tolist(), tag
            close(sums, s64, rel=1e-5)
            if r and (h <= 2 * r or w <= 2 * r):                     # the window does not fit: everything exactly zero, no error
                assert not bool(sums.any()) and not bool(counts.any()) and not bool(grad.any()), tag
                assert not bool(c64.any()) and not bool(g64.any())
            _check_grad(tag, grad, g64, g32)
        for order in (1, 2):
            for image in (A, None):
                tag = f"{name} level {l} ({h} x {w}) direction {d} smoothness order {order} {'image' if image is not None else 'no image'}"
                # as the objective launches it: the flow in level pixels, scale * the slice
                runs = []
                for sliced in (False, True):
                    leaf = (stacked if sliced else part).detach().clone().requires_grad_(True)
                    arg = scale * (leaf[d * N:(d + 1) * N] if sliced else leaf)
                    sums = pa.smoothness_sums(arg, image, ur.ALPHA, 1e-3, 0.5, order)
                    (sums * up_gpu).sum().backward()
                    runs.append((sums.detach(), leaf.grad[d * N:(d + 1) * N] if sliced else leaf.grad))
                (sums, grad), (sums_v, grad_v) = runs
                assert torch.equal(sums, sums_v) and torch.equal(grad, grad_v), tag
                img_cpu = None if image is None else image.cpu()
                scaled = (scale * part).cpu()                        # the float32 product the kernel reads
                s64, g64 = _ref_smooth(order, scaled, img_cpu, up, torch.float64)
                _, g32 = _ref_smooth(order, scaled, img_cpu, up, torch.float32)
                print(f"{tag}: sums {sums.tolist()} ref {s64.tolist()}")
                close(sums, s64, rel=1e-5)
                # autograd multiplied the kernel's gradient by scale on the way to the leaf; the reference differentiates with
                # respect to the scaled flow.  Undoing the factor costs one float32 rounding, 6e-8, against a bound of 2e-5
                _check_grad(tag, grad / scale, g64, g32)
                if order == 2 and h < 3 and w < 3:
                    assert not bool(sums.any()) and not bool(grad.any()), tag
                if order == 2 and h == 2 and w >= 3:
                    # no term along y: a row's sums and gradient do not depend on the other row -- exactly
                    other = (scale * part).detach().clone()
                    other[:, 1] = other[:, 1] * 1.5 + 0.25
                    other.requires_grad_(True)
                    pa.smoothness_sums(other, image, ur.ALPHA, 1e-3, 0.5, 2).backward(up_gpu)
                    base = (scale * part).detach().clone().requires_grad_(True)
                    pa.smoothness_sums(base, image, ur.ALPHA, 1e-3, 0.5, 2).backward(up_gpu)
                    assert torch.equal(other.grad[:, 0], base.grad[:, 0]), tag


# ------------------------------------------------------------------ C2: the composed objective
def _gpu_run(pa, obj, name, two, masks=None):
    im0, im1 = (t.cuda() for t in orf.frames(name))
    final, pyramid = orf.flows(name, two)
    leaves = [t.cuda().requires_grad_(True) for t in [final] + pyramid]
    loss, terms = obj(im0, im1, leaves[0], leaves[1:], masks=masks)
    loss.backward()
    return loss.detach(), terms, [t.grad for t in leaves]


def _same_bits(a, b):
    (la, ta, ga), (lb, tb, gb) = a, b
    assert torch.equal(la, lb) and set(ta) == set(tb)
    for k in ta:
        if k == "levels":
            assert all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(ta[k], tb[k])), (ta[k], tb[k])
        else:
            assert float(ta[k]) == float(tb[k]), k
    for x, y in zip(ga, gb):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("frames_name", list(orf.FRAMES))
@pytest.mark.parametrize("cfg_name", list(orf.CONFIGS))
def test_objective_vs_float64_restatement(pa, cfg_name, frames_name):
    cfg = orf.config(cfg_name)
    N, H, W, C = orf.FRAMES[frames_name]
    two = cfg["occlusion"] != "none"
    obj = pa.UnsupObjective(**cfg)
    got = _gpu_run(pa, obj, frames_name, two)
    loss, terms, grads = got
    masks = None
    if two:                                     # the GPU's masks go to both sides: they are pinned by their own tests
        final = orf.flows(frames_name, True)[0].cuda()
        masks = obj.masks(final[:N], final[N:])[:2]
    cpu_masks = None if masks is None else tuple(m.cpu() for m in masks)
    l64, t64, _, g64 = orf.run(cfg, frames_name, cpu_masks, torch.float64)
    l32, _, _, g32 = orf.run(cfg, frames_name, cpu_masks, torch.float32)
    tag = f"{cfg_name} {frames_name}"
    print(f"{tag}: loss {float(loss):.8f} ref {float(l64):.8f} rel err {abs(float(loss) - float(l64)) / float(l64):.3e} "
          f"(float32 torch {abs(float(l32) - float(l64)) / float(l64):.3e})")
    assert abs(float(loss) - float(l64)) <= 2e-5 * float(l64)
    # every reported term
    names = {"base": obj.term, "ssim": "ssim", "smoothness": "smoothness", "consistency": "consistency"}
    assert set(terms) == {names.get(k, k) for k in t64}, (sorted(terms), sorted(t64))
    for k, want in t64.items():
        if k == "levels":
            continue
        have, want = float(terms[names.get(k, k)]), float(want)
        print(f"{tag}: {k} {have:.8f} ref {want:.8f}")
        assert abs(have - want) <= 1e-5 * want, k
    if "levels" in t64:
        print(f"{tag}: levels {terms['levels']} ref {t64['levels']}")
        assert len(terms["levels"]) == 5
        for l, (have, want) in enumerate(zip(terms["levels"], t64["levels"])):
            skipped = orf.skipped(cfg, *orf.level_shapes(frames_name)[l])
            assert math.isnan(want) == skipped
            assert (math.isnan(have) and math.isnan(want)) or abs(have - want) <= 1e-5 * want, l
    # the gradients: flows_final, then the five pyramid flows
    for i, (g, r64, r32) in enumerate(zip(grads, g64, g32)):
        _check_grad(f"{tag} {'flows_final' if i == 0 else f'flows_pyramid[{i - 1}]'}", g, r64, r32)
    weights = cfg["level_weights"] or (0.0,) * 5
    for l, wl in enumerate(weights):
        if wl == 0 or orf.skipped(cfg, *orf.level_shapes(frames_name)[l]):
            assert grads[1 + l] is None or not bool(grads[1 + l].any()), l
            assert not bool(g64[1 + l].any())
        else:
            assert grads[1 + l] is not None and bool(grads[1 + l].any()), l
    # a second run, and precomputed masks in place of the objective's own: the same bits
    _same_bits(got, _gpu_run(pa, obj, frames_name, two))
    if two:
        _same_bits(got, _gpu_run(pa, obj, frames_name, two, masks=masks))
        # all-true masks: the data terms are those without a mask, bit for bit
        ones = (torch.ones((N, H, W), dtype=torch.bool, device="cuda"),) * 2
        _, t_ones, _ = _gpu_run(pa, obj, frames_name, two, masks=ones)
        im0, im1 = (t.cuda() for t in orf.frames(frames_name))
        final, pyramid = (orf.flows(frames_name, True)[0].cuda(), [p.cuda() for p in orf.flows(frames_name, True)[1]])
        ways = lambda a, b, f: ((a, b, f[:N]), (b, a, f[N:]))
        for key, fn in ((obj.term, obj.data_term), ("ssim", obj.ssim_term)):
            if key in t_ones:
                plain = 0.5 * sum(fn(a, b, f) for a, b, f in ways(im0, im1, final))
                assert float(t_ones[key]) == float(plain), key
        pyr0, pyr1 = pa.frame_pyramid(im0, orf.FACTORS), pa.frame_pyramid(im1, orf.FACTORS)
        for l, value in enumerate(t_ones["levels"]):
            if math.isnan(value):
                continue
            s = pa.level_flow_scale(pyramid[l], (H, W))
            p = sum(obj.data_term(a, b, f, None, flow_scale=s) for a, b, f in ways(pyr0[l], pyr1[l], pyramid[l])) / 2 \
                if cfg["ssim_weight"] < 1 else None
            q = sum(obj.ssim_term(a, b, f, None, flow_scale=s) for a, b, f in ways(pyr0[l], pyr1[l], pyramid[l])) / 2 \
                if cfg["ssim_weight"] > 0 else None
            assert value == float(obj.blend(p, q)), l
        assert t_ones["occluded"] == 0.0


def test_zero_level_weights_are_the_final_only_objective(pa):
    plain = _gpu_run(pa, pa.UnsupObjective(), "n2_64x128", False)
    zeros = _gpu_run(pa, pa.UnsupObjective(level_weights=(0, 0, 0, 0, 0)), "n2_64x128", False)
    _same_bits(plain, zeros)
    assert "levels" not in plain[1] and all(g is None for g in plain[2][1:])


# ------------------------------------------------------------------ C3: one run through the network
def test_objective_trains_the_module_bit_reproducibly(pa):
    """PWCDCNetModule(seed=3) on the smooth pair in both orders (batch 2), UnFlow's configuration with every level: the gradient
    of the weights is finite, non-zero, not the final-only gradient, and the same bits on a second run."""
    from tests import util
    im0, im1 = (torch.from_numpy(a).cuda() for a in util.smooth_images(1, 64, 128))
    cfg = orf.config("unflow")
    runs = []
    for levels in (True, True, False):
        obj = pa.UnsupObjective(**dict(cfg, level_weights=cfg["level_weights"] if levels else None))
        model = pa.PWCDCNetModule(seed=3)
        final, pyramid = model(torch.cat([im0, im1]), torch.cat([im1, im0]))
        loss, terms = obj(im0, im1, final, pyramid)
        loss.backward()
        runs.append((loss.detach().clone(), model.flat.grad.clone(), terms))
    torch.cuda.synchronize()
    (loss, grad, terms), (loss2, grad2, _), (loss_f, grad_f, terms_f) = runs
    print(f"loss {float(loss):.6f} (final only {float(loss_f):.6f}), levels {terms['levels']}, |grad| max {float(grad.abs().max()):.3e}, "
          f"|grad - final only| max {float((grad - grad_f).abs().max()):.3e}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    assert not torch.equal(grad, grad_f) and "levels" not in terms_f
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
