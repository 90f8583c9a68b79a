"""Validates tests/objective_ref.py, the float64 restatement of the label-free objective, and its cases without a GPU: central
finite differences against autograd, the restatement against a hand-written sum of the single references, zero level weights,
the guarantees of the cases (so that a GPU test cannot pass by being empty), and the argument checks of
pwcnet_amd.UnsupObjective that run on CPU tensors."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import census_ref as cr
from tests import objective_ref as orf
from tests import pyramid_ref as pr
from tests import unflow_ref as uf
from tests import unsup_ref as ur

CASES = [(c, f) for c in orf.CONFIGS for f in orf.FRAMES]


def _masks(cfg, frames_name):
    if cfg["occlusion"] == "none":
        return None
    return orf.host_masks(cfg, orf.flows(frames_name, True)[0], orf.FRAMES[frames_name][0])


@functools.lru_cache(maxsize=None)
def _run64(cfg_name, frames_name):
    cfg = orf.config(cfg_name)
    return orf.run(cfg, frames_name, _masks(cfg, frames_name), torch.float64)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("cfg_name", ["unflow", "arflow"])
def test_autograd_gradient_matches_central_differences(cfg_name):
    """Directional central differences (step 1e-6 along two random directions per tensor; the 0.1 distance from the integers keeps
    every sample in its cell) for flows_final and the two finest pyramid flows, masks held constant."""
    frames_name = "n2_64x128"
    cfg = orf.config(cfg_name)
    masks = _masks(cfg, frames_name)
    im0, im1 = orf.frames(frames_name)
    final, pyramid = orf.flows(frames_name, True)
    base = [t.double() for t in [final] + pyramid]
    _, _, _, grads = _run64(cfg_name, frames_name)

    def value(tensors):
        with torch.no_grad():
            return float(orf.objective_ref(cfg, im0, im1, tensors[0], tensors[1:], masks)[0])

    rs = np.random.RandomState(3)
    for i in (0, 4, 5):
        for _ in range(2):
            v = torch.from_numpy(rs.uniform(-1, 1, size=tuple(base[i].shape)))
            step = 1e-6
            up = [t + step * v if j == i else t for j, t in enumerate(base)]
            down = [t - step * v if j == i else t for j, t in enumerate(base)]
            fd = (value(up) - value(down)) / (2 * step)
            an = float((grads[i] * v).sum())
            print(f"{cfg_name} tensor {i}: finite difference {fd:.9e} autograd {an:.9e}")
            assert abs(fd - an) <= 1e-6 * max(abs(an), float(grads[i].abs().sum()) * 1e-3), (i, fd, an)


def test_restatement_is_the_hand_written_sum_one_direction():
    """charbonnier, no occlusion, level weights (1, 1, 1, 1, 1) on (1, 128, 192, 3): term by term from the single references."""
    name = "n1_128x192"
    N, H, W, C = orf.FRAMES[name]
    im0, im1 = (t.double() for t in orf.frames(name))
    final, pyramid = orf.flows(name, False)
    s, c, _ = ur.photometric_ref(im0, im1, final.double(), 1.0, None, 1e-3, 0.5)
    total = float(s.sum()) / (C * int(c.sum())) + 0.1 * float(ur.smoothness_ref(final.double(), im0, 10.0, 1e-3, 0.5).sum()) / (N * H * W)
    values = []
    for f, fl in zip(orf.FACTORS, pyramid):
        a, b = (pr.frame_pyramid_ref(t.float(), [f])[0].double() for t in (im0, im1))
        h, w = fl.shape[1:3]
        scale = 20.0 / f
        s, c, _ = ur.photometric_ref(a, b, fl.double(), scale, None, 1e-3, 0.5)
        values.append(float(s.sum()) / (C * int(c.sum())))
        total += values[-1] + 0.1 * float(ur.smoothness_ref(scale * fl.double(), a, 10.0, 1e-3, 0.5).sum()) / (N * h * w)
    loss, terms, _, _ = _run64("levels", name)
    assert abs(float(loss) - total) <= 1e-12 * total
    assert np.allclose(terms["levels"], values, rtol=1e-12, atol=0)


def test_restatement_is_the_hand_written_sum_two_directions():
    """UnFlow's terms on flows_final alone (census r = 1 under fb masks, second-order smoothness, consistency)."""
    name = "n2_64x128"
    N, H, W, C = orf.FRAMES[name]
    cfg = dict(orf.config("unflow"), level_weights=None)
    masks = _masks(cfg, name)
    im0, im1 = (t.double() for t in orf.frames(name))
    final = orf.flows(name, True)[0].double()
    fw, bw = final[:N], final[N:]
    census = []
    for a, b, f, m in ((im0, im1, fw, masks[0]), (im1, im0, bw, masks[1])):
        s, c, _ = cr.census_ref(a, b, f, 1.0, m, radius=1)
        census.append(float(s.sum()) / int(c.sum()))
    smooth = [float(uf.smoothness2_ref(f, a, 10.0, 1e-3, 0.5).sum()) / (N * H * W) for f, a in ((fw, im0), (bw, im1))]
    cons = uf.fb_consistency_ref(fw, bw, 1.0, masks[0], masks[1], 1e-3, 0.5)
    cons = uf.consistency_loss_ref(cons[0], cons[1], cons[3], cons[4])
    total = 0.5 * sum(census) + 0.1 * 0.5 * sum(smooth) + 0.2 * cons
    loss, terms, _ = orf.objective_ref(cfg, im0.float(), im1.float(), final, None, masks)
    assert abs(float(loss) - total) <= 1e-12 * total
    assert abs(float(terms["base"]) - 0.5 * sum(census)) <= 1e-12 and abs(float(terms["consistency"]) - cons) <= 1e-12
    assert terms["occluded"] == 1.0 - float(masks[0].sum() + masks[1].sum()) / (2 * N * H * W) and "levels" not in terms


def test_zero_level_weights_give_the_final_only_value():
    name = "n2_64x128"
    im0, im1 = orf.frames(name)
    final, pyramid = (orf.flows(name, False)[0].double(), [p.double() for p in orf.flows(name, False)[1]])
    plain = orf.objective_ref(orf.config("final_only"), im0, im1, final, None)
    zeros = orf.objective_ref(dict(orf.config("final_only"), level_weights=(0.0,) * 5), im0, im1, final, pyramid)
    assert float(plain[0]) == float(zeros[0]) and "levels" not in zeros[1]
    assert float(plain[0]) == float(_run64("final_only", name)[0])


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("frames_name", list(orf.FRAMES))
@pytest.mark.parametrize("two", [False, True])
def test_case_flows_keep_off_the_integers(frames_name, two):
    N, H, W, _ = orf.FRAMES[frames_name]
    final, pyramid = orf.flows(frames_name, two)
    assert final.shape == ((2 * N if two else N), H, W, 2)
    assert [tuple(p.shape[1:3]) for p in pyramid] == orf.level_shapes(frames_name)
    for fl, scale in [(final, 1.0)] + [(p, orf.level_scale(p.shape[2], W)) for p in pyramid]:
        fl = fl.numpy()
        cx, cy = uf._coordinates(fl, scale)
        assert float(np.abs(cx - np.round(cx)).min()) >= 0.1
        exact = fl[..., 1] == 0.0                  # a one-row level: image 0's vertical component is exactly 0 (tiny_flow)
        first = np.arange(fl.shape[0]) % N == 0     # image 0 of each direction
        assert not exact.any() or (fl.shape[1] == 1 and exact[first].all() and not exact[~first].any())
        if (~exact).any():
            assert float(np.abs(cy - np.round(cy))[~exact].min()) >= 0.1


@pytest.mark.parametrize("cfg_name,frames_name", CASES)
def test_case_preconditions(cfg_name, frames_name):
    """Every level that is not skipped has contributing pixels in each direction (on a one-row level: in image 0); the levels
    that enter the loss carry a reference gradient above 1e-3 of the level's largest at 5 % of their pixels at least -- a level of
    one or two rows: a non-zero reference gradient; a level with weight 0 or skipped: none at all."""
    cfg = orf.config(cfg_name)
    N = orf.FRAMES[frames_name][0]
    loss, terms, touched, grads = _run64(cfg_name, frames_name)
    assert math.isfinite(float(loss)) and float(loss) > 0
    directions = 2 if cfg["occlusion"] != "none" else 1
    weights = cfg["level_weights"] or (0.0,) * 5
    for d in range(directions):
        assert all(bool(touched["final"][d * N + n].any()) for n in range(N))
    assert orf.gradient_share(grads[0]) >= 0.05
    for l, (h, w) in enumerate(orf.level_shapes(frames_name)):
        if cfg["level_weights"] is None or orf.skipped(cfg, h, w):
            assert l not in touched and not bool(grads[1 + l].any())
            assert cfg["level_weights"] is None or math.isnan(terms["levels"][l])
            continue
        assert terms["levels"][l] > 0
        for d in range(directions):
            part = touched[l][d * N:(d + 1) * N]
            assert bool(part.any()) if h == 1 else all(bool(part[n].any()) for n in range(N)), (l, d)
        if weights[l] == 0:
            assert not bool(grads[1 + l].any())
        elif h <= 2:
            assert bool(grads[1 + l].any())
        else:
            assert orf.gradient_share(grads[1 + l]) >= 0.05, (l, orf.gradient_share(grads[1 + l]))
    if directions == 2:
        assert 0.05 <= terms["occluded"] <= 0.8


# ------------------------------------------------------------------ pwcnet_amd.UnsupObjective on CPU tensors
@pytest.mark.parametrize("kw", [dict(photo="l1"), dict(occlusion="both"), dict(census_radius=4), dict(ssim_radius=0),
                                dict(smooth_order=3), dict(ssim_weight=1.5), dict(ssim_weight=-0.1), dict(photo_eps=0.0),
                                dict(photo_q=1.5), dict(edge_alpha=-1.0), dict(occ_alpha2=-1.0), dict(occ_min_range=-0.5),
                                dict(consistency_weight=-1.0), dict(consistency_weight=0.2), dict(occ_pool=0.0), dict(occ_pool=1.5),
                                dict(level_weights=(1, -1, 1, 1, 1)), dict(level_weights=())])
def test_objective_refuses_a_bad_configuration(kw):
    from pwcnet_amd import UnsupObjective
    with pytest.raises(ValueError):
        UnsupObjective(**kw)


def test_objective_configuration():
    from pwcnet_amd import UnsupObjective
    assert UnsupObjective().level_weights is None and UnsupObjective(level_weights=(0, 0, 0, 0, 0)).level_weights is None
    assert UnsupObjective(level_weights=[0, 0, 1, 0, 1]).level_weights == (0.0, 0.0, 1.0, 0.0, 1.0)
    assert UnsupObjective().term == "photometric" and UnsupObjective(photo="census").term == "census"
    assert UnsupObjective(occlusion="range", consistency_weight=0.2).consistency_weight == 0.2


def test_objective_checks_its_tensors_before_any_launch():
    from pwcnet_amd import UnsupObjective
    im = torch.zeros((2, 64, 128, 3))
    flows, stacked = torch.zeros((2, 64, 128, 2)), torch.zeros((4, 64, 128, 2))
    pyramid = [torch.zeros((2, 64 // f, 128 // f, 2)) for f in (64, 32, 16, 8, 4)]
    mask = torch.ones((2, 64, 128), dtype=torch.bool)
    plain, fb = UnsupObjective(), UnsupObjective(occlusion="fb")
    levels = UnsupObjective(level_weights=(1, 1, 1, 1, 1))
    for call in (lambda: plain(im, im[:1], flows), lambda: plain(im, im, stacked), lambda: fb(im, im, flows),
                 lambda: plain(im, im, flows[..., :1]), lambda: plain(im, im, flows, masks=(mask, mask)),
                 lambda: fb(im, im, stacked, masks=(mask,)), lambda: fb(im, im, stacked, masks=(mask, mask[:1])),
                 lambda: levels(im, im, flows), lambda: levels(im, im, flows, pyramid[:4]),
                 lambda: levels(im, im, flows, pyramid[:4] + [stacked[:, :16, :32]]),
                 lambda: levels(im, im, flows, pyramid[:4] + [flows[:, :16, :30]])):
        with pytest.raises(ValueError, match="UnsupObjective"):
            call()
    # a well-formed call on CPU tensors gets as far as the first term's device check: no quiet fall-back
    for obj, f in ((plain, flows), (levels, flows)):
        with pytest.raises(ValueError, match="GPU only"):
            obj(im, im, f, pyramid)
