"""Yardstick of the label-free objective (pwcnet_amd/objective.py): the objective stated a second time, in plain torch on the
reference functions of the single terms -- photometric_ref, census_ref, ssim_ref, smoothness_ref, smoothness2_ref,
fb_consistency_ref, frame_pyramid_ref, mask_pyramid_ref -- from the definitions in the docstrings of pwcnet_amd/unsup.py and
pwcnet_amd/pyramid.py and DESIGN.md sections 8 to 12, and the inputs of the GPU tests.  Run in float64 it is the reference and
torch.autograd gives the reference gradients; run in float32 it gives the error a straightforward fp32 composition makes on the
same inputs.  Not a test file; tests/test_host_objective.py validates it without a GPU (finite differences, a hand-written sum of
the single references, the cases' guarantees), tests/test_gpu_objective.py holds the HIP path to it.

Definition.  A DIRECTION is (first frame A, second frame B, flow F from A to B, mask M of A's pixels or None).  Its terms:
    base(A, B, F, M, s)   the mean of rho over the contributing pixels and channels (charbonnier) or of rho(h) over the
                          contributing centres (census), the flow taken as s * F pixels
    ssim(A, B, F, M, s)   the mean of (1 - SSIM) / 2 over the contributing centres and channels
    data                  (1 - w) base + w ssim, w = ssim_weight (w = 0: base alone, w = 1: ssim alone)
    smooth(G, A)          the edge-weighted sum of rho over the first (second) differences of G, G in pixels, over N H W
Without occlusion there is one direction (images_0, images_1, flows, None); with it two, (images_0, images_1, the first N flows,
m_fw) and (images_1, images_0, the last N flows, m_bw), and every term is the MEAN over the directions.
    objective = data + smooth_weight smooth                                        on flows_final, s = 1
              + consistency_weight consistency(fw, bw, m_fw, m_bw)                 on flows_final
              + sum_l W_l (data_l + smooth_weight smooth_l)                        on the levels that are not skipped
Level l: the frames are the block means by the factor W / w_l, the masks the blocks of which at least occ_pool is valid, the
flow flows_pyramid[l] with s_l = 20 w_l / W (px / 20 of the full frame -> the level's own pixels), smooth_l on s_l * flow.  A
level is skipped -- contributes nothing, its value is nan -- when a window of a term in use does not fit: min(h, w) <= 2 radius.
The masks are inputs: they are discontinuous in the flow and pinned by the tests of fb_valid and range_valid.
"""
import functools

import numpy as np
import torch

from tests import census_ref as cr
from tests import fb_ref as fr
from tests import pyramid_ref as pr
from tests import splat_ref as sr
from tests import ssim_ref as sm
from tests import unflow_ref as uf
from tests import unsup_ref as ur

DEFAULTS = dict(photo="charbonnier", census_radius=3, photo_eps=1e-3, photo_q=0.5, ssim_weight=0.0, ssim_radius=1,
                smooth_weight=0.1, smooth_order=1, edge_alpha=10.0, occlusion="none", occ_alpha1=0.01, occ_alpha2=0.5,
                occ_min_range=0.5, consistency_weight=0.0, level_weights=None, occ_pool=0.5)
ONES = (1.0, 1.0, 1.0, 1.0, 1.0)
# the configurations of tests/test_gpu_objective.py: what differs from train.py's defaults
CONFIGS = {
    "final_only": dict(),
    "levels": dict(level_weights=ONES),
    "census3_range": dict(photo="census", census_radius=3, occlusion="range", level_weights=(0.32, 0.08, 0.02, 0.01, 0.005)),
    "unflow": dict(photo="census", census_radius=1, occlusion="fb", smooth_order=2, consistency_weight=0.2, level_weights=ONES),
    "arflow": dict(ssim_weight=0.85, ssim_radius=1, occlusion="fb", level_weights=ONES),
    "ssim_only": dict(ssim_weight=1.0, level_weights=(0.0, 0.0, 1.0, 0.0, 1.0)),
}
FRAMES = {"n2_64x128": (2, 64, 128, 3), "n1_128x192": (1, 128, 192, 3)}
FACTORS = (64, 32, 16, 8, 4)               # flows_pyramid's order, coarse -> fine


def config(name):
    return dict(DEFAULTS, **CONFIGS[name])


def level_shapes(frames):
    N, H, W, _ = FRAMES[frames]
    return [(H // f, W // f) for f in FACTORS]


def level_scale(w, W):
    """20 / 2^level: a pyramid flow is in px / 20 of the full frame, the level is W / w times smaller."""
    return 20.0 * w / W


# ------------------------------------------------------------------ the restatement
def _mean_over_pixels(ref, A, B, F, M, s, channels, **kw):
    sums, counts, contributing = ref(A, B, F, s, M, **kw)
    return sums.sum() / (channels * max(int(counts.sum()), 1)), contributing


def direction_data(cfg, A, B, F, M, s):
    """(data term of one direction, base value or None, ssim value or None, the pixels that contribute to either)."""
    w = cfg["ssim_weight"]
    base = ssim = None
    touched = torch.zeros(F.shape[:3], dtype=torch.bool)
    if w < 1:
        if cfg["photo"] == "census":
            base, c = _mean_over_pixels(cr.census_ref, A, B, F, M, s, 1, radius=cfg["census_radius"])
        else:
            base, c = _mean_over_pixels(ur.photometric_ref, A, B, F, M, s, A.shape[3], eps=cfg["photo_eps"], q=cfg["photo_q"])
        touched = touched | c
    if w > 0:
        ssim, c = _mean_over_pixels(sm.ssim_ref, A, B, F, M, s, A.shape[3], radius=cfg["ssim_radius"])
        touched = touched | c
    data = base if ssim is None else ssim if base is None else (1 - w) * base + w * ssim
    return data, base, ssim, touched


def direction_smooth(cfg, G, A):
    ref = ur.smoothness_ref if cfg["smooth_order"] == 1 else uf.smoothness2_ref
    return ref(G, A, cfg["edge_alpha"], cfg["photo_eps"], cfg["photo_q"]).sum() / (G.shape[0] * G.shape[1] * G.shape[2])


def skipped(cfg, h, w):
    census = cfg["ssim_weight"] < 1 and cfg["photo"] == "census"
    ssim = cfg["ssim_weight"] > 0
    return (census and min(h, w) <= 2 * cfg["census_radius"]) or (ssim and min(h, w) <= 2 * cfg["ssim_radius"])


def _mean(values):
    values = [v for v in values if v is not None]
    return sum(values) / len(values) if values else None


def objective_ref(cfg, im0, im1, flows_final, flows_pyramid, masks=None):
    """(loss, terms, touched) in the dtype of the flows.  im0, im1: float32 (N,H,W,C); flows_final: (N,H,W,2), with occlusion
    (2N,H,W,2); flows_pyramid: five level flows or None; masks: (m_fw, m_bw) bool with occlusion.  terms: "base" (absent with
    ssim_weight 1), "ssim", "smoothness", "occluded", "consistency" as 0-dim tensors / a float, "levels": a list, nan for a
    skipped level.  touched: per level index (and "final") the (batch, h, w) pixels that contribute to a data term."""
    dt = flows_final.dtype
    N, H, W, C = im0.shape
    two = cfg["occlusion"] != "none"
    assert (masks is not None) == two and flows_final.shape[0] == (2 * N if two else N)

    def directions(A0, A1, F, m):
        if not two:
            return [(A0, A1, F, None)]
        return [(A0, A1, F[:N], m[0]), (A1, A0, F[N:], m[1])]

    def data_and_smooth(A0, A1, F, m, s):
        ways = directions(A0.to(dt), A1.to(dt), F, m)
        per = [direction_data(cfg, A, B, Fd, M, s) for A, B, Fd, M in ways]
        smooth = _mean([direction_smooth(cfg, s * Fd, A) for A, _, Fd, _ in ways])
        return _mean([p[0] for p in per]), _mean([p[1] for p in per]), _mean([p[2] for p in per]), smooth, \
            torch.cat([p[3] for p in per])

    terms, touched = {}, {}
    data, base, ssim, smooth, touched["final"] = data_and_smooth(im0, im1, flows_final, masks, 1.0)
    loss = data + cfg["smooth_weight"] * smooth
    if base is not None:
        terms["base"] = base.detach()
    if ssim is not None:
        terms["ssim"] = ssim.detach()
    terms["smoothness"] = smooth.detach()
    if two:
        terms["occluded"] = 1.0 - float(masks[0].sum() + masks[1].sum()) / (2 * N * H * W)
    if cfg["consistency_weight"] > 0:
        s_a, c_a, _, s_b, c_b, _ = uf.fb_consistency_ref(flows_final[:N], flows_final[N:], 1.0, masks[0], masks[1],
                                                         cfg["photo_eps"], cfg["photo_q"])
        consistency = (s_a.sum() + s_b.sum()) / (2 * max(int(c_a.sum() + c_b.sum()), 1))
        loss = loss + cfg["consistency_weight"] * consistency
        terms["consistency"] = consistency.detach()
    weights = cfg["level_weights"]
    if weights is not None and any(w != 0 for w in weights):
        factors = [W // F.shape[2] for F in flows_pyramid]
        pyr0, pyr1 = pr.frame_pyramid_ref(im0, factors), pr.frame_pyramid_ref(im1, factors)
        pooled = [pr.mask_pyramid_ref(m, factors, cfg["occ_pool"])[0] for m in masks] if two else None
        terms["levels"] = []
        for l, (wl, F) in enumerate(zip(weights, flows_pyramid)):
            h, w = F.shape[1:3]
            if skipped(cfg, h, w):
                terms["levels"].append(float("nan"))
                continue
            m = (pooled[0][l], pooled[1][l]) if two else None
            data_l, _, _, smooth_l, touched[l] = data_and_smooth(pyr0[l], pyr1[l], F, m, level_scale(w, W))
            terms["levels"].append(float(data_l.detach()))
            if wl != 0:
                loss = loss + wl * (data_l + cfg["smooth_weight"] * smooth_l)
    return loss, terms, touched


# ------------------------------------------------------------------ inputs
def _multiscale(rs, N, H, W, C):
    """Frames in [0, 1] with contrast at every scale: random fields at 1/64 .. 1/4 of the size and at full size, each held
    constant over its blocks, summed -- a block mean at any level keeps the coarser fields whole."""
    x = np.zeros((N, H, W, C))
    for f, amp in ((64, 0.30), (32, 0.25), (16, 0.20), (8, 0.20), (4, 0.15), (1, 0.25)):
        x += amp * np.kron(rs.uniform(-1, 1, size=(N, H // f, W // f, C)), np.ones((1, f, f, 1)))
    return ((x - x.min()) / (x.max() - x.min())).astype(np.float32)


@functools.lru_cache(maxsize=None)
def frames(name):
    """(im0, im1) float32 torch tensors; read-only."""
    N, H, W, C = FRAMES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    return torch.from_numpy(_multiscale(rs, N, H, W, C)), torch.from_numpy(_multiscale(rs, N, H, W, C))


def tiny_flow(N, h, w, scale, seed):
    """A level of one or two rows (1 x 2, 2 x 4, 2 x 3), built directly: unsup_ref.build_case's 10-40 % out-of-frame share
    cannot be asserted on two to eight pixels.  The same off-integer rule: scale * flow = an integer that keeps the pixel inside
    the frame (x + i in [0, w - 2], y + j in [0, h - 2]) + a continuous part in [0.1, 0.9]; about a quarter of the pixels is
    thrown out of the frame along x.
    h = 1: the only in-frame ordinate of a one-row level is the integer 0, so NO off-integer flow samples inside it -- what a
    trained network gives at that level.  Image 0 therefore gets a vertical component of EXACTLY 0 (times any scale: exactly 0
    in float32 and float64, so both take the same corner with weight 0; not a near-integer sample) and contributes; every other
    image keeps the rule along y too and contributes nothing, the realistic case."""
    rs = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    px = np.zeros((N, h, w, 2))
    px[..., 0] = rs.randint(0, w - 1, size=(N, h, w)) - xs + rs.uniform(uf.LO, uf.HI, size=(N, h, w))
    if h > 1:
        px[..., 1] = rs.randint(0, h - 1, size=(N, h, w)) - ys + rs.uniform(uf.LO, uf.HI, size=(N, h, w))
    else:
        px[1:, ..., 1] = rs.uniform(uf.LO, uf.HI, size=(N - 1, h, w))
    out = rs.uniform(size=(N, h, w)) < 0.25
    out[:, 0, 0] = False                                              # at least one pixel per image stays
    px[..., 0] = np.where(out, w + 2 + px[..., 0], px[..., 0])
    flow = (px / scale).astype(np.float32)
    cx, cy = uf._coordinates(flow, scale)
    assert float(np.abs(cx - np.round(cx)).min()) >= 0.1
    exact = flow[..., 1] == 0.0
    assert not exact.any() or h == 1
    if (~exact).any():
        assert float(np.abs(cy - np.round(cy))[~exact].min()) >= 0.1
    return flow


def _level_kw(h, w):
    """The tile and the largest integer motion of a level's flow: small enough that most of a small level stays in frame."""
    m = min(h, w)
    return dict(block=max(2, min(5, m // 2)), max_off=1 if m <= 8 else 2 if m <= 16 else 3)


def level_flow(N, h, w, scale, seed):
    """One direction's flow of a level, float32 (N,h,w,2): scale * flow keeps 0.1 from the integers (unsup_ref.build_case, which
    asserts that, its 10-40 % of out-of-frame pixels and a contributing pixel in every image; levels of one or two rows:
    tiny_flow)."""
    if h <= 2:
        return tiny_flow(N, h, w, scale, seed)
    return ur.build_case(N, h, w, 3, flow_scale=scale, seed=seed, masked=False, **_level_kw(h, w))["flow"]


# (frames, stacked 2N layout) -> the seed of flows_final and, per level, the seed of each direction: the first seeds, counting up
# from 0 on the CPU, at which build_case's own assertions hold and every configuration of CONFIGS finds contributing pixels in
# every direction of every level it does not skip (tests/test_host_objective.py asserts all of it on the float64 reference)
SEEDS = {
    ("n2_64x128", False): (0, ((0,), (0,), (114,), (3,), (0,))),
    ("n2_64x128", True): (0, ((0, 1), (0, 1), (52, 101), (3, 7), (0, 3))),
    ("n1_128x192", False): (0, ((0,), (11,), (0,), (2,), (0,))),
    ("n1_128x192", True): (0, ((0, 1), (11, 20), (0, 1), (2, 3), (0, 1))),
}


def final_flow(frames_name, two, seed):
    N, H, W, _ = FRAMES[frames_name]
    if two:
        pair = uf.build_case(N, H, W, 1.0, seed=seed, masked=False, noise=0.4)
        return np.concatenate([pair["fw"], pair["bw"]])
    return level_flow(N, H, W, 1.0, seed)


@functools.lru_cache(maxsize=None)
def flows(frames_name, two):
    """(flows_final, [five pyramid flows]) float32 torch tensors, independent of one another (not network outputs); read-only.
    two: the stacked 2N layout -- flows_final from unflow_ref.build_case (a forward flow and a backward flow that is consistent
    with it up to noise and the tile seams, both 0.1 off the integers), every level two independent directions."""
    N, H, W, _ = FRAMES[frames_name]
    seed, level_seeds = SEEDS[frames_name, two]
    pyramid = [np.concatenate([level_flow(N, h, w, level_scale(w, W), s) for s in seeds])
               for (h, w), seeds in zip(level_shapes(frames_name), level_seeds)]
    return torch.from_numpy(final_flow(frames_name, two, seed)), [torch.from_numpy(p) for p in pyramid]


def host_masks(cfg, final, N):
    """The float64 masks of the configuration's occlusion mode (the GPU tests pass the GPU's own masks instead)."""
    fw, bw = final[:N].double(), final[N:].double()
    if cfg["occlusion"] == "fb":
        a, b = fr.fb_ref(fw, bw, 1.0, cfg["occ_alpha1"], cfg["occ_alpha2"])
        return a.mask, b.mask
    return sr.splat_ref(None, bw)[1] >= cfg["occ_min_range"], sr.splat_ref(None, fw)[1] >= cfg["occ_min_range"]


def run(cfg, frames_name, masks, dt):
    """The restatement in dtype dt on the case's inputs: (loss, terms, touched, [gradient w.r.t. flows_final, then w.r.t. each
    pyramid flow -- zeros where nothing reaches a flow])."""
    im0, im1 = frames(frames_name)
    final, pyramid = flows(frames_name, cfg["occlusion"] != "none")
    leaves = [t.to(dt).clone().requires_grad_(True) for t in [final] + pyramid]
    loss, terms, touched = objective_ref(cfg, im0, im1, leaves[0], leaves[1:], masks)
    loss.backward()
    return loss.detach(), terms, touched, [torch.zeros_like(t) if t.grad is None else t.grad for t in leaves]


def gradient_share(grad):
    """The share of a flow's pixels whose reference gradient is above 1e-3 of the largest."""
    mag = grad.abs().amax(dim=3)
    return float((mag > 1e-3 * float(mag.max())).double().mean()) if float(mag.max()) > 0 else 0.0
