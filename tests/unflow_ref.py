"""Yardstick of the two last terms of UnFlow's loss (pwcnet_amd/unsup.py smoothness_*(order=2) and fb_consistency_*;
csrc/pwc_unsup.hip, csrc/pwc_fbcheck.hip): restatements in torch ops on plain indexing and torch.where -- run in float64 they are
the reference, torch.autograd gives the reference gradient with respect to the flow (both flows for the consistency term), run in
float32 they give the error a straightforward fp32 composition makes on the same inputs (on the device of their arguments: the
float32 run on the GPU is what scripts/bench_unflow.py times the kernels against) -- and the seeded cases of the GPU tests.
Not a test file; tests/test_host_unflow.py validates it without a GPU (finite differences, the builder's guarantees).

The C entries take alpha, flow_scale, eps and q as `float`: the restatements round them to float32 first and compute everything
else in the dtype of the flows."""
import functools

import numpy as np
import torch

from tests import fb_ref as fr
from tests import unsup_ref as ur
from tests.unsup_ref import rho


def _f32(*values):
    return tuple(float(np.float32(v)) for v in values)


# ------------------------------------------------------------------ second-order smoothness
def smoothness2_ref(flow, image=None, alpha=10.0, eps=1e-3, q=0.5):
    """sums (N,): rho of the second differences of the flow along x (centres 1 .. W - 2) and y (centres 1 .. H - 2), weighted by
    exp(-alpha * mean_c |image difference across the centre|).  W < 3: no x terms; H < 3: no y terms."""
    alpha, eps, q = _f32(alpha, eps, q)
    N, H, W, _ = flow.shape
    out = torch.zeros((N,), dtype=flow.dtype, device=flow.device)
    if W >= 3:
        t = rho(flow[:, :, :-2] - 2 * flow[:, :, 1:-1] + flow[:, :, 2:], eps, q).sum(3)
        if image is not None:
            t = t * torch.exp(-alpha * (image[:, :, 2:] - image[:, :, :-2]).abs().mean(3))
        out = out + t.sum(dim=(1, 2))
    if H >= 3:
        t = rho(flow[:, :-2] - 2 * flow[:, 1:-1] + flow[:, 2:], eps, q).sum(3)
        if image is not None:
            t = t * torch.exp(-alpha * (image[:, 2:] - image[:, :-2]).abs().mean(3))
        out = out + t.sum(dim=(1, 2))
    return out


# ------------------------------------------------------------------ consistency term
def _consistency_direction(own, other, scale, valid, eps, q):
    """(sums (N,), counts (N,) int64, contributing (N,H,W) bool) of one direction.  Pixels that do not contribute are selected
    out BEFORE any arithmetic (their own flow and their four samples are replaced by 0), so that NaN there reaches neither a sum
    nor, through 0 * NaN, a gradient.  floor and clip carry no gradient."""
    N, H, W, _ = own.shape
    dt, dev = own.dtype, own.device
    zero = torch.zeros((), dtype=dt, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev), indexing="ij")
    m = torch.ones((N, H, W), dtype=torch.bool, device=dev) if valid is None else valid != 0
    f = scale * torch.where(m.unsqueeze(3), own, zero)
    px, py = xs + f[..., 0], ys + f[..., 1]
    inside = m & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    px, py = torch.where(inside, px, zero), torch.where(inside, py, zero)
    fx0, fy0 = torch.floor(px).detach(), torch.floor(py).detach()
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    wx, wy = (px - fx0).unsqueeze(3), (py - fy0).unsqueeze(3)
    n = torch.arange(N, device=dev).reshape(N, 1, 1).expand(N, H, W)
    sel = inside.unsqueeze(3)
    v00, v01 = torch.where(sel, other[n, y0, x0], zero), torch.where(sel, other[n, y0, x1], zero)
    v10, v11 = torch.where(sel, other[n, y1, x0], zero), torch.where(sel, other[n, y1, x1], zero)
    g = scale * ((1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11))
    e = torch.where(sel, f, zero) + g
    term = torch.where(inside, rho(e, eps, q).sum(3), zero)
    return term.sum(dim=(1, 2)), inside.sum(dim=(1, 2)), inside


def fb_consistency_ref(flow_a, flow_b, flow_scale=1.0, valid_a=None, valid_b=None, eps=1e-3, q=0.5):
    """(sums_a, counts_a, contributing_a, sums_b, counts_b, contributing_b) in the dtype of the flows; differentiable with
    respect to both flows."""
    scale, eps, q = _f32(flow_scale, eps, q)
    return (_consistency_direction(flow_a, flow_b, scale, valid_a, eps, q)
            + _consistency_direction(flow_b, flow_a, scale, valid_b, eps, q))


def consistency_loss_ref(sums_a, counts_a, sums_b, counts_b):
    return float(sums_a.sum() + sums_b.sum()) / (2 * max(int(counts_a.sum() + counts_b.sum()), 1))


# ------------------------------------------------------------------ inputs of the consistency cases
LO, HI = 0.1 + 0.8e-3, 0.9 - 0.8e-3          # the continuous part, drawn 1e-3 inside [0.1, 0.9]: the division by flow_scale rounds


def _coordinates(flow, flow_scale):
    """The sample coordinates the kernels see: the stored fp32 flow times the fp32 flow_scale, in double."""
    N, H, W, _ = flow.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    s = np.float64(np.float32(flow_scale))
    return xs + s * flow[..., 0].astype(np.float64), ys + s * flow[..., 1].astype(np.float64)


def _assert_off_the_integers(flow, flow_scale, where=None):
    for c in _coordinates(flow, flow_scale):
        c = c if where is None else c[where]
        assert float(np.abs(c - np.round(c)).min()) >= 0.1, "a sample coordinate closer than 0.1 px to an integer"


def build_case(N, H, W, flow_scale=1.0, seed=0, masked=True, empty=None, block=6, max_off=3, noise=0.5):
    """tests/fb_ref.py build_case with the continuous part of every displacement in [0.1, 0.9], numpy float32 (masks bool, or None):

      fw        flow_scale * fw = an integer field, constant on block x block tiles, of up to max_off px, plus a continuous part
                uniform in [0.1, 0.9] per pixel and component.
      bw        flow_scale * bw = -(that integer looked up where the pixel came from) - 1 + a continuous part: 1 - (the looked-up
                one) + uniform noise of amplitude `noise`, clipped to [0.1, 0.9] -- consistent up to the noise and the tile seams.
      empty     the index of an image whose every sample point, in both directions, is out of frame.
      valid_fw, valid_bw   ~70 % True each.  fw_nan, bw_nan: the same flows with NaN at the masked pixels that no contributing
                pixel of the other direction reads a corner from.

    Asserted here, on the CPU: every sample coordinate of both directions is at least 0.1 px from an integer (the kinks of floor
    and the frame border), so a float32 and a float64 evaluation take the same corners."""
    rs = np.random.RandomState(seed)
    th, tw = -(-H // block), -(-W // block)
    off = np.kron(rs.randint(-max_off, max_off + 1, size=(N, th, tw, 2)).astype(np.float64), np.ones((1, block, block, 1)))[:, :H, :W]
    frac = rs.uniform(LO, HI, size=(N, H, W, 2))
    fw_px = off + frac
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    n_idx = np.arange(N).reshape(N, 1, 1) + np.zeros((N, H, W), np.int64)
    sx = np.clip(np.rint(xs - fw_px[..., 0]), 0, W - 1).astype(np.int64)
    sy = np.clip(np.rint(ys - fw_px[..., 1]), 0, H - 1).astype(np.int64)
    bw_px = -off[n_idx, sy, sx] - 1.0 + np.clip(1.0 - frac[n_idx, sy, sx] + rs.uniform(-noise, noise, size=(N, H, W, 2)), LO, HI)
    if empty is not None:
        fw_px[empty, ..., 0] = W + 2.0 + frac[empty, ..., 0]
        bw_px[empty, ..., 0] = -(W + 3.0) + frac[empty, ..., 0]
    fw, bw = (fw_px / flow_scale).astype(np.float32), (bw_px / flow_scale).astype(np.float32)
    _assert_off_the_integers(fw, flow_scale)
    _assert_off_the_integers(bw, flow_scale)
    valid_fw = (rs.uniform(size=(N, H, W)) < 0.7) if masked else None
    valid_bw = (rs.uniform(size=(N, H, W)) < 0.7) if masked else None
    case = {"N": N, "H": H, "W": W, "flow_scale": float(flow_scale), "fw": fw, "bw": bw, "valid_fw": valid_fw,
            "valid_bw": valid_bw, "empty": empty}
    fw_nan, bw_nan = fw.copy(), bw.copy()
    if masked:
        out = fb_consistency_ref(torch.from_numpy(fw).double(), torch.from_numpy(bw).double(), flow_scale,
                                 torch.from_numpy(valid_fw), torch.from_numpy(valid_bw))
        s = np.float64(np.float32(flow_scale))
        fw_nan[~valid_fw & ~fr._sampled(s * bw.astype(np.float64), out[5].numpy())] = np.nan
        bw_nan[~valid_bw & ~fr._sampled(s * fw.astype(np.float64), out[2].numpy())] = np.nan
        assert np.isnan(fw_nan).any() and np.isnan(bw_nan).any()
    case.update(fw_nan=fw_nan, bw_nan=bw_nan)
    return case


CELL = (18.3, 11.6)            # (x, y): where every pixel of the contention case's forward flow points to


def build_contention_case(N=2, H=23, W=37, seed=7):
    """Every pixel of fw points into ONE cell: displacement (18.3 - x, 11.6 - y), so all N * H * W forward pixels scatter onto the
    same four corners of bw's gradient.  bw: an integer in {-1, 0, 1} plus a continuous part in [0.1, 0.9]; no masks."""
    rs = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fw = np.zeros((N, H, W, 2))
    fw[..., 0], fw[..., 1] = CELL[0] - xs, CELL[1] - ys
    bw = rs.randint(-1, 2, size=(N, H, W, 2)) + rs.uniform(LO, HI, size=(N, H, W, 2))
    fw, bw = fw.astype(np.float32), bw.astype(np.float32)
    _assert_off_the_integers(fw, 1.0)
    _assert_off_the_integers(bw, 1.0)
    px, py = _coordinates(fw, 1.0)
    assert np.all(np.floor(px) == np.floor(CELL[0])) and np.all(np.floor(py) == np.floor(CELL[1]))
    return {"N": N, "H": H, "W": W, "flow_scale": 1.0, "fw": fw, "bw": bw, "valid_fw": None, "valid_bw": None, "empty": None,
            "fw_nan": fw, "bw_nan": bw}


# The consistency cases of tests/test_gpu_unflow.py: name -> (build_case arguments, (eps, q)).  N = 2; 23 x 37: odd sizes, tail
# lanes, 4 parts; 272 x 256: 272 > 256 parts of an image, so the grid-stride loop and the capped partition run.  flow_scale in
# {1, 5}, both (eps, q) pairs, ~70 % masks with NaN behind them and no masks, one image that is out of frame everywhere.
CASES = {
    "23x37_s1_a": (dict(N=2, H=23, W=37, flow_scale=1.0, seed=1, noise=0.5), (1e-3, 0.5)),
    "23x37_s5_b_empty": (dict(N=2, H=23, W=37, flow_scale=5.0, seed=2, empty=1, noise=0.3), (1e-2, 0.45)),
    "23x37_s1_b_nomask": (dict(N=2, H=23, W=37, flow_scale=1.0, seed=3, masked=False, noise=0.3), (1e-2, 0.45)),
    "272x256_s5_a": (dict(N=2, H=272, W=256, flow_scale=5.0, seed=4, noise=0.5), (1e-3, 0.5)),
    "272x256_s1_b_nomask": (dict(N=2, H=272, W=256, flow_scale=1.0, seed=5, masked=False, noise=0.3), (1e-2, 0.45)),
}
CONTENTION = "23x37_contention"
UPSTREAM = ((0.75, -1.5), (-0.5, 1.25))        # the gradients that reach (sums_fw[n], sums_bw[n]), N = 2: of both signs
SMOOTH_CASES = ur.CASES                         # the second-order cases: tests/unsup_ref.py's inputs, (eps, q) and ALPHA
ALPHA = ur.ALPHA


def _t(a, dt):
    return torch.from_numpy(a).to(dt)


def consistency_run(case, eps, q, dt, upstream=UPSTREAM):
    """(sums_fw, counts_fw, contributing_fw, sums_bw, counts_bw, contributing_bw, dflow_fw, dflow_bw): the restatement in dtype
    dt on the flows WITHOUT the NaN behind the masks, and the gradient of sum_n upstream[0][n] sums_fw[n] + upstream[1][n]
    sums_bw[n] with respect to both flows."""
    fw, bw = _t(case["fw"], dt).requires_grad_(True), _t(case["bw"], dt).requires_grad_(True)
    vf = None if case["valid_fw"] is None else torch.from_numpy(case["valid_fw"])
    vb = None if case["valid_bw"] is None else torch.from_numpy(case["valid_bw"])
    s_a, c_a, in_a, s_b, c_b, in_b = fb_consistency_ref(fw, bw, case["flow_scale"], vf, vb, eps, q)
    ((s_a * torch.tensor(upstream[0], dtype=dt)).sum() + (s_b * torch.tensor(upstream[1], dtype=dt)).sum()).backward()
    return s_a.detach(), c_a, in_a, s_b.detach(), c_b, in_b, fw.grad, bw.grad


@functools.lru_cache(maxsize=None)
def reference(name):
    """A consistency case, its float64 reference and the same formulas run in float32 -- computed once per process and shared;
    treat it as read-only."""
    if name == CONTENTION:
        case, (eps, q) = build_contention_case(), (1e-3, 0.5)
    else:
        kw, (eps, q) = CASES[name]
        case = build_case(**kw)
    return {"case": case, "eps": eps, "q": q, "run64": consistency_run(case, eps, q, torch.float64),
            "run32": consistency_run(case, eps, q, torch.float32)}


def _smooth2_run(case, eps, q, dt, with_image):
    flow = _t(case["flow"], dt).requires_grad_(True)
    sums = smoothness2_ref(flow, _t(case["im0"], dt) if with_image else None, ALPHA, eps, q)
    (sums * torch.tensor(ur.UPSTREAM, dtype=dt)).sum().backward()
    return sums.detach(), flow.grad


@functools.lru_cache(maxsize=None)
def smooth_reference(name):
    """A second-order smoothness case (tests/unsup_ref.py's inputs): (sums, gradient of sum_n unsup_ref.UPSTREAM[n] sums[n]) in
    float64 and float32, with the image (`smooth`) and without (`smooth_noimg`)."""
    kw, (eps, q) = SMOOTH_CASES[name]
    case = ur.build_case(**kw)
    ref = {"case": case, "eps": eps, "q": q}
    for key, img in (("smooth", True), ("smooth_noimg", False)):
        ref[key + "64"], ref[key + "32"] = _smooth2_run(case, eps, q, torch.float64, img), _smooth2_run(case, eps, q, torch.float32, img)
    return ref
