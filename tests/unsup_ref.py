"""Yardstick of the self-supervised losses (pwcnet_amd/unsup.py, csrc/pwc_unsup.hip): restatements of the two terms in torch
ops on plain indexing and torch.where -- run in float64 they are the reference, torch.autograd gives the reference gradient,
and run in float32 they give the error a straightforward fp32 composition makes on the same inputs -- and the builders of the
inputs.  Not a test file; tests/test_host_unsup.py validates it without a GPU (finite differences, the builder's guarantees).
"""
import functools

import numpy as np
import torch


def rho(d, eps, q):
    """Generalised Charbonnier (d^2 + eps^2)^q."""
    return (d * d + eps * eps) ** q


def photometric_ref(im0, im1, flow, flow_scale=1.0, valid=None, eps=1e-3, q=0.5):
    """(sums (N,), counts (N,) int64, contributing (N,H,W) bool) in the dtype of the inputs.  Pixels that do not contribute are
    selected out BEFORE any arithmetic (their flow, their images_0 pixel and their four samples are replaced by 0), so that NaN
    there reaches neither a sum nor, through 0 * NaN, a gradient."""
    N, H, W, C = im0.shape
    dt = flow.dtype
    zero = torch.zeros((), dtype=dt)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    m = torch.ones((N, H, W), dtype=torch.bool) if valid is None else valid.bool()
    fl = torch.where(m.unsqueeze(3), flow, zero)
    px, py = xs + flow_scale * fl[..., 0], ys + flow_scale * fl[..., 1]
    inside = m & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    px, py = torch.where(inside, px, zero), torch.where(inside, py, zero)
    fx0, fy0 = torch.floor(px).detach(), torch.floor(py).detach()
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    wx, wy = (px - fx0).unsqueeze(3), (py - fy0).unsqueeze(3)
    n = torch.arange(N).reshape(N, 1, 1).expand(N, H, W)
    sel = inside.unsqueeze(3)
    v00, v01 = torch.where(sel, im1[n, y0, x0], zero), torch.where(sel, im1[n, y0, x1], zero)
    v10, v11 = torch.where(sel, im1[n, y1, x0], zero), torch.where(sel, im1[n, y1, x1], zero)
    warped = (1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11)
    d = torch.where(sel, im0, zero) - warped
    term = torch.where(inside, rho(d, eps, q).sum(3), zero)
    return term.sum(dim=(1, 2)), inside.sum(dim=(1, 2)), inside


def smoothness_ref(flow, image=None, alpha=10.0, eps=1e-3, q=0.5):
    """sums (N,): forward differences of the flow along x and y, weighted by exp(-alpha * mean_c |image difference|)."""
    dx, dy = flow[:, :, 1:] - flow[:, :, :-1], flow[:, 1:] - flow[:, :-1]
    tx, ty = rho(dx, eps, q).sum(3), rho(dy, eps, q).sum(3)
    if image is not None:
        tx = tx * torch.exp(-alpha * (image[:, :, 1:] - image[:, :, :-1]).abs().mean(3))
        ty = ty * torch.exp(-alpha * (image[:, 1:] - image[:, :-1]).abs().mean(3))
    return tx.sum(dim=(1, 2)) + ty.sum(dim=(1, 2))


# ------------------------------------------------------------------ inputs
def build_case(N, H, W, C, flow_scale=1.0, seed=0, masked=True, empty=None, eps=1e-3, block=5, max_off=3, far=0.25):
    """Inputs of one case, numpy float32 (the mask bool, or None):

      flow       (N,H,W,2), in units of 1 / flow_scale px: flow_scale * flow = integer field + frac, frac uniform in
                 [0.1, 0.9] per component (drawn 1e-3 inside the ends: the division by flow_scale rounds), so that every
                 sample coordinate keeps 0.1 from the integers -- the frame border and the kinks of floor.  The integer field is
                 constant on block x block tiles (small and large differences for the smoothness term): the share `far` of
                 the tiles is thrown out of the frame, the others move by up to max_off px.
      im1        uniform noise; im0: noise, and at ~30 % of the pixels the float64 sample of im1 plus up to 3 eps -- the small
                 differences at which rho' magnifies rounding errors.
      valid      ~70 % True.  empty: the index of an image whose EVERY tile is thrown out (no pixel of it contributes).
      flow_nan, im0_nan, im1_nan   the same with NaN at the invalid pixels (im1: at those no contributing pixel samples).

    Asserted here, on the CPU, so that a test cannot pass by leaving cases out: the distance of every sample coordinate of a
    valid pixel to the nearest integer is >= 0.1; between 10 % and 40 % of the pixels (of the images other than `empty`) are out
    of frame; every image but `empty` has a contributing pixel and `empty` has none."""
    rs = np.random.RandomState(seed)
    th, tw = -(-H // block), -(-W // block)
    off = rs.randint(-max_off, max_off + 1, size=(N, th, tw, 2)).astype(np.float64)
    out = rs.uniform(size=(N, th, tw)) < far
    if empty is not None:
        out[empty] = True
    thrown = np.zeros((N, th, tw, 2))
    axis = rs.randint(0, 2, size=(N, th, tw))
    sign = rs.choice([-1.0, 1.0], size=(N, th, tw))
    thrown[..., 0] = np.where(axis == 0, sign * (W + 2), 0.0)
    thrown[..., 1] = np.where(axis == 1, sign * (H + 2), 0.0)
    off = np.where(out[..., None], thrown, off)
    integer = np.kron(off, np.ones((1, block, block, 1)))[:, :H, :W]
    frac = 0.1 + 0.8 * rs.uniform(1e-3, 1 - 1e-3, size=(N, H, W, 2))
    flow = ((integer + frac) / flow_scale).astype(np.float32)
    valid = (rs.uniform(size=(N, H, W)) < 0.7) if masked else None

    # the coordinates the kernels see: the stored fp32 flow times flow_scale
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    px, py = xs + np.float64(np.float32(flow_scale)) * flow[..., 0], ys + np.float64(np.float32(flow_scale)) * flow[..., 1]
    for c in (px, py):
        assert float(np.abs(c - np.round(c)).min()) >= 0.1, "a sample coordinate closer than 0.1 to an integer"
    oof = ~((px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1))
    keep = [n for n in range(N) if n != empty]
    share = float(oof[keep].mean())
    assert 0.10 <= share <= 0.40, f"{share:.3f} of the pixels out of frame"
    contributing = ~oof if valid is None else (~oof & valid)
    for n in range(N):
        assert bool(contributing[n].any()) == (n != empty), (n, empty)

    im1 = rs.uniform(0, 1, size=(N, H, W, C)).astype(np.float32)
    im0 = rs.uniform(0, 1, size=(N, H, W, C)).astype(np.float32)
    x0, y0 = np.clip(np.floor(px), 0, W - 1).astype(np.int64), np.clip(np.floor(py), 0, H - 1).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    n_idx = np.arange(N).reshape(N, 1, 1) + np.zeros((N, H, W), np.int64)
    wx, wy = (px - np.floor(px))[..., None], (py - np.floor(py))[..., None]
    i64 = im1.astype(np.float64)
    warped = (1 - wy) * ((1 - wx) * i64[n_idx, y0, x0] + wx * i64[n_idx, y0, x1]) + \
        wy * ((1 - wx) * i64[n_idx, y1, x0] + wx * i64[n_idx, y1, x1])
    near = contributing & (rs.uniform(size=(N, H, W)) < 0.3)
    im0[near] = (warped[near] + rs.uniform(-3 * eps, 3 * eps, size=(int(near.sum()), C))).astype(np.float32)

    case = {"N": N, "H": H, "W": W, "C": C, "flow_scale": float(flow_scale), "im0": im0, "im1": im1, "flow": flow,
            "valid": valid, "contributing": contributing, "empty": empty}
    flow_nan, im0_nan, im1_nan = flow.copy(), im0.copy(), im1.copy()
    if valid is not None:
        sampled = np.zeros((N, H, W), bool)
        for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
            sampled[n_idx[contributing], yy[contributing], xx[contributing]] = True
        flow_nan[~valid] = np.nan
        im0_nan[~valid] = np.nan
        im1_nan[~valid & ~sampled] = np.nan
        assert np.isnan(im1_nan).any() and np.isnan(flow_nan).any()
    case.update(flow_nan=flow_nan, im0_nan=im0_nan, im1_nan=im1_nan)
    return case


# The cases of tests/test_gpu_unsup.py: name -> (build_case arguments, (eps, q)).  23 x 37: odd sizes, tail lanes, 4 parts;
# 272 x 256: 272 > 256 parts of an image, so the grid-stride loop and the capped partition run.  C in {1, 3, 4}, flow_scale in
# {1, 20 / 4}, both (eps, q) pairs, masks (with NaN behind them) and no mask, one image that contributes nothing.
CASES = {
    "23x37_c3_s1": (dict(N=2, H=23, W=37, C=3, flow_scale=1.0, seed=1), (1e-3, 0.5)),
    "23x37_c1_s5_empty": (dict(N=2, H=23, W=37, C=1, flow_scale=5.0, seed=2, empty=1, eps=1e-2), (1e-2, 0.45)),
    "23x37_c4_s1_nomask": (dict(N=2, H=23, W=37, C=4, flow_scale=1.0, seed=3, masked=False, eps=1e-2), (1e-2, 0.45)),
    "272x256_c4_s5": (dict(N=2, H=272, W=256, C=4, flow_scale=5.0, seed=4), (1e-3, 0.5)),
    "272x256_c3_s1_nomask": (dict(N=2, H=272, W=256, C=3, flow_scale=1.0, seed=5, masked=False, eps=1e-2), (1e-2, 0.45)),
}
UPSTREAM = (0.75, -1.5)        # the gradient that reaches sums[n] (N = 2): per image, of both signs
ALPHA = 10.0


def _t(a, dt):
    return torch.from_numpy(a).to(dt)


def _photo_run(case, eps, q, dt):
    flow = _t(case["flow"], dt).requires_grad_(True)
    valid = None if case["valid"] is None else torch.from_numpy(case["valid"])
    sums, counts, _ = photometric_ref(_t(case["im0"], dt), _t(case["im1"], dt), flow, case["flow_scale"], valid, eps, q)
    (sums * torch.tensor(UPSTREAM, dtype=dt)).sum().backward()
    return sums.detach(), counts, flow.grad


def _smooth_run(case, eps, q, dt, with_image):
    flow = _t(case["flow"], dt).requires_grad_(True)
    sums = smoothness_ref(flow, _t(case["im0"], dt) if with_image else None, ALPHA, eps, q)
    (sums * torch.tensor(UPSTREAM, dtype=dt)).sum().backward()
    return sums.detach(), flow.grad


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, its float64 reference (sums, counts, gradient of sum_n UPSTREAM[n] * sums[n] w.r.t. the flow) and the same
    formulas run in float32 -- computed once per process and shared; treat it as read-only."""
    kw, (eps, q) = CASES[name]
    case = build_case(**kw)
    ref = {"case": case, "eps": eps, "q": q}
    ref["photo64"], ref["photo32"] = _photo_run(case, eps, q, torch.float64), _photo_run(case, eps, q, torch.float32)
    for key, img in (("smooth", True), ("smooth_noimg", False)):
        ref[key + "64"], ref[key + "32"] = _smooth_run(case, eps, q, torch.float64, img), _smooth_run(case, eps, q, torch.float32, img)
    return ref
