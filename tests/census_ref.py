"""Yardstick of the soft census term (pwcnet_amd/unsup.py census_*, csrc/pwc_census.hip): its restatement in torch ops on plain
indexing and torch.where -- run in float64 it is the reference and torch.autograd gives the reference gradient, run in float32 it
gives the error a straightforward fp32 composition makes on the same inputs -- the closed form of the gradient with respect to
the warped grey plane, and the table of the GPU tests' cases, built from tests.unsup_ref.build_case.  Not a test file;
tests/test_host_census.py validates it without a GPU (finite differences, closed form against autograd, the cases' guarantees).
"""
import functools

import numpy as np
import torch

from tests import unsup_ref as ur


def tau(t, c1):
    return t / torch.sqrt(c1 + t * t)


def grey_planes(im0, im1, flow, flow_scale=1.0, scale=255.0):
    """(a, b, inside): a = scale * mean_c im0, b = scale * mean_c (bilinear sample of im1 at the pixel moved by flow_scale *
    flow) where the sample point is inside the frame (photometric_ref's test, floor, corners and weights) and 0 elsewhere, each
    (N,H,W).  A pixel whose flow is not finite is out of frame; it is selected out BEFORE any arithmetic, so that it reaches
    neither b nor, through 0 * NaN, a gradient."""
    N, H, W, C = im0.shape
    dt = flow.dtype
    dev = flow.device
    zero = torch.zeros((), dtype=dt, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev), indexing="ij")
    finite = torch.isfinite(flow).all(dim=3)
    fl = torch.where(finite.unsqueeze(3), flow, zero)
    px, py = xs + flow_scale * fl[..., 0], ys + flow_scale * fl[..., 1]
    inside = finite & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    px, py = torch.where(inside, px, zero), torch.where(inside, py, zero)
    fx0, fy0 = torch.floor(px).detach(), torch.floor(py).detach()
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    wx, wy = (px - fx0).unsqueeze(3), (py - fy0).unsqueeze(3)
    n = torch.arange(N, device=dev).reshape(N, 1, 1).expand(N, H, W)
    warped = (1 - wy) * ((1 - wx) * im1[n, y0, x0] + wx * im1[n, y0, x1]) + wy * ((1 - wx) * im1[n, y1, x0] + wx * im1[n, y1, x1])
    b = torch.where(inside, scale * warped.mean(3), zero)
    return scale * im0.mean(3), b, inside


def offsets(radius):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def window_h(a, b, radius, c1, c2):
    """h at the pixels `radius` from every border, (N, H - 2 radius, W - 2 radius); H, W > 2 radius."""
    H, W = a.shape[1:]
    r = radius
    ac, bc = a[:, r:H - r, r:W - r], b[:, r:H - r, r:W - r]
    h = torch.zeros_like(ac)
    for dy, dx in offsets(r):
        t0 = a[:, r + dy:H - r + dy, r + dx:W - r + dx] - ac
        t1 = b[:, r + dy:H - r + dy, r + dx:W - r + dx] - bc
        d = (tau(t0, c1) - tau(t1, c1)) ** 2
        h = h + d / (c2 + d)
    return h / len(offsets(r))


def centres(inside, valid, radius):
    """(N,H,W) bool: the contributing pixels -- `radius` from every border, in frame, valid."""
    N, H, W = inside.shape
    r = radius
    out = torch.zeros((N, H, W), dtype=torch.bool, device=inside.device)
    if H > 2 * r and W > 2 * r:
        out[:, r:H - r, r:W - r] = (inside if valid is None else inside & valid.bool())[:, r:H - r, r:W - r]
    return out


def sums_from_planes(a, b, contributing, radius, c1, c2, eps, q):
    N, H, W = a.shape
    r = radius
    if not (H > 2 * r and W > 2 * r):
        return (b * 0).sum(dim=(1, 2))
    term = torch.where(contributing[:, r:H - r, r:W - r], ur.rho(window_h(a, b, r, c1, c2), eps, q),
                       torch.zeros((), dtype=a.dtype, device=a.device))
    return term.sum(dim=(1, 2))


def census_ref(im0, im1, flow, flow_scale=1.0, valid=None, radius=3, scale=255.0, c1=0.81, c2=0.1, eps=1e-2, q=0.4):
    """(sums (N,), counts (N,) int64, contributing (N,H,W) bool) in the dtype and on the device of the inputs.  The mask and the in-frame test
    select centres only: a neighbour is always read (b is 0 at an out-of-frame one)."""
    a, b, inside = grey_planes(im0, im1, flow, flow_scale, scale)
    contributing = centres(inside, valid, radius)
    return sums_from_planes(a, b, contributing, radius, c1, c2, eps, q), contributing.sum(dim=(1, 2)), contributing


def closed_form_dLdb(a, b, contributing, upstream, radius, c1, c2, eps, q):
    """dL/db of L = sum_n upstream[n] * sums[n], (N,H,W), by the formula the gather kernel implements:
        G(p) = upstream[n] rho'(h(p)) / K where p contributes, else 0
        D(t0, t1) = c2 / (c2 + d)^2 * 2 (tau(t1) - tau(t0)) * c1 / (c1 + t1^2)^(3/2)
        dL/db(q) = -sum_o (G(q) + G(q+o)) D(t0(q,o), t1(q,o))    over the offsets with q+o inside the image."""
    N, H, W = a.shape
    r = radius
    K = len(offsets(r))
    G = torch.zeros_like(a)
    if H > 2 * r and W > 2 * r:
        h = window_h(a, b, r, c1, c2)
        rho_grad = 2 * q * h * (h * h + eps * eps) ** (q - 1)
        G[:, r:H - r, r:W - r] = torch.where(contributing[:, r:H - r, r:W - r], upstream.reshape(N, 1, 1) * rho_grad / K,
                                             torch.zeros((), dtype=a.dtype, device=a.device))
    pad = torch.nn.functional.pad
    ap, bp, Gp = (pad(t, (r, r, r, r)) for t in (a, b, G))          # zeros outside the image: G = 0 there switches the term off
    out = torch.zeros_like(a)
    for dy, dx in offsets(r):
        sl = (slice(None), slice(r + dy, r + dy + H), slice(r + dx, r + dx + W))
        t0, t1 = ap[sl] - a, bp[sl] - b
        d = (tau(t0, c1) - tau(t1, c1)) ** 2
        D = c2 / (c2 + d) ** 2 * 2 * (tau(t1, c1) - tau(t0, c1)) * c1 / (c1 + t1 * t1) ** 1.5
        out = out - (G + Gp[sl]) * D
    return out


# ------------------------------------------------------------------ the cases of tests/test_gpu_census.py
# name -> (build_case arguments, census arguments).  23 x 37: odd sizes, tile seams in both directions (32 x 8 tiles), interior
# 17 x 31 at radius 3; 272 x 256: 272 tiles, more than the 256 parts of an image, so parts take a second tile; 5 x 9 at radius 3:
# no interior, everything is zero.  radius in {1, 2, 3}, C in {1, 3, 4}, scale in {255, 8}, flow_scale in {1, 5}, masked and not,
# one image that contributes nothing.  The seeds are those at which build_case's own assertions hold.
CASES = {
    "23x37_r3_c3_s1_k255": (dict(N=2, H=23, W=37, C=3, flow_scale=1.0, seed=1), dict(radius=3, scale=255.0)),
    "23x37_r1_c1_s5_k8_empty": (dict(N=2, H=23, W=37, C=1, flow_scale=5.0, seed=2, empty=1, eps=1e-2), dict(radius=1, scale=8.0)),
    "23x37_r2_c4_s1_k8_nomask": (dict(N=2, H=23, W=37, C=4, flow_scale=1.0, seed=3, masked=False, eps=1e-2),
                                 dict(radius=2, scale=8.0)),
    "272x256_r3_c4_s5_k255": (dict(N=2, H=272, W=256, C=4, flow_scale=5.0, seed=4), dict(radius=3, scale=255.0)),
    "272x256_r1_c3_s1_k8_nomask": (dict(N=2, H=272, W=256, C=3, flow_scale=1.0, seed=5, masked=False, eps=1e-2),
                                   dict(radius=1, scale=8.0)),
    "5x9_r3_c3_s1_k255": (dict(N=2, H=5, W=9, C=3, flow_scale=1.0, seed=0, masked=False), dict(radius=3, scale=255.0)),
}
CONSTS = dict(c1=0.81, c2=0.1, eps=1e-2, q=0.4)


def _t(a, dt):
    return torch.from_numpy(a).to(dt)


def run(case, kw, dt, flow=None):
    """(sums, counts, gradient of sum_n UPSTREAM[n] * sums[n] w.r.t. the flow, contributing) of census_ref in dtype dt."""
    fl = _t(case["flow"] if flow is None else flow, dt).requires_grad_(True)
    valid = None if case["valid"] is None else torch.from_numpy(case["valid"])
    sums, counts, contributing = census_ref(_t(case["im0"], dt), _t(case["im1"], dt), fl, case["flow_scale"], valid, **kw, **CONSTS)
    (sums * torch.tensor(ur.UPSTREAM, dtype=dt)).sum().backward()
    return sums.detach(), counts, fl.grad, contributing


def nonfinite_flow(case):
    """The case's flow with NaN, +Inf and -Inf at ~6 % of the pixels (a seeded set): those pixels are out of frame, b is 0 there."""
    rs = np.random.RandomState(77)
    flow = case["flow"].copy()
    hit = rs.uniform(size=flow.shape[:3]) < 0.06
    bad = rs.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=int(hit.sum()))
    flow[hit, 0] = bad
    flow[hit, 1] = np.where(rs.uniform(size=bad.shape) < 0.5, bad, flow[hit, 1])          # one bad component is enough
    return flow


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, its float64 reference (run64: sums, counts, gradient, contributing; inside: the in-frame pixels) and the same
    formulas run in float32 -- computed once per process and shared; treat it as
    read-only.  Asserted here, on the CPU, so that a case cannot pass by being empty (build_case asserts the 10-40 % of
    out-of-frame pixels itself): every image with an interior other than `empty` has contributing pixels, `empty` has none, and
    at least 5 % of the pixels carry a reference gradient above 1e-3 of the largest."""
    kw_case, kw = CASES[name]
    case = ur.build_case(**kw_case)
    ref = {"case": case, "kw": dict(kw), "run64": run(case, kw, torch.float64), "run32": run(case, kw, torch.float32)}
    ref["inside"] = grey_planes(_t(case["im0"], torch.float64), _t(case["im1"], torch.float64), _t(case["flow"], torch.float64),
                                case["flow_scale"], kw["scale"])[2]
    _, counts, grad, _ = ref["run64"]
    r = kw["radius"]
    if case["H"] > 2 * r and case["W"] > 2 * r:
        for n in range(case["N"]):
            assert (int(counts[n]) > 0) == (n != case["empty"]), (name, n, counts.tolist())
        keep = [n for n in range(case["N"]) if n != case["empty"]]
        mag = grad[keep].abs().amax(dim=3)
        share = float((mag > 1e-3 * float(mag.max())).double().mean())
        assert share >= 0.05, f"{name}: {share:.3f} of the pixels carry a gradient"
        ref["grad_share"] = share
    else:
        assert not bool(counts.any()) and not bool(grad.any())
        ref["grad_share"] = 0.0
    return ref
