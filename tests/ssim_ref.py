"""Yardstick of the SSIM term (pwcnet_amd/unsup.py ssim_*, csrc/pwc_ssim.hip): its restatement in torch ops on plain indexing
(shifted slices, torch.where) -- run in float64 it is the reference and torch.autograd gives the reference gradient, run in
float32 it gives the error a straightforward fp32 composition makes on the same inputs -- the closed form of the gradient with
respect to the warped frame (the alpha / beta / gamma split that the gather kernel implements), and the table of the GPU tests'
cases, built from tests.unsup_ref.build_case.  Not a test file; tests/test_host_ssim.py validates it without a GPU (finite
differences, closed form against autograd, the cases' guarantees).

Definition.  x = images_0; y(p, c) = the photometric term's bilinear sample of images_1 at p moved by flow_scale * flow[p] (in
frame iff 0 <= px <= W - 1 and 0 <= py <= H - 1; a flow that is not finite is out of frame).  Per channel, over the n = (2r+1)^2
pixels of the window of centre p, centred:
    mu_x = mean x, mu_y = mean y, s_x = mean (x - mu_x)^2, s_y = mean (y - mu_y)^2, s_xy = mean (x - mu_x)(y - mu_y),
    SSIM = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_x + s_y + c2)),  term(p, c) = (1 - SSIM) / 2.
A centre contributes iff it is r from every border, valid, and EVERY pixel of its window is in frame.
"""
import functools

import torch

from tests import census_ref as cr
from tests import unsup_ref as ur

C1, C2 = 0.01 ** 2, 0.03 ** 2
nonfinite_flow = cr.nonfinite_flow          # NaN, +Inf and -Inf at ~6 % of the pixels (a seeded set): those pixels are out of frame


def warped(im1, flow, flow_scale=1.0):
    """(y (N,H,W,C), inside (N,H,W) bool): the bilinear sample of im1 at the pixel moved by flow_scale * flow where the sample
    point is inside the frame (photometric_ref's test, floor, corners and weights) and 0 elsewhere.  A pixel whose flow is not
    finite is out of frame; it is selected out BEFORE any arithmetic, so that it reaches neither y nor, through 0 * NaN, a
    gradient."""
    N, H, W, C = im1.shape
    dt, dev = flow.dtype, flow.device
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
    y = (1 - wy) * ((1 - wx) * im1[n, y0, x0] + wx * im1[n, y0, x1]) + wy * ((1 - wx) * im1[n, y1, x0] + wx * im1[n, y1, x1])
    return torch.where(inside.unsqueeze(3), y, zero), inside


def offsets(radius):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]


def _shift(t, r, dy, dx):
    H, W = t.shape[1:3]
    return t[:, r + dy:H - r + dy, r + dx:W - r + dx]


def window_stats(x, y, radius, c1=C1, c2=C2):
    """(mu_x, mu_y, A1, A2, B1, B2) at the pixels `radius` from every border, each (N, H - 2 radius, W - 2 radius, C)."""
    r, n = radius, len(offsets(radius))
    mux = sum(_shift(x, r, dy, dx) for dy, dx in offsets(r)) / n
    muy = sum(_shift(y, r, dy, dx) for dy, dx in offsets(r)) / n
    sx = sy = sxy = 0
    for dy, dx in offsets(r):
        ex, ey = _shift(x, r, dy, dx) - mux, _shift(y, r, dy, dx) - muy
        sx, sy, sxy = sx + ex * ex, sy + ey * ey, sxy + ex * ey
    return mux, muy, 2 * mux * muy + c1, 2 * (sxy / n) + c2, mux * mux + muy * muy + c1, sx / n + sy / n + c2


def window_terms(x, y, radius, c1=C1, c2=C2):
    """(1 - SSIM) / 2 per interior centre and channel, (N, H - 2 radius, W - 2 radius, C); H, W > 2 radius."""
    _, _, A1, A2, B1, B2 = window_stats(x, y, radius, c1, c2)
    return (1 - A1 * A2 / (B1 * B2)) / 2


def centres(inside, valid, radius):
    """(N,H,W) bool: the contributing centres -- `radius` from every border, valid, every pixel of the window in frame."""
    N, H, W = inside.shape
    r = radius
    out = torch.zeros((N, H, W), dtype=torch.bool, device=inside.device)
    if H > 2 * r and W > 2 * r:
        whole = torch.ones((N, H - 2 * r, W - 2 * r), dtype=torch.bool, device=inside.device)
        for dy, dx in offsets(r):
            whole = whole & _shift(inside, r, dy, dx)
        out[:, r:H - r, r:W - r] = whole if valid is None else whole & valid.bool()[:, r:H - r, r:W - r]
    return out


def sums_from_planes(x, y, contributing, radius, c1=C1, c2=C2):
    N, H, W, C = x.shape
    r = radius
    if not (H > 2 * r and W > 2 * r):
        return (y * 0).sum(dim=(1, 2, 3))
    term = torch.where(contributing[:, r:H - r, r:W - r].unsqueeze(3), window_terms(x, y, r, c1, c2),
                       torch.zeros((), dtype=y.dtype, device=y.device))
    return term.sum(dim=(1, 2, 3))


def ssim_ref(im0, im1, flow, flow_scale=1.0, valid=None, radius=1, c1=C1, c2=C2):
    """(sums (N,), counts (N,) int64, contributing (N,H,W) bool) in the dtype and on the device of the inputs."""
    y, inside = warped(im1, flow, flow_scale)
    contributing = centres(inside, valid, radius)
    return sums_from_planes(im0, y, contributing, radius, c1, c2), contributing.sum(dim=(1, 2)), contributing


def closed_form_dLdy(x, y, contributing, upstream, radius, c1=C1, c2=C2):
    """dL/dy of L = sum_n upstream[n] * sums[n], (N,H,W,C), by the formula the kernels implement: per contributing centre p
        beta_p = (2/n) A1 / (B1 B2),  gamma_p = -(2/n) S / B2,
        alpha_p = (2/n) (mu_x A2 / (B1 B2) - S mu_y / B1) - beta_p mu_x - gamma_p mu_y,
    so that dS/dy_q = alpha_p + beta_p x_q + gamma_p y_q for q in the window of p, and
        dL/dy(q) = -1/2 upstream[n] (sum_p alpha_p + x_q sum_p beta_p + y_q sum_p gamma_p)   over the centres within r of q."""
    N, H, W, C = x.shape
    r, n = radius, len(offsets(radius))
    out = torch.zeros_like(y)
    if not (H > 2 * r and W > 2 * r):
        return out
    mux, muy, A1, A2, B1, B2 = window_stats(x, y, r, c1, c2)
    S = A1 * A2 / (B1 * B2)
    u = -0.5 * upstream.reshape(N, 1, 1, 1) / n
    beta, gamma = u * 2 * A1 / (B1 * B2), -u * 2 * S / B2
    alpha = u * (2 * mux * A2 / (B1 * B2) - 2 * S * muy / B1) - beta * mux - gamma * muy
    sel = contributing[:, r:H - r, r:W - r].unsqueeze(3)
    zero = torch.zeros((), dtype=y.dtype, device=y.device)
    box = []
    for coef in (alpha, beta, gamma):
        # the interior plane, zero where the centre does not contribute, padded by 2 r: the box sum of the centres within r of q
        plane = torch.nn.functional.pad(torch.where(sel, coef, zero), (0, 0, 2 * r, 2 * r, 2 * r, 2 * r))
        box.append(sum(plane[:, r + dy:r + dy + H, r + dx:r + dx + W] for dy, dx in offsets(r)))
    return box[0] + x * box[1] + y * box[2]


# ------------------------------------------------------------------ the cases of tests/test_gpu_ssim.py
# name -> (build_case arguments, radius, low contrast).  23 x 37: odd sizes, tile seams in both directions (32 x 8 tiles);
# 272 x 256: 272 tiles, more than the 256 parts of an image, so parts take a second tile; 5 x 9 at radius 3: no interior,
# everything is zero.  radius in {1, 2, 3}, C in {1, 3, 4}, flow_scale in {1, 5}, masked and not, one image that contributes
# nothing, one low-contrast pair (both images remapped to 0.5 + 0.05 (im - 0.5): c2 dominates the variances, the coefficients of
# the gradient grow to ~1 / (n c2) and cancel).  For radius >= 2 the flow is constant on 8 x 8 blocks of which 15 % are thrown out
# of frame: under the whole-window rule build_case's defaults (5 x 5, 25 %) leave 3-9 % of the interior at 23 x 37, radius 3.
# The seeds are those at which build_case's own assertions and reference()'s hold.
_WIDE = dict(block=8, far=0.15)
CASES = {
    "23x37_r1_c3_s1": (dict(N=2, H=23, W=37, C=3, flow_scale=1.0, seed=1), 1, False),
    "23x37_r2_c1_s5_empty": (dict(N=2, H=23, W=37, C=1, flow_scale=5.0, seed=2, empty=1, eps=1e-2, **_WIDE), 2, False),
    "23x37_r3_c4_s1_nomask": (dict(N=2, H=23, W=37, C=4, flow_scale=1.0, seed=3, masked=False, eps=1e-2, **_WIDE), 3, False),
    "23x37_r1_c3_s5_lowcontrast": (dict(N=2, H=23, W=37, C=3, flow_scale=5.0, seed=6), 1, True),
    "272x256_r3_c4_s5": (dict(N=2, H=272, W=256, C=4, flow_scale=5.0, seed=4, **_WIDE), 3, False),
    "272x256_r1_c3_s1_nomask": (dict(N=2, H=272, W=256, C=3, flow_scale=1.0, seed=5, masked=False, eps=1e-2), 1, False),
    "5x9_r3_c3_s1": (dict(N=2, H=5, W=9, C=3, flow_scale=1.0, seed=0, masked=False, **_WIDE), 3, False),
}


def build(name):
    kw_case, radius, low = CASES[name]
    case = ur.build_case(**kw_case)
    if low:
        for k in ("im0", "im1"):
            case[k] = (0.5 + 0.05 * (case[k].astype("float64") - 0.5)).astype("float32")
    return case, radius


def _t(a, dt):
    return torch.from_numpy(a).to(dt)


def run(case, radius, dt, flow=None):
    """(sums, counts, gradient of sum_n UPSTREAM[n] * sums[n] w.r.t. the flow, contributing) of ssim_ref in dtype dt."""
    fl = _t(case["flow"] if flow is None else flow, dt).requires_grad_(True)
    valid = None if case["valid"] is None else torch.from_numpy(case["valid"])
    sums, counts, contributing = ssim_ref(_t(case["im0"], dt), _t(case["im1"], dt), fl, case["flow_scale"], valid, radius)
    (sums * torch.tensor(ur.UPSTREAM, dtype=dt)).sum().backward()
    return sums.detach(), counts, fl.grad, contributing


def near(contributing, radius):
    """Pixels with a contributing centre within `radius` (themselves included)."""
    return torch.nn.functional.max_pool2d(contributing[:, None].double(), 2 * radius + 1, 1, radius)[:, 0] > 0


def interior_share(case, contributing, radius, n):
    """The share of image n's interior that contributes."""
    return float(contributing[n].sum()) / ((case["H"] - 2 * radius) * (case["W"] - 2 * radius))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, its float64 reference (run64: sums, counts, gradient, contributing; inside: the in-frame pixels) and the same
    formulas run in float32 -- computed once per process and shared; treat it as read-only.  Asserted here, on the CPU, so that a
    case cannot pass by being empty (build_case asserts the 10-40 % of out-of-frame pixels itself): every image with an interior
    other than `empty` has at least 10 % of its interior contributing, `empty` has none, at least 5 % of the pixels carry a
    reference gradient above 1e-3 of the largest, and every per-pixel term of the reference lies in [-1e-9, 1 + 1e-9]."""
    case, r = build(name)
    ref = {"case": case, "radius": r, "run64": run(case, r, torch.float64), "run32": run(case, r, torch.float32)}
    x, im1, fl = (_t(case[k], torch.float64) for k in ("im0", "im1", "flow"))
    y, ref["inside"] = warped(im1, fl, case["flow_scale"])
    _, counts, grad, contributing = ref["run64"]
    ref["shares"] = []
    if case["H"] > 2 * r and case["W"] > 2 * r:
        terms = window_terms(x, y, r)[contributing[:, r:case["H"] - r, r:case["W"] - r]]
        ref["term_range"] = (float(terms.min()), float(terms.max()))
        assert -1e-9 <= ref["term_range"][0] and ref["term_range"][1] <= 1 + 1e-9, (name, ref["term_range"])
        for n in range(case["N"]):
            share = interior_share(case, contributing, r, n)
            ref["shares"].append(share)
            assert (share == 0.0) if n == case["empty"] else (share >= 0.10), (name, n, share)
        keep = [n for n in range(case["N"]) if n != case["empty"]]
        mag = grad[keep].abs().amax(dim=3)
        share = float((mag > 1e-3 * float(mag.max())).double().mean())
        assert share >= 0.05, f"{name}: {share:.3f} of the pixels carry a gradient"
        ref["grad_share"] = share
    else:
        assert not bool(counts.any()) and not bool(grad.any())
        ref["grad_share"], ref["term_range"] = 0.0, (0.0, 0.0)
    return ref
