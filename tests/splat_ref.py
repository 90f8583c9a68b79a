"""Yardstick of forward splatting (pwcnet_amd/splat.py, csrc/pwc_splat.hip): the float64 torch restatement -- index_add over the
four corners, the same in-frame rules, differentiable by torch.autograd -- the explicit float64 gradient formulas with the sum of
the absolute values of every element's terms (the scale of the GPU tests' gradient bound), and the inputs of the GPU tests.
tests/test_host_splat.py validates all of it without a GPU: hand-computed cases, the explicit gradients against autograd, and
the conditions on the inputs that the GPU tests rely on."""
import functools

import numpy as np
import torch


def _scale(flow_scale):
    """flow_scale as the library receives it: a float32."""
    return float(np.float32(flow_scale))


def _cells(flow, valid, flow_scale):
    """Per source pixel: contributes (bool), x0, y0 (int64), wx, wy (float64; 0 where the pixel does not contribute)."""
    N, H, W, _ = flow.shape
    s = _scale(flow_scale)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    px = xs + s * flow[..., 0].double()
    py = ys + s * flow[..., 1].double()
    ok = (px > -1) & (px < W) & (py > -1) & (py < H)                   # (False for a NaN)
    if valid is not None:
        ok = ok & valid.bool()
    px = torch.where(ok, px, torch.zeros_like(px))
    py = torch.where(ok, py, torch.zeros_like(py))
    fx0, fy0 = torch.floor(px.detach()), torch.floor(py.detach())
    return ok, fx0.long(), fy0.long(), px - fx0, py - fy0


def _corners(ok, x0, y0, wx, wy, H, W):
    """The four corners: (inside (bool), flat target index (clamped where not inside), b, db/dpx, db/dpy)."""
    N = ok.shape[0]
    img = torch.arange(N).view(N, 1, 1) * (H * W)
    for k in range(4):
        dx, dy = k & 1, k >> 1
        cx, cy = x0 + dx, y0 + dy
        inside = ok & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        t = img + cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)
        ax, ay = (wx if dx else 1 - wx), (wy if dy else 1 - wy)
        yield inside, t, ax * ay, (1.0 if dx else -1.0) * ay, (1.0 if dy else -1.0) * ax


def splat_ref(x, flow, w=None, valid=None, flow_scale=1.0, mode="sum"):
    """(out (N,H,W,C) float64 or None, coverage (N,H,W) float64, cnt (N,H,W) int64): the number of contributions per target."""
    N, H, W, _ = flow.shape
    ok, x0, y0, wx, wy = _cells(flow, valid, flow_scale)
    C = 0 if x is None else x.shape[3]
    wt = torch.ones((N, H, W), dtype=torch.float64) if w is None else w.double()
    num = torch.zeros((N * H * W, C), dtype=torch.float64)
    den = torch.zeros((N * H * W,), dtype=torch.float64)
    cnt = torch.zeros((N * H * W,), dtype=torch.int64)
    for inside, t, b, _, _ in _corners(ok, x0, y0, wx, wy, H, W):
        sel, idx = inside.reshape(-1), t.reshape(-1)
        idx = idx[sel]
        bw = (b * wt).reshape(-1)[sel]
        den = den.index_add(0, idx, bw)
        cnt = cnt.index_add(0, idx, torch.ones_like(idx))
        if C:
            num = num.index_add(0, idx, bw[:, None] * x.double().reshape(-1, C)[sel])
    den, cnt = den.view(N, H, W), cnt.view(N, H, W)
    if not C:
        return None, den, cnt
    num = num.view(N, H, W, C)
    if mode == "average":
        pos = (den > 0)[..., None]
        num = torch.where(pos, num / torch.where(den > 0, den, torch.ones_like(den))[..., None], torch.zeros_like(num))
    elif mode != "sum":
        raise ValueError(mode)
    return num, den, cnt


def splat_grads_ref(x, flow, w, valid, flow_scale, mode, g_out, g_cov):
    """The gradient of (g_out * out).sum() + (g_cov * coverage).sum() by the explicit formulas (include/pwc_hip.h), float64:
    ((dx, dw, dflow), (A_dx, A_dw, A_dflow)), A the sum of the absolute values of the element's terms.  x None: dx, A_dx None."""
    N, H, W, _ = flow.shape
    s = _scale(flow_scale)
    with torch.no_grad():
        ok, x0, y0, wx, wy = _cells(flow, valid, flow_scale)
        C = 0 if x is None else x.shape[3]
        wt = torch.ones((N, H, W), dtype=torch.float64) if w is None else w.double()
        xd = torch.zeros((N, H, W, 0), dtype=torch.float64) if x is None else x.double()
        g = torch.zeros((N, H, W, C), dtype=torch.float64) if g_out is None else g_out.double()
        gc = torch.zeros((N, H, W), dtype=torch.float64) if g_cov is None else g_cov.double()
        ga, gca = g.abs(), gc.abs()
        if mode == "average":
            out, den, _ = splat_ref(x, flow, w, valid, flow_scale, "average")
            pos = den > 0
            inv = torch.where(pos, 1.0 / torch.where(pos, den, torch.ones_like(den)), torch.zeros_like(den))[..., None]
            g, ga = g * inv, ga * inv
            gc = gc - (out * g).sum(-1)
            gca = gca + (out.abs() * ga).sum(-1)
        g, ga, gc, gca = g.reshape(N * H * W, C), ga.reshape(N * H * W, C), gc.reshape(-1), gca.reshape(-1)
        S, Sx, Sy = (torch.zeros((N, H, W, C), dtype=torch.float64) for _ in range(3))
        Sa, Sxa, Sya = (torch.zeros((N, H, W, C), dtype=torch.float64) for _ in range(3))
        T, Tx, Ty, Ta, Txa, Tya = (torch.zeros((N, H, W), dtype=torch.float64) for _ in range(6))
        for inside, t, b, bx, by in _corners(ok, x0, y0, wx, wy, H, W):
            m = inside.double()
            b, bx, by = b * m, bx * m, by * m
            gk, gka = g[t.reshape(-1)].view(N, H, W, C), ga[t.reshape(-1)].view(N, H, W, C)
            ck, cka = gc[t.reshape(-1)].view(N, H, W), gca[t.reshape(-1)].view(N, H, W)
            S += b[..., None] * gk; Sx += bx[..., None] * gk; Sy += by[..., None] * gk
            Sa += b[..., None] * gka; Sxa += bx.abs()[..., None] * gka; Sya += by.abs()[..., None] * gka
            T += b * ck; Tx += bx * ck; Ty += by * ck
            Ta += b * cka; Txa += bx.abs() * cka; Tya += by.abs() * cka
        dx = wt[..., None] * S if C else None
        a_dx = wt.abs()[..., None] * Sa if C else None
        dw = (xd * S).sum(-1) + T
        a_dw = (xd.abs() * Sa).sum(-1) + Ta
        dflow = torch.stack([s * wt * ((xd * Sx).sum(-1) + Tx), s * wt * ((xd * Sy).sum(-1) + Ty)], dim=-1)
        a_dflow = torch.stack([abs(s) * wt.abs() * ((xd.abs() * Sxa).sum(-1) + Txa),
                               abs(s) * wt.abs() * ((xd.abs() * Sya).sum(-1) + Tya)], dim=-1)
    return (dx, dw, dflow), (a_dx, a_dw, a_dflow), ok


def autograd_grads(x, flow, w, valid, flow_scale, mode, g_out, g_cov):
    """The same gradient by torch.autograd on splat_ref, float64."""
    xd = None if x is None else x.double().requires_grad_(True)
    fd = flow.double().requires_grad_(True)
    wd = (torch.ones(flow.shape[:3], dtype=torch.float64) if w is None else w.double()).requires_grad_(True)
    out, cov, _ = splat_ref(xd, fd, wd, valid, flow_scale, mode)
    total = (cov * g_cov.double()).sum() if g_cov is not None else cov.sum() * 0
    if out is not None and g_out is not None:
        total = total + (out * g_out.double()).sum()
    total.backward()
    return (None if xd is None else xd.grad), wd.grad, fd.grad


# ------------------------------------------------------------------ the inputs of the GPU tests
# name: (N, H, W, C, amplitude of the smooth flow in px).  Frames (2, 9, 13) and (2, 24, 40); C in {1, 3, 5}.
CASES = {"9x13_c1": (2, 9, 13, 1, 2.0), "9x13_c3": (2, 9, 13, 3, 2.0), "24x40_c3": (2, 24, 40, 3, 6.0),
         "24x40_c5": (2, 24, 40, 5, 6.0)}
FLOW_SCALE = 1.0
MIN_DEN = 2.0 ** -10          # the average mode is compared where the reference denominator is at least this
MIN_DEN_GRAD = 2.0 ** -6      # ... and the average mode's gradient inputs keep every positive denominator above this


def smooth_flow(N, H, W, amp, seed):
    """A smooth flow of amplitude ~amp px (a rotation-like field, different per image) plus +-0.3 px of noise, float32."""
    rs = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flow = np.empty((N, H, W, 2))
    for n in range(N):
        ph = 0.7 * n + 0.3
        flow[n, ..., 0] = amp * np.sin(2 * np.pi * y / H + ph) * np.cos(np.pi * x / W - ph)
        flow[n, ..., 1] = amp * np.cos(2 * np.pi * x / W - ph) * np.sin(np.pi * y / H + 2 * ph)
    flow += rs.uniform(-0.3, 0.3, size=flow.shape)
    return flow.astype(np.float32)


def mid_cell_flow(flow, lo=0.2, hi=0.8):
    """The flow with every target point's fractional parts moved into [lo, hi]: every bilinear weight is then at least lo^2."""
    N, H, W, _ = flow.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = flow.astype(np.float64).copy()
    for c, grid in ((0, x), (1, y)):
        p = grid + out[..., c]
        f = np.floor(p)
        out[..., c] = f + np.clip(p - f, lo + 1e-3, hi - 1e-3) - grid
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case, torch float32 on the CPU: x in [0, 1], w in [0.5, 2], the flow, the flow for the gradient tests of
    the average mode, random upstream gradients."""
    N, H, W, C, amp = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    flow = smooth_flow(N, H, W, amp, rs.randint(1 << 30))
    c = dict(name=name, N=N, H=H, W=W, C=C,
             x=torch.from_numpy(rs.uniform(0, 1, (N, H, W, C)).astype(np.float32)),
             w=torch.from_numpy(rs.uniform(0.5, 2, (N, H, W)).astype(np.float32)),
             flow=torch.from_numpy(flow), flow_mid=torch.from_numpy(mid_cell_flow(flow)),
             flow_bw=torch.from_numpy(smooth_flow(N, H, W, amp, rs.randint(1 << 30))),
             g_out=torch.from_numpy(rs.uniform(-1, 1, (N, H, W, C)).astype(np.float32)),
             g_cov=torch.from_numpy(rs.uniform(-1, 1, (N, H, W)).astype(np.float32)))
    return c


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """(out, coverage, cnt) of the case, float64, computed once and shared."""
    c = case(name)
    with torch.no_grad():
        return splat_ref(c["x"], c["flow"], c["w"], None, FLOW_SCALE, mode)


@functools.lru_cache(maxsize=None)
def grad_reference(name, mode):
    """splat_grads_ref of the case (the average mode on flow_mid), float64, computed once and shared."""
    c = case(name)
    flow = c["flow_mid"] if mode == "average" else c["flow"]
    return splat_grads_ref(c["x"], flow, c["w"], None, FLOW_SCALE, mode, c["g_out"], c["g_cov"])


def left_frame_share(flow, flow_scale=1.0):
    ok = _cells(flow, None, flow_scale)[0]
    return 1.0 - float(ok.double().mean())
