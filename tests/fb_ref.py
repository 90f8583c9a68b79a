"""Yardstick of the forward-backward occlusion masks (pwcnet_amd/unsup.py fb_valid, csrc/pwc_fbcheck.hip): the restatement of the
check in float64 torch ops on plain indexing and torch.where, and the seeded cases of the GPU tests.  Not a test file;
tests/test_host_fbcheck.py validates it without a GPU (an analytic scene with known occlusions, the near-tie cap of every case).

The C entry takes flow_scale, alpha1 and alpha2 as `float`: the restatement rounds them to float32 first and computes everything
else in float64, as the kernel does.  A pixel's MARGIN is alpha1 (|f|^2 + |g|^2) + alpha2 - |f + g|^2; it is valid iff it passes
its input mask, its sample point is in frame and margin >= 0 (false for a NaN; an Inf in the sampled flow makes the margin
Inf - Inf = NaN).  Pixels that are masked out or out of frame report margin -inf."""
import collections
import functools

import numpy as np
import torch

# mask (N,H,W) bool; counts (N,) int64; margin, bound (N,H,W) float64: bound = alpha1 (|f|^2 + |g|^2) + alpha2, what a near-tie
# is measured against; candidate (N,H,W) bool: unmasked and in frame -- the pixels whose margin decides
Direction = collections.namedtuple("Direction", "mask counts margin bound candidate")
NEAR_TIE = 1e-9


def _direction(own, other, scale, alpha1, alpha2, valid):
    N, H, W, _ = own.shape
    dt = torch.float64
    zero = torch.zeros((), dtype=dt)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    m = torch.ones((N, H, W), dtype=torch.bool) if valid is None else valid != 0
    f = scale * torch.where(m.unsqueeze(3), own, zero)
    px, py = xs + f[..., 0], ys + f[..., 1]
    inside = m & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    px, py = torch.where(inside, px, zero), torch.where(inside, py, zero)
    fx0, fy0 = torch.floor(px), torch.floor(py)
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    wx, wy = (px - fx0).unsqueeze(3), (py - fy0).unsqueeze(3)
    n = torch.arange(N).reshape(N, 1, 1).expand(N, H, W)
    g = scale * ((1 - wy) * ((1 - wx) * other[n, y0, x0] + wx * other[n, y0, x1])
                 + wy * ((1 - wx) * other[n, y1, x0] + wx * other[n, y1, x1]))
    d = f + g
    bound = alpha1 * ((f * f).sum(3) + (g * g).sum(3)) + alpha2
    margin = bound - (d * d).sum(3)
    mask = inside & (margin >= 0)
    ninf = torch.full((), -float("inf"), dtype=dt)
    return Direction(mask, mask.sum(dim=(1, 2)), torch.where(inside, margin, ninf), torch.where(inside, bound, zero), inside)


def fb_ref(flow_a, flow_b, flow_scale=1.0, alpha1=0.01, alpha2=0.5, valid_a=None, valid_b=None):
    """(Direction a, Direction b) of two (N,H,W,2) flows (any float dtype; computed in float64)."""
    scale, alpha1, alpha2 = (float(np.float32(v)) for v in (flow_scale, alpha1, alpha2))
    fa, fb = flow_a.to(torch.float64), flow_b.to(torch.float64)
    return (_direction(fa, fb, scale, alpha1, alpha2, valid_a), _direction(fb, fa, scale, alpha1, alpha2, valid_b))


def near_ties(direction):
    """(N,H,W) bool: the candidates whose margin is within NEAR_TIE * max(1, bound) of 0 -- where a different order of the
    float64 operations may decide differently."""
    return direction.candidate & (direction.margin.abs() <= NEAR_TIE * torch.clamp(direction.bound, min=1.0))


# ------------------------------------------------------------------ inputs
def _sampled(flow_px, candidate):
    """(N,H,W) bool: the pixels a candidate of the direction with displacement flow_px (px, float64) reads a corner from."""
    N, H, W, _ = flow_px.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    px, py = xs + flow_px[..., 0], ys + flow_px[..., 1]
    x0, y0 = np.floor(px[candidate]).astype(np.int64), np.floor(py[candidate]).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    n = (np.arange(N).reshape(N, 1, 1) + np.zeros((N, H, W), np.int64))[candidate]
    out = np.zeros((N, H, W), bool)
    for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
        out[n, yy, xx] = True
    return out


def build_case(N, H, W, flow_scale=1.0, alphas=(0.01, 0.5), seed=0, masked=True, empty=None, nonfinite=False, block=6, max_off=3,
               noise=0.5):
    """Inputs of one case, numpy float32 (masks bool, or None):

      fw        (N,H,W,2), in units of 1 / flow_scale px: flow_scale * fw = an integer field, constant on block x block tiles,
                of up to max_off px, plus a continuous part uniform in [0, 1) per pixel and component.
      bw        flow_scale * bw = -(that displacement looked up where the pixel came from: at q - fw(q), rounded and clipped) +
                uniform noise of amplitude `noise` px per component: consistent up to the noise and the tile seams, so that the
                share of valid pixels among the candidates is neither ~0 nor ~1.
      empty     the index of an image whose every sample point, in both directions, is out of frame.
      nonfinite NaN, +Inf and -Inf at ~2 % of the pixels of both flows (a seeded set per flow).
      valid_fw, valid_bw   ~70 % True each.  fw_nan, bw_nan: the same flows with NaN at the masked pixels that no candidate of
                the other direction reads a corner from (the kernel reads no flow at a masked pixel of its own direction, but the
                other direction samples wherever its flows point)."""
    rs = np.random.RandomState(seed)
    th, tw = -(-H // block), -(-W // block)
    off = np.kron(rs.randint(-max_off, max_off + 1, size=(N, th, tw, 2)).astype(np.float64), np.ones((1, block, block, 1)))[:, :H, :W]
    fw_px = off + rs.uniform(0.0, 1.0, size=(N, H, W, 2))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    n_idx = np.arange(N).reshape(N, 1, 1) + np.zeros((N, H, W), np.int64)
    sx = np.clip(np.rint(xs - fw_px[..., 0]), 0, W - 1).astype(np.int64)
    sy = np.clip(np.rint(ys - fw_px[..., 1]), 0, H - 1).astype(np.int64)
    bw_px = -fw_px[n_idx, sy, sx] + rs.uniform(-noise, noise, size=(N, H, W, 2))
    if empty is not None:
        fw_px[empty, ..., 0], bw_px[empty, ..., 0] = W + 2.0, -(W + 2.0)
    fw, bw = (fw_px / flow_scale).astype(np.float32), (bw_px / flow_scale).astype(np.float32)
    if nonfinite:
        for fl in (fw, bw):
            hit = rs.uniform(size=(N, H, W)) < 0.02
            bad = rs.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=int(hit.sum()))
            fl[hit, 0] = bad
            fl[hit, 1] = np.where(rs.uniform(size=bad.shape) < 0.5, bad, fl[hit, 1])       # one bad component is enough
    valid_fw = (rs.uniform(size=(N, H, W)) < 0.7) if masked else None
    valid_bw = (rs.uniform(size=(N, H, W)) < 0.7) if masked else None
    case = {"N": N, "H": H, "W": W, "flow_scale": float(flow_scale), "alphas": tuple(alphas), "fw": fw, "bw": bw,
            "valid_fw": valid_fw, "valid_bw": valid_bw, "empty": empty, "nonfinite": nonfinite}
    fw_nan, bw_nan = fw.copy(), bw.copy()
    if masked:
        a, b = fb_ref(torch.from_numpy(fw), torch.from_numpy(bw), flow_scale, *alphas, torch.from_numpy(valid_fw),
                      torch.from_numpy(valid_bw))
        s = np.float64(np.float32(flow_scale))
        fw_nan[~valid_fw & ~_sampled(s * bw.astype(np.float64), b.candidate.numpy())] = np.nan
        bw_nan[~valid_bw & ~_sampled(s * fw.astype(np.float64), a.candidate.numpy())] = np.nan
        assert np.isnan(fw_nan).any() and np.isnan(bw_nan).any()
    case.update(fw_nan=fw_nan, bw_nan=bw_nan)
    return case


# The cases of tests/test_gpu_fbcheck.py: N = 2; 23 x 37: odd sizes, tail lanes, 4 parts; 272 x 256: 272 > 256 parts of an image,
# so the grid-stride loop and the capped partition run (the sizes of tests/unsup_ref.py, for the same reasons).  flow_scale in
# {1, 5}, (alpha1, alpha2) in {(0.01, 0.5), (0, 0.25)}, ~70 % input masks with NaN behind them and no masks, one image that is
# out of frame everywhere, one pair with NaN and Inf at unmasked pixels.  The noise amplitudes put the valid share of the
# candidates between 30 % and 70 % (asserted in tests/test_host_fbcheck.py).
CASES = {
    "23x37_s1_a": dict(N=2, H=23, W=37, flow_scale=1.0, alphas=(0.01, 0.5), seed=1, noise=0.5),
    "23x37_s5_b_empty": dict(N=2, H=23, W=37, flow_scale=5.0, alphas=(0.0, 0.25), seed=2, empty=1, noise=0.3),
    "23x37_s1_a_nonfinite": dict(N=2, H=23, W=37, flow_scale=1.0, alphas=(0.01, 0.5), seed=3, masked=False, nonfinite=True, noise=0.5),
    "272x256_s5_a": dict(N=2, H=272, W=256, flow_scale=5.0, alphas=(0.01, 0.5), seed=4, noise=0.5),
    "272x256_s1_b_nomask": dict(N=2, H=272, W=256, flow_scale=1.0, alphas=(0.0, 0.25), seed=5, masked=False, noise=0.3),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case and its float64 reference (a, b: the two Directions, on the flows WITHOUT the NaN behind the masks) -- computed
    once per process and shared; treat it as read-only."""
    case = build_case(**CASES[name])
    vf = None if case["valid_fw"] is None else torch.from_numpy(case["valid_fw"])
    vb = None if case["valid_bw"] is None else torch.from_numpy(case["valid_bw"])
    a, b = fb_ref(torch.from_numpy(case["fw"]), torch.from_numpy(case["bw"]), case["flow_scale"], *case["alphas"], vf, vb)
    return {"case": case, "a": a, "b": b}
