"""numpy float64 restatement of the projective path, operation for operation (include/pwc_hip.h, "projective motion"): the
homography fit of csrc/pwc_homography.hip with its partition, tree and part order, projective.h's position, and the projective
residual, warp, plate and plate difference.  tests/test_host_homography.py checks it on the CPU against independent routes;
tests/test_gpu_homography.py holds the kernels to it bit for bit.  Also the seeded inputs both share.

Every product, quotient and sum below is one numpy operation on float64 values in the order the kernel performs it; numpy forms
no fused multiply-add.  The elimination, the known-pixel rule, the partition and the sampling arithmetic are the ones of
tests/motion_ref.py and tests/plate_ref.py, imported, not copied.
"""
import functools

import numpy as np

from tests import motion_ref as MR
from tests import plate_ref as PR

f8 = np.float64
SUMS = 23
MIN_COUNT = 4
PIVOT = 1e-9
SENTINEL = MR.SENTINEL
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


# ------------------------------------------------------------------ the fit
def pixel_terms(flow, known, g, first, scale):
    """The 23 terms of every pixel in flat order, 0.0 where the pixel adds nothing: (terms (HW, 23), left out of the pass (HW,))."""
    H, W = known.shape
    hw = H * W
    xh, yh, _, _, s = MR.normalised(H, W)
    k = known.reshape(hw)
    with np.errstate(all="ignore"):
        u, v = flow[..., 0].reshape(hw).astype(f8), flow[..., 1].reshape(hw).astype(f8)
        xp, yp = xh + (u / s), yh + (v / s)
        if first:
            w = np.ones(hw, f8)
            behind = np.zeros(hw, bool)
        else:
            g = [f8(q) for q in g]
            D = ((g[6] * xh) + (g[7] * yh)) + f8(1.0)
            behind = ~(D > 0.0)
            rx = (((((g[0] * xh) + (g[1] * yh)) + g[2]) / D) - xp) * s
            ry = (((((g[3] * xh) + (g[4] * yh)) + g[5]) / D) - yp) * s
            w = (f8(1.0) / (f8(1.0) + (((rx * rx) + (ry * ry)) / (f8(scale) * f8(scale))))) / (D * D)
        wx, wy = w * xh, w * yh
        b = [w, wx, wy, wx * xh, wx * yh, wy * yh]
        q = (xp * xp) + (yp * yp)
        terms = np.stack(b + [t * xp for t in b] + [t * yp for t in b] + [t * q for t in b[1:]], axis=1)
    return np.where((k & ~behind)[:, None], terms, 0.0), k & behind


def image_sums(flow, known, g, first, scale):
    """The 23 sums and the count of one image in the kernel's order: lanes, tree, parts."""
    H, W = known.shape
    hw, parts = H * W, MR.parts_of(H, W)
    terms, _ = pixel_terms(flow, known, g, first, scale)
    stride = parts * 256
    rounds = (hw + stride - 1) // stride
    padded = np.zeros((rounds * stride, SUMS), f8)
    padded[:hw] = terms
    lanes = np.zeros((stride, SUMS), f8)
    for r in range(rounds):
        lanes = lanes + padded[r * stride:(r + 1) * stride]
    red = lanes.reshape(parts, 256, SUMS).copy()
    step = 128
    while step > 0:
        red[:, :step] = red[:, :step] + red[:, step:2 * step]
        step >>= 1
    S = np.zeros(SUMS, f8)
    for p in range(parts):
        S = S + red[p, 0]
    return S, int(known.sum())


def system(S):
    """The lower triangle (8 x 8 lists) and the right-hand side, unknowns in the order (g2 g0 g1 g5 g3 g4 g6 g7)."""
    S = [f8(v) for v in S]
    z = f8(0.0)
    A = [[S[0], z, z, z, z, z, z, z],
         [S[1], S[3], z, z, z, z, z, z],
         [S[2], S[4], S[5], z, z, z, z, z],
         [z, z, z, S[0], z, z, z, z],
         [z, z, z, S[1], S[3], z, z, z],
         [z, z, z, S[2], S[4], S[5], z, z],
         [-S[7], -S[9], -S[10], -S[13], -S[15], -S[16], S[20], z],
         [-S[8], -S[10], -S[11], -S[14], -S[16], -S[17], S[21], S[22]]]
    return A, [S[6], S[7], S[8], S[12], S[13], S[14], -S[18], -S[19]]


def solve(S, count):
    """(g0 .. g7 or None where degenerate, the pivots reached)."""
    if count < MIN_COUNT:
        return None, []
    A, rhs = system(S)
    with np.errstate(all="ignore"):
        x, d = MR.ldlt(A, [rhs], f8(PIVOT) * f8(S[0]))
    if x is None:
        return None, d
    r = x[0]
    return [r[1], r[2], r[0], r[4], r[5], r[3], r[6], r[7]], d


def pixel_matrix(g, H, W):
    """(M = T^-1 G T divided by its [2][2] entry, good): the last pass of the solve."""
    _, _, cx, cy, s = MR.normalised(H, W)
    g = [f8(q) for q in g]
    rows = [(g[0], g[1], g[2]), (g[3], g[4], g[5]), (g[6], g[7], f8(1.0))]
    with np.errstate(all="ignore"):
        a = [(h[0] / s, h[1] / s, h[2] - (((h[0] * cx) + (h[1] * cy)) / s)) for h in rows]
        e = [(s * a[0][j]) + (cx * a[2][j]) for j in range(3)] + [(s * a[1][j]) + (cy * a[2][j]) for j in range(3)] + list(a[2])
        good = bool(e[8] > 0.0)
        m = [v / e[8] for v in e]
        good = good and all(np.isfinite(v) for v in m)
        if good:
            for x, y in ((0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0)):
                good = good and bool((((m[6] * f8(x)) + (m[7] * f8(y))) + f8(1.0)) > 0.0)
    return np.array(m, f8).reshape(3, 3), good


def fit(flows, valid=None, iters=4, scale=1.0):
    """pwc_homography_fit_f64: dict(matrices (N,3,3) f8, ok (N,) bool, count (N,) int32, weight_sum (N,) f8, params (N,8) f8 in the
    normalised frame, pivots: per image the pivots of the last pass over its weight sum, left_out: per image and pass the known
    pixels with D <= 0)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    known = MR.known_mask(flows, valid)
    out = dict(matrices=np.zeros((N, 3, 3), f8), ok=np.zeros(N, bool), count=np.zeros(N, np.int32), weight_sum=np.zeros(N, f8),
               params=np.zeros((N, 8), f8), pivots=[], left_out=[])
    for n in range(N):
        g, good, d, S, cnt, left = [f8(v) for v in IDENTITY], True, [], None, 0, []
        for it in range(iters + 1):
            left.append(int(pixel_terms(flows[n], known[n], g, it == 0, scale)[1].sum()))
            S, cnt = image_sums(flows[n], known[n], g, it == 0, scale)
            sol, d = solve(S, cnt)
            good = good and sol is not None                # degenerate once, degenerate for good
            g = sol if good else [f8(v) for v in IDENTITY]
        M, fine = pixel_matrix(g, H, W)
        good = good and fine
        out["matrices"][n] = M if good else np.eye(3)
        out["ok"][n], out["count"][n], out["weight_sum"][n], out["params"][n] = good, cnt, S[0], g
        with np.errstate(all="ignore"):
            out["pivots"].append([float(x / S[0]) for x in d])
        out["left_out"].append(left)
    return out


# ------------------------------------------------------------------ the position and its consumers
def finite(M):
    return bool(np.isfinite(np.asarray(M, f8)).all())


def position(M, x, y):
    """projective.h's POSITION at the arrays x, y: (there bool, sx, sy); sx, sy are meaningless where not there."""
    M = np.asarray(M, f8)
    with np.errstate(all="ignore"):
        D = ((M[2, 0] * x) + (M[2, 1] * y)) + M[2, 2]
        there = D > 0.0
        sx = (((M[0, 0] * x) + (M[0, 1] * y)) + M[0, 2]) / D
        sy = (((M[1, 0] * x) + (M[1, 1] * y)) + M[1, 2]) / D
    return there, sx, sy


def residual(flows, matrices, valid=None, threshold=3.0):
    """pwc_motion_residual_projective_f32: (residual (N,H,W,2) float32, inlier (N,H,W) bool)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    known = MR.known_mask(flows, valid)
    res = np.full((N, H, W, 2), SENTINEL, np.float32)
    inl = np.zeros((N, H, W), bool)
    y, x = np.meshgrid(np.arange(H, dtype=f8), np.arange(W, dtype=f8), indexing="ij")
    thr2 = f8(threshold) * f8(threshold)
    for n in range(N):
        if not finite(matrices[n]):
            continue
        there, sx, sy = position(matrices[n], x, y)
        with np.errstate(all="ignore"):
            ru, rv = flows[n, ..., 0].astype(f8) - (sx - x), flows[n, ..., 1].astype(f8) - (sy - y)
            k = known[n] & there
            res[n, ..., 0] = np.where(k, ru.astype(np.float32), SENTINEL)
            res[n, ..., 1] = np.where(k, rv.astype(np.float32), SENTINEL)
            inl[n] = k & (((ru * ru) + (rv * rv)) <= thr2)
    return res, inl


def _sample(M, out_h, out_w, src):
    """tests/plate_ref.py's _sample with the projective position: (inside, v, corner indices)."""
    H, W = src.shape[:2]
    ys, xs = np.meshgrid(np.arange(out_h, dtype=f8), np.arange(out_w, dtype=f8), indexing="ij")
    there, sx, sy = position(M, xs, ys)
    with np.errstate(all="ignore"):
        inside = there & (sx >= 0.0) & (sx <= float(W - 1)) & (sy >= 0.0) & (sy <= float(H - 1))
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx1, wy1 = (sx - fx0)[..., None], (sy - fy0)[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    s = src.astype(f8)
    with np.errstate(all="ignore"):
        top = (wx0 * s[y0, x0]) + (wx1 * s[y0, x1])
        bot = (wx0 * s[y1, x0]) + (wx1 * s[y1, x1])
        v = (wy0 * top) + (wy1 * bot)
    return inside, v, (y0, y1, x0, x1)


def warp(frames, matrices):
    """pwc_warp_projective: (out (N,H,W,C) in the frames' dtype, covered (N,H,W) bool)."""
    frames = np.asarray(frames)
    N, H, W, C = frames.shape
    out = np.zeros_like(frames)
    cov = np.zeros((N, H, W), bool)
    for n in range(N):
        if not finite(matrices[n]):
            continue
        inside, v, _ = _sample(matrices[n], H, W, frames[n])
        out[n] = np.where(inside[..., None], PR._rounded(v, frames.dtype), np.zeros((), frames.dtype))
        cov[n] = inside
    return out, cov


def plate_build(frames, matrices, canvas, mode=PR.MEDIAN, use=None, masks=None, min_count=1):
    """pwc_plate_build_projective: tests/plate_ref.py's plate_build with FINITE and POSITION in place of the affine rule."""
    T, H, W, C = frames.shape
    Hc, Wc = canvas
    u8 = frames.dtype == np.uint8
    present = np.zeros((T, Hc, Wc), bool)
    values = np.zeros((T, Hc, Wc, C), f8)
    for t in range(T):
        if (use is not None and not use[t]) or not finite(matrices[t]):
            continue
        inside, v, idx = _sample(matrices[t], Hc, Wc, frames[t])
        ok = inside
        if masks is not None:
            ok = ok & PR._all_corners(masks[t] != 0, idx)
        if not u8:
            ok = ok & PR._all_corners(np.isfinite(frames[t]).all(axis=-1), idx)
        present[t], values[t] = ok, v
    n = present.sum(axis=0)
    if mode == PR.MEAN:
        s = np.zeros((Hc, Wc, C), f8)
        for t in range(T):
            with np.errstate(all="ignore"):
                s = np.where(present[t][..., None], s + values[t], s)
        with np.errstate(all="ignore"):
            plate = PR._rounded(s / n[..., None].astype(f8), frames.dtype)
    else:
        r = PR._rounded(values, frames.dtype)
        k = r.astype(np.int64) if u8 else PR.key(r.view(np.uint32)).astype(np.int64)
        k = np.sort(np.where(present[..., None], k, np.int64(1) << 40), axis=0)
        rank = np.maximum((n - 1) // 2, 0)
        pick = np.take_along_axis(k, np.broadcast_to(rank[None, ..., None], (1, Hc, Wc, C)), axis=0)[0]
        pick = np.where(n[..., None] > 0, pick, 0)
        plate = pick.astype(np.uint8) if u8 else PR.unkey(pick.astype(np.uint32)).view(np.float32)
    plate = np.where((n >= min_count)[..., None], plate, np.zeros((), frames.dtype)).astype(frames.dtype)
    return np.ascontiguousarray(plate), n.astype(np.uint8)


def plate_difference(frames, plate, count, matrices, threshold, min_count=1):
    """pwc_plate_difference_projective: (difference (T,H,W) float32, foreground (T,H,W) bool, known (T,H,W) bool)."""
    T, H, W, C = frames.shape
    u8 = frames.dtype == np.uint8
    difference = np.zeros((T, H, W), np.float32)
    foreground = np.zeros((T, H, W), bool)
    known = np.zeros((T, H, W), bool)
    for t in range(T):
        if not finite(matrices[t]):
            continue
        inside, s, idx = _sample(matrices[t], H, W, plate)
        ok = inside & PR._all_corners(count >= min_count, idx)
        if not u8:
            ok = ok & np.isfinite(frames[t]).all(axis=-1) & PR._all_corners(np.isfinite(plate).all(axis=-1), idx)
        d = np.zeros((H, W), f8)
        with np.errstate(all="ignore"):
            for c in range(C):
                e = np.abs(frames[t, ..., c].astype(f8) - s[..., c])
                d = np.where(e > d, e, d)
            difference[t] = np.where(ok, d.astype(np.float32), np.float32(0.0))
            foreground[t] = ok & (d > threshold)
        known[t] = ok
    return difference, foreground, known


# ------------------------------------------------------------------ the host helpers' definitions (projective=True)
def normalise(M):
    return M / M[2, 2]


def corners_of(H, W):
    return np.array([[0.0, 0.0, 1.0], [W - 1.0, 0.0, 1.0], [0.0, H - 1.0, 1.0], [W - 1.0, H - 1.0, 1.0]]).T


def project(M, pts):
    """(x, y, D) of the columns of pts (3, K) under M."""
    q = np.asarray(M, f8) @ pts
    return q[0] / q[2], q[1] / q[2], q[2]


# ------------------------------------------------------------------ the seeded inputs of the host and the GPU tests
SHAPES = ((17, 33), (48, 64), (64, 128))
M6, M7 = 2e-4, -1e-4


def true_matrix(H, W, m6=M6, m7=M7, seed=0):
    """A pixel homography near the identity: a small rotation, scale and shift, and the perspective terms m6, m7."""
    rs = np.random.RandomState(100 + seed)
    ang, sc = np.deg2rad(rs.uniform(-2.0, 2.0)), rs.uniform(0.97, 1.03)
    M = np.array([[sc * np.cos(ang), -sc * np.sin(ang), rs.uniform(-3.0, 3.0)],
                  [sc * np.sin(ang), sc * np.cos(ang), rs.uniform(-3.0, 3.0)],
                  [m6, m7, 1.0]], f8)
    return M


def exact_flow(M, H, W):
    """The float32 flow of the pixel matrix M: (M p) / D - p."""
    y, x = np.meshgrid(np.arange(H, dtype=f8), np.arange(W, dtype=f8), indexing="ij")
    D = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    return np.stack([(M[0, 0] * x + M[0, 1] * y + M[0, 2]) / D - x, (M[1, 0] * x + M[1, 1] * y + M[1, 2]) / D - y], axis=-1).astype(np.float32)


def outlier_block(H, W):
    """A block of about 15 % of the pixels (half the height, 30 % of the width)."""
    rect = np.zeros((H, W), bool)
    y0, x0 = int(round(0.25 * H)), int(round(0.35 * W))
    rect[y0:y0 + (H + 1) // 2, x0:x0 + int(round(0.3 * W))] = True
    return rect


@functools.lru_cache(maxsize=None)
def scene(H, W, seed=0, outliers=False, noise=0.0, m6=M6, m7=M7):
    """(flow (H,W,2) float32, the true pixel matrix, the block's mask), read-only: the exact flow of true_matrix, `noise` px of
    normal noise, and (outliers) the block moved by 9 px on its own."""
    M = true_matrix(H, W, m6, m7, seed)
    flow = exact_flow(M, H, W).astype(f8)
    rect = outlier_block(H, W) if outliers else np.zeros((H, W), bool)
    if noise:
        flow = flow + np.random.RandomState(seed).normal(0.0, noise, size=flow.shape)
    flow[rect] += (9.0, 0.0)
    flow = flow.astype(np.float32)
    for a in (flow, M, rect):
        a.setflags(write=False)
    return flow, M, rect


def corner_error(M, truth, H, W):
    """The largest distance in pixels between where M and where truth send the four frame corners."""
    pts = corners_of(H, W)
    ax, ay, _ = project(M, pts)
    bx, by, _ = project(truth, pts)
    return float(np.sqrt((ax - bx) ** 2 + (ay - by) ** 2).max())


@functools.lru_cache(maxsize=None)
def reference_fit(H, W, iters, seed=0, outliers=False, noise=0.0):
    """fit(...) of scene(...) as a batch of one, computed once per process."""
    return fit(scene(H, W, seed, outliers, noise)[0][None], None, iters, 1.0)
