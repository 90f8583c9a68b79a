"""numpy float64 restatement of csrc/pwc_motion.hip, operation for operation (include/pwc_hip.h, "dominant motion"): the fit with
its partition, tree and part order, the residual, the affine warp.  tests/test_host_motion.py checks it on the CPU against
independent routes; tests/test_gpu_motion.py holds the kernels to it bit for bit.  Also the seeded inputs both share.

Every product and sum below is one numpy operation on float64 values in the order the kernel performs it; numpy forms no fused
multiply-add.  `mutate` switches on one deliberate fault at a time, for the host tests that show the shared inputs tell it apart.
"""
import numpy as np

MODELS = ("translation", "similarity", "affine")
MIN_COUNT = {"translation": 1, "similarity": 2, "affine": 3}
SENTINEL = np.float32(1e10)
PIVOT = 1e-9
f8 = np.float64


def known_mask(flows, valid=None):
    """flow_io.flow_valid's rule and the mask: (N,H,W) bool."""
    with np.errstate(invalid="ignore"):
        k = (np.abs(flows[..., 0]) <= np.float32(1e9)) & (np.abs(flows[..., 1]) <= np.float32(1e9))
    return k if valid is None else k & (np.asarray(valid) != 0)


def parts_of(H, W):
    return min((H * W + 255) // 256, 256)


def normalised(H, W):
    """(xh, yh) of every pixel in flat order, cx, cy, s."""
    cx, cy, s = f8(W - 1) / f8(2.0), f8(H - 1) / f8(2.0), f8(max(H, W)) / f8(2.0)
    i = np.arange(H * W)
    return ((i % W).astype(f8) - cx) / s, ((i // W).astype(f8) - cy) / s, cx, cy, s


def image_sums(flow, known, params, first, scale, mutate=None):
    """The twelve sums and the count of one image in the kernel's order: lanes, tree, parts."""
    H, W = known.shape
    hw, parts = H * W, parts_of(H, W)
    xh, yh, _, _, _ = normalised(H, W)
    k = known.reshape(hw)
    with np.errstate(all="ignore"):
        u, v = flow[..., 0].reshape(hw).astype(f8), flow[..., 1].reshape(hw).astype(f8)
        if first:
            w = np.ones(hw, f8)
        else:
            p = [f8(q) for q in params]
            ru = u - ((p[0] + (p[1] * xh)) + (p[2] * yh))
            rv = v - ((p[3] + (p[4] * xh)) + (p[5] * yh))
            w = f8(1.0) / (f8(1.0) + (((ru * ru) + (rv * rv)) / (f8(scale) * f8(scale))))
        wx, wy = w * xh, w * yh
        terms = np.stack([w, wx, wy, wx * xh, wx * yh, wy * yh, w * u, wx * u, wy * u, w * v, wx * v, wy * v], axis=1)
    if mutate == "no_cross":
        terms[:, 4] = 0.0
    terms = np.where(k[:, None], terms, 0.0)           # a pixel that is skipped adds nothing; no sum is ever -0.0
    stride = parts * 256
    rounds = (hw + stride - 1) // stride
    padded = np.zeros((rounds * stride, 12), f8)
    padded[:hw] = terms
    lanes = np.zeros((stride, 12), f8)
    for r in range(rounds):                            # lane (b, t) adds pixel b 256 + t + r parts 256, r ascending
        lanes = lanes + padded[r * stride:(r + 1) * stride]
    red = lanes.reshape(parts, 256, 12).copy()
    step = 128
    while step > 0:                                    # the 8 steps of the tree on (256, 12) arrays
        red[:, :step] = red[:, :step] + red[:, step:2 * step]
        step >>= 1
    S = np.zeros(12, f8)
    for b in range(parts):                             # the parts in index order
        S = S + red[b, 0]
    return S, int(k.sum())


def ldlt(A, rhs, tol):
    """L D L^T elimination without pivoting of the lower triangle of A (K x K) with the right-hand sides `rhs` (R x K), the
    kernel's motion_ldlt.  (solutions or None, the pivots reached)."""
    K = len(A)
    t = [[f8(0.0)] * K for _ in range(K)]
    l = [[f8(0.0)] * K for _ in range(K)]
    d = []
    for j in range(K):
        for i in range(j, K):
            val = f8(A[i][j])
            for k in range(j):
                val = val - (l[i][k] * t[j][k])
            t[i][j] = val
        d.append(t[j][j])
        if not d[j] > tol:
            return None, d
        for i in range(j + 1, K):
            l[i][j] = t[i][j] / d[j]
    out = []
    for r in rhs:
        z = []
        for i in range(K):
            val = f8(r[i])
            for k in range(i):
                val = val - (l[i][k] * z[k])
            z.append(val)
        x = [f8(0.0)] * K
        for i in range(K - 1, -1, -1):
            val = z[i] / d[i]
            for k in range(i + 1, K):
                val = val - (l[k][i] * x[k])
            x[i] = val
        out.append(x)
    return out, d


def solve(S, count, model):
    """(the six parameters or None where degenerate, the pivots reached)."""
    S = [f8(s) for s in S]
    tol = f8(PIVOT) * S[0]
    if count < MIN_COUNT[model]:
        return None, []
    if model == "translation":
        if not S[0] > tol:
            return None, [S[0]]
        return [S[6] / S[0], f8(0.0), f8(0.0), S[9] / S[0], f8(0.0), f8(0.0)], [S[0]]
    if model == "similarity":
        q = S[3] + S[5]
        z = f8(0.0)
        A = [[S[0], z, z, z], [z, S[0], z, z], [S[1], S[2], q, z], [-S[2], S[1], z, q]]
        x, d = ldlt(A, [[S[6], S[9], S[7] + S[11], S[10] - S[8]]], tol)
        if x is None:
            return None, d
        a0, b0, al, be = x[0]
        return [a0, al, -be, b0, be, al], d
    A = [[S[0], 0, 0], [S[1], S[3], 0], [S[2], S[4], S[5]]]
    x, d = ldlt(A, [[S[6], S[7], S[8]], [S[9], S[10], S[11]]], tol)
    if x is None:
        return None, d
    return x[0] + x[1], d


def pixel_matrix(p, H, W):
    _, _, cx, cy, s = normalised(H, W)
    p = [f8(q) for q in p]
    return np.array([[f8(1.0) + (p[1] / s), p[2] / s, p[0] - (((p[1] * cx) + (p[2] * cy)) / s)],
                     [p[4] / s, f8(1.0) + (p[5] / s), p[3] - (((p[4] * cx) + (p[5] * cy)) / s)],
                     [0.0, 0.0, 1.0]], f8)


def fit(flows, valid=None, model="affine", iters=4, scale=1.0, mutate=None):
    """pwc_motion_fit_f64: dict(matrices (N,3,3) f8, ok (N,) bool, count (N,) int32, weight_sum (N,) f8, params (N,6) f8 in the
    normalised frame, pivots: per image the pivots of the last pass over its weight sum)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    known = known_mask(flows, valid)
    out = dict(matrices=np.zeros((N, 3, 3), f8), ok=np.zeros(N, bool), count=np.zeros(N, np.int32), weight_sum=np.zeros(N, f8),
               params=np.zeros((N, 6), f8), pivots=[])
    for n in range(N):
        params, good, d, S, cnt = [f8(0.0)] * 6, True, [], None, 0
        for it in range(iters + 1):
            S, cnt = image_sums(flows[n], known[n], params, it == 0, scale, mutate)
            sol, d = solve(S, cnt, model)
            good = good and sol is not None                # degenerate once, degenerate for good
            params = sol if good else [f8(0.0)] * 6
        out["matrices"][n] = pixel_matrix(params, H, W)
        out["ok"][n], out["count"][n], out["weight_sum"][n], out["params"][n] = good, cnt, S[0], params
        with np.errstate(all="ignore"):
            out["pivots"].append([float(x / S[0]) for x in d])
    return out


def _affine_ok(M):
    with np.errstate(invalid="ignore"):
        return bool(M[2, 0] == 0.0 and M[2, 1] == 0.0 and M[2, 2] == 1.0 and np.isfinite(M[:2]).all())


def residual(flows, matrices, valid=None, threshold=3.0):
    """pwc_motion_residual_f32: (residual (N,H,W,2) float32, inlier (N,H,W) bool)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    known = known_mask(flows, valid)
    res = np.full((N, H, W, 2), SENTINEL, np.float32)
    inl = np.zeros((N, H, W), bool)
    y, x = np.meshgrid(np.arange(H, dtype=f8), np.arange(W, dtype=f8), indexing="ij")
    thr2 = f8(threshold) * f8(threshold)
    for n in range(N):
        M = np.asarray(matrices[n], f8)
        if not _affine_ok(M):
            continue
        with np.errstate(all="ignore"):
            mu = (((M[0, 0] * x) + (M[0, 1] * y)) + M[0, 2]) - x
            mv = (((M[1, 0] * x) + (M[1, 1] * y)) + M[1, 2]) - y
            ru, rv = flows[n, ..., 0].astype(f8) - mu, flows[n, ..., 1].astype(f8) - mv
            k = known[n]
            res[n, ..., 0] = np.where(k, ru.astype(np.float32), SENTINEL)
            res[n, ..., 1] = np.where(k, rv.astype(np.float32), SENTINEL)
            inl[n] = k & (((ru * ru) + (rv * rv)) <= thr2)
    return res, inl


def warp(frames, matrices, mutate=None):
    """pwc_warp_affine: (out (N,H,W,C) in the frames' dtype, covered (N,H,W) bool)."""
    frames = np.asarray(frames)
    N, H, W, C = frames.shape
    out = np.zeros_like(frames)
    cov = np.zeros((N, H, W), bool)
    y, x = np.meshgrid(np.arange(H, dtype=f8), np.arange(W, dtype=f8), indexing="ij")
    for n in range(N):
        M = np.asarray(matrices[n], f8)
        if not _affine_ok(M):
            continue
        with np.errstate(all="ignore"):
            sx = ((M[0, 0] * x) + (M[0, 1] * y)) + M[0, 2]
            sy = ((M[1, 0] * x) + (M[1, 1] * y)) + M[1, 2]
            inside = (sx >= 0.0) & (sy >= 0.0) & (sy <= f8(H - 1)) & ((sx < f8(W - 1)) if mutate == "strict_last_column"
                                                                       else (sx <= f8(W - 1)))
            sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
            fx0, fy0 = np.floor(sx), np.floor(sy)
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            wx1, wy1 = sx - fx0, sy - fy0
            wx0, wy0 = f8(1.0) - wx1, f8(1.0) - wy1
            f = frames[n].astype(f8)
            for c in range(C):
                top = (wx0 * f[y0, x0, c]) + (wx1 * f[y0, x1, c])
                bot = (wx0 * f[y1, x0, c]) + (wx1 * f[y1, x1, c])
                val = (wy0 * top) + (wy1 * bot)
                if frames.dtype == np.uint8:
                    r = np.rint(val)
                    val = np.where(r >= 255.0, 255.0, np.where(r >= 0.0, r, 0.0))      # (a NaN fails both: 0)
                out[n, ..., c] = np.where(inside, val, 0.0).astype(frames.dtype)
            cov[n] = inside
    return out, cov


# ---------------------------------------------------------------- the seeded inputs of the host and the GPU tests
TRUE_PARAMS = (1.5, 2.0, -1.0, -0.5, 0.8, 1.2)     # a0 a1 a2 b0 b1 b2 in pixels, the normalised frame
SHAPES = ((13, 19), (17, 16), (32, 48))


def scene(H, W, seed=0, noise=0.05, outliers=True, params=TRUE_PARAMS):
    """An affine flow with `noise` px of normal noise and a rectangle of 26 to 29 % of the pixels moved by (8, -6) px on its own:
    (flow (H,W,2) float32, the rectangle's mask)."""
    rs = np.random.RandomState(seed)
    xh, yh, _, _, _ = normalised(H, W)
    a0, a1, a2, b0, b1, b2 = params
    flow = np.stack([a0 + a1 * xh + a2 * yh, b0 + b1 * xh + b2 * yh], axis=1).reshape(H, W, 2)
    flow = flow + rs.normal(0.0, noise, size=flow.shape) if noise else flow
    rect = np.zeros((H, W), bool)
    if outliers:
        y0, x0 = int(round(0.2 * H)), int(round(0.3 * W))
        rect[y0:y0 + (H + 1) // 2, x0:x0 + int(0.55 * W)] = True
        flow[rect] += (8.0, -6.0)
    return flow.astype(np.float32), rect


def batch(H, W, N=1, seed=0, **kw):
    return np.stack([scene(H, W, seed + n, **kw)[0] for n in range(N)])


def random_frames(N, H, W, C, dtype, seed=0):
    rs = np.random.RandomState(seed)
    if dtype == np.uint8:
        return rs.randint(0, 256, size=(N, H, W, C)).astype(np.uint8)
    return rs.uniform(-0.25, 1.25, size=(N, H, W, C)).astype(np.float32)
