"""numpy float64 restatement of the epipolar path, operation for operation (include/pwc_hip.h, "epipolar motion"): the
fundamental-matrix fit of csrc/pwc_fundamental.hip with its partition, tree and part order, motion_jacobi.h's cyclic Jacobi
decomposition as a scalar loop, and the Sampson residual.  tests/test_host_fundamental.py checks it on the CPU against
numpy.linalg.eigh and numpy.linalg.svd; tests/test_gpu_fundamental.py holds the kernels to it bit for bit.  Also the seeded test
scene both share.

Every product, quotient, sum and square root below is one numpy operation on float64 values in the order the kernel performs it;
numpy forms no fused multiply-add and its sqrt is correctly rounded.  The known-pixel rule, the partition and the normalised
coordinates are the ones of tests/motion_ref.py, imported, not copied.
"""
import functools

import numpy as np

from tests import motion_ref as MR

f8 = np.float64
SUMS = 36
MIN_COUNT = 8
SWEEPS = 10
EIGEN_FLOOR = 1e-9
SENTINEL = MR.SENTINEL
# a_k = P[PK[k]] Q[QK[k]] with P = (1, x', y'), Q = (1, xh, yh): a = (x' xh, x' yh, x', y' xh, y' yh, y', xh, yh, 1)
PK = (1, 1, 1, 2, 2, 2, 0, 0, 0)
QK = (1, 2, 0, 1, 2, 0, 1, 2, 0)
# the monomial of a pair of P's (or of Q's): (1, x, y, x x, x y, y y)
MONO = ((0, 1, 2), (1, 3, 4), (2, 4, 5))


# ------------------------------------------------------------------ motion_jacobi.h
def jacobi(A, sweeps=SWEEPS):
    """The cyclic Jacobi decomposition of the symmetric K x K matrix A (lists or an array; the upper triangle is read):
    (eigenvalues: the diagonal reached, K floats; V: K x K lists, column j the eigenvector of eigenvalue j)."""
    K = len(A)
    a = [[f8(A[min(i, j)][max(i, j)]) for j in range(K)] for i in range(K)]
    v = [[f8(1.0) if i == j else f8(0.0) for j in range(K)] for i in range(K)]
    one, two = f8(1.0), f8(2.0)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(K - 1):
                for q in range(p + 1, K):
                    apq = a[p][q]
                    if apq == 0.0:
                        continue
                    theta = (a[q][q] - a[p][p]) / (two * apq)
                    t = (one if theta >= 0.0 else -one) / (np.abs(theta) + np.sqrt((theta * theta) + one))
                    c = one / np.sqrt((t * t) + one)
                    s = t * c
                    for k in range(K):
                        if k != p and k != q:
                            akp, akq = a[k][p], a[k][q]
                            a[k][p] = a[p][k] = (c * akp) - (s * akq)
                            a[k][q] = a[q][k] = (s * akp) + (c * akq)
                    a[p][p] = a[p][p] - (t * apq)
                    a[q][q] = a[q][q] + (t * apq)
                    a[p][q] = a[q][p] = f8(0.0)
                    for k in range(K):
                        vkp, vkq = v[k][p], v[k][q]
                        v[k][p] = (c * vkp) - (s * vkq)
                        v[k][q] = (s * vkp) + (c * vkq)
    return [a[i][i] for i in range(K)], v


def smallest(d, skip=-1):
    """The index of the smallest of d (but `skip`), ties to the lowest."""
    best = -1
    for j in range(len(d)):
        if j != skip and (best < 0 or d[j] < d[best]):
            best = j
    return best


# ------------------------------------------------------------------ the fit
def pixel_terms(flow, known, F, first, scale):
    """The 36 terms of every pixel in flat order, 0.0 where the pixel adds nothing: (terms (HW, 36), left out of the pass (HW,),
    the weights (HW,))."""
    H, W = known.shape
    hw = H * W
    xh, yh, _, _, s = MR.normalised(H, W)
    k = known.reshape(hw)
    with np.errstate(all="ignore"):
        u, v = flow[..., 0].reshape(hw).astype(f8), flow[..., 1].reshape(hw).astype(f8)
        xp, yp = xh + (u / s), yh + (v / s)
        if first:
            w = np.ones(hw, f8)
            out = np.zeros(hw, bool)
        else:
            f = [f8(q) for q in np.asarray(F, f8).reshape(9)]
            l0 = ((f[0] * xh) + (f[1] * yh)) + f[2]
            l1 = ((f[3] * xh) + (f[4] * yh)) + f[5]
            l2 = ((f[6] * xh) + (f[7] * yh)) + f[8]
            r = ((xp * l0) + (yp * l1)) + l2
            m0 = ((f[0] * xp) + (f[3] * yp)) + f[6]
            m1 = ((f[1] * xp) + (f[4] * yp)) + f[7]
            g = (((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1)
            out = ~(g > 0.0)
            d2 = ((r * r) / g) * (s * s)
            w = (f8(1.0) / (f8(1.0) + (d2 / (f8(scale) * f8(scale))))) / g
        wx, wy = w * xh, w * yh
        b = [w, wx, wy, wx * xh, wx * yh, wy * yh]
        pa = [None, xp, yp, xp * xp, xp * yp, yp * yp]
        terms = np.stack(b + [t * pa[i] for i in range(1, 6) for t in b], axis=1)
    return np.where((k & ~out)[:, None], terms, 0.0), k & out, w


def image_sums(flow, known, F, first, scale):
    """The 36 sums and the count of one image in the kernel's order: lanes, tree, parts."""
    H, W = known.shape
    hw, parts = H * W, MR.parts_of(H, W)
    terms, _, _ = pixel_terms(flow, known, F, first, scale)
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


def moment_matrix(S):
    """The symmetric 9 x 9 matrix sum w a a^T from the 36 sums: entry (k, l) is S[6 mono(P_k, P_l) + mono(Q_k, Q_l)]."""
    return [[f8(S[6 * MONO[PK[k]][PK[l]] + MONO[QK[k]][QK[l]]]) for l in range(9)] for k in range(9)]


def solve(S, count):
    """One solve: (F^ rank 2 as 9 floats or None where degenerate, v the epipole in normalised coordinates, (l0 / tr, l1 / tr))."""
    zero = f8(0.0)
    if count < MIN_COUNT:
        return None, [zero] * 3, [zero, zero]
    A = moment_matrix(S)
    tr = A[0][0]
    for i in range(1, 9):
        tr = tr + A[i][i]
    d, V = jacobi(A)
    j0 = smallest(d)
    j1 = smallest(d, j0)
    with np.errstate(all="ignore"):
        eig = [d[j0] / tr, d[j1] / tr]
        good = bool(d[j1] > (f8(EIGEN_FLOOR) * tr))
        F = [V[k][j0] for k in range(9)]
        B = [[((F[i] * F[j]) + (F[3 + i] * F[3 + j])) + (F[6 + i] * F[6 + j]) for j in range(3)] for i in range(3)]
        e, U = jacobi(B)
        jv = smallest(e)
        v = [U[k][jv] for k in range(3)]
        for i in range(3):
            ui = ((F[3 * i] * v[0]) + (F[3 * i + 1] * v[1])) + (F[3 * i + 2] * v[2])
            for j in range(3):
                F[3 * i + j] = F[3 * i + j] - (ui * v[j])
        good = good and all(np.isfinite(x) for x in F) and all(np.isfinite(x) for x in v) and all(np.isfinite(x) for x in eig)
    return (F if good else None), v, eig


def pixel_matrix(F, v, H, W):
    """The last pass: (F = T^T F^ T over its Frobenius norm, the largest entry positive, 9 floats; the epipole T^-1 v; finite)."""
    _, _, cx, cy, s = MR.normalised(H, W)
    with np.errstate(all="ignore"):
        a = []
        for i in range(3):
            h = F[3 * i:3 * i + 3]
            a.append([h[0] / s, h[1] / s, h[2] - (((h[0] * cx) + (h[1] * cy)) / s)])
        m = [a[0][j] / s for j in range(3)] + [a[1][j] / s for j in range(3)] + \
            [a[2][j] - (((a[0][j] * cx) + (a[1][j] * cy)) / s) for j in range(3)]
        q = m[0] * m[0]
        for j in range(1, 9):
            q = q + (m[j] * m[j])
        nrm = np.sqrt(q)
        m = [x / nrm for x in m]
        big = 0
        for j in range(1, 9):
            if np.abs(m[j]) > np.abs(m[big]):
                big = j
        if m[big] < 0.0:
            m = [-x for x in m]
        e = [(s * v[0]) + (cx * v[2]), (s * v[1]) + (cy * v[2]), v[2]]
        fine = all(np.isfinite(x) for x in m) and all(np.isfinite(x) for x in e)
    return m, e, fine


def fit(flows, valid=None, iters=4, scale=1.0):
    """pwc_fundamental_fit_f64: dict(matrices (N,3,3) f8, ok (N,) bool, count (N,) int32, weight_sum (N,) f8, eigen (N,2) f8,
    epipole (N,3) f8, normalised (N,3,3) f8: the rank-2 F^ of the last pass, left_out: per image and pass the known pixels with
    g <= 0)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    known = MR.known_mask(flows, valid)
    out = dict(matrices=np.zeros((N, 3, 3), f8), ok=np.zeros(N, bool), count=np.zeros(N, np.int32), weight_sum=np.zeros(N, f8),
               eigen=np.zeros((N, 2), f8), epipole=np.zeros((N, 3), f8), normalised=np.zeros((N, 3, 3), f8), left_out=[])
    zeros = [f8(0.0)] * 9
    for n in range(N):
        F, good, v, eig, S, cnt, left = zeros, True, [f8(0.0)] * 3, [f8(0.0)] * 2, None, 0, []
        for it in range(iters + 1):
            left.append(int(pixel_terms(flows[n], known[n], F, it == 0, scale)[1].sum()))
            S, cnt = image_sums(flows[n], known[n], F, it == 0, scale)
            if good:                                       # degenerate once, degenerate for good: eigen stays that pass's
                sol, v, eig = solve(S, cnt)
                good = sol is not None
            F = sol if good else zeros
        m, e, fine = pixel_matrix(F, v, H, W) if good else (zeros, [f8(0.0)] * 3, False)
        good = good and fine
        out["matrices"][n] = np.array(m if good else zeros, f8).reshape(3, 3)
        out["epipole"][n] = e if good else [0.0] * 3
        out["ok"][n], out["count"][n], out["weight_sum"][n], out["eigen"][n], out["normalised"][n] = \
            good, cnt, S[0], eig, np.array(F, f8).reshape(3, 3)
        out["left_out"].append(left)
    return out


# ------------------------------------------------------------------ the residual
def residual(flows, matrices, valid=None, threshold=1.0):
    """pwc_epipolar_residual_f32: (distance (N,H,W) float32, inlier (N,H,W) bool)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    known = MR.known_mask(flows, valid)
    dist = np.full((N, H, W), SENTINEL, np.float32)
    inl = np.zeros((N, H, W), bool)
    y, x = np.meshgrid(np.arange(H, dtype=f8), np.arange(W, dtype=f8), indexing="ij")
    for n in range(N):
        f = [f8(q) for q in np.asarray(matrices[n], f8).reshape(9)]
        if all(q == 0.0 for q in f):
            continue
        with np.errstate(all="ignore"):
            xp, yp = x + flows[n, ..., 0].astype(f8), y + flows[n, ..., 1].astype(f8)
            l0 = ((f[0] * x) + (f[1] * y)) + f[2]
            l1 = ((f[3] * x) + (f[4] * y)) + f[5]
            l2 = ((f[6] * x) + (f[7] * y)) + f[8]
            r = ((xp * l0) + (yp * l1)) + l2
            m0 = ((f[0] * xp) + (f[3] * yp)) + f[6]
            m1 = ((f[1] * xp) + (f[4] * yp)) + f[7]
            g = (((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1)
            d = np.abs(r) / np.sqrt(g)
            k = known[n] & (g > 0.0)
            dist[n] = np.where(k, d.astype(np.float32), SENTINEL)
            inl[n] = k & (d <= f8(threshold))              # (of the double, before the rounding)
    return dist, inl


# ------------------------------------------------------------------ the seeded test scene of the host and the GPU tests
ROTATION = (0.004, -0.006, 0.003)
TRANSLATION = (0.4, 0.1, 0.3)
BLOCK_FLOW = (-2.5, 3.0)


def block_mask(H, W):
    """The block [H/4, H/4 + H/5) x [W/8, W/8 + W/5) that moves on its own."""
    rect = np.zeros((H, W), bool)
    rect[H // 4:H // 4 + H // 5, W // 8:W // 8 + W // 5] = True
    return rect


@functools.lru_cache(maxsize=None)
def scene(H, W, seed=0, block=True, noise=0.0, translation=TRANSLATION):
    """(flow (H,W,2) float32, the block's mask), read-only: a pinhole camera (focal length W, principal point at the centre)
    that rotates by ROTATION (second order) and translates by `translation` through the depth
    Z = 4 + 3 sin(5 x / W) cos(4 y / H) + 1.5 [x > 0.6 W]; `noise` px of normal noise; (block) the block moved by BLOCK_FLOW."""
    y, x = np.meshgrid(np.arange(H, dtype=f8), np.arange(W, dtype=f8), indexing="ij")
    fl, cx, cy = float(W), (W - 1) / 2.0, (H - 1) / 2.0
    Z = 4.0 + 3.0 * np.sin(5.0 * x / W) * np.cos(4.0 * y / H) + 1.5 * (x > 0.6 * W)
    X = np.stack([(x - cx) / fl * Z, (y - cy) / fl * Z, Z], axis=-1)
    wx, wy, wz = ROTATION
    K = np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])
    R = np.eye(3) + K + 0.5 * (K @ K)
    Y = X @ R.T + np.asarray(translation, f8)
    flow = np.stack([fl * Y[..., 0] / Y[..., 2] + cx - x, fl * Y[..., 1] / Y[..., 2] + cy - y], axis=-1)
    if noise:
        flow = flow + np.random.RandomState(seed).normal(0.0, noise, size=flow.shape)
    rect = block_mask(H, W) if block else np.zeros((H, W), bool)
    flow[rect] += BLOCK_FLOW
    flow = flow.astype(np.float32)
    for a in (flow, rect):
        a.setflags(write=False)
    return flow, rect


def batch(N, H, W, block=True):
    """N images of the scene: image 0 exact, the others with 0.02 px of noise of their own seed."""
    return np.stack([scene(H, W, n, block, 0.0 if n == 0 else 0.02)[0] for n in range(N)])


@functools.lru_cache(maxsize=None)
def reference_fit(H, W, iters=4, seed=0, block=True, noise=0.0):
    """fit(...) of scene(...) as a batch of one, computed once per process."""
    return fit(scene(H, W, seed, block, noise)[0][None], None, iters, 1.0)
