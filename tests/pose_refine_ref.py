"""numpy float64 restatement of csrc/pwc_pose_refine.hip, operation for operation (include/pwc_hip.h, "pose refinement"): the
fixed pixel set, the per-pixel terms of a pass, the 22 sums with "dominant motion"'s partition, tree and part order, the 5 x 5
elimination, the Cayley update of the rotation and the tangent-plane update of the translation, the best-pass rule.
tests/test_host_pose_refine.py checks it on the CPU against the test scene's own pose and depth; tests/test_gpu_pose_refine.py holds
the kernels to it bit for bit.

Every product, quotient, sum and square root below is one numpy operation on float64 values in the order the kernel performs it;
numpy forms no fused multiply-add and its sqrt is correctly rounded.  The rays, the known-pixel rule, FINE, the elimination and the
seeded scene are the ones of tests/pose_ref.py, tests/fundamental_ref.py and tests/motion_ref.py, imported, not copied.
"""
import numpy as np

from tests import fundamental_ref as FR
from tests import pose_ref as PR

MR = FR.MR
f8 = np.float64
SUMS = 22
MIN_SAMPLES = 5
PIVOT = 1e-9
ZERO, ONE, TWO = f8(0.0), f8(1.0), f8(2.0)


def _cross(a, b):
    return [(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])]


# ------------------------------------------------------------------ the tangent basis of t
def basis(t):
    """BASIS of the header: (b1, b2), three floats each.  b1 = (e_i x t) / |e_i x t| for the entry i of t smallest in magnitude, ties
    to the lowest index; b2 = t x b1."""
    t = [f8(q) for q in t]
    with np.errstate(all="ignore"):
        m = [np.abs(q) for q in t]
        i = 0
        if m[1] < m[i]:
            i = 1
        if m[2] < m[i]:
            i = 2
        if i == 0:
            nrm = np.sqrt((t[2] * t[2]) + (t[1] * t[1]))
            b1 = [ZERO, (-t[2]) / nrm, t[1] / nrm]
        elif i == 1:
            nrm = np.sqrt((t[2] * t[2]) + (t[0] * t[0]))
            b1 = [t[2] / nrm, ZERO, (-t[0]) / nrm]
        else:
            nrm = np.sqrt((t[1] * t[1]) + (t[0] * t[0]))
            b1 = [(-t[1]) / nrm, t[0] / nrm, ZERO]
        return b1, _cross(t, b1)


# ------------------------------------------------------------------ the per-pixel core
def epipolar_terms(R, t, k, d0x, d0y, d1x, d1y):
    """EPIPOLAR of the header for every pixel: (a (3), c (3), e (3), r, g), arrays."""
    R = [f8(q) for q in np.asarray(R, f8).reshape(9)]
    t = [f8(q) for q in np.asarray(t, f8).reshape(3)]
    fx, fy = f8(k[0]), f8(k[1])
    a = [((R[0] * d0x) + (R[1] * d0y)) + R[2], ((R[3] * d0x) + (R[4] * d0y)) + R[5], ((R[6] * d0x) + (R[7] * d0y)) + R[8]]
    c = [(d1y * a[2]) - a[1], a[0] - (d1x * a[2]), (d1x * a[1]) - (d1y * a[0])]
    e = [(d1y * t[2]) - t[1], t[0] - (d1x * t[2]), (d1x * t[1]) - (d1y * t[0])]
    r = ((e[0] * a[0]) + (e[1] * a[1])) + (e[2] * a[2])
    l0, l1 = ((t[1] * a[2]) - (t[2] * a[1])) / fx, ((t[2] * a[0]) - (t[0] * a[2])) / fy
    m0 = (((R[0] * e[0]) + (R[3] * e[1])) + (R[6] * e[2])) / fx
    m1 = (((R[1] * e[0]) + (R[4] * e[1])) + (R[7] * e[2])) / fy
    g = (((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1)
    return a, c, e, r, g


def pixel_set(flow, known, R0, t0, k, threshold):
    """The pixels of one image that take part, (H,W) bool: KNOWN, g > 0 and |r| / sqrt(g) <= threshold under the INPUT pose."""
    with np.errstate(all="ignore"):
        _, _, d0x, d0y, d1x, d1y = PR.rays(flow, k)
        _, _, _, r, g = epipolar_terms(R0, t0, k, d0x, d0y, d1x, d1y)
        return known & (g > 0.0) & ((np.abs(r) / np.sqrt(g)) <= f8(threshold))


def pixel_terms(flow, inset, R, t, k, scale):
    """The 22 terms of every pixel in flat order under the pose (R, t), 0.0 where the pixel adds nothing: (HW, 22)."""
    H, W = inset.shape
    hw = H * W
    with np.errstate(all="ignore"):
        _, _, d0x, d0y, d1x, d1y = PR.rays(flow, k)
        a, c, e, r, g = epipolar_terms(R, t, k, d0x, d0y, d1x, d1y)
        b1, b2 = basis(t)
        sg = np.sqrt(g)
        rho = r / sg
        d2 = (r * r) / g
        w = ONE / (ONE + (d2 / (f8(scale) * f8(scale))))
        ae = _cross(a, e)
        J = [ae[0] / sg, ae[1] / sg, ae[2] / sg,
             (-(((c[0] * b1[0]) + (c[1] * b1[1])) + (c[2] * b1[2]))) / sg,
             (-(((c[0] * b2[0]) + (c[1] * b2[1])) + (c[2] * b2[2]))) / sg]
        wJ = [w * q for q in J]
        cols = [wJ[i] * J[j] for i in range(5) for j in range(i + 1)] + [wJ[i] * rho for i in range(5)] + [w, w * d2]
        terms = np.stack([np.broadcast_to(q, (H, W)) for q in cols], axis=-1).reshape(hw, SUMS)
        use = (inset & (g > 0.0)).reshape(hw)
    return np.where(use[:, None], terms, 0.0)


def image_sums(terms, H, W):
    """The 22 sums of one image in the kernel's order: lanes, tree, parts."""
    hw, parts = H * W, MR.parts_of(H, W)
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
    return S


# ------------------------------------------------------------------ the solve
def system(S):
    """(the lower triangle of the 5 x 5 matrix as rows, the right-hand side -b, the pivot floor 1e-9 trace)."""
    A = [[ZERO] * 5 for _ in range(5)]
    j = 0
    for i in range(5):
        for q in range(i + 1):
            A[i][q] = f8(S[j])
            j += 1
    rhs = [-f8(S[15 + i]) for i in range(5)]
    tr = A[0][0]
    for i in range(1, 5):
        tr = tr + A[i][i]
    return A, rhs, f8(PIVOT) * tr


def cayley(delta):
    """C(omega) of the header as 9 floats, a = omega / 2."""
    a = [f8(delta[0]) / TWO, f8(delta[1]) / TWO, f8(delta[2]) / TWO]
    q = ((a[0] * a[0]) + (a[1] * a[1])) + (a[2] * a[2])
    p, den = ONE - q, ONE + q
    return [(p + (TWO * (a[0] * a[0]))) / den, ((TWO * (a[0] * a[1])) - (TWO * a[2])) / den, ((TWO * (a[0] * a[2])) + (TWO * a[1])) / den,
            ((TWO * (a[1] * a[0])) + (TWO * a[2])) / den, (p + (TWO * (a[1] * a[1]))) / den, ((TWO * (a[1] * a[2])) - (TWO * a[0])) / den,
            ((TWO * (a[2] * a[0])) - (TWO * a[1])) / den, ((TWO * (a[2] * a[1])) + (TWO * a[0])) / den, (p + (TWO * (a[2] * a[2]))) / den]


def update(R, t, delta):
    """UPDATE of the header: the pose after the step delta = (omega, beta1, beta2): (R 9 floats, t 3 floats)."""
    R = [f8(q) for q in np.asarray(R, f8).reshape(9)]
    t = [f8(q) for q in np.asarray(t, f8).reshape(3)]
    with np.errstate(all="ignore"):
        C = cayley(delta)
        Rn = [((C[3 * r] * R[c]) + (C[3 * r + 1] * R[3 + c])) + (C[3 * r + 2] * R[6 + c]) for r in range(3) for c in range(3)]
        b1, b2 = basis(t)
        u = [(t[i] + (f8(delta[3]) * b1[i])) + (f8(delta[4]) * b2[i]) for i in range(3)]
        nrm = np.sqrt(((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2]))
        return Rn, [q / nrm for q in u]


def _finite(values):
    return all(PR._finite(q) for q in values)


# ------------------------------------------------------------------ pwc_pose_refine_f64
def refine(flows, rotation, translation, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0):
    """dict(rotation (N,3,3), translation (N,3) f8, ok (N,) bool, samples, best_pass (N,) int32, cost (N, iters + 1), weight_sum (N,)
    f8, frozen (N,) int: the pass that froze the image or -1, inset (N,H,W) bool, systems: per image the (A, rhs, tol) it solved)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    K = np.broadcast_to(np.asarray(intrinsics, f8), (N, 4))
    known = MR.known_mask(flows, valid)
    out = dict(rotation=np.zeros((N, 3, 3), f8), translation=np.zeros((N, 3), f8), ok=np.zeros(N, bool), samples=np.zeros(N, np.int32),
               best_pass=np.zeros(N, np.int32), cost=np.zeros((N, iters + 1), f8), weight_sum=np.zeros(N, f8),
               frozen=np.full(N, -1), inset=np.zeros((N, H, W), bool), systems=[[] for _ in range(N)])
    for n in range(N):
        k = [f8(q) for q in K[n]]
        R0 = [f8(q) for q in np.asarray(rotation[n], f8).reshape(9)]
        t0 = [f8(q) for q in np.asarray(translation[n], f8).reshape(3)]
        if all(q == 0.0 for q in R0) or not PR.intrinsics_fine(k):
            continue                                       # OFF
        inset = pixel_set(flows[n], known[n], R0, t0, k, threshold)
        out["inset"][n], out["samples"][n] = inset, int(inset.sum())
        if out["samples"][n] < MIN_SAMPLES:
            continue
        out["ok"][n] = True
        R, t = R0, t0
        for it in range(iters + 1):
            S = image_sums(pixel_terms(flows[n], inset, R, t, k, scale), H, W)
            fin = _finite(S)
            if it == 0:
                out["cost"][n, 0], out["rotation"][n], out["translation"][n], out["weight_sum"][n] = S[21], np.reshape(R, (3, 3)), t, S[20]
            elif not fin:
                out["frozen"][n] = it
                break
            else:
                out["cost"][n, it] = S[21]
                if S[21] < out["cost"][n, out["best_pass"][n]]:
                    out["best_pass"][n], out["rotation"][n], out["translation"][n], out["weight_sum"][n] = it, np.reshape(R, (3, 3)), t, S[20]
            if it == iters:
                break
            step = None
            if fin:
                A, rhs, tol = system(S)
                out["systems"][n].append((A, rhs, tol))
                with np.errstate(all="ignore"):
                    x, _ = MR.ldlt(A, [rhs], tol)
                if x is not None:
                    Rn, tn = update(R, t, x[0])
                    if _finite(Rn + tn):
                        step = (Rn, tn)
            if step is None:
                out["frozen"][n] = it
                break
            R, t = step
    return out


def flow_depth(flows, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0, min_parallax=0.25, refine_iters=0):
    """pwcnet_amd.flow_depth(..., refine=refine_iters) chained from the restatements: (depth, known, the pose used (rotation,
    translation), the closed-form pose dict, the refine dict or None, inlier)."""
    fit = FR.fit(flows, valid, iters, scale)
    _, inl = FR.residual(flows, fit["matrices"], valid, threshold)
    p = PR.pose(flows, fit["matrices"], intrinsics, valid, threshold)
    rot, tra, ref = p["rotation"], p["translation"], None
    if refine_iters > 0:
        ref = refine(flows, rot, tra, intrinsics, valid, refine_iters, scale, threshold)
        rot = np.where(ref["ok"][:, None, None], ref["rotation"], rot)
        tra = np.where(ref["ok"][:, None], ref["translation"], tra)
    dep, kn, _ = PR.depth(flows, rot, tra, intrinsics, inl, min_parallax)
    return dep, kn, (rot, tra), p, ref, inl
