"""numpy float64 restatement of the pose path, operation for operation (include/pwc_hip.h, "relative pose and depth"): the
decomposition of E = K^T F K of csrc/pwc_pose.hip with motion_jacobi.h's rotations, the cheirality vote, the selection and the
depth kernel.  tests/test_host_pose.py checks it on the CPU against numpy.linalg.svd and the test scene's own pose and depth;
tests/test_gpu_pose.py holds the kernels to it bit for bit.

Every product, quotient, sum and square root below is one numpy operation on float64 values in the order the kernel performs it;
numpy forms no fused multiply-add and its sqrt is correctly rounded.  The Jacobi decomposition, the Sampson terms' order, the
known-pixel rule and the seeded scene are the ones of tests/fundamental_ref.py and tests/motion_ref.py, imported, not copied.
The vote computes all FOUR triangulations; the kernel computes two and negates (a negation is exact), so the counts agree.
"""
import numpy as np

from tests import fundamental_ref as FR
from tests import motion_ref as MR

f8 = np.float64
SENTINEL = MR.SENTINEL
FINITE = f8(1.7976931348623157e308)


def _finite(v):
    with np.errstate(invalid="ignore"):
        return bool(np.abs(v) <= FINITE)


def intrinsics_fine(k):
    return all(_finite(q) for q in k) and bool(k[0] > 0.0) and bool(k[1] > 0.0)


def _cross(a, b):
    return [(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])]


# ------------------------------------------------------------------ decompose
def decompose(F, k):
    """One image: dict(good, Ra, Rb (9 floats each), t (3), singular (2), essential (9)); zeros where not good."""
    zero9, zero = [f8(0.0)] * 9, f8(0.0)
    bad = dict(good=False, Ra=zero9, Rb=zero9, t=[zero] * 3, singular=[zero, zero], essential=zero9)
    f = [f8(q) for q in np.asarray(F, f8).reshape(9)]
    k = [f8(q) for q in np.asarray(k, f8).reshape(4)]
    if all(q == 0.0 for q in f) or not intrinsics_fine(k):
        return bad
    fx, fy, cx, cy = k
    with np.errstate(all="ignore"):
        G = []
        for i in range(3):
            G += [f[3 * i] * fx, f[3 * i + 1] * fy, ((f[3 * i] * cx) + (f[3 * i + 1] * cy)) + f[3 * i + 2]]
        E = [fx * G[j] for j in range(3)] + [fy * G[3 + j] for j in range(3)] + \
            [((cx * G[j]) + (cy * G[3 + j])) + G[6 + j] for j in range(3)]
        B = [[((E[i] * E[j]) + (E[3 + i] * E[3 + j])) + (E[6 + i] * E[6 + j]) for j in range(3)] for i in range(3)]
        lam, V = FR.jacobi(B)
        j0 = FR.smallest(lam)
        ja, jb = [j for j in range(3) if j != j0]
        v1, v2, v3 = ([V[i][j] for i in range(3)] for j in (ja, jb, j0))
        s1, s2 = np.sqrt(lam[ja]), np.sqrt(lam[jb])
        s3 = np.sqrt(lam[j0]) if lam[j0] > 0.0 else zero
        good = bool(s1 > 0.0) and bool(s2 > 0.0)
        sing = [s2 / s1, s3 / s1]
        u1 = [(((E[3 * i] * v1[0]) + (E[3 * i + 1] * v1[1])) + (E[3 * i + 2] * v1[2])) / s1 for i in range(3)]
        u2 = [(((E[3 * i] * v2[0]) + (E[3 * i + 1] * v2[1])) + (E[3 * i + 2] * v2[2])) / s2 for i in range(3)]
        u3 = _cross(u1, u2)
        nrm = np.sqrt(((u3[0] * u3[0]) + (u3[1] * u3[1])) + (u3[2] * u3[2]))
        u3 = [q / nrm for q in u3]
        c = _cross(v1, v2)
        det = ((c[0] * v3[0]) + (c[1] * v3[1])) + (c[2] * v3[2])
        if det < 0.0:
            v3 = [-q for q in v3]
        Ra = [((u2[r] * v1[c_]) - (u1[r] * v2[c_])) + (u3[r] * v3[c_]) for r in range(3) for c_ in range(3)]
        Rb = [((u1[r] * v2[c_]) - (u2[r] * v1[c_])) + (u3[r] * v3[c_]) for r in range(3) for c_ in range(3)]
    good = good and all(_finite(q) for q in Ra + Rb + u3 + E + sing)
    if not good:
        return bad
    return dict(good=True, Ra=Ra, Rb=Rb, t=u3, singular=sing, essential=E)


def candidates(d):
    """The four (R (3,3), t (3,)) of a decomposition in the kernel's order."""
    Ra, Rb, t = np.array(d["Ra"], f8).reshape(3, 3), np.array(d["Rb"], f8).reshape(3, 3), np.array(d["t"], f8)
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


# ------------------------------------------------------------------ the per-pixel core
def grid(H, W):
    y, x = np.meshgrid(np.arange(H, dtype=f8), np.arange(W, dtype=f8), indexing="ij")
    return x, y


def rays(flow, k):
    """(x', y', d0x, d0y, d1x, d1y) of every pixel of one (H,W,2) float32 flow."""
    H, W, _ = flow.shape
    x, y = grid(H, W)
    fx, fy, cx, cy = (f8(q) for q in k)
    xp, yp = x + flow[..., 0].astype(f8), y + flow[..., 1].astype(f8)
    return xp, yp, (x - cx) / fx, (y - cy) / fy, (xp - cx) / fx, (yp - cy) / fy


def triangulate(R, t, d0x, d0y, d1x, d1y):
    """TRIANGULATE of the header: (a0, a1, a2, den, Z0, Z1), arrays."""
    R = [f8(q) for q in np.asarray(R, f8).reshape(9)]
    t = [f8(q) for q in np.asarray(t, f8).reshape(3)]
    a0 = ((R[0] * d0x) + (R[1] * d0y)) + R[2]
    a1 = ((R[3] * d0x) + (R[4] * d0y)) + R[5]
    a2 = ((R[6] * d0x) + (R[7] * d0y)) + R[8]
    c0, c1, c2 = (d1y * a2) - a1, a0 - (d1x * a2), (d1x * a1) - (d1y * a0)
    e0, e1, e2 = (d1y * t[2]) - t[1], t[0] - (d1x * t[2]), (d1x * t[1]) - (d1y * t[0])
    den = ((c0 * c0) + (c1 * c1)) + (c2 * c2)
    z0 = (-(((c0 * e0) + (c1 * e1)) + (c2 * e2))) / den
    z1 = (z0 * a2) + t[2]
    return a0, a1, a2, den, z0, z1


def voters_of(flow, known, F, threshold):
    """The pixels that vote: known and a Sampson inlier of F in pixel coordinates (fundamental_ref.residual's rule)."""
    _, inl = FR.residual(flow[None], np.asarray(F, f8).reshape(1, 3, 3), known[None], threshold)
    return inl[0]


# ------------------------------------------------------------------ pwc_camera_pose_f64
def pose(flows, matrices, intrinsics, valid=None, threshold=1.0):
    """dict(rotation (N,3,3), translation (N,3) f8, ok (N,) bool, votes (N,4), voters (N,) int32, singular (N,2), essential (N,3,3)
    f8, winner (N,) int, voting (N,H,W) bool)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    K = np.broadcast_to(np.asarray(intrinsics, f8), (N, 4))
    known = MR.known_mask(flows, valid)
    out = dict(rotation=np.zeros((N, 3, 3), f8), translation=np.zeros((N, 3), f8), ok=np.zeros(N, bool), votes=np.zeros((N, 4), np.int32),
               voters=np.zeros(N, np.int32), singular=np.zeros((N, 2), f8), essential=np.zeros((N, 3, 3), f8), winner=np.zeros(N, int),
               voting=np.zeros((N, H, W), bool))
    for n in range(N):
        d = decompose(matrices[n], K[n])
        if not d["good"]:
            continue
        out["singular"][n], out["essential"][n] = d["singular"], np.array(d["essential"], f8).reshape(3, 3)
        vote = voters_of(flows[n], known[n], matrices[n], threshold)
        with np.errstate(all="ignore"):
            _, _, d0x, d0y, d1x, d1y = rays(flows[n], K[n])
            cand = candidates(d)
            for j, (R, t) in enumerate(cand):
                _, _, _, den, z0, z1 = triangulate(R, t, d0x, d0y, d1x, d1y)
                out["votes"][n, j] = int((vote & (den > 0.0) & (z0 > 0.0) & (z1 > 0.0)).sum())
        out["voting"][n], out["voters"][n] = vote, int(vote.sum())
        best = 0
        for j in range(1, 4):
            if out["votes"][n, j] > out["votes"][n, best]:
                best = j
        out["winner"][n] = best
        if out["voters"][n] > 0 and 2 * int(out["votes"][n, best]) > int(out["voters"][n]):
            out["ok"][n], out["rotation"][n], out["translation"][n] = True, cand[best][0], cand[best][1]
    return out


# ------------------------------------------------------------------ pwc_triangulate_depth_f32
def depth(flows, rotation, translation, intrinsics, valid=None, min_parallax=0.25):
    """(depth (N,H,W) float32, known (N,H,W) bool, parallax (N,H,W) float32)."""
    flows = np.asarray(flows, np.float32)
    N, H, W, _ = flows.shape
    K = np.broadcast_to(np.asarray(intrinsics, f8), (N, 4))
    seen = MR.known_mask(flows, valid)
    dep = np.full((N, H, W), SENTINEL, np.float32)
    kn = np.zeros((N, H, W), bool)
    par = np.zeros((N, H, W), np.float32)
    for n in range(N):
        k = [f8(q) for q in K[n]]
        if not np.asarray(rotation[n]).any() or not intrinsics_fine(k):
            continue
        with np.errstate(all="ignore"):
            xp, yp, d0x, d0y, d1x, d1y = rays(flows[n], k)
            a0, a1, a2, den, z0, z1 = triangulate(rotation[n], translation[n], d0x, d0y, d1x, d1y)
            ex, ey = xp - ((k[0] * (a0 / a2)) + k[2]), yp - ((k[1] * (a1 / a2)) + k[3])
            pp = np.sqrt((ex * ex) + (ey * ey))
            front = seen[n] & (a2 > 0.0)
            good = front & (den > 0.0) & (z0 > 0.0) & (z1 > 0.0) & (pp >= f8(min_parallax))
            par[n] = np.where(front, pp.astype(np.float32), np.float32(0.0))
            dep[n] = np.where(good, z0.astype(np.float32), SENTINEL)
            kn[n] = good
    return dep, kn, par


def flow_depth(flows, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0, min_parallax=0.25):
    """pwcnet_amd.flow_depth chained from the restatements: (depth, known, parallax, the pose dict, the fit dict, inlier)."""
    fit = FR.fit(flows, valid, iters, scale)
    _, inl = FR.residual(flows, fit["matrices"], valid, threshold)
    p = pose(flows, fit["matrices"], intrinsics, valid, threshold)
    dep, kn, par = depth(flows, p["rotation"], p["translation"], intrinsics, inl, min_parallax)
    return dep, kn, par, p, fit, inl


# ------------------------------------------------------------------ the scene's own pose and depth (tests/fundamental_ref.scene)
def scene_intrinsics(H, W):
    return np.array([W, W, (W - 1) / 2.0, (H - 1) / 2.0], f8)


def scene_rotation():
    wx, wy, wz = FR.ROTATION
    K = np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])
    return np.eye(3) + K + 0.5 * (K @ K)


def scene_translation(translation=FR.TRANSLATION):
    t = np.asarray(translation, f8)
    return t / np.linalg.norm(t)


def scene_depth(H, W, translation=FR.TRANSLATION):
    """The scene's depth map in baselines: Z / |t|."""
    x, y = grid(H, W)
    Z = 4.0 + 3.0 * np.sin(5.0 * x / W) * np.cos(4.0 * y / H) + 1.5 * (x > 0.6 * W)
    return Z / np.linalg.norm(np.asarray(translation, f8))


def rotation_error(R, want):
    """The angle of R want^T in degrees, from the skew part (accurate for small angles, where arccos is not)."""
    D = np.asarray(R) @ np.asarray(want).T
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.degrees(np.arctan2(s, (np.trace(D) - 1.0) / 2.0)))


def direction_error(t, want):
    """The angle between two directions in degrees (atan2 of cross and dot)."""
    t, want = np.asarray(t, f8), np.asarray(want, f8)
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(t, want)), float(t @ want))))
