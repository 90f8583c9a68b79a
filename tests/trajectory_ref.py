"""numpy restatement of the scale chain and the camera trajectory, operation for operation (include/pwc_hip.h, "scale chain and
camera trajectory"): the per-pixel sample and its float32 key, the lower median as a selection by digits of 11, 11 and 10 bits, the
sequential chain, and the streaming rule.  tests/test_host_trajectory.py checks it on the CPU against a sort and the sequence
scene's truth; tests/test_gpu_trajectory.py holds the kernels to it bit for bit.

Every product, quotient and sum below is one numpy operation on float64 values in the order the kernel performs it; numpy forms no
fused multiply-add.  RAYS, TRIANGULATE and the known-pixel rule are tests/pose_ref.py's and tests/motion_ref.py's, imported, not
copied.

Also the SEQUENCE SCENE: tests/fundamental_ref.scene is one pair whose depth is given in the first camera and cannot be continued
to a third frame.  Here a gentle height field Z = h(X, Y) in world coordinates is seen by cameras with small rotations and
translations of DIFFERENT lengths; every camera's pixels are ray-cast by bisection in float64 and the points projected into the
next camera for the flow, so the truth is exact: ratio[j] = |t_j| / |t_(j-1)|, the poses, and every camera's depth map.
"""
import numpy as np

from tests import motion_ref as MR
from tests import pose_ref as PR

f8 = np.float64
SENTINEL = MR.SENTINEL
FLT_MAX = np.float32(3.4028234663852886e38)
DIGITS = ((21, 2048), (10, 2048), (0, 1024))         # (shift, bins) of the three digits of a key


# ------------------------------------------------------------------ the per-pixel sample
def _zero(R):
    return not np.asarray(R).any()


def seam_keys(flow_a, R_a, t_a, k_a, known_a, R_b, depth_b, known_b):
    """The (H,W) uint32 keys of one seam: the bits of r = (float)(Z1 / d) where pixel p of the earlier pair is a sample, else 0."""
    H, W, _ = flow_a.shape
    keys = np.zeros((H, W), np.uint32)
    k = [f8(q) for q in np.asarray(k_a, f8).reshape(4)]
    if _zero(R_a) or _zero(R_b) or not PR.intrinsics_fine(k):
        return keys
    flow_a = np.asarray(flow_a, np.float32)
    ok = (np.asarray(known_a) != 0) & MR.known_mask(flow_a[None])[0]
    with np.errstate(all="ignore"):
        qx, qy, d0x, d0y, d1x, d1y = PR.rays(flow_a, k)
        ok &= (qx >= 0.0) & (qx <= f8(W - 1)) & (qy >= 0.0) & (qy <= f8(H - 1))
        fx0, fy0 = np.floor(np.where(ok, qx, 0.0)), np.floor(np.where(ok, qy, 0.0))
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        kb = np.asarray(known_b) != 0
        ok &= kb[y0, x0] & kb[y0, x1] & kb[y1, x0] & kb[y1, x1]
        D = np.asarray(depth_b, np.float32).astype(f8)
        wx1, wy1 = qx - fx0, qy - fy0
        wx0, wy0 = f8(1.0) - wx1, f8(1.0) - wy1
        top = (wx0 * D[y0, x0]) + (wx1 * D[y0, x1])
        bot = (wx0 * D[y1, x0]) + (wx1 * D[y1, x1])
        d = (wy0 * top) + (wy1 * bot)
        _, _, _, den, _, z1 = PR.triangulate(R_a, t_a, d0x, d0y, d1x, d1y)
        ok &= (den > 0.0) & (z1 > 0.0) & (d > 0.0)
        r = (z1 / d).astype(np.float32)
        ok &= (r > np.float32(0.0)) & (r <= FLT_MAX)
    keys[ok] = r[ok].view(np.uint32)
    return keys


# ------------------------------------------------------------------ the selection
def select_key(keys):
    """(key, n): the non-zero key of rank (n - 1) // 2 in ascending order by the kernel's three digits, and n; (0, 0) for none."""
    keys = np.asarray(keys, np.uint32).reshape(-1)
    keys = keys[keys != 0]
    n = int(keys.size)
    if n == 0:
        return np.uint32(0), 0
    rank, bits = (n - 1) // 2, 0
    for shift, bins in DIGITS:
        hist = np.bincount((keys >> np.uint32(shift)).astype(np.int64) & (bins - 1), minlength=bins)
        before, b = 0, 0
        while b < bins - 1 and before + int(hist[b]) <= rank:
            before += int(hist[b])
            b += 1
        bits |= b << shift
        rank -= before
        keys = keys[((keys >> np.uint32(shift)).astype(np.int64) & (bins - 1)) == b]
    return np.uint32(bits), n


def lower_median(values):
    """The same by a sort, for positive float32 values: (value of rank (n - 1) // 2, n)."""
    v = np.sort(np.asarray(values, np.float32).reshape(-1))
    return (v[(v.size - 1) // 2], int(v.size)) if v.size else (np.float32(0.0), 0)


# ------------------------------------------------------------------ pwc_scale_links_f32
def _state_of(flows, rotation, translation, K, depth, known):
    return dict(flow=flows[-1], rotation=rotation[-1], translation=translation[-1], intrinsics=K[-1], depth=depth[-1], known=known[-1])


def links(flows, rotation, translation, intrinsics, depth, known, state=None):
    """(ratio (T,) float32, samples (T,) int32)."""
    flows = np.asarray(flows, np.float32)
    T = flows.shape[0]
    K = np.broadcast_to(np.asarray(intrinsics, f8), (T, 4))
    ratio, samples = np.zeros(T, np.float32), np.zeros(T, np.int32)
    for j in range(T):
        if j == 0 and state is None:
            continue
        a = (state["flow"], state["rotation"], state["translation"], state["intrinsics"], state["known"]) if j == 0 else \
            (flows[j - 1], rotation[j - 1], translation[j - 1], K[j - 1], known[j - 1])
        key, n = select_key(seam_keys(*a, rotation[j], depth[j], known[j]))
        ratio[j], samples[j] = np.array([key], np.uint32).view(np.float32)[0], n
    return ratio, samples


# ------------------------------------------------------------------ pwc_camera_trajectory_f64
def _identity():
    return [[f8(1.0) if r == q else f8(0.0) for q in range(3)] for r in range(3)], [f8(0.0)] * 3


def chain(rotation, translation, ratio, samples, min_samples=64, state=None):
    """dict(trajectory (T+1,3,4) f8, scales (T,) f8, segment (T,) int32, linked (T,) bool, segment_state (2,) int32)."""
    T = len(rotation)
    A, c = _identity()
    scale, seg, opened, before = f8(0.0), -1, 0, False
    if state is not None:
        row = np.asarray(state["row"], f8)
        A, c = [[row[r, q] for q in range(3)] for r in range(3)], [row[r, 3] for r in range(3)]
        scale, seg, opened = f8(state["scale"]), int(state["segment"][0]), int(state["segment"][1])
        before = not _zero(state["rotation"])
    out = dict(trajectory=np.zeros((T + 1, 3, 4), f8), scales=np.zeros(T, f8), segment=np.zeros(T, np.int32), linked=np.zeros(T, bool))

    def put(i):
        out["trajectory"][i, :, :3], out["trajectory"][i, :, 3] = np.array(A, f8), np.array(c, f8)

    for j in range(T):
        R = [[f8(rotation[j][r][q]) for q in range(3)] for r in range(3)]
        t = [f8(q) for q in translation[j]]
        ok = not _zero(rotation[j])
        rj = np.float32(ratio[j])
        link = ok and before and int(samples[j]) >= int(min_samples) and bool(rj > np.float32(0.0)) and bool(rj <= FLT_MAX)
        if ok and not link:
            A, c = _identity()
        put(j)
        if not ok:
            scale, seg = f8(0.0), -1
        elif link:
            scale = scale * f8(rj)
        else:
            scale, seg, opened = f8(1.0), opened, opened + 1
        out["scales"][j], out["segment"][j], out["linked"][j] = scale, seg, link
        if ok:
            with np.errstate(all="ignore"):
                B = [[((R[r][0] * A[0][q]) + (R[r][1] * A[1][q])) + (R[r][2] * A[2][q]) for q in range(3)] for r in range(3)]
                c = [(((R[r][0] * c[0]) + (R[r][1] * c[1])) + (R[r][2] * c[2])) + (scale * t[r]) for r in range(3)]
            A = B
        else:
            A, c = _identity()
        before = ok
    put(T)
    out["segment_state"] = np.array([seg, opened], np.int32)
    return out


def trajectory(flows, rotation, translation, intrinsics, depth, known, min_samples=64, state=None):
    """pwcnet_amd.camera_trajectory: (the chain's dict with ratio and samples added, the state for the next call)."""
    flows = np.asarray(flows, np.float32)
    T = flows.shape[0]
    K = np.broadcast_to(np.asarray(intrinsics, f8), (T, 4))
    ratio, samples = links(flows, rotation, translation, K, depth, known, state)
    out = chain(rotation, translation, ratio, samples, min_samples, state)
    out.update(ratio=ratio, samples=samples)
    nxt = _state_of(flows, rotation, translation, K, depth, known)
    nxt.update(row=out["trajectory"][T].copy(), scale=out["scales"][T - 1], segment=out["segment_state"])
    return out, nxt


KEYS = ("ratio", "samples", "linked", "scales", "segment", "trajectory")


def streamed(flows, rotation, translation, intrinsics, depth, known, batch, min_samples=64):
    """The streaming rule: the sequence in pieces of `batch` pairs, each call given the state of the one before; row 0 of a call
    replaces the last row of the call before.  The same dict as trajectory()'s."""
    T = len(flows)
    K = np.broadcast_to(np.asarray(intrinsics, f8), (T, 4))
    out = dict(trajectory=np.zeros((T + 1, 3, 4), f8), scales=np.zeros(T, f8), segment=np.zeros(T, np.int32), linked=np.zeros(T, bool),
               ratio=np.zeros(T, np.float32), samples=np.zeros(T, np.int32))
    state = None
    for i in range(0, T, batch):
        s = slice(i, min(i + batch, T))
        part, state = trajectory(flows[s], rotation[s], translation[s], K[s], depth[s], known[s], min_samples, state)
        for key in KEYS[:5]:
            out[key][s] = part[key]
        out["trajectory"][s.start:s.stop + 1] = part["trajectory"]
    return out


def flow_trajectory(flows, intrinsics, valid=None, iters=4, scale=1.0, threshold=1.0, min_parallax=0.25, min_samples=64):
    """pwcnet_amd.flow_trajectory chained from the restatements: (depth, known, the pose dict, the trajectory dict)."""
    dep, kn, _, p, _, _ = PR.flow_depth(flows, intrinsics, valid, iters, scale, threshold, min_parallax)
    out, _ = trajectory(flows, p["rotation"], p["translation"], intrinsics, dep, kn, min_samples)
    return dep, kn, p, out


# ------------------------------------------------------------------ the sequence scene
BASELINES = (0.30, 0.45, 0.20, 0.36)
DIRECTIONS = ((1.0, 0.3, 0.2), (0.8, -0.5, 0.3), (0.9, 0.2, -0.25), (0.7, 0.6, 0.15))
ROTATIONS = ((0.004, -0.006, 0.003), (-0.005, 0.004, 0.006), (0.003, 0.005, -0.004), (-0.004, -0.003, 0.005))
Z_RANGE = (4.0, 8.0)


def height(X, Y):
    """The surface Z = h(X, Y): gradient below 1 in X and 0.7 in Y, so no ray of these cameras meets it twice."""
    return 6.0 + 0.8 * np.sin(1.0 * X + 0.4) * np.cos(0.8 * Y - 0.2) + 0.15 * X


def rodrigues(w):
    w = np.asarray(w, f8)
    th = np.linalg.norm(w)
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + (np.sin(th) / th) * Kx + ((1.0 - np.cos(th)) / (th * th)) * (Kx @ Kx)


def scene_intrinsics(H, W):
    return PR.scene_intrinsics(H, W)


def scene_poses(T):
    """The true relative poses: (R (T,3,3), t (T,3) with |t_j| = BASELINES[j])."""
    R = np.stack([rodrigues(ROTATIONS[j % 4]) for j in range(T)])
    t = np.stack([np.asarray(DIRECTIONS[j % 4], f8) / np.linalg.norm(DIRECTIONS[j % 4]) * BASELINES[j % 4] for j in range(T)])
    return R, t


def scene_cameras(T):
    """World-to-camera [A | c] of the T + 1 cameras, the world being camera 0, in scene units."""
    R, t = scene_poses(T)
    A, c = [np.eye(3)], [np.zeros(3)]
    for j in range(T):
        A.append(R[j] @ A[-1])
        c.append(R[j] @ c[-1] + t[j])
    return np.stack(A), np.stack(c)


def raycast(A, c, k, H, W):
    """The depth map of camera [A | c]: per pixel the s > 0 with the point A^T (s d - c) on the surface, by bisection."""
    x, y = PR.grid(H, W)
    d = np.stack([(x - k[2]) / k[0], (y - k[3]) / k[1], np.ones_like(x)], axis=-1)
    o, v = -(A.T @ c), d @ A                                                  # the ray o + s v in the world (v = A^T d)
    lo, hi = (Z_RANGE[0] - o[2]) / v[..., 2], (Z_RANGE[1] - o[2]) / v[..., 2]
    for _ in range(64):                                                       # an interval of 4 / 2^64: below one ulp of s
        mid = 0.5 * (lo + hi)
        P = o + mid[..., None] * v
        above = P[..., 2] < height(P[..., 0], P[..., 1])                       # the point is still in front of the surface
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return 0.5 * (lo + hi)


def sequence(T, H, W):
    """dict(flows (T,H,W,2) float32, depths (T+1,H,W) f8 in scene units, R, t, A, c, K): the exact flows of the T pairs."""
    k = scene_intrinsics(H, W)
    R, t = scene_poses(T)
    A, c = scene_cameras(T)
    x, y = PR.grid(H, W)
    depths = np.stack([raycast(A[i], c[i], k, H, W) for i in range(T + 1)])
    flows = np.zeros((T, H, W, 2), np.float32)
    for j in range(T):
        X = np.stack([(x - k[2]) / k[0] * depths[j], (y - k[3]) / k[1] * depths[j], depths[j]], axis=-1) @ R[j].T + t[j]
        flows[j, ..., 0] = (k[0] * X[..., 0] / X[..., 2] + k[2]) - x
        flows[j, ..., 1] = (k[1] * X[..., 1] / X[..., 2] + k[3]) - y
    return dict(flows=flows, depths=depths, R=R, t=t, A=A, c=c, K=k)


def true_scales(T):
    b = np.array([BASELINES[j % 4] for j in range(T)], f8)
    return b / b[0]


def centre(row):
    """The camera's centre -A^T c of a (3,4) row [A | c]."""
    row = np.asarray(row, f8)
    return -(row[:, :3].T @ row[:, 3])


def scale_error(scales, T):
    return float(np.max(np.abs(np.asarray(scales, f8) / true_scales(T) - 1.0)))


def unit_centre_error(T):
    """centre_error of what there was before the chain: the true poses with every scale 1."""
    Rm, t = scene_poses(T)
    A, c = np.eye(3), np.zeros(3)
    for j in range(T):
        A, c = Rm[j] @ A, Rm[j] @ c + t[j] / np.linalg.norm(t[j])
    return centre_error(np.concatenate([A, c[:, None]], axis=1), T)


def centre_error(row, T):
    """The last camera's centre against the truth in the first pair's baseline, relative to the truth's length."""
    A, c = scene_cameras(T)
    want = -(A[T].T @ c[T]) / BASELINES[0]
    return float(np.linalg.norm(centre(row) - want) / np.linalg.norm(want))
