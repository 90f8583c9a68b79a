"""The background plate restated in numpy from the text of include/pwc_hip.h, "background plate": plate_build and
plate_difference, operation for operation in float64 (numpy forms no fused multiply-add), and the definitions of the host helpers
plate_path, plate_canvas and canvas_matrices.  The median here is a SORT of the ordered keys and a pick of rank (n - 1) // 2 --
another route than the kernel's bit-by-bit selection.  case(...) makes seeded clips; reference(...) caches their results."""
import functools
import math

import numpy as np

MEDIAN, MEAN = "median", "mean"


# ------------------------------------------------------------------ the definition
def affine_finite(M):
    """WARP's rule: the last row exactly 0 0 1, the first two rows finite."""
    return bool(M[2, 0] == 0.0 and M[2, 1] == 0.0 and M[2, 2] == 1.0 and np.isfinite(M[:2]).all())


def key(bits):
    """The ordered key of float32 bit patterns (uint32): negative floats reversed below the positive ones, -0 < +0."""
    bits = bits.astype(np.uint32)
    return np.where(bits >> 31 != 0, bits ^ np.uint32(0xFFFFFFFF), bits ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = k.astype(np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)


def _sample(M, out_h, out_w, src):
    """The SAMPLE of `src` (H,W,C) at every pixel of an out_h x out_w grid under the affine rows of M: (inside (h,w) bool,
    v (h,w,C) float64, the corner indices).  Outside pixels are sampled at (0, 0) and must be ignored."""
    H, W = src.shape[:2]
    ys, xs = np.meshgrid(np.arange(out_h, dtype=np.float64), np.arange(out_w, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        sx = ((M[0, 0] * xs) + (M[0, 1] * ys)) + M[0, 2]
        sy = ((M[1, 0] * xs) + (M[1, 1] * ys)) + M[1, 2]
        inside = (sx >= 0.0) & (sx <= float(W - 1)) & (sy >= 0.0) & (sy <= float(H - 1))
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx1, wy1 = (sx - fx0)[..., None], (sy - fy0)[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    s = src.astype(np.float64)
    with np.errstate(all="ignore"):
        top = (wx0 * s[y0, x0]) + (wx1 * s[y0, x1])
        bot = (wx0 * s[y1, x0]) + (wx1 * s[y1, x1])
        v = (wy0 * top) + (wy1 * bot)
    return inside, v, (y0, y1, x0, x1)


def _all_corners(flag, idx):
    y0, y1, x0, x1 = idx
    return flag[y0, x0] & flag[y0, x1] & flag[y1, x0] & flag[y1, x1]


def _rounded(v, dtype):
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)
    with np.errstate(all="ignore"):
        return v.astype(np.float32)


def plate_build(frames, matrices, canvas, mode=MEDIAN, use=None, masks=None, min_count=1):
    """(plate (Hc,Wc,C), count (Hc,Wc) uint8) of pwc_plate_build."""
    T, H, W, C = frames.shape
    Hc, Wc = canvas
    u8 = frames.dtype == np.uint8
    present = np.zeros((T, Hc, Wc), bool)
    values = np.zeros((T, Hc, Wc, C), np.float64)
    for t in range(T):
        if (use is not None and not use[t]) or not affine_finite(matrices[t]):
            continue
        inside, v, idx = _sample(matrices[t], Hc, Wc, frames[t])
        ok = inside
        if masks is not None:
            ok = ok & _all_corners(masks[t] != 0, idx)
        if not u8:
            ok = ok & _all_corners(np.isfinite(frames[t]).all(axis=-1), idx)
        present[t], values[t] = ok, v
    n = present.sum(axis=0)
    if mode == MEAN:
        s = np.zeros((Hc, Wc, C), np.float64)
        for t in range(T):
            with np.errstate(all="ignore"):
                s = np.where(present[t][..., None], s + values[t], s)
        with np.errstate(all="ignore"):
            plate = _rounded(s / n[..., None].astype(np.float64), frames.dtype)
    else:
        r = _rounded(values, frames.dtype)
        k = r.astype(np.int64) if u8 else key(r.view(np.uint32)).astype(np.int64)
        k = np.where(present[..., None], k, np.int64(1) << 40)              # absent samples sort behind every present one
        k = np.sort(k, axis=0)
        rank = np.maximum((n - 1) // 2, 0)
        pick = np.take_along_axis(k, np.broadcast_to(rank[None, ..., None], (1, Hc, Wc, C)), axis=0)[0]
        pick = np.where(n[..., None] > 0, pick, 0)
        plate = pick.astype(np.uint8) if u8 else unkey(pick.astype(np.uint32)).view(np.float32)
    plate = np.where((n >= min_count)[..., None], plate, np.zeros((), frames.dtype)).astype(frames.dtype)
    return np.ascontiguousarray(plate), n.astype(np.uint8)


def plate_difference(frames, plate, count, matrices, threshold, min_count=1):
    """(difference (T,H,W) float32, foreground (T,H,W) bool, known (T,H,W) bool) of pwc_plate_difference."""
    T, H, W, C = frames.shape
    u8 = frames.dtype == np.uint8
    difference = np.zeros((T, H, W), np.float32)
    foreground = np.zeros((T, H, W), bool)
    known = np.zeros((T, H, W), bool)
    for t in range(T):
        if not affine_finite(matrices[t]):
            continue
        inside, s, idx = _sample(matrices[t], H, W, plate)
        ok = inside & _all_corners(count >= min_count, idx)
        if not u8:
            ok = ok & np.isfinite(frames[t]).all(axis=-1) & _all_corners(np.isfinite(plate).all(axis=-1), idx)
        d = np.zeros((H, W), np.float64)
        with np.errstate(all="ignore"):
            for c in range(C):
                e = np.abs(frames[t, ..., c].astype(np.float64) - s[..., c])
                d = np.where(e > d, e, d)
            difference[t] = np.where(ok, d.astype(np.float32), np.float32(0.0))
            foreground[t] = ok & (d > threshold)
        known[t] = ok
    return difference, foreground, known


# ------------------------------------------------------------------ the host helpers' definitions
def plate_path(matrices, ok=None, anchor=0):
    M = np.asarray(matrices, np.float64)
    T = M.shape[0]
    ok = np.ones(T, bool) if ok is None else np.asarray(ok, bool)
    P = np.tile(np.eye(3), (T + 1, 1, 1))
    reach = np.zeros(T + 1, bool)
    reach[anchor] = True
    t = anchor
    while t < T and ok[t]:
        P[t + 1] = M[t] @ P[t]
        P[t + 1, 2] = (0.0, 0.0, 1.0)
        reach[t + 1] = True
        t += 1
    t = anchor - 1
    while t >= 0 and ok[t]:
        P[t] = np.linalg.inv(M[t]) @ P[t + 1]
        P[t, 2] = (0.0, 0.0, 1.0)
        reach[t] = True
        t -= 1
    return P, reach


def plate_canvas(to_frame, reach, H, W, margin=0):
    pts = np.array([[0.0, 0.0, 1.0], [W - 1.0, 0.0, 1.0], [0.0, H - 1.0, 1.0], [W - 1.0, H - 1.0, 1.0]]).T
    q = np.concatenate([np.linalg.inv(to_frame[t]) @ pts for t in range(len(reach)) if reach[t]], axis=1)
    x0, x1 = math.floor(q[0].min()) - margin, math.ceil(q[0].max()) + margin
    y0, y1 = math.floor(q[1].min()) - margin, math.ceil(q[1].max()) + margin
    return x0, y0, y1 - y0 + 1, x1 - x0 + 1


def canvas_matrices(to_frame, x0, y0):
    shift = np.array([[1.0, 0.0, float(x0)], [0.0, 1.0, float(y0)], [0.0, 0.0, 1.0]])
    mats = np.asarray(to_frame, np.float64) @ shift
    mats[:, 2] = (0.0, 0.0, 1.0)
    inv = np.stack([np.linalg.inv(m) for m in mats])
    inv[:, 2] = (0.0, 0.0, 1.0)
    return mats, inv


# ------------------------------------------------------------------ cases
def smooth_field(rs, shape, amp, cells=4):
    """A smooth random field of the given (H, W) shape in [-amp, amp]: bilinear interpolation of a coarse random grid."""
    H, W = shape
    gh, gw = max(2, -(-H // cells) + 1), max(2, -(-W // cells) + 1)
    grid = rs.uniform(-amp, amp, size=(gh, gw))
    yy, xx = np.arange(H) / cells, np.arange(W) / cells
    y0, x0 = np.minimum(yy.astype(int), gh - 2), np.minimum(xx.astype(int), gw - 2)
    wy, wx = (yy - y0)[:, None], (xx - x0)[None, :]
    return ((1 - wy) * ((1 - wx) * grid[y0][:, x0] + wx * grid[y0][:, x0 + 1]) +
            wy * ((1 - wx) * grid[y0 + 1][:, x0] + wx * grid[y0 + 1][:, x0 + 1]))


@functools.lru_cache(maxsize=None)
def case(T, H, W, Hc, Wc, C, dtype, special=False, seed=11):
    """A seeded clip, read-only:
      frames    (T,H,W,C) uint8 / float32 in [0, 1]: one smooth picture, a few grey levels of noise per frame, and a bright
                square that sits elsewhere in every frame
      matrices  (T,3,3) float64, canvas -> frame: the offset that centres the frame on the canvas, a shift of up to 4 px, a
                rotation of up to 3 degrees about the frame's centre and a scale in 0.95 .. 1.05; every third frame (from 0) a
                pure integer shift, whose samples are the frame's own values.  Part of the canvas is seen by no frame, part by all.
      frame_matrices  their inverses (frame -> canvas), last row 0 0 1
      masks     (T,H,W) uint8 with a rectangle of zeros in every frame;  use  (T,) uint8 with frame 1 (if any) switched off
    special (float frames): a block of -0.0 in the even and +0.0 in the odd frames, a block that holds 0.25 in every frame
    (duplicates), and an Inf, a -Inf and a NaN at single pixels of three frames."""
    rs = np.random.RandomState(seed + 1000 * T + 31 * H + 7 * W + C)
    picture = np.stack([smooth_field(rs, (H, W), 90.0) + 128.0 for _ in range(C)], axis=-1)
    levels = picture[None] + rs.normal(0.0, 5.0, size=(T, H, W, C))
    for t in range(T):
        y, x = (2 + 5 * t) % max(H - 3, 1), (3 + 7 * t) % max(W - 3, 1)
        levels[t, y:y + 4, x:x + 4] = 250.0
    if np.dtype(dtype) == np.uint8:
        frames = np.clip(np.rint(levels), 0, 255).astype(np.uint8)
    else:
        frames = (np.clip(levels, 0, 255) / 255.0).astype(np.float32)
        if special:
            frames[0::2, H // 2 - 4:H // 2 + 8, 2:18] = -0.0
            frames[1::2, H // 2 - 4:H // 2 + 8, 2:18] = 0.0
            frames[:, 1:6, W // 2:W // 2 + 8] = 0.25
            frames[0, min(3, H - 1), min(4, W - 1), 0] = np.inf
            frames[1 % T, H - 1, W - 1, C - 1] = -np.inf
            frames[2 % T, H // 3, W // 3, 0] = np.nan
    matrices = np.zeros((T, 3, 3), np.float64)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    ox, oy = (Wc - W) // 2, (Hc - H) // 2
    for t in range(T):
        if t % 3 == 0:
            A = np.eye(2)
            shift = rs.randint(-3, 4, size=2).astype(np.float64)
        else:
            ang, sc = np.deg2rad(rs.uniform(-3.0, 3.0)), rs.uniform(0.95, 1.05)
            A = sc * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
            shift = rs.uniform(-4.0, 4.0, size=2)
        # canvas (x, y) -> frame: p = A ((x - ox, y - oy) - centre) + centre + shift
        b = np.array([cx, cy]) + shift - A @ np.array([cx + ox, cy + oy])
        matrices[t] = [[A[0, 0], A[0, 1], b[0]], [A[1, 0], A[1, 1], b[1]], [0.0, 0.0, 1.0]]
    frame_matrices = np.stack([np.linalg.inv(m) for m in matrices])
    frame_matrices[:, 2] = (0.0, 0.0, 1.0)
    masks = np.ones((T, H, W), np.uint8)
    for t in range(T):
        y, x = (H // 3 + 2 * t) % H, (W // 4 + 3 * t) % W
        masks[t, y:y + 3, x:x + 5] = 0
    use = np.ones(T, np.uint8)
    if T > 1:
        use[1] = 0
    out = dict(frames=frames, matrices=matrices, frame_matrices=frame_matrices, masks=masks, use=use)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(T, H, W, Hc, Wc, C, dtype, mode, masks=False, use=False, min_count=1, special=False, threshold=None):
    """(plate, count[, difference, foreground, known]) of the restatement on case(...), computed once per process; read-only.
    threshold: also the difference of the case's frames against that plate."""
    c = case(T, H, W, Hc, Wc, C, dtype, special)
    out = plate_build(c["frames"], c["matrices"], (Hc, Wc), mode, c["use"] if use else None, c["masks"] if masks else None, min_count)
    if threshold is not None:
        out = out + plate_difference(c["frames"], out[0], out[1], c["frame_matrices"], threshold, min_count)
    for a in out:
        a.setflags(write=False)
    return out
