"""Yardstick of the temporal filter (pwcnet_amd.temporal, csrc/pwc_temporal.hip): the definition of include/pwc_hip.h, "temporal
filter", restated in numpy float64, vectorised over the pixels of one output frame, the carried position rounded to float32
explicitly and every operation in the stated order -- the kernel forms no fused multiply-add, so the GPU tests ask for BIT
equality -- and the seeded cases of those tests.  Not a test file; tests/test_host_temporal.py checks it without a GPU: its step
against tests/track_ref.py's on the same inputs, hand-made clips whose result is known, and its pieces against one call.

For output frame i and pixel p: acc = a(p), wsum = 1; for s = +1 then -1, q = p, k = 1 .. R: frame i + s k outside the clip ends
the direction; one step of track_points (any outcome but VISIBLE ends the direction); d2 = the mean over the patch offsets inside
the frame and the channels of (a(p + o) - b(q + o))^2, b the bilinear sample of frame i + s k with q's fractional part and the
corner coordinates clamped to the frame; w = 1 / (1 + d2 / sigma^2), 0 beyond max_distance; acc += w b(q), wsum += w.
"""
import functools

import numpy as np

VISIBLE, LEFT, OCCLUDED, UNKNOWN = 1, 2, 3, 4
SENTINEL = 1e10


def _known(c):
    with np.errstate(invalid="ignore"):
        return (np.abs(c) <= np.float32(1e9)).all(axis=-1)


def _inside(qx, qy, H, W):
    with np.errstate(invalid="ignore"):
        return (qx >= 0.0) & (qx <= float(W - 1)) & (qy >= 0.0) & (qy <= float(H - 1))


def _sample_flow(F, M, qx, qy, ok):
    """(good (n,), S (n,2) float64): the flow F (H,W,2), mask M or None, sampled at the points that are `ok` (inside the frame)."""
    H, W, _ = F.shape
    qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
    fx0, fy0 = np.floor(qx), np.floor(qy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx, wy = (qx - fx0)[:, None], (qy - fy0)[:, None]
    corners = ((y0, x0), (y0, x1), (y1, x0), (y1, x1))
    good = ok.copy()
    if M is not None:
        for cy, cx in corners:
            good &= M[cy, cx] != 0
    for cy, cx in corners:
        good = good & _known(F[cy, cx])
    c00, c01, c10, c11 = (np.where(good[:, None], F[cy, cx].astype(np.float64), 0.0) for cy, cx in corners)
    ux, uy = 1.0 - wx, 1.0 - wy
    return good, (uy * ((ux * c00) + (wx * c01))) + (wy * ((ux * c10) + (wx * c11)))


def step(F, Fm, G, Gm, x, y, live, alpha1, alpha2):
    """One step of the points that are `live` (VISIBLE going in): (x, y float32 (n,), status (n,) uint8).  The status of a point
    that is not live is 0 and its position is kept; LEFT, UNKNOWN and OCCLUDED keep the position they had, as a direction that
    has ended never reads it again."""
    H, W, _ = F.shape
    a1, a2 = np.float64(np.float32(alpha1)), np.float64(np.float32(alpha2))
    qx, qy = x.astype(np.float64), y.astype(np.float64)
    in_a = live & _inside(qx, qy, H, W)
    ok_b, S = _sample_flow(F, Fm, qx, qy, in_a)
    rx, ry = qx + S[:, 0], qy + S[:, 1]
    in_c = ok_b & _inside(rx, ry, H, W)
    status = np.zeros(x.shape, np.uint8)
    status[live & ~in_a] = LEFT
    status[in_a & ~ok_b] = UNKNOWN
    status[ok_b & ~in_c] = LEFT
    through = in_c
    if G is not None:
        ok_d, b = _sample_flow(G, Gm, rx, ry, in_c)
        d0, d1 = S[:, 0] + b[:, 0], S[:, 1] + b[:, 1]
        bound = (a1 * (((S[:, 0] * S[:, 0]) + (S[:, 1] * S[:, 1])) + ((b[:, 0] * b[:, 0]) + (b[:, 1] * b[:, 1])))) + a2
        margin = bound - ((d0 * d0) + (d1 * d1))
        with np.errstate(invalid="ignore"):
            fine = margin >= 0.0
        status[in_c & ~ok_d] = UNKNOWN
        status[ok_d & ~fine] = OCCLUDED
        through = ok_d & fine
    status[through] = VISIBLE
    with np.errstate(invalid="ignore", over="ignore"):
        nx = np.where(through, rx.astype(np.float32), x).astype(np.float32)
        ny = np.where(through, ry.astype(np.float32), y).astype(np.float32)
    return nx, ny, status


def grey(frames):
    """The grey levels (float64) of a clip: the byte, or 255 v with a NaN read as 0."""
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        return frames.astype(np.float64)
    assert frames.dtype == np.float32
    v = frames.astype(np.float64)
    return np.where(np.isnan(v), 0.0, 255.0 * v)


def temporal_filter(frames, flows_fw, flows_bw, radius=2, sigma=10.0, patch=1, fb_check=True, alpha1=0.01, alpha2=0.5,
                    max_distance=None, valids_fw=None, valids_bw=None, out_range=None, details=False):
    """(filtered, support) of pwcnet_amd.temporal_filter on numpy arrays; details: also a dict with status (n, 2, R, H, W) uint8,
    how the step to frame i + k (direction 0) or i - k (direction 1) ended (0: not taken), and weight (n, 2, R, H, W) float64."""
    frames = np.asarray(frames)
    T, H, W, C = frames.shape
    R, P = int(radius), int(patch)
    i0, i1 = (0, T) if out_range is None else out_range
    g = grey(frames)
    s2 = np.float64(sigma) * np.float64(sigma)
    md_on = max_distance is not None and max_distance > 0
    md2 = np.float64(max_distance) * np.float64(max_distance) if md_on else None
    py, px = (a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    n = py.size
    offsets = [(oy, ox) for oy in range(-P, P + 1) for ox in range(-P, P + 1)]
    inside = {(oy, ox): (px + ox >= 0) & (px + ox < W) & (py + oy >= 0) & (py + oy < H) for oy, ox in offsets}
    count = (sum(m.astype(np.int64) for m in inside.values()) * C).astype(np.float64)
    filtered = np.zeros((i1 - i0, H, W, C), frames.dtype)
    support = np.zeros((i1 - i0, H, W), np.uint8)
    info = dict(status=np.zeros((i1 - i0, 2, R, H, W), np.uint8), weight=np.zeros((i1 - i0, 2, R, H, W), np.float64))
    vf = (lambda j: None) if valids_fw is None else (lambda j: np.asarray(valids_fw[j]))
    vb = (lambda j: None) if valids_bw is None else (lambda j: np.asarray(valids_bw[j]))
    for i in range(i0, i1):
        own = g[i]
        acc = own[py, px].copy()                                               # (n, C)
        wsum = np.ones(n, np.float64)
        sup = np.zeros(n, np.int64)
        for d in range(2):
            x, y = px.astype(np.float32), py.astype(np.float32)
            alive = np.ones(n, bool)
            for k in range(1, R + 1):
                f = i - k if d else i + k
                if f < 0 or f >= T:
                    break
                j = i - k if d else i + k - 1
                F, Fm, G, Gm = (flows_bw[j], vb(j), flows_fw[j], vf(j)) if d else (flows_fw[j], vf(j), flows_bw[j], vb(j))
                x, y, st = step(np.asarray(F), Fm, np.asarray(G) if fb_check else None, Gm if fb_check else None, x, y, alive, alpha1, alpha2)
                info["status"][i - i0, d, k - 1] = st.reshape(H, W)
                alive = alive & (st == VISIBLE)
                qx, qy = np.where(alive, x, 0).astype(np.float64), np.where(alive, y, 0).astype(np.float64)
                fx0, fy0 = np.floor(qx), np.floor(qy)
                x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
                wx, wy = (qx - fx0)[:, None], (qy - fy0)[:, None]
                ux, uy = 1.0 - wx, 1.0 - wy
                other = g[f]
                col = lambda jx: np.clip(x0 + jx, 0, W - 1)                    # noqa: E731
                row = lambda jy: np.clip(y0 + jy, 0, H - 1)                    # noqa: E731
                h = lambda jx, jy: (ux * other[row(jy), col(jx)]) + (wx * other[row(jy), col(jx + 1)])     # noqa: E731
                total = np.zeros(n, np.float64)
                centre = None
                for oy, ox in offsets:
                    b = (uy * h(ox, oy)) + (wy * h(ox, oy + 1))
                    if (oy, ox) == (0, 0):
                        centre = b
                    a = own[np.clip(py + oy, 0, H - 1), np.clip(px + ox, 0, W - 1)]
                    for c in range(C):
                        df = a[:, c] - b[:, c]
                        total = np.where(inside[oy, ox], total + (df * df), total)
                d2 = total / count
                w = 1.0 / (1.0 + (d2 / s2))
                if md_on:
                    w = np.where(d2 > md2, 0.0, w)
                w = np.where(alive, w, 0.0)
                acc = np.where(alive[:, None], acc + (w[:, None] * centre), acc)
                wsum = np.where(alive, wsum + w, wsum)
                sup += alive & (w > 0.0)
                info["weight"][i - i0, d, k - 1] = w.reshape(H, W)
        v = acc / wsum[:, None]
        if frames.dtype == np.uint8:
            t = np.rint(v)
            out = np.where(t >= 255.0, 255, np.where(t >= 0.0, t, 0)).astype(np.uint8)
        else:
            out = (v / 255.0).astype(np.float32)
        filtered[i - i0] = out.reshape(H, W, C)
        support[i - i0] = sup.reshape(H, W).astype(np.uint8)
    return (filtered, support, info) if details else (filtered, support)


def plan_windows(T, radius, batch):
    """pwcnet_amd.temporal.plan_windows, restated."""
    pieces = []
    for o in range(0, T, batch):
        e = min(o + batch, T)
        pieces.append((max(o - radius, 0), min(e + radius, T), o, e))
    return pieces


def by_pieces(frames, flows_fw, flows_bw, radius, batch, valids_fw=None, valids_bw=None, run=temporal_filter, **kw):
    """The clip fed by plan_windows' pieces to `run` (the restatement, or a wrapper of the GPU call), concatenated."""
    T = frames.shape[0]
    outs = []
    for cs, ce, o0, o1 in plan_windows(T, radius, batch):
        outs.append(run(frames[cs:ce], flows_fw[cs:ce - 1], flows_bw[cs:ce - 1], radius=radius,
                        valids_fw=None if valids_fw is None else valids_fw[cs:ce - 1],
                        valids_bw=None if valids_bw is None else valids_bw[cs:ce - 1], out_range=(o0 - cs, o1 - cs), **kw)[:2])
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


# ------------------------------------------------------------------ cases
def smooth_field(rs, shape, amp, cells=6):
    """A smooth random field of the given (H, W) shape in [-amp, amp]: bilinear interpolation of a coarse random grid."""
    H, W = shape
    gh, gw = max(2, -(-H // cells) + 1), max(2, -(-W // cells) + 1)
    grid = rs.uniform(-amp, amp, size=(gh, gw))
    yy, xx = np.arange(H) / cells, np.arange(W) / cells
    y0, x0 = np.minimum(yy.astype(int), gh - 2), np.minimum(xx.astype(int), gw - 2)
    wy, wx = (yy - y0)[:, None], (xx - x0)[None, :]
    return ((1 - wy) * ((1 - wx) * grid[y0][:, x0] + wx * grid[y0][:, x0 + 1]) +
            wy * ((1 - wx) * grid[y0 + 1][:, x0] + wx * grid[y0 + 1][:, x0 + 1]))


def _lookup(field, x, y):
    """Bilinear lookup (float64, clamped) of an (H, W, 2) field."""
    H, W, _ = field.shape
    x, y = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    x0, y0 = np.minimum(np.floor(x).astype(int), max(W - 2, 0)), np.minimum(np.floor(y).astype(int), max(H - 2, 0))
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx, wy = (x - x0)[..., None], (y - y0)[..., None]
    return (1 - wy) * ((1 - wx) * field[y0, x0] + wx * field[y0, x1]) + wy * ((1 - wx) * field[y1, x0] + wx * field[y1, x1])


@functools.lru_cache(maxsize=None)
def case(T, H, W, C, dtype, seed=5, amp=2.5):
    """A seeded clip, read-only:
      frames            (T,H,W,C) uint8 / float32 in [0, 1]: a smooth picture plus noise of a few grey levels per frame
      fw, bw            (T-1,H,W,2) float32: smooth random flows of up to amp pixels; bw[j] is the negative of fw[j] looked up where
                        the pixel came from (two fixed-point rounds) plus uniform noise of 0.05 px -- consistent with fw[j] -- but for
                        a band of columns where 3 px are added, so that the forward-backward check fails there
      fw_s, bw_s        the same flows with the .flo sentinel, a NaN and an Inf at a few pixels of each (frames of 16 pixels and more)
      valid_fw, valid_bw  (T-1,H,W) uint8 with a rectangle of zeros each; fw_nan, bw_nan: fw_s, bw_s with NaN behind the zeros."""
    rs = np.random.RandomState(seed + 1000 * T + 31 * H + W)
    picture = np.stack([smooth_field(rs, (H, W), 90.0, cells=4) + 128.0 for _ in range(C)], axis=-1)
    levels = picture[None] + rs.normal(0.0, 6.0, size=(T, H, W, C)) + 10.0 * rs.uniform(-1, 1, size=(T, 1, 1, 1))
    if np.dtype(dtype) == np.uint8:
        frames = np.clip(np.rint(levels), 0, 255).astype(np.uint8)
    else:
        frames = (np.clip(levels, 0, 255) / 255.0).astype(np.float32)
    n = max(T - 1, 0)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fw = np.zeros((n, H, W, 2), np.float32)
    bw = np.zeros((n, H, W, 2), np.float32)
    for j in range(n):
        f = np.stack([smooth_field(rs, (H, W), amp), smooth_field(rs, (H, W), amp)], axis=-1)
        back = -_lookup(f, xs, ys)
        for _ in range(2):
            back = -_lookup(f, xs + back[..., 0], ys + back[..., 1])
        back = back + rs.uniform(-0.05, 0.05, size=back.shape)
        lo = (W // 3 + 2 * j) % max(W, 1)
        back[:, lo:lo + max(W // 8, 1)] += 3.0
        fw[j], bw[j] = f.astype(np.float32), back.astype(np.float32)
    if H == 1:                                                                 # a one-row frame: only a zero keeps a walk inside
        fw[..., 1], bw[..., 1] = 0.0, 0.0
    if W == 1:
        fw[..., 0], bw[..., 0] = 0.0, 0.0
    fw_s, bw_s = fw.copy(), bw.copy()
    valid_fw, valid_bw = np.ones((n, H, W), np.uint8), np.ones((n, H, W), np.uint8)
    for j in range(n):
        y, x = (3 + 2 * j) % H, (5 + 3 * j) % W
        if H * W >= 16:                                                        # (a smaller frame would be unknown all over)
            fw_s[j, y, x, 0] = SENTINEL
            fw_s[j, (y + 1) % H, x, 1] = np.nan
            bw_s[j, (y + 5) % H, (x + 7) % W] = (np.inf, SENTINEL)
        valid_fw[j, (H // 2):(H // 2 + 3), (W // 4):(W // 4 + 4)] = 0
        valid_bw[j, (H // 3):(H // 3 + 2), (W // 2):(W // 2 + 5)] = 0
    fw_nan, bw_nan = fw_s.copy(), bw_s.copy()
    fw_nan[valid_fw == 0] = np.nan
    bw_nan[valid_bw == 0] = np.nan
    out = dict(frames=frames, fw=fw, bw=bw, fw_s=fw_s, bw_s=bw_s, valid_fw=valid_fw, valid_bw=valid_bw, fw_nan=fw_nan, bw_nan=bw_nan)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(T, H, W, C, dtype, radius, patch, masks, fb_check, max_distance):
    """(filtered, support, details) of the restatement on case(T, H, W, C, dtype) -- the sentinel flows, with the masks where
    `masks` -- computed once per process; read-only."""
    c = case(T, H, W, C, dtype)
    return temporal_filter(c["frames"], c["fw_s"], c["bw_s"], radius=radius, patch=patch, fb_check=fb_check, max_distance=max_distance,
                           valids_fw=c["valid_fw"] if masks else None, valids_bw=c["valid_bw"] if masks else None, details=True)
