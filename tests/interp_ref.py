"""Numpy float64 restatement of pwc_interp.hip (include/pwc_hip.h, "frame interpolation"), operation for operation.

    interpolate(frames_0, frames_1, flows_fw, flows_bw, times, ...) -> dict

Every step is the kernel's IEEE double operation in the kernel's order; the fixed-point rounding of each contribution is stated
explicitly (np.rint(v * 2**36) into int64 sums), so the sums, the `source` codes and the quotients are the kernel's up to exp.
Besides the outputs the dict holds, per output element and direction, the number of contributions `cnt`, the denominators `den`,
the ranges `rng`, the quotients `c`, the unrounded value `value`, and the arguments `exp_args` exp was called with.
"""
import numpy as np

FIX = 2.0 ** 36
CLAMP = 10.0
SHAPES = [(2, 13, 19, 3), (1, 1, 7, 1), (1, 5, 1, 2), (3, 16, 16, 16)]       # (N, H, W, M)
MIN_RANGE = 0.5
ALPHA = 20.0


def to_double(frames):
    """A frame as the kernel reads it: a byte v is v / 255.0, a float32 is widened."""
    if frames.dtype == np.uint8:
        return frames.astype(np.float64) / 255.0
    assert frames.dtype == np.float32
    return frames.astype(np.float64)


def known(flow):
    """flow_io.flow_valid's rule: both components finite and at most 1e9 in magnitude."""
    with np.errstate(invalid="ignore"):
        return (np.abs(flow[..., 0]) <= np.float32(1e9)) & (np.abs(flow[..., 1]) <= np.float32(1e9))


def match_weight(own, other, f0, f1, alpha):
    """exp(-min(alpha e, 10)) per pixel of (N,H,W); exp(-10) where the flow points out of the other frame.  Returns (w, args)."""
    N, H, W, _ = own.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore"):
        qx, qy = xs[None] + f0, ys[None] + f1
        inside = (qx >= 0.0) & (qx <= W - 1) & (qy >= 0.0) & (qy <= H - 1)
    qx, qy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)
    fx0, fy0 = np.floor(qx), np.floor(qy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx1, wy1 = qx - fx0, qy - fy0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    n = np.arange(N)[:, None, None]
    e = np.zeros((N, H, W))
    for c in range(3):
        o = other[..., c]
        top = wx0 * o[n, y0, x0] + wx1 * o[n, y0, x1]
        bot = wx0 * o[n, y1, x0] + wx1 * o[n, y1, x1]
        e = e + np.abs(own[..., c] - (wy0 * top + wy1 * bot))
    e = e / 3.0
    ae = alpha * e
    args = -np.where(inside, np.where(ae < CLAMP, ae, CLAMP), CLAMP)
    return np.exp(args), args


def interpolate(frames_0, frames_1, flows_fw, flows_bw, times, alpha=ALPHA, min_range=MIN_RANGE, valid_fw=None, valid_bw=None,
                weights_fw=None, weights_bw=None):
    times = np.atleast_1d(np.asarray(times, np.float64))
    assert frames_0.dtype == frames_1.dtype and 1 <= times.size <= 16 and ((times >= 0) & (times <= 1)).all()
    alpha, min_range = np.float64(np.float32(alpha)), np.float64(np.float32(min_range))
    N, H, W, _ = flows_fw.shape
    M = times.size
    col = [to_double(frames_0), to_double(frames_1)]
    flows, valids, weights = [flows_fw, flows_bw], [valid_fw, valid_bw], [weights_fw, weights_bw]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    acc = np.zeros((2, 5, N * M * H * W), np.int64)
    cnt = np.zeros((2, N * M * H * W), np.int64)
    exp_args = []
    for k in range(2):
        keep = known(flows[k])
        if valids[k] is not None:
            keep &= valids[k].astype(bool)
        f0 = np.where(keep, flows[k][..., 0], np.float32(0)).astype(np.float64)
        f1 = np.where(keep, flows[k][..., 1], np.float32(0)).astype(np.float64)
        if weights[k] is not None:
            w = weights[k].astype(np.float64)
            with np.errstate(invalid="ignore"):
                keep &= (w >= 0.0) & (w < np.inf)
            assert not (w[keep] >= 2.0 ** 26).any(), "the poison case is not restated"
            w = np.where(keep, w, 0.0)
        else:
            w, args = match_weight(col[k], col[1 - k], f0, f1, alpha)
            exp_args.append(args[keep])
        n_idx = np.broadcast_to(np.arange(N)[:, None, None], (N, H, W))
        for m in range(M):
            s = times[m] if k == 0 else 1.0 - times[m]
            px, py = xs[None] + s * f0, ys[None] + s * f1
            ok = keep & (px > -1.0) & (px < W) & (py > -1.0) & (py < H)
            fx0, fy0 = np.floor(px), np.floor(py)
            wx, wy = px - fx0, py - fy0
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            for corner in range(4):
                dx, dy = corner & 1, corner >> 1
                cx, cy = x0 + dx, y0 + dy
                sel = ok & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
                b = ((wx if dx else 1.0 - wx) * (wy if dy else 1.0 - wy))[sel]
                bw = b * w[sel]
                t = ((n_idx[sel] * M + m) * H + cy[sel]) * W + cx[sel]
                for j in range(3):
                    np.add.at(acc[k, j], t, np.rint(bw * col[k][..., j][sel] * FIX).astype(np.int64))
                np.add.at(acc[k, 3], t, np.rint(bw * FIX).astype(np.int64))
                np.add.at(acc[k, 4], t, np.rint(b * FIX).astype(np.int64))
                np.add.at(cnt[k], t, (b != 0.0).astype(np.int64))           # (b == 0: five exact zeros, no rounding)
    acc = acc.reshape(2, 5, N, M, H, W)
    cnt = cnt.reshape(2, N, M, H, W)
    rng = acc[:, 4].astype(np.float64) * (1.0 / FIX)
    covered = (rng >= min_range) & (acc[:, 3] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = acc[:, :3].astype(np.float64) / acc[:, 3].astype(np.float64)[:, None]          # (2, 3, N, M, H, W)
    source = (covered[0].astype(np.uint8) + 2 * covered[1].astype(np.uint8)).astype(np.uint8)
    a0 = (1.0 - times)[None, :, None, None, None]
    a1 = times[None, :, None, None, None]
    c0, c1 = np.moveaxis(c[0], 0, -1), np.moveaxis(c[1], 0, -1)                                 # (N, M, H, W, 3)
    fade0, fade1 = col[0][:, None], col[1][:, None]
    code = source[..., None]
    both = a0 * np.where(code == 3, c0, fade0) + a1 * np.where(code == 3, c1, fade1)
    value = np.where(code == 1, c0, np.where(code == 2, c1, both))
    if frames_0.dtype == np.uint8:
        frames_t = np.clip(np.rint(255.0 * value), 0.0, 255.0).astype(np.uint8)
    else:
        frames_t = value.astype(np.float32)
    return dict(frames_t=frames_t, source=source, value=value, cnt=np.moveaxis(cnt, 0, -1), den=np.moveaxis(acc[:, 3], 0, -1)
                .astype(np.float64) * (1.0 / FIX), rng=np.moveaxis(rng, 0, -1), c=np.stack([c0, c1], axis=-2),
                covered=np.moveaxis(covered, 0, -1), exp_args=np.concatenate(exp_args) if exp_args else np.zeros(0),
                times=times)


def near_threshold(ref, min_range=MIN_RANGE):
    """(N,M,H,W) bool: the outputs whose range_k lies within cnt_k 2^-37 (1 + 2^-20) of min_range in either direction -- the
    pixels whose `source` code a comparison leaves out."""
    e = ref["cnt"] * 2.0 ** -37 * (1.0 + 2.0 ** -20)
    return (np.abs(ref["rng"] - np.float64(np.float32(min_range))) <= e).any(axis=-1)


# ---------------------------------------------------------------- seeded inputs
def build_inputs(N, H, W, seed=0, dtype=np.float32, block=3):
    """Frames that match along smooth flows in most places, and flows whose blocks of `block` x `block` pixels are, by a seeded
    draw, ordinary, unknown in one direction (the .flo sentinel, a NaN), unknown in both, or fast (up to 3 px: collisions and
    real holes).  Masks drop a further 5 % of the sources."""
    rs = np.random.RandomState(1000 + seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(0.7 * xs + 0.3 * ys + c) for c in range(3)], axis=-1)
    f0 = np.clip(base[None] + rs.uniform(-0.05, 0.05, size=(N, H, W, 3)), 0, 1)
    f1 = np.clip(np.roll(base, 1, axis=1)[None] + rs.uniform(-0.05, 0.05, size=(N, H, W, 3)), 0, 1)
    fw = (np.array([1.0, 0.0]) + rs.uniform(-0.45, 0.45, size=(N, H, W, 2))).astype(np.float32)
    bw = (np.array([-1.0, 0.0]) + rs.uniform(-0.45, 0.45, size=(N, H, W, 2))).astype(np.float32)
    kind = rs.randint(0, 6, size=(N, -(-H // block), -(-W // block)))
    kind = np.repeat(np.repeat(kind, block, axis=1), block, axis=2)[:, :H, :W]
    fast = kind == 4
    fw[fast] = rs.uniform(-3, 3, size=(int(fast.sum()), 2)).astype(np.float32)
    bw[fast] = rs.uniform(-3, 3, size=(int(fast.sum()), 2)).astype(np.float32)
    bad = [np.float32(1e10), np.float32("nan"), np.float32("inf")]
    for flow, kinds in ((bw, (1, 3)), (fw, (2, 3))):
        sel = np.isin(kind, kinds)
        flow[sel, rs.randint(0, 2, size=int(sel.sum()))] = np.asarray(bad)[rs.randint(0, 3, size=int(sel.sum()))]
    if dtype == np.uint8:
        f0, f1 = np.rint(255 * f0).astype(np.uint8), np.rint(255 * f1).astype(np.uint8)
    else:
        f0, f1 = f0.astype(np.float32), f1.astype(np.float32)
    valid_fw = (rs.uniform(size=(N, H, W)) >= 0.05).astype(np.uint8)
    valid_bw = (rs.uniform(size=(N, H, W)) >= 0.05).astype(np.uint8)
    return dict(frames_0=f0, frames_1=f1, flows_fw=fw, flows_bw=bw, valid_fw=valid_fw, valid_bw=valid_bw)


def times_of(M):
    """M times in [0, 1]: the in-betweens k / (M + 1), and from M = 4 on the two ends as well."""
    if M >= 4:
        return [k / (M - 1) for k in range(M)]
    return [k / (M + 1) for k in range(1, M + 1)]


_CACHE = {}


def case(shape, dtype=np.float32, masks=True, given_weights=False):
    """(inputs, kwargs, reference) of a seeded case, computed once and shared; nobody writes into them."""
    key = (tuple(shape), np.dtype(dtype).name, masks, given_weights)
    if key not in _CACHE:
        N, H, W, M = shape
        inp = build_inputs(N, H, W, seed=SHAPES.index(tuple(shape)) if tuple(shape) in SHAPES else 99, dtype=dtype)
        if not masks:
            inp["valid_fw"] = inp["valid_bw"] = None
        kw = dict(times=times_of(M))
        if given_weights:
            rs = np.random.RandomState(77)
            for k in ("weights_fw", "weights_bw"):
                w = rs.uniform(0.01, 4.0, size=(N, H, W)).astype(np.float32)
                w[rs.uniform(size=w.shape) < 0.03] = np.float32(-1.0)
                w[rs.uniform(size=w.shape) < 0.03] = np.float32("nan")
                kw[k] = w
        for a in list(inp.values()) + [v for v in kw.values() if isinstance(v, np.ndarray)]:
            if a is not None:
                a.setflags(write=False)
        _CACHE[key] = (inp, kw, interpolate(**inp, **kw))
    return _CACHE[key]
