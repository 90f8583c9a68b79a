"""Yardstick of the training augmentation (pwcnet_amd/augment.py, csrc/pwc_augment.hip): its arithmetic restated in numpy.  Run in
float64 (the default) it is the reference, unrounded; run with dtype=np.float32 every step of it -- the records, the sample
coordinates, the weights, the blends, the colour formula, the flow's way through I1 -- is float32 arithmetic, the planted fault
that shows the tests' bound can tell "formed in double, rounded once" from a straightforward float32 composition.  Not a test
file; tests/test_host_augment.py validates it without a GPU, tests/test_gpu_augment.py holds the kernel to it.

Per sample a record of 32 doubles (include/pwc_hip.h): M0 (0..5), M1 (6..11), I1 = M1^-1 (12..17), the photometric records of
frame 0 (18..23) and frame 1 (24..29): gain r, g, b; gamma; contrast; brightness.  Output pixel p = (x, y):
    q0 = M0 p, q1 = M1 p                       (m[0] x + m[1] y) + m[2], every operation rounded on its own
    frame value: q clamped into the frame, x0 = floor(qx), fx = qx - x0, x1 = min(x0 + 1, W - 1), likewise y,
                 (1 - fy) ((1 - fx) a + fx b) + fy ((1 - fx) c + fx d), then unless the record is (1, 1, 1, 1, 1, 0)
                 clamp((pow(clamp(v gain_c, 0, 1), gamma) - 0.5) contrast + 0.5 + brightness, 0, 1)   (gamma == 1: no pow)
    flow: (u, v) = flow sampled at the UN-clamped q0 (bilinear, or the tap floor(q + 0.5)), out_flow = I1 (q0 + (u, v)) - p
    valid: q0 inside [0, W - 1] x [0, H - 1] and every tap used labelled (a corner of weight exactly zero is not a tap);
           elsewhere out_flow = 0.
"""
import functools

import numpy as np

PHOTO_IDENTITY = (1.0, 1.0, 1.0, 1.0, 1.0, 0.0)


def to_float32(images):
    """uint8 frames as the float32 the kernel reads them as, float(double(v) / 255.0); float32 frames as they are."""
    if images.dtype == np.uint8:
        return (images.astype(np.float64) / 255.0).astype(np.float32)
    assert images.dtype == np.float32, images.dtype
    return images


def invert(m):
    """Inverse of the affine map (a b c; d e f), float64."""
    A = np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0.0, 0.0, 1.0]], np.float64)
    return np.linalg.inv(A)[:2].reshape(6)


def record(m0, m1=None, photo0=PHOTO_IDENTITY, photo1=None):
    m1 = m0 if m1 is None else m1
    r = np.zeros(32, np.float64)
    r[0:6], r[6:12], r[12:18] = m0, m1, invert(m1)
    r[18:24], r[24:30] = photo0, photo0 if photo1 is None else photo1
    return r


def similarity(centre, crop_centre, zoom=1.0, deg=0.0, mirror=False, shift=(0.0, 0.0)):
    """The map that puts the crop's centre on `centre` + shift of the frame (x, y order), magnified by zoom, rotated, mirrored."""
    t = np.deg2rad(deg)
    lin = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.diag([-1.0 if mirror else 1.0, 1.0]) / zoom
    off = np.asarray(centre, np.float64) + np.asarray(shift, np.float64) - lin @ np.asarray(crop_centre, np.float64)
    return np.array([lin[0, 0], lin[0, 1], off[0], lin[1, 0], lin[1, 1], off[1]], np.float64)


def crop_record(y0, x0):
    return record(np.array([1.0, 0.0, x0, 0.0, 1.0, y0]))


def _map(m, x, y):
    return (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]


def _blend(a, b, c, d, fx, fy, one):
    return (one - fy) * ((one - fx) * a + fx * b) + fy * ((one - fx) * c + fx * d)


def _frame(im, ph, qx, qy, dtype):
    """im (H, W, 3) float32 -> (value (OH, OW, 3) in dtype, unrounded; S: the corners' largest magnitude)."""
    H, W = im.shape[:2]
    x = im.astype(dtype)
    qx, qy = np.clip(qx, dtype(0), dtype(W - 1)), np.clip(qy, dtype(0), dtype(H - 1))
    flx, fly = np.floor(qx), np.floor(qy)
    fx, fy = (qx - flx)[..., None], (qy - fly)[..., None]
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    a, b, c, d = x[y0, x0], x[y0, x1], x[y1, x0], x[y1, x1]
    v = _blend(a, b, c, d, fx, fy, dtype(1))
    S = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d))).astype(np.float64)
    if tuple(ph) != PHOTO_IDENTITY:
        gain, gamma, contrast, brightness = ph[0:3].astype(dtype), dtype(ph[3]), dtype(ph[4]), dtype(ph[5])
        v = np.clip(v * gain, dtype(0), dtype(1))
        if ph[3] != 1.0:
            v = np.power(v, gamma)
        v = ((v - dtype(0.5)) * contrast + dtype(0.5)) + brightness
        v = np.clip(v, dtype(0), dtype(1))
    assert v.dtype == dtype
    return v, S


def _frac_distance(q, to_half):
    f = q - np.floor(q)
    return np.abs(f - 0.5) if to_half else np.minimum(f, 1.0 - f)


def augment(im0, im1, params, crop_hw, flow=None, valid=None, nearest=False, dtype=np.float64):
    """im0, im1: (N, H, W, 3) uint8 / float32; params (N, 32) float64; flow (N, H, W, 2) float32 or None; valid (N, H, W) bool
    or None.  Returns a dict: out0, out1 (N, OH, OW, 3) in `dtype`, NOT rounded to float32; S0, S1 their scales; ulps0, ulps1
    (N,) the float32 ulps the GPU test allows (0.5, or 1 where a pow was taken); and with a flow: flow (N, OH, OW, 2), Sf (the
    corners' largest magnitude and max(H, W)), valid (N, OH, OW) bool, margin: the smallest distance (float64 px) of a sample
    coordinate from a decision boundary -- the frame's edge, .5 for nearest taps, the integers (where the set of taps changes)
    when some label of the sample is missing.  A sample whose M0 is integer-valued has exact coordinates and no margin to keep."""
    N, H, W, _ = im0.shape
    OH, OW = crop_hw
    x0f, x1f = to_float32(im0), to_float32(im1)
    ys, xs = np.meshgrid(np.arange(OH).astype(dtype), np.arange(OW).astype(dtype), indexing="ij")
    res = {k: [] for k in ("out0", "out1", "S0", "S1", "flow", "Sf", "valid")}
    res["ulps0"], res["ulps1"] = np.full(N, 0.5), np.full(N, 0.5)
    margin = np.inf
    for n in range(N):
        rec = params[n]
        r = rec.astype(dtype)
        q0x, q0y = _map(r[0:6], xs, ys)
        q1x, q1y = _map(r[6:12], xs, ys)
        assert q0x.dtype == dtype
        for k, (im, ph, qx, qy) in enumerate(((x0f[n], rec[18:24], q0x, q0y), (x1f[n], rec[24:30], q1x, q1y))):
            v, S = _frame(im, ph, qx, qy, dtype)
            res[f"out{k}"].append(v)
            res[f"S{k}"].append(S)
            if tuple(ph) != PHOTO_IDENTITY and ph[3] != 1.0:
                res[f"ulps{k}"][n] = 1.0
        if flow is None:
            continue
        fl = flow[n].astype(dtype)
        lab = np.ones((H, W), bool) if valid is None else valid[n]
        inside = (q0x >= 0) & (q0x <= W - 1) & (q0y >= 0) & (q0y <= H - 1)
        sx, sy = np.where(inside, q0x, dtype(0)), np.where(inside, q0y, dtype(0))
        if nearest:
            tx = np.minimum(np.floor(sx + dtype(0.5)).astype(np.int64), W - 1)
            ty = np.minimum(np.floor(sy + dtype(0.5)).astype(np.int64), H - 1)
            ok = inside & lab[ty, tx]
            uv = np.where(ok[..., None], fl[ty, tx], dtype(0))
            Sc = np.abs(uv).max(axis=-1)
        else:
            flx, fly = np.floor(sx), np.floor(sy)
            fx, fy = sx - flx, sy - fly
            tx0, ty0 = flx.astype(np.int64), fly.astype(np.int64)
            tx1, ty1 = np.where(fx > 0, tx0 + 1, tx0), np.where(fy > 0, ty0 + 1, ty0)
            ok = inside & lab[ty0, tx0] & lab[ty0, tx1] & lab[ty1, tx0] & lab[ty1, tx1]
            a, b, c, d = (np.where(ok[..., None], fl[yy, xx], dtype(0)) for yy, xx in ((ty0, tx0), (ty0, tx1), (ty1, tx0), (ty1, tx1)))
            uv = _blend(a, b, c, d, fx[..., None], fy[..., None], dtype(1))
            Sc = np.max(np.abs(np.stack([a, b, c, d])), axis=(0, -1))
        p1x, p1y = _map(r[12:18], q0x + uv[..., 0], q0y + uv[..., 1])
        out = np.stack([p1x - xs, p1y - ys], axis=-1)
        out = np.where(ok[..., None], out, dtype(0))
        assert out.dtype == dtype
        res["flow"].append(out)
        res["valid"].append(ok)
        res["Sf"].append(np.broadcast_to(np.maximum(Sc.astype(np.float64), float(max(H, W)))[..., None], out.shape))
        if not np.array_equal(rec[0:6], np.round(rec[0:6])):
            ex, ey = _map(rec[0:6], xs.astype(np.float64), ys.astype(np.float64))
            edge = np.minimum(np.minimum(np.abs(ex), np.abs(ex - (W - 1))), np.minimum(np.abs(ey), np.abs(ey - (H - 1))))
            margin = min(margin, float(edge.min()))
            ins = (ex >= 0) & (ex <= W - 1) & (ey >= 0) & (ey <= H - 1)
            if ins.any() and (nearest or not lab.all()):
                margin = min(margin, float(_frac_distance(ex[ins], nearest).min()), float(_frac_distance(ey[ins], nearest).min()))
    out = {k: np.stack(v) for k, v in res.items() if isinstance(v, list) and v}
    out["ulps0"], out["ulps1"] = res["ulps0"], res["ulps1"]
    if flow is not None:
        out["margin"] = margin
    return out


def ulp32(x):
    """The spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def excess(y, ref, S, ulps=0.5):
    """Per element |y - ref| - (ulps ulp32(ref) + 1e-9 S): at most 0 for a float32 `y` that is the once-rounded value of the
    float64 `ref` (1e-9 S: three orders above what a few double operations on coordinates below 2^11 px move, 30 x below a
    float32 half-ulp).  ulps: a scalar or (N,), one entry per sample."""
    ulps = np.asarray(ulps, np.float64).reshape((-1,) + (1,) * (ref.ndim - 1))
    err = np.abs(y.astype(np.float64) - ref.astype(np.float64))
    return err - (ulps * ulp32(ref) + 1e-9 * S)


# ---------------------------------------------------------------------------------------------- the GPU test's inputs
# name, N, (H, W), (OH, OW), sparse labels.  Explicit records (below), written down before any run; every one keeps the
# margin of at least 1e-6 px that exact comparison of out_valid and of the nearest taps needs (tests/test_host_augment.py asserts it).
GEOMETRIES = [
    ("2x37x53-16x24", 2, (37, 53), (16, 24), False),          # odd sizes, unaligned uint8 rows, a batch stride
    ("1x64x96-32x64", 1, (64, 96), (32, 64), False),          # zoom 1.3, rotation 17 deg, mirror, a relative transform
    ("1x5x7-1x1", 1, (5, 7), (1, 1), False),                  # a single output pixel
    ("1x24x40-24x40", 1, (24, 40), (24, 40), False),          # identity, the crop is the frame
    ("2x33x45-16x24-outside", 2, (33, 45), (16, 24), False),  # part of the crop outside: clamped frames, out_valid 0, out_flow 0
    ("2x37x53-16x24-sparse", 2, (37, 53), (16, 24), True),    # 30 % unlabelled, 1e10 planted there
]
GEOM_IDS = [g[0] for g in GEOMETRIES]
MIN_MARGIN = 1e-6


def _centres(hw, crop_hw):
    return ((hw[1] - 1) / 2.0, (hw[0] - 1) / 2.0), ((crop_hw[1] - 1) / 2.0, (crop_hw[0] - 1) / 2.0)


@functools.lru_cache(maxsize=None)
def records(g):
    _, N, hw, chw, _ = GEOMETRIES[g]
    c, pc = _centres(hw, chw)
    full = (1.1, 0.93, 1.04, 1.3, 1.15, 0.03)
    if g in (0, 5):
        m0 = similarity(c, pc, zoom=1.1, deg=5.0, shift=(1.3, -0.6))
        m1 = similarity(c, pc, zoom=1.1, deg=5.0, shift=(2.0, -1.0))
        first = record(m0, m1, full, (1.12, 0.95, 1.02, 1.3, 1.15, 0.04))
        if g == 0:                                                         # mirrored, shifted by fractions; colour without a pow
            second = record(similarity(c, pc, mirror=True, shift=(-3.37, 2.21)), None, (0.9, 1.05, 1.2, 1.0, 0.85, -0.02))
        else:                                                              # the plain crop at (5, 7): exact coordinates
            second = crop_record(5, 7)
        return np.stack([first, second])
    if g == 1:
        m0 = similarity(c, pc, zoom=1.3, deg=17.0, mirror=True, shift=(2.7, -1.9))
        m1 = similarity(c, pc, zoom=1.3 * 1.02, deg=18.5, mirror=True, shift=(4.0, -2.7))
        return record(m0, m1, (0.85, 1.1, 1.0, 0.8, 1.2, -0.05), (0.86, 1.08, 1.01, 0.8, 1.2, -0.04))[None]
    if g == 2:
        m0 = similarity((2.3, 1.6), (0.0, 0.0), zoom=0.9, deg=30.0)
        m1 = similarity((2.7, 1.9), (0.0, 0.0), zoom=0.9, deg=31.0)
        return record(m0, m1, (1.2, 0.9, 1.1, 1.0, 1.0, 0.0))[None]
    if g == 3:
        return crop_record(0, 0)[None]
    if g == 4:
        first = record(np.array([1.0, 0.0, -5.25, 0.0, 1.0, 22.3]), np.array([1.0, 0.0, -4.75, 0.0, 1.0, 22.6]))
        m0 = similarity((40.2, 3.7), pc, zoom=0.8, deg=25.0)
        m1 = similarity((41.0, 3.1), pc, zoom=0.8, deg=26.0)
        return np.stack([first, record(m0, m1, full)])
    raise IndexError(g)


@functools.lru_cache(maxsize=None)
def inputs(g):
    """(im0 uint8, im1 uint8, flow float32, valid bool or None) of geometry g, seeded."""
    _, N, (H, W), _, sparse = GEOMETRIES[g]
    rng = np.random.RandomState(700 + g)
    im0 = rng.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    im1 = rng.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    flow = rng.uniform(-8.0, 8.0, size=(N, H, W, 2)).astype(np.float32)
    valid = None
    if sparse:
        valid = rng.uniform(size=(N, H, W)) >= 0.3
        flow[~valid] = 1e10
    return im0, im1, flow, valid


@functools.lru_cache(maxsize=None)
def reference(g, nearest, dtype=np.float64):
    """The reference of geometry g (uint8 and float32 frames hold the same values: the float32 ones are to_float32 of the uint8)."""
    im0, im1, flow, valid = inputs(g)
    return augment(im0, im1, records(g), GEOMETRIES[g][3], flow, valid, nearest, dtype)


def violations(got, ref):
    """How many elements of `got` (out0, out1, flow as float32 arrays, valid as bool) miss the GPU test's bound against the
    float64 `ref`, and the worst excess: {name: (count, worst)}.  valid is compared exactly."""
    out = {}
    for k, S, ulps in (("out0", "S0", ref["ulps0"]), ("out1", "S1", ref["ulps1"]), ("flow", "Sf", 0.5)):
        e = excess(got[k], ref[k], ref[S], ulps)
        out[k] = (int((e > 0).sum()), float(e.max()))
    out["valid"] = (int((got["valid"] != ref["valid"]).sum()), 0.0)
    return out
