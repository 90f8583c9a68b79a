"""Float64 numpy restatement of pwcnet_amd.vis (csrc/pwc_flowvis.hip): what tests/test_host_vis.py pins to the host code that
exists (flow_io.flow_to_color, infer_continuous.pyramid_montage) and tests/test_gpu_vis.py compares the kernels with.

    random_flows(N, H, W, seed, integer)             the test fields
    scaled(flows, flow_scale)                        the ONE float32 product per component
    known(flows)                                     flow_io.flow_valid's rule
    max_radius(flows, valid, flow_scale)             (N,) float64
    color(flows, max_rad, valid, flow_scale)         (bytes (N,H,W,3) uint8, t (N,H,W,3) float64 = 255 * col before the floor)
    error_color(flows, flows_gt, valid)              (N,H,W,3) uint8
    frame_bytes(frames)                              uint8 through, float32 as rint(255 x) clamped, NaN -> 0
    montage(frames, flows_list, flow_scales)         (bytes (N,h,W_total,3), t (N,h,W_total,3) float64 -- NaN in the frame tile)
    white(flows, valid, flow_scale)                  the pixels that must be exactly white; montage_white(...) for a montage
    check_color(got, want, t)                        the colour rule of the GPU tests; the number of values that used the allowance
"""
import numpy as np

from pwcnet_amd import flow_io

ERR_EDGES = np.array([0.0625, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0])
ERR_COLORS = np.array([(49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144),
                       (253, 174, 97), (244, 109, 67), (215, 48, 39), (165, 0, 38)], np.uint8)
NEAR = 1e-9                                              # |t - rint(t)| below which a byte may be rint(t) or rint(t) - 1


def random_flows(N, H, W, seed, integer=False, sigma=7.0):
    """(N,H,W,2) float32: N(0, sigma^2) components, or (integer) whole numbers in -3 .. 3 -- flows along both axes and the
    diagonals, whose hues land on wheel entries."""
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-3, 4, (N, H, W, 2)).astype(np.float32)
    return (rng.standard_normal((N, H, W, 2)) * sigma).astype(np.float32)


def scaled(flows, flow_scale=1.0):
    flows = np.asarray(flows, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return flows * np.float32(flow_scale)


def known(flows):
    return flow_io.flow_valid(flows)


def _keep(flows, valid, flow_scale):
    f = scaled(flows, flow_scale)
    keep = known(f)
    if valid is not None:
        keep = keep & (np.asarray(valid) != 0)
    return f.astype(np.float64), keep


def max_radius(flows, valid=None, flow_scale=1.0):
    f, keep = _keep(flows, valid, flow_scale)
    with np.errstate(invalid="ignore", over="ignore"):
        rad = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1])
    rad = np.where(keep, rad, 0.0)
    return rad.reshape(rad.shape[0], -1).max(axis=1)


def color(flows, max_rad=None, valid=None, flow_scale=1.0):
    """flow_io.flow_to_color's arithmetic, line for line, per image with max_rad[n] (None: the image's own maximum)."""
    f, keep = _keep(flows, valid, flow_scale)
    N = f.shape[0]
    if max_rad is None:
        max_rad = max_radius(flows, valid, flow_scale)
    max_rad = np.broadcast_to(np.asarray(max_rad, np.float64), (N,))
    u = np.where(keep, f[..., 0], 0.0)
    v = np.where(keep, f[..., 1], 0.0)
    rad = np.sqrt(u * u + v * v)
    scale = (max_rad + np.finfo(np.float64).eps)[:, None, None]
    u, v, rad = u / scale, v / scale, rad / scale
    wheel = flow_io.color_wheel()
    ncols = wheel.shape[0]
    fk = (np.arctan2(-v, -u) / np.pi + 1.0) / 2.0 * (ncols - 1)
    k0 = np.floor(fk).astype(np.int64)
    k1 = (k0 + 1) % ncols
    fr = (fk - k0)[..., None]
    col = (1 - fr) * wheel[k0] / 255.0 + fr * wheel[k1] / 255.0
    inside = (rad <= 1)[..., None]
    col = np.where(inside, 1 - rad[..., None] * (1 - col), col * 0.75)
    t = 255.0 * col
    return np.floor(t).astype(np.uint8), t


def error_color(flows, flows_gt, valid=None):
    p = np.asarray(flows, np.float32)
    g = np.asarray(flows_gt, np.float32)
    shown = known(g)
    if valid is not None:
        shown = shown & (np.asarray(valid) != 0)
    pk = known(p)
    p64 = np.where(pk[..., None], p, 0).astype(np.float64)
    g64 = np.where(shown[..., None], g, 0).astype(np.float64)
    du, dv = p64[..., 0] - g64[..., 0], p64[..., 1] - g64[..., 1]
    d_err = np.sqrt(du * du + dv * dv)
    d_mag = np.sqrt(g64[..., 0] * g64[..., 0] + g64[..., 1] * g64[..., 1])
    n_err = d_err / 3.0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = (d_err / d_mag) / 0.05
    n_err = np.where(d_mag != 0, np.minimum(n_err, rel), n_err)
    bins = error_bin(n_err)
    bins = np.where(pk, bins, len(ERR_COLORS) - 1)
    out = ERR_COLORS[bins]
    out[~shown] = 0
    return out


def error_bin(n_err):
    """The bin lo <= n_err < hi of the table."""
    return np.searchsorted(ERR_EDGES, np.asarray(n_err, np.float64), side="right")


def frame_bytes(frames):
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        return frames.copy()
    assert frames.dtype == np.float32
    t = np.rint(255.0 * frames.astype(np.float64))
    t = np.where(np.isnan(t), 0.0, np.clip(t, 0.0, 255.0))
    return t.astype(np.uint8)


def tile_indices(h, src_h, src_w):
    """pyramid_montage's integers: (rows, columns) of the source read by a tile of height h."""
    tile_w = h * src_w // src_h
    return np.arange(h) * src_h // h, np.arange(tile_w) * src_w // tile_w


def montage(frames, flows_list, flow_scales=None):
    frames = np.asarray(frames)
    h = frames.shape[1]
    fb = frame_bytes(frames)
    tiles, ts = [fb], [np.full(fb.shape, np.nan)]
    scales = [1.0] * len(flows_list) if flow_scales is None else flow_scales
    for f, s in zip(flows_list, scales):
        c, t = color(f, None, None, s)
        ry, rx = tile_indices(h, c.shape[1], c.shape[2])
        tiles.append(c[:, ry][:, :, rx])
        ts.append(t[:, ry][:, :, rx])
    return np.concatenate(tiles, axis=2), np.concatenate(ts, axis=2)


def white(flows, valid=None, flow_scale=1.0):
    """(N,H,W) bool: the pixels that must be exactly (255, 255, 255) -- unknown, masked, and exactly zero after the scale."""
    f, keep = _keep(flows, valid, flow_scale)
    return ~keep | (f == 0).all(axis=-1)


def montage_white(frames, flows_list, flow_scales=None):
    """white() of every flow tile of montage(), resampled as the tile is; False over the frame tile."""
    frames = np.asarray(frames)
    h = frames.shape[1]
    scales = [1.0] * len(flows_list) if flow_scales is None else flow_scales
    tiles = [np.zeros(frames.shape[:3], bool)]
    for f, s in zip(flows_list, scales):
        ry, rx = tile_indices(h, f.shape[1], f.shape[2])
        tiles.append(white(f, None, s)[:, ry][:, :, rx])
    return np.concatenate(tiles, axis=2)


def near_integer(t):
    """Where the restatement's own t lies within NEAR of an integer (NaN: a value with no colour rule, never near)."""
    with np.errstate(invalid="ignore"):
        return np.abs(t - np.rint(t)) <= NEAR


def allowed(t, exact=None):
    """The values under the allowance: near an integer, and not of a pixel that `exact` ((N,H,W) bool: the unknown, masked and
    zero-flow pixels, which must be exactly white) takes out of it."""
    near = near_integer(t)
    return near if exact is None else near & ~np.asarray(exact)[..., None]


def check_color(got, want, t, exact=None):
    """The colour rule: got == floor(t) (= want), except that where t lies within NEAR of an integer r the value may be r or
    r - 1 -- decided by the restatement's t alone.  Where t is NaN (a frame tile) and at the pixels of `exact` got must equal
    want.  Returns (values that differ from want, values under the allowance); raises AssertionError on a value outside the
    rule."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape == t.shape, (got.shape, want.shape, t.shape)
    near = allowed(t, exact)
    r = np.where(near, np.rint(np.where(near, t, 0.0)), 0).astype(np.int64)
    ok = (got == want) | (near & ((got == np.clip(r, 0, 255)) | (got == np.clip(r - 1, 0, 255))))
    assert bool(ok.all()), f"{int((~ok).sum())} values outside the colour rule, first at {np.argwhere(~ok)[0].tolist()}"
    return int((got != want).sum()), int(near.sum())
