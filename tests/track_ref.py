"""Yardstick of point tracking (pwcnet_amd.track, csrc/pwc_track.hip): the step of include/pwc_hip.h, "point tracking", restated in
numpy float64, vectorised over the points, with the carried state rounded to float32 explicitly and every operation in the
stated order -- the kernel forms no fused multiply-add, so the GPU tests ask for BIT equality -- and the seeded cases of those
tests.  Not a test file; tests/test_host_track.py checks it without a GPU against an independent scalar Python loop, its fold
property, and the conditions its cases have to meet.

One step carries the state (x, y) float32, s across the step flow F, checked against G where given:
    terminal s (LEFT, UNKNOWN, OCCLUDED with stop_on_occlusion, a byte that is no status code): position and status repeat
    A  the point is not in [0, W - 1] x [0, H - 1] (a NaN fails)                         -> LEFT, position kept
    B  a corner masked out in F's mask or unknown (flow_io.flow_valid's rule), all four   -> UNKNOWN, position kept
       S = ((1 - wy) ((1 - wx) F00 + wx F01)) + (wy ((1 - wx) F10 + wx F11)), r = q + S
    C  r is not in the frame                                                              -> LEFT, position kept
    D  (G given) a bad corner of G around r                                               -> UNKNOWN, position kept
       b = G sampled at r, d = S + b, margin = a1 ((S0 S0 + S1 S1) + (b0 b0 + b1 b1)) + a2 - (d0 d0 + d1 d1)
       not (margin >= 0) -> OCCLUDED else VISIBLE, position (float32)r
"""
import functools

import numpy as np

from tests import fb_ref

UNSEEN, VISIBLE, LEFT, OCCLUDED, UNKNOWN = range(5)
NAMES = ("UNSEEN", "VISIBLE", "LEFT", "OCCLUDED", "UNKNOWN")
SENTINEL = 1e10
# how a step ended: not taken (terminal state, or the point is not stepped), the exits of the definition, or through (VISIBLE)
EXIT_NONE, EXIT_A, EXIT_B, EXIT_C, EXIT_D_UNKNOWN, EXIT_D_OCCLUDED, EXIT_THROUGH = range(7)


def _known(c):
    """flow_io.flow_valid's rule per record: both components finite with |.| <= 1e9."""
    with np.errstate(invalid="ignore"):
        return (np.abs(c) <= np.float32(1e9)).all(axis=-1)


def _inside(qx, qy, H, W):
    with np.errstate(invalid="ignore"):
        return (qx >= 0.0) & (qx <= float(W - 1)) & (qy >= 0.0) & (qy <= float(H - 1))


def _sample(F, M, qx, qy, ok, read=None):
    """(good (n,) bool, S (n,2) float64): the sample of the frame F (H,W,2) float32, mask M (H,W) or None, at the points that are
    `ok` (inside the frame); good: every corner unmasked and known.  read (H,W) bool: the pixels whose flow is loaded are set."""
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
    if read is not None:                                                       # a masked corner's flow is not loaded
        for cy, cx in corners:
            read[cy[good], cx[good]] = True
    for cy, cx in corners:
        good = good & _known(F[cy, cx])
    c00, c01, c10, c11 = (np.where(good[:, None], F[cy, cx].astype(np.float64), 0.0) for cy, cx in corners)
    ux, uy = 1.0 - wx, 1.0 - wy
    S = (uy * ((ux * c00) + (wx * c01))) + (wy * ((ux * c10) + (wx * c11)))
    return good, S


def step(F, Fm, G, Gm, x, y, s, alpha1, alpha2, stop, read_f=None, read_g=None):
    """One step of every point: (x, y float32 (n,), s uint8 (n,), exit (n,)) from the state x, y, s."""
    H, W, _ = F.shape
    a1, a2 = np.float64(np.float32(alpha1)), np.float64(np.float32(alpha2))
    live = (s == VISIBLE) | ((s == OCCLUDED) & (not stop))
    qx, qy = x.astype(np.float64), y.astype(np.float64)
    in_a = live & _inside(qx, qy, H, W)
    ok_b, S = _sample(F, Fm, qx, qy, in_a, read_f)
    rx, ry = qx + S[:, 0], qy + S[:, 1]
    in_c = ok_b & _inside(rx, ry, H, W)
    ex = np.full(s.shape, EXIT_NONE, np.int64)
    ex[live & ~in_a] = EXIT_A
    ex[in_a & ~ok_b] = EXIT_B
    ex[ok_b & ~in_c] = EXIT_C
    through = in_c
    occluded = np.zeros_like(in_c)
    if G is not None:
        ok_d, b = _sample(G, Gm, rx, ry, in_c, read_g)
        d0, d1 = S[:, 0] + b[:, 0], S[:, 1] + b[:, 1]
        bound = (a1 * (((S[:, 0] * S[:, 0]) + (S[:, 1] * S[:, 1])) + ((b[:, 0] * b[:, 0]) + (b[:, 1] * b[:, 1])))) + a2
        margin = bound - ((d0 * d0) + (d1 * d1))
        with np.errstate(invalid="ignore"):
            occluded = ok_d & ~(margin >= 0.0)
        ex[in_c & ~ok_d] = EXIT_D_UNKNOWN
        through = ok_d
    ex[through] = EXIT_THROUGH
    ex[occluded] = EXIT_D_OCCLUDED
    ns = s.copy()
    ns[(ex == EXIT_A) | (ex == EXIT_C)] = LEFT
    ns[(ex == EXIT_B) | (ex == EXIT_D_UNKNOWN)] = UNKNOWN
    ns[ex == EXIT_THROUGH] = VISIBLE
    ns[ex == EXIT_D_OCCLUDED] = OCCLUDED
    with np.errstate(invalid="ignore", over="ignore"):
        nx = np.where(through, rx.astype(np.float32), x)                       # rounded once
        ny = np.where(through, ry.astype(np.float32), y)
    return nx.astype(np.float32), ny.astype(np.float32), ns, ex


def track(flows_fw, points, flows_bw=None, start=None, status=None, valids_fw=None, valids_bw=None, direction="forward", alpha1=0.01,
          alpha2=0.5, stop_on_occlusion=True, details=False):
    """(tracks (T+1,P,2) float32, status (T+1,P) uint8) of pwcnet_amd.track_points on numpy arrays; details: also a dict with
    exits_fw (T,P) and exits_bw (T,P) -- how the step across flow t ended on the way up and on the way down -- and read_fw,
    read_bw (T,H,W) bool, the pixels whose flow some track loaded."""
    flows_fw, points = np.asarray(flows_fw), np.asarray(points)
    assert flows_fw.dtype == np.float32 and points.dtype == np.float32 and direction in ("forward", "both")
    T, H, W, _ = flows_fw.shape
    P = points.shape[0]
    assert direction == "forward" or flows_bw is not None
    s0 = np.zeros(P, np.int64) if start is None else np.asarray(start).astype(np.int64)
    fresh = _inside(points[:, 0].astype(np.float64), points[:, 1].astype(np.float64), H, W)
    st0 = np.where(fresh, VISIBLE, LEFT).astype(np.uint8)
    if status is not None:                                                     # the streaming form
        given = np.asarray(status) != UNSEEN
        s0 = np.where(given, 0, s0)
        st0 = np.where(given, np.asarray(status), st0).astype(np.uint8)
    incall = (s0 >= 0) & (s0 <= T)
    tracks = np.broadcast_to(points[None], (T + 1, P, 2)).copy()
    out = np.zeros((T + 1, P), np.uint8)                                       # UNSEEN at the query position
    idx = np.arange(P)
    out[np.where(incall, s0, 0)[incall], idx[incall]] = st0[incall]
    info = dict(exits_fw=np.zeros((T, P), np.int64), exits_bw=np.zeros((T, P), np.int64), read_fw=np.zeros((T, H, W), bool),
                read_bw=np.zeros((T, H, W), bool))
    vf = (lambda t: None) if valids_fw is None else (lambda t: np.asarray(valids_fw[t]))
    vb = (lambda t: None) if valids_bw is None or flows_bw is None else (lambda t: np.asarray(valids_bw[t]))
    x, y, s = points[:, 0].copy(), points[:, 1].copy(), st0.copy()
    for t in range(T):                                                         # up: slice t -> t + 1
        act = incall & (s0 <= t)
        frozen = np.where(act, s, LEFT).astype(np.uint8)                       # a point that is not stepped reads nothing
        nx, ny, ns, ex = step(flows_fw[t], vf(t), None if flows_bw is None else flows_bw[t], vb(t), x, y, frozen, alpha1, alpha2,
                              stop_on_occlusion, info["read_fw"][t], info["read_bw"][t])
        x, y, s = np.where(act, nx, x), np.where(act, ny, y), np.where(act, ns, s).astype(np.uint8)
        info["exits_fw"][t] = np.where(act, ex, EXIT_NONE)
        tracks[t + 1, act, 0], tracks[t + 1, act, 1], out[t + 1, act] = x[act], y[act], s[act]
    if direction == "both":
        x, y, s = points[:, 0].copy(), points[:, 1].copy(), st0.copy()
        for t in range(T, 0, -1):                                              # down: slice t -> t - 1, the roles swapped
            act = incall & (s0 >= t)
            frozen = np.where(act, s, LEFT).astype(np.uint8)
            nx, ny, ns, ex = step(flows_bw[t - 1], vb(t - 1), flows_fw[t - 1], vf(t - 1), x, y, frozen, alpha1, alpha2,
                                  stop_on_occlusion, info["read_bw"][t - 1], info["read_fw"][t - 1])
            x, y, s = np.where(act, nx, x), np.where(act, ny, y), np.where(act, ns, s).astype(np.uint8)
            info["exits_bw"][t - 1] = np.where(act, ex, EXIT_NONE)
            tracks[t - 1, act, 0], tracks[t - 1, act, 1], out[t - 1, act] = x[act], y[act], s[act]
    return (tracks, out, info) if details else (tracks, out)


def histogram(status_slice):
    """'VISIBLE 120 LEFT 40 ...' of one slice of a status array."""
    return " ".join(f"{n} {int((np.asarray(status_slice) == c).sum())}" for c, n in enumerate(NAMES))


# ------------------------------------------------------------------ cases
def build_flows(T, H, W, seed, noise=0.1, max_off=1, block=10, tile=10, keep=0.7, bad=0.002, drop=0.995):
    """The flows and masks of a seeded sequence, numpy:
      fw, bw        (T,H,W,2) float32: tests/fb_ref.build_case's consistent pair per frame pair -- an integer field constant on
                    block x block tiles of up to max_off px plus a continuous part, the backward flow its negative looked up
                    where the pixel came from plus uniform noise: consistent up to the noise and the tile seams -- with the
                    .flo sentinel, NaN, +Inf and -Inf at a seeded share `bad` of the pixels of each.
      valid_fw, valid_bw   (T,H,W) uint8, about 70 % ones: a pattern of tile x tile cells kept with probability `keep`, the same
                    in every frame (a point has to be able to survive several steps of an all-four-corners rule), and a
                    seeded share 1 - drop of the remaining pixels dropped per frame and direction.
      fw_nan, bw_nan       the same flows with NaN at EVERY masked-out pixel (a masked corner's flow is never loaded)."""
    base = fb_ref.build_case(T, H, W, seed=seed, masked=False, block=block, max_off=max_off, noise=noise)
    fw, bw = base["fw"].copy(), base["bw"].copy()
    rs = np.random.RandomState(seed + 7919)
    for fl in (fw, bw):
        hit = rs.uniform(size=(T, H, W)) < bad
        kinds = rs.randint(0, 4, size=int(hit.sum()))
        vals = np.array([SENTINEL, np.nan, np.inf, -np.inf], np.float32)[kinds]
        comp = rs.randint(0, 3, size=vals.shape)                               # x, y, or both components
        sub = fl[hit]
        sub[comp != 1, 0] = vals[comp != 1]
        sub[comp != 0, 1] = vals[comp != 0]
        fl[hit] = sub
    cells = rs.uniform(size=(-(-H // tile), -(-W // tile))) < keep
    pattern = np.kron(cells.astype(np.uint8), np.ones((tile, tile), np.uint8))[:H, :W].astype(bool)
    valid_fw = (pattern[None] & (rs.uniform(size=(T, H, W)) < drop)).astype(np.uint8)
    valid_bw = (pattern[None] & (rs.uniform(size=(T, H, W)) < drop)).astype(np.uint8)
    fw_nan, bw_nan = fw.copy(), bw.copy()
    fw_nan[valid_fw == 0] = np.nan
    bw_nan[valid_bw == 0] = np.nan
    return dict(T=T, H=H, W=W, fw=fw, bw=bw, valid_fw=valid_fw, valid_bw=valid_bw, fw_nan=fw_nan, bw_nan=bw_nan)


def build_queries(T, H, W, P, seed):
    """(points (P,2) float32, start (P,) int32): random sub-pixel points, one in six at integers, points on x = W - 1, on
    y = H - 1 and the corner itself, one in sixteen outside the frame (by a fraction of a pixel and by far), one NaN; start
    spread over 0 .. T, and T + 1, T + 3 (not in the call) for about one in twelve."""
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.uniform(0, W - 1, size=P), rs.uniform(0, H - 1, size=P)], axis=1)
    kind = rs.uniform(size=P)
    whole = kind < 1 / 6
    pts[whole] = np.floor(pts[whole])
    pts[(kind >= 0.20) & (kind < 0.24), 0] = W - 1
    pts[(kind >= 0.24) & (kind < 0.28), 1] = H - 1
    out = np.nonzero((kind >= 0.30) & (kind < 0.3625))[0]
    side = rs.randint(0, 4, size=out.size)                                     # beyond the left, right, top, bottom edge
    dist = rs.choice([0.25, 1.0, 7.5 * W], size=out.size)
    pts[out, 0] = np.where(side == 0, -dist, np.where(side == 1, W - 1 + dist, pts[out, 0]))
    pts[out, 1] = np.where(side == 2, -dist, np.where(side == 3, H - 1 + dist, pts[out, 1]))
    pts = pts.astype(np.float32)
    if P >= 4:
        pts[0] = (W - 1, H - 1)
        pts[1] = (0, 0)
        pts[2] = (np.nan, 3.0)
        pts[3] = (np.float32(W - 1) + np.float32(0.5), 1.0)
    start = rs.randint(0, T + 1, size=P).astype(np.int32)
    late = rs.uniform(size=P) < 1 / 12
    start[late] = np.where(rs.uniform(size=int(late.sum())) < 0.5, T + 1, T + 3)
    return pts, start


# The seed and the builder's defaults were chosen on the CPU, on the restatement alone, so that the conditions of
# tests/test_host_track.py hold: at the last slice of "fw_check_masks" every state but UNSEEN holds 5 % of the points, VISIBLE 20 %.
MAIN = dict(T=5, H=23, W=37, P=300, seed=28)
# the variants of the main case: the check and its alphas, the direction, stop_on_occlusion, masks, start given
VARIANTS = {
    "fw_nocheck_masks": dict(check=False, masks=True, start=False),
    "fw_nocheck_nomasks_start": dict(check=False, masks=False, start=True),
    "fw_check_masks": dict(check=True, masks=True, start=False),                   # THE main case of the conditions
    "fw_check_nomasks_start": dict(check=True, masks=False, start=True),
    "fw_check_b_masks_start": dict(check=True, alphas=(0.0, 0.25), masks=True, start=True),
    "both_masks_start": dict(check=True, direction="both", masks=True, start=True),
    "both_nomasks_start": dict(check=True, direction="both", masks=False, start=True),
    "nostop_masks": dict(check=True, stop=False, masks=True, start=False),
    "nostop_nomasks_start": dict(check=True, stop=False, masks=False, start=True),
    # the streaming form: every point enters slice 0 in a given state, two in three VISIBLE wherever they are -- the only way a
    # step meets a point outside the frame (exit A): a fresh query there is LEFT from the start and a step never leaves the frame
    "stream_masks": dict(check=True, masks=True, start=True, stream=True),
}


@functools.lru_cache(maxsize=None)
def main_inputs():
    """The flows and the queries of the main case -- computed once per process and shared; treat them as read-only."""
    flows = build_flows(MAIN["T"], MAIN["H"], MAIN["W"], MAIN["seed"])
    points, start = build_queries(MAIN["T"], MAIN["H"], MAIN["W"], MAIN["P"], MAIN["seed"] + 1)
    return flows, points, start


def variant_kwargs(name, nan_behind_masks=False):
    """The keyword arguments (numpy arrays) of `track` / of pwcnet_amd.track_points for a variant of the main case."""
    v = VARIANTS[name]
    flows, points, start = main_inputs()
    fw, bw = (flows["fw_nan"], flows["bw_nan"]) if nan_behind_masks and v["masks"] else (flows["fw"], flows["bw"])
    a1, a2 = v.get("alphas", (0.01, 0.5))
    status = None
    if v.get("stream"):
        rs = np.random.RandomState(MAIN["seed"] + 2)
        status = rs.choice(np.array([VISIBLE, VISIBLE, VISIBLE, VISIBLE, OCCLUDED, LEFT, UNKNOWN, UNSEEN, 9], np.uint8), size=points.shape[0])
        status[:4] = VISIBLE
    return dict(status=status, flows_fw=fw, points=points, flows_bw=bw if v["check"] else None, start=start if v["start"] else None,
                valids_fw=flows["valid_fw"] if v["masks"] else None,
                valids_bw=flows["valid_bw"] if v["masks"] and v["check"] else None, direction=v.get("direction", "forward"),
                alpha1=a1, alpha2=a2, stop_on_occlusion=v.get("stop", True))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(tracks, status, details) of the restatement for a variant -- computed once per process; read-only."""
    return track(details=True, **variant_kwargs(name))
