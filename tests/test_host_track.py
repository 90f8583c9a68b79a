"""Point tracking without a GPU: the numpy restatement of tests/track_ref.py against an independent scalar Python loop, its fold
property, the conditions its seeded cases have to meet (asserted on the restatement alone), the argument checks of
pwcnet_amd.track_points, grid_points and infer_continuous.py's --track SPEC parser."""
import math
import os
import re

import numpy as np
import pytest
import torch

import infer_continuous
import pwcnet_amd
from pwcnet_amd import _lib, track as TK
from tests import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement against a scalar loop
def _scalar_sample(F, M, qx, qy):
    """None where a corner is masked out or unknown, else (S0, S1): Python floats (IEEE doubles), one point."""
    H, W, _ = F.shape
    x0, y0 = math.floor(qx), math.floor(qy)
    x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
    wx, wy = qx - x0, qy - y0
    corners = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    if M is not None and not all(M[c] for c in corners):
        return None
    vals = [[float(F[c][k]) for k in range(2)] for c in corners]
    if not all(math.isfinite(v) and abs(v) <= 1e9 for c in vals for v in c):
        return None
    return tuple(((1.0 - wy) * (((1.0 - wx) * vals[0][k]) + (wx * vals[1][k]))) + (wy * (((1.0 - wx) * vals[2][k]) + (wx * vals[3][k])))
                 for k in range(2))


def _scalar_step(F, Fm, G, Gm, x, y, s, a1, a2, stop):
    H, W, _ = F.shape
    if not (s == R.VISIBLE or (s == R.OCCLUDED and not stop)):
        return x, y, s
    qx, qy = float(x), float(y)
    inside = lambda u, v: 0.0 <= u <= W - 1 and 0.0 <= v <= H - 1                  # noqa: E731  (False for a NaN)
    if not inside(qx, qy):
        return x, y, R.LEFT
    S = _scalar_sample(F, Fm, qx, qy)
    if S is None:
        return x, y, R.UNKNOWN
    rx, ry = qx + S[0], qy + S[1]
    if not inside(rx, ry):
        return x, y, R.LEFT
    ns = R.VISIBLE
    if G is not None:
        b = _scalar_sample(G, Gm, rx, ry)
        if b is None:
            return x, y, R.UNKNOWN
        d0, d1 = S[0] + b[0], S[1] + b[1]
        bound = (a1 * (((S[0] * S[0]) + (S[1] * S[1])) + ((b[0] * b[0]) + (b[1] * b[1])))) + a2
        if not (bound - ((d0 * d0) + (d1 * d1)) >= 0.0):
            ns = R.OCCLUDED
    return np.float32(rx), np.float32(ry), ns


def _scalar_track(flows_fw, points, flows_bw=None, start=None, status=None, valids_fw=None, valids_bw=None, direction="forward",
                  alpha1=0.01, alpha2=0.5, stop_on_occlusion=True):
    T, H, W, _ = flows_fw.shape
    P = points.shape[0]
    a1, a2 = float(np.float32(alpha1)), float(np.float32(alpha2))
    tracks = np.zeros((T + 1, P, 2), np.float32)
    out = np.zeros((T + 1, P), np.uint8)
    at = lambda a, t: None if a is None else a[t]                                 # noqa: E731
    for p in range(P):
        px, py = points[p]
        tracks[:, p] = points[p]
        s0 = 0 if start is None else int(start[p])
        if status is not None and status[p] != R.UNSEEN:
            s0, st = 0, int(status[p])
        elif s0 > T:
            continue
        else:
            st = R.VISIBLE if (0.0 <= float(px) <= W - 1 and 0.0 <= float(py) <= H - 1) else R.LEFT
        out[s0, p] = st
        x, y, s = px, py, st
        for t in range(s0, T):
            x, y, s = _scalar_step(flows_fw[t], at(valids_fw, t), at(flows_bw, t), at(valids_bw, t), x, y, s, a1, a2, stop_on_occlusion)
            tracks[t + 1, p], out[t + 1, p] = (x, y), s
        if direction == "both":
            x, y, s = px, py, st
            for t in range(s0, 0, -1):
                x, y, s = _scalar_step(flows_bw[t - 1], at(valids_bw, t - 1), flows_fw[t - 1], at(valids_fw, t - 1), x, y, s, a1, a2,
                                       stop_on_occlusion)
                tracks[t - 1, p], out[t - 1, p] = (x, y), s
    return tracks, out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _small_case():
    T, H, W, P = 3, 7, 9, 60
    fl = R.build_flows(T, H, W, seed=5, tile=4, block=3, bad=0.02, keep=0.8)
    pts, start = R.build_queries(T, H, W, P, seed=6)
    return fl, pts, start


@pytest.mark.parametrize("config", [
    dict(), dict(check=True), dict(check=True, masks=True), dict(check=True, masks=True, stop_on_occlusion=False),
    dict(check=True, masks=True, direction="both", use_start=True), dict(check=True, alpha1=0.0, alpha2=0.25, use_start=True),
    dict(masks=True, use_start=True, stream=True), dict(check=True, stop_on_occlusion=False, direction="both", use_start=True)])
def test_restatement_equals_a_scalar_loop(config):
    fl, pts, start = _small_case()
    cfg = dict(config)
    check, masks, use_start, stream = (cfg.pop(k, False) for k in ("check", "masks", "use_start", "stream"))
    status = None
    if stream:
        status = np.random.RandomState(2).choice(np.array([0, 1, 1, 1, 2, 3, 4, 7], np.uint8), size=pts.shape[0])
    kw = dict(flows_bw=fl["bw"] if check else None, start=start if use_start else None, status=status,
              valids_fw=fl["valid_fw"] if masks else None, valids_bw=fl["valid_bw"] if masks and check else None, **cfg)
    got_t, got_s = R.track(fl["fw"], pts, **kw)
    want_t, want_s = _scalar_track(fl["fw"], pts, **kw)
    assert got_t.dtype == np.float32 and got_s.dtype == np.uint8 and got_t.shape == (4, 60, 2) and got_s.shape == (4, 60)
    assert np.array_equal(got_s, want_s)
    assert np.array_equal(_bits(got_t), _bits(want_t))
    assert len(set(np.unique(got_s[-1]).tolist())) >= 3                          # (not a case in which nothing happens)


def test_restatement_folds():
    """One call over T flows equals a call over the first T1 followed by a call over the rest fed with slice T1."""
    for name in ("fw_check_masks", "fw_check_nomasks_start", "nostop_masks", "fw_nocheck_masks", "stream_masks"):
        kw = R.variant_kwargs(name)
        whole_t, whole_s, _ = R.reference(name)
        for T1 in (1, 2, 4):
            cut = lambda a, lo, hi: None if a is None else a[lo:hi]                # noqa: E731
            first = dict(kw, flows_fw=kw["flows_fw"][:T1], flows_bw=cut(kw["flows_bw"], 0, T1), valids_fw=cut(kw["valids_fw"], 0, T1),
                         valids_bw=cut(kw["valids_bw"], 0, T1))
            t1, s1 = R.track(**first)
            start = None if kw["start"] is None else np.maximum(kw["start"] - T1, 0).astype(np.int32)
            rest = dict(kw, flows_fw=kw["flows_fw"][T1:], flows_bw=cut(kw["flows_bw"], T1, None), valids_fw=cut(kw["valids_fw"], T1, None),
                        valids_bw=cut(kw["valids_bw"], T1, None), points=t1[T1], status=s1[T1], start=start)
            t2, s2 = R.track(**rest)
            assert np.array_equal(s1, whole_s[:T1 + 1]) and np.array_equal(_bits(t1), _bits(whole_t[:T1 + 1])), (name, T1)
            assert np.array_equal(s2, whole_s[T1:]) and np.array_equal(_bits(t2), _bits(whole_t[T1:])), (name, T1)


# ------------------------------------------------------------------ conditions on the builder
def test_main_case_reaches_every_state_and_exit():
    flows, points, start = R.main_inputs()
    share = float(flows["valid_fw"].mean())
    assert 0.6 <= share <= 0.8 and 0.6 <= float(flows["valid_bw"].mean()) <= 0.8           # "about 70 %"
    assert np.isnan(flows["fw_nan"][flows["valid_fw"] == 0]).all() and np.isnan(flows["bw_nan"][flows["valid_bw"] == 0]).all()
    for fl in (flows["fw"], flows["bw"]):
        assert (fl == np.float32(1e10)).any() and np.isnan(fl).any() and np.isinf(fl).any()
    x, y = points[:, 0], points[:, 1]
    W, H = R.MAIN["W"], R.MAIN["H"]
    assert np.isnan(x).sum() == 1 and (x == W - 1).sum() >= 3 and (y == H - 1).sum() >= 3
    assert ((x == np.floor(x)) & (y == np.floor(y))).sum() >= 20 and ((x != np.floor(x)) & (y != np.floor(y))).sum() >= 100
    with np.errstate(invalid="ignore"):
        assert ((x < 0) | (x > W - 1) | (y < 0) | (y > H - 1)).sum() >= 8
    assert set(range(R.MAIN["T"] + 1)) <= set(start.tolist()) and (start > R.MAIN["T"]).sum() >= 5

    _, status, _ = R.reference("fw_check_masks")
    last = status[-1]
    P = last.size
    print("main case, last slice:", R.histogram(last))
    for code in (R.VISIBLE, R.LEFT, R.OCCLUDED, R.UNKNOWN):
        assert (last == code).sum() >= 0.05 * P, R.NAMES[code]
    assert (last == R.VISIBLE).sum() >= 0.2 * P
    # every exit of the step: B, C and both of D in the main case itself; A only where a point is handed in VISIBLE outside the
    # frame (a fresh query there is LEFT from the start and no step leaves the frame): the streaming variant
    taken = set(np.unique(R.reference("fw_check_masks")[2]["exits_fw"]).tolist())
    assert {R.EXIT_B, R.EXIT_C, R.EXIT_D_UNKNOWN, R.EXIT_D_OCCLUDED, R.EXIT_THROUGH} <= taken
    assert R.EXIT_A in set(np.unique(R.reference("stream_masks")[2]["exits_fw"]).tolist())
    for name in ("both_masks_start", "both_nomasks_start"):
        down = set(np.unique(R.reference(name)[2]["exits_bw"]).tolist())
        assert {R.EXIT_C, R.EXIT_D_OCCLUDED, R.EXIT_THROUGH} <= down, name
        assert (R.reference(name)[1][0] != R.UNSEEN).sum() >= 0.8 * P           # tracked down to frame 0
    for name in ("nostop_masks", "nostop_nomasks_start"):
        s = R.reference(name)[1]
        assert ((s[:-1] == R.OCCLUDED) & (s[1:] == R.VISIBLE)).any(), name
    # points that are not in the call are UNSEEN throughout, at the query position
    tr, s, _ = R.reference("fw_check_nomasks_start")
    late = start > R.MAIN["T"]
    assert (s[:, late] == R.UNSEEN).all() and np.array_equal(_bits(tr[:, late]), _bits(np.broadcast_to(points[late], tr[:, late].shape)))


# ------------------------------------------------------------------ the Python surface
def test_status_constants_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    for name in ("UNSEEN", "VISIBLE", "LEFT", "OCCLUDED", "UNKNOWN", "FORWARD", "BOTH"):
        value = int(re.search(rf"PWC_TRACK_{name} = (\d+)", header).group(1))
        assert getattr(_lib, f"TRACK_{name}") == value
        if name not in ("FORWARD", "BOTH"):
            assert getattr(TK, name) == value == getattr(R, name) and TK.STATUS_NAMES[value] == name == R.NAMES[value]
    assert "pwc_track.hip" in _lib.SOURCES and "pwc_track_points_f32" in _lib.SIGNATURES
    assert pwcnet_amd.track_points is TK.track_points and pwcnet_amd.grid_points is TK.grid_points


def test_track_points_names_the_argument_it_refuses():
    f = torch.zeros((3, 5, 6, 2))
    p = torch.zeros((4, 2))
    ok = dict(flows_fw=f, points=p)

    def refuses(exc, word, **kw):
        with pytest.raises(exc, match=word):
            TK.track_points(**dict(ok, **kw))

    refuses(TypeError, "flows_fw", flows_fw=f.double())
    refuses(ValueError, "flows_fw", flows_fw=torch.zeros((3, 5, 6, 3)))
    refuses(ValueError, "flows_fw", flows_fw=torch.zeros((0, 5, 6, 2)))
    refuses(ValueError, "flows_bw", flows_bw=torch.zeros((2, 5, 6, 2)))
    refuses(TypeError, "flows_bw", flows_bw=f.half())
    refuses(TypeError, "valids_fw", valids_fw=torch.zeros((3, 5, 6)))
    refuses(ValueError, "valids_fw", valids_fw=torch.zeros((3, 5, 7), dtype=torch.bool))
    refuses(ValueError, "valids_bw", valids_bw=torch.zeros((3, 5, 6), dtype=torch.bool))              # without flows_bw
    refuses(ValueError, "valids_bw", flows_bw=f, valids_bw=torch.zeros((3, 6, 5), dtype=torch.bool).transpose(1, 2))
    refuses(TypeError, "points", points=p.double())
    refuses(TypeError, "points", points=[[0.0, 0.0]])
    refuses(ValueError, "points", points=torch.zeros((4, 3)))
    refuses(ValueError, "points", points=torch.zeros((0, 2)))
    refuses(TypeError, "start", start=torch.zeros(4, dtype=torch.int64))
    refuses(ValueError, "start", start=torch.zeros(5, dtype=torch.int32))
    refuses(ValueError, "start", start=torch.tensor([0, 1, -1, 2], dtype=torch.int32))
    refuses(TypeError, "status", status=torch.zeros(4, dtype=torch.bool))
    refuses(ValueError, "status", status=torch.zeros((4, 1), dtype=torch.uint8))
    refuses(ValueError, "direction", direction="backward")
    refuses(ValueError, "direction", direction="both")                                                # without flows_bw
    refuses(ValueError, "alpha1", flows_bw=f, alpha1=-0.1)
    refuses(ValueError, "alpha2", flows_bw=f, alpha2=float("nan"))
    refuses(ValueError, "flows_fw: the tensor is on cpu")                                             # everything right but the device


def test_grid_points():
    g = TK.grid_points(64, 64, 16)
    assert g.dtype == torch.float32 and tuple(g.shape) == (16, 2) and not g.is_cuda
    assert g[:5].tolist() == [[8.0, 8.0], [24.0, 8.0], [40.0, 8.0], [56.0, 8.0], [8.0, 24.0]]
    g = TK.grid_points(5, 9, 4, offset=0)
    assert g.tolist() == [[0.0, 0.0], [4.0, 0.0], [8.0, 0.0], [0.0, 4.0], [4.0, 4.0], [8.0, 4.0]]
    assert TK.grid_points(5, 9, 4, offset=(1, 3)).tolist() == [[1.0, 3.0], [5.0, 3.0]]
    assert tuple(TK.grid_points(448, 1024, 4).shape) == (112 * 256, 2)
    for bad in (dict(stride=0), dict(stride=2.0), dict(stride=4, offset=9), dict(stride=4, offset=(0, 5)), dict(stride=4, offset=-1)):
        with pytest.raises(ValueError):
            TK.grid_points(5, 9, **bad)


def test_track_spec_parser(tmp_path):
    pts, start = infer_continuous.parse_track_spec("grid:16", 4, 64, 64)
    assert pts.dtype == np.float32 and start.dtype == np.int32 and pts.shape == (16, 2) and not start.any()
    assert np.array_equal(pts, TK.grid_points(64, 64, 16).numpy())
    spec = tmp_path / "queries.txt"
    spec.write_text("# frame x y\n0 1.5 2.25\n\n3 10 0   # the last frame\n1 -4 7e0\n")
    pts, start = infer_continuous.parse_track_spec(str(spec), 4, 64, 64)
    assert pts.tolist() == [[1.5, 2.25], [10.0, 0.0], [-4.0, 7.0]] and start.tolist() == [0, 3, 1]
    for text, word in (("4 1 1\n", "outside the sequence"), ("-1 1 1\n", "outside the sequence"), ("0 1\n", "frame x y"),
                       ("0 1 2 3\n", "frame x y"), ("a 1 2\n", "frame x y"), ("# nothing\n", "no query point")):
        spec.write_text(text)
        with pytest.raises(ValueError, match=word):
            infer_continuous.parse_track_spec(str(spec), 4, 64, 64)
    for bad in ("grid:0", "grid:x", "grid:-3", str(tmp_path / "missing.txt")):
        with pytest.raises(ValueError, match="--track"):
            infer_continuous.parse_track_spec(bad, 4, 64, 64)
    args = infer_continuous.build_parser().parse_args(["-i", "a.png", "b.png"])
    assert args.track is None and args.track_fb is False
