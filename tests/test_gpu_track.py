"""Point tracking on the GPU (pwc_track.hip, pwcnet_amd.track, infer_continuous.py --track) against the numpy restatement of
tests/track_ref.py (checked on the CPU by tests/test_host_track.py).

The kernel's operations are IEEE double + - x, floor and comparisons in a fixed order, with no fused multiply-add, and the
restatement performs the same operations in the same order: the yardstick is BIT EQUALITY of `tracks` and of `status`, no
tolerance and no near-tie allowance.  Every case prints P, T and the histogram of the states at the last slice before it
asserts (profiles/track_gpu_test_figures.txt)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import track as TK  # the feature: without it nothing here can be collected
from tests import track_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.track_points is TK.track_points
    return pwcnet_amd


def _up(a):
    return a if a is None or not isinstance(a, np.ndarray) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(P, **kw):
    """pwcnet_amd.track_points on numpy arguments; numpy results."""
    tracks, status = P.track_points(**{k: _up(v) for k, v in kw.items()})
    assert tracks.dtype == torch.float32 and status.dtype == torch.uint8 and tracks.is_contiguous() and status.is_contiguous()
    return tracks.cpu().numpy(), status.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(tag, got, want):
    (gt, gs), (wt, ws) = got, want[:2]
    assert gt.shape == wt.shape and gs.shape == ws.shape, tag
    print(f"track {tag}: P {ws.shape[1]} T {ws.shape[0] - 1} last slice {R.histogram(ws[-1])}; status differs at "
          f"{int((gs != ws).sum())}, position bits at {int((_bits(gt) != _bits(wt)).any(axis=-1).sum())} of {ws.size}")
    assert np.array_equal(gs, ws), tag
    assert np.array_equal(_bits(gt), _bits(wt)), tag


@pytest.mark.parametrize("name", sorted(R.VARIANTS))
def test_main_case_equals_the_restatement_bit_for_bit(P, name):
    got = _run(P, **R.variant_kwargs(name))
    _check(name, got, R.reference(name))
    if R.VARIANTS[name]["start"] and not R.VARIANTS[name].get("stream"):       # start > T: not in the call
        late = R.main_inputs()[2] > R.MAIN["T"]
        assert late.sum() >= 5 and (got[1][:, late] == R.UNSEEN).all()


def test_one_pixel_frame_clamps_every_corner(P):
    """1 x 1, T = 2: x1 = min(x0 + 1, 0) = x0 and the same in y; the only point inside is (0, 0)."""
    pts = np.array([[0.0, 0.0], [-0.0, 0.0], [0.25, 0.0], [0.0, -1.0], [np.nan, 0.0]], np.float32)
    cases = {
        "still": ([[0.0, 0.0], [-0.0, 0.0]], [[0.0, 0.0], [0.0, -0.0]]),
        "leaves": ([[0.0, 0.0], [0.5, 0.0]], [[0.0, 0.0], [-0.5, 0.0]]),
        "occluded": ([[0.0, 0.0], [0.0, 0.0]], [[0.0, 3.0], [0.0, 0.0]]),
        "unknown": ([[0.0, 0.0], [1e10, 0.0]], [[np.inf, 0.0], [0.0, 0.0]]),
    }
    for tag, (fw, bw) in cases.items():
        fw, bw = (np.asarray(a, np.float32).reshape(2, 1, 1, 2) for a in (fw, bw))
        for kw in (dict(), dict(flows_bw=bw), dict(flows_bw=bw, direction="both", start=np.array([2, 1, 0, 2, 1], np.int32)),
                   dict(flows_bw=bw, stop_on_occlusion=False, valids_fw=np.ones((2, 1, 1), np.uint8))):
            _check(f"1x1 {tag} {sorted(kw)}", _run(P, flows_fw=fw, points=pts, **kw), R.track(fw, pts, **kw))
    still = _run(P, flows_fw=np.zeros((2, 1, 1, 2), np.float32), points=pts)[1]
    assert still[:, 0].tolist() == [R.VISIBLE] * 3 and still[:, 2].tolist() == [R.LEFT] * 3


def test_exact_ties_and_frame_edges(P):
    """3 x 4, T = 1, every value exact: steps that land ON the last column, the last row and the origin stay inside (<=), steps
    that miss the frame by 2^-20 and 2^-30 leave it, and a margin of exactly 0 is VISIBLE (>=)."""
    H, W = 3, 4
    fw, bw = np.zeros((1, H, W, 2), np.float32), np.zeros((1, H, W, 2), np.float32)
    fw[0, 1, 1] = (2.0, 0.0)                                                   # (1,1) -> (3,1): x = W - 1
    fw[0, 0, 3] = (0.0, 2.0)                                                   # (3,0) -> (3,2): y = H - 1
    fw[0, 2, 2] = (-2.0, -2.0)                                                 # (2,2) -> (0,0)
    fw[0, 2, 0] = (-2.0 ** -30, 0.0)                                           # (0,2) -> x < 0
    fw[0, 1, 3] = (2.0 ** -20, 0.0)                                            # (3,1) -> x > W - 1
    fw[0, 0, 1] = (0.5, 0.0)                                                   # (1,0) -> (1.5,0), b = 0: |S + b|^2 = 0.25
    bw[0, 1, 3], bw[0, 2, 3], bw[0, 0, 0] = (-2.0, 0.0), (0.0, -2.0), (2.0, 2.0)   # the first three come back exactly
    pts = np.array([[1, 1], [3, 0], [2, 2], [0, 2], [3, 1], [1, 0]], np.float32)
    kw = dict(flows_bw=bw, alpha1=0.0, alpha2=0.25)
    want = R.track(fw, pts, **kw)
    assert want[1][1].tolist() == [R.VISIBLE, R.VISIBLE, R.VISIBLE, R.LEFT, R.LEFT, R.VISIBLE]
    assert want[0][1].tolist() == [[3, 1], [3, 2], [0, 0], [0, 2], [3, 1], [1.5, 0]]
    _check("ties and edges", _run(P, flows_fw=fw, points=pts, **kw), want)
    kw = dict(flows_bw=bw, alpha1=0.0, alpha2=float(np.nextafter(np.float32(0.25), np.float32(0))))
    want = R.track(fw, pts, **kw)
    assert want[1][1].tolist() == [R.VISIBLE, R.VISIBLE, R.VISIBLE, R.LEFT, R.LEFT, R.OCCLUDED]
    _check("ties and edges, alpha2 one ulp below", _run(P, flows_fw=fw, points=pts, **kw), want)


def test_channel_slices_give_the_bits_of_contiguous_flows(P):
    """Flows as channels 1:3 of a 4-channel buffer (pointer off the 8-byte boundary: two 4-byte loads per record) against
    contiguous ones (one 8-byte load)."""
    for name in ("fw_check_masks", "both_masks_start"):
        kw = {k: _up(v) for k, v in R.variant_kwargs(name).items()}
        wide = {}
        for k in ("flows_fw", "flows_bw"):
            buf = torch.full(tuple(kw[k].shape[:3]) + (4,), float("nan"), dtype=torch.float32, device="cuda")
            buf[..., 1:3] = kw[k]
            wide[k] = buf[..., 1:3]
            assert wide[k].data_ptr() % 8 == 4 and kw[k].data_ptr() % 8 == 0
        plain = P.track_points(**kw)
        sliced = P.track_points(**dict(kw, **wide))
        got = tuple(t.cpu().numpy() for t in sliced)
        _check(f"slices {name}", got, R.reference(name))
        assert np.array_equal(_bits(got[0]), _bits(plain[0].cpu().numpy())) and torch.equal(sliced[1], plain[1])


@pytest.mark.parametrize("name", ["fw_check_masks", "fw_check_nomasks_start", "nostop_masks", "fw_nocheck_masks", "stream_masks"])
def test_two_calls_through_status_equal_one(P, name):
    """T = 5 in one call against T = 2 then T = 3, the second fed slice 2 through points= / status= and start - 2."""
    kw = {k: _up(v) for k, v in R.variant_kwargs(name).items()}
    whole_t, whole_s = P.track_points(**kw)
    cut = lambda a, lo, hi: None if a is None else a[lo:hi]                        # noqa: E731
    first = dict(kw, **{k: cut(kw[k], 0, 2) for k in ("flows_fw", "flows_bw", "valids_fw", "valids_bw")})
    t1, s1 = P.track_points(**first)
    rest = dict(kw, **{k: cut(kw[k], 2, None) for k in ("flows_fw", "flows_bw", "valids_fw", "valids_bw")})
    rest.update(points=t1[2], status=s1[2], start=None if kw["start"] is None else (kw["start"] - 2).clamp(min=0))
    t2, s2 = P.track_points(**rest)
    got = (torch.cat([t1[:2], t2]).cpu().numpy(), torch.cat([s1[:2], s2]).cpu().numpy())
    _check(f"fold {name}", got, R.reference(name))
    assert torch.equal(s1[2], s2[0]) and np.array_equal(_bits(t1[2].cpu().numpy()), _bits(t2[0].cpu().numpy()))
    assert np.array_equal(_bits(got[0]), _bits(whole_t.cpu().numpy())) and np.array_equal(got[1], whole_s.cpu().numpy())


def test_a_point_alone_gives_the_bits_it_gives_among_300(P):
    for name in ("both_masks_start", "nostop_masks"):
        kw = {k: _up(v) for k, v in R.variant_kwargs(name).items()}
        tracks, status = P.track_points(**kw)
        for p in (0, 1, 2, 3, 17, 64, 65, 255, 256, 299):
            one = dict(kw, points=kw["points"][p:p + 1], start=None if kw["start"] is None else kw["start"][p:p + 1])
            t1, s1 = P.track_points(**one)
            assert torch.equal(s1[:, 0], status[:, p]), (name, p)
            assert np.array_equal(_bits(t1[:, 0].cpu().numpy()), _bits(tracks[:, p].cpu().numpy())), (name, p)


def _call(fw, bw, vfw, vbw, T, H, W, points, start, status_in, n, direction, a1, a2, stop, tracks, status, fw_cs=2, bw_cs=2):
    """pwc_track_points_f32 on raw addresses (integers or None)."""
    p = lambda v: None if v is None else ctypes.c_void_p(v)                        # noqa: E731
    return _lib.lib().pwc_track_points_f32(p(fw), fw_cs, p(bw), bw_cs, p(vfw), p(vbw), T, H, W, p(points), p(start), p(status_in), n,
                                           direction, a1, a2, stop, p(tracks), p(status), _lib.current_stream())


def test_more_points_than_the_grid_cap_has_lanes(P):
    """P = 4096 * 256 + 77 on an 8 x 8 frame, T = 1: the grid-stride pass.  The outputs are filled with a sentinel first, every
    element has to be overwritten, and the last 77 points (every point, in fact) equal the restatement."""
    n, T, H, W = 4096 * 256 + 77, 1, 8, 8
    fl = R.build_flows(T, H, W, seed=9, tile=4, block=4, bad=0.03)             # (three of the four mask cells kept)
    rs = np.random.RandomState(4)
    pts = np.stack([rs.uniform(-0.5, W - 0.5, size=n), rs.uniform(-0.5, H - 0.5, size=n)], axis=1).astype(np.float32)
    pts[-77::7] = np.floor(pts[-77::7])
    pts[-1] = (W - 1, H - 1)
    start = (rs.uniform(size=n) < 0.1).astype(np.int32) * rs.randint(1, 3, size=n).astype(np.int32)     # 0; 1 (the last slice); 2 (not in the call)
    want = R.track(fl["fw"], pts, fl["bw"], start=start, valids_fw=fl["valid_fw"], valids_bw=fl["valid_bw"])
    g = {k: _up(fl[k]) for k in ("fw", "bw", "valid_fw", "valid_bw")}
    gp, gs = _up(pts), _up(start)
    tracks = torch.full((T + 1, n, 2), -12345.0, dtype=torch.float32, device="cuda")
    status = torch.full((T + 1, n), 0xEE, dtype=torch.uint8, device="cuda")
    rc = _call(g["fw"].data_ptr(), g["bw"].data_ptr(), g["valid_fw"].data_ptr(), g["valid_bw"].data_ptr(), T, H, W, gp.data_ptr(),
               gs.data_ptr(), None, n, _lib.TRACK_FORWARD, 0.01, 0.5, 1, tracks.data_ptr(), status.data_ptr())
    assert rc == 0
    got = (tracks.cpu().numpy(), status.cpu().numpy())
    left = int((got[1] == 0xEE).sum()) + int((got[0] == np.float32(-12345.0)).sum())
    print(f"track grid cap: {n} points, {left} elements left at the sentinel")
    assert left == 0
    assert np.array_equal(got[1][:, -77:], want[1][:, -77:]) and np.array_equal(_bits(got[0][:, -77:]), _bits(want[0][:, -77:]))
    _check("grid cap", got, want)


@pytest.mark.parametrize("name", ["fw_nocheck_masks", "fw_check_masks", "both_masks_start", "nostop_masks"])
def test_nan_where_no_track_reads_changes_no_bit(P, name):
    """NaN behind EVERY mask (a masked corner's flow is never loaded), and at the unmasked pixels no track loads."""
    kw = R.variant_kwargs(name, nan_behind_masks=True)
    info = R.reference(name)[2]
    fw, bw = kw["flows_fw"].copy(), None if kw["flows_bw"] is None else kw["flows_bw"].copy()
    assert np.isnan(fw[kw["valids_fw"] == 0]).all() and (~info["read_fw"]).sum() >= 100 and info["read_fw"].sum() >= 100
    fw[~info["read_fw"]] = np.nan
    if bw is not None:
        assert np.isnan(bw[kw["valids_bw"] == 0]).all() and info["read_bw"].sum() >= 100
        bw[~info["read_bw"]] = np.nan
    _check(f"nan {name}", _run(P, **dict(kw, flows_fw=fw, flows_bw=bw)), R.reference(name))


def test_refusals_leave_the_outputs_untouched(P):
    fw = torch.zeros((1, 2, 2, 4), dtype=torch.float32, device="cuda")
    pts = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
    start = torch.zeros(2, dtype=torch.int32, device="cuda")
    tracks = torch.full((2, 2, 2), 7.0, dtype=torch.float32, device="cuda")
    status = torch.full((2, 2), 0xEE, dtype=torch.uint8, device="cuda")
    f, q, s, t, o = fw.data_ptr(), pts.data_ptr(), start.data_ptr(), tracks.data_ptr(), status.data_ptr()
    good = dict(fw=f, bw=None, vfw=None, vbw=None, T=1, H=2, W=2, points=q, start=s, status_in=None, n=2,
                direction=_lib.TRACK_FORWARD, a1=0.01, a2=0.5, stop=1, tracks=t, status=o)
    big = (1 << 24) + 1
    refused = [
        (EINVAL, dict(fw=None)), (EINVAL, dict(points=None)), (EINVAL, dict(tracks=None)), (EINVAL, dict(status=None)),
        (EINVAL, dict(T=0)), (EINVAL, dict(H=0)), (EINVAL, dict(W=-1)), (EINVAL, dict(n=0)),
        (EINVAL, dict(fw_cs=1)), (EINVAL, dict(bw=f, bw_cs=1)),
        (EINVAL, dict(direction=_lib.TRACK_BOTH)), (EINVAL, dict(direction=2, bw=f)),
        (EINVAL, dict(bw=f, a1=-1.0)), (EINVAL, dict(bw=f, a2=float("nan"))),
        (ERANGE, dict(H=big, W=1)), (ERANGE, dict(H=1, W=big)), (ERANGE, dict(H=1 << 16, W=1 << 15)), (ERANGE, dict(H=1 << 16, W=1 << 16)),
        (ERANGE, dict(T=65536)),
        (EALIGN, dict(fw=f + 2)), (EALIGN, dict(bw=f + 1)), (EALIGN, dict(points=q + 2)), (EALIGN, dict(tracks=t + 2)),
        (EALIGN, dict(start=s + 2)),
    ]
    for code, change in refused:
        assert _call(**dict(good, **change)) == code, change
    torch.cuda.synchronize()
    assert bool((tracks == 7.0).all()) and bool((status == 0xEE).all())
    print(f"track refusals: {len(refused)} calls refused, outputs untouched")
    # (the largest sizes that pass the range checks are not run: they are sizes of memory, not of the grid)
    assert _call(**good) == 0 and _call(**dict(good, fw=f + 4, fw_cs=4)) == 0       # and an accepted call writes every element
    torch.cuda.synchronize()
    assert bool((status != 0xEE).all()) and bool((tracks != 7.0).all())
    with pytest.raises(_lib.PwcHipError, match="track points"):
        P.track_points(torch.zeros((1, 1, big, 2), device="cuda"), pts)


def test_tracker_streams_batches_with_the_check(P, tmp_path):
    """infer_continuous.Tracker fed two batches (2 and 3 flows, with the reversed flows) against the restatement over all five."""
    import infer_continuous
    kw = R.variant_kwargs("fw_check_nomasks_start")
    tracker = infer_continuous.Tracker(kw["points"], kw["start"], R.MAIN["T"] + 1, str(tmp_path / "o"))
    fw, bw = _up(kw["flows_fw"]), _up(kw["flows_bw"])
    tracker.add(0, fw[:2], bw[:2])
    assert tuple(tracker.points.shape) == (R.MAIN["P"], 2) and tuple(tracker.state.shape) == (R.MAIN["P"],)
    tracker.add(2, fw[2:], bw[2:])
    tracker.save()
    got = (np.load(tmp_path / "o" / "tracks.npy"), np.load(tmp_path / "o" / "tracks_status.npy"))
    _check("tracker, batches of 2 and 3", got, R.reference("fw_check_nomasks_start"))


def test_infer_continuous_track_cli(P, tmp_path):
    """The CLI in a fresh child process: four 64 x 64 frames, un-learned weights, --track grid:16 --batch 2 (the tracks cross the
    batch boundary).  tracks.npy equals the restatement run on the .flo files read back, bit for bit, and the .flo / .png
    files are those of a run without the flag, byte for byte."""
    from PIL import Image
    from pwcnet_amd import flow_io
    rng = np.random.RandomState(3)
    base = rng.uniform(0, 255, size=(64, 64, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(4):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o"), "--track", "grid:16"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    out = tmp_path / "o" / "seq"
    flows = np.stack([flow_io.read_flo(str(out / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)])
    pts = TK.grid_points(64, 64, 16).numpy()
    got = (np.load(tmp_path / "o" / "tracks.npy"), np.load(tmp_path / "o" / "tracks_status.npy"))
    assert got[0].shape == (4, 16, 2) and got[0].dtype == np.float32 and got[1].shape == (4, 16) and got[1].dtype == np.uint8
    assert np.array_equal(_bits(got[0][0]), _bits(pts)) and (got[1][0] == R.VISIBLE).all()
    _check("cli grid:16", got, R.track(flows, pts))
    run = subprocess.run(cli + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert not (tmp_path / "plain" / "tracks.npy").exists() and not (tmp_path / "plain" / "tracks_status.npy").exists()
    for i in range(3):                                                         # the flag changes nothing else
        for ext in (".flo", ".png"):
            assert (tmp_path / "plain" / "seq" / f"frame_{i:02d}{ext}").read_bytes() == (out / f"frame_{i:02d}{ext}").read_bytes()


def test_infer_continuous_track_fb_cli(P, tmp_path):
    """--track FILE --track_fb --fit pad on 70 x 100 frames, one child process: the reversed pairs are run and refitted too.  The
    backward flows are not written, so the check itself is test_tracker_streams_batches_with_the_check's business; here every
    point must sit where the restatement WITHOUT the check (on the .flo files read back) puts it, up to and including the
    first slice at which the check stops it."""
    from PIL import Image
    from pwcnet_amd import flow_io
    rng = np.random.RandomState(4)
    base = rng.uniform(0, 255, size=(70, 100, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(4):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(seq / f"frame_{i:02d}.png")
    spec = tmp_path / "queries.txt"
    spec.write_text("0 10.5 20.25\n0 99 69\n1 50 35\n3 7 7\n2 -3 5\n0 64.75 0\n")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1",
                          "--batch", "2", "--fit", "pad", "--out", str(tmp_path / "o"), "--track", str(spec), "--track_fb"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    flows = np.stack([flow_io.read_flo(str(tmp_path / "o" / "seq" / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)])
    assert flows.shape == (3, 70, 100, 2)
    pts = np.array([[10.5, 20.25], [99, 69], [50, 35], [7, 7], [-3, 5], [64.75, 0]], np.float32)
    start = np.array([0, 0, 1, 3, 2, 0], np.int32)
    tracks, status = np.load(tmp_path / "o" / "tracks.npy"), np.load(tmp_path / "o" / "tracks_status.npy")
    want_t, want_s = R.track(flows, pts, start=start)
    print(f"track cli --track_fb: P 6 T 3 last slice {R.histogram(status[-1])}; without the check {R.histogram(want_s[-1])}")
    assert tracks.shape == (4, 6, 2) and status.shape == (4, 6)
    for p in range(6):
        for t in range(4):
            assert status[t, p] == want_s[t, p] or (want_s[t, p] == R.VISIBLE and status[t, p] in (R.OCCLUDED, R.UNKNOWN)), (p, t)
            if status[t, p] != R.UNKNOWN:
                assert np.array_equal(_bits(tracks[t, p]), _bits(want_t[t, p])), (p, t)
            if status[t, p] != want_s[t, p]:
                break                                                          # stopped by the check: the rest repeats
    assert status[3, 3] == R.VISIBLE and (status[:3, 3] == R.UNSEEN).all() and (status[2:, 4] == R.LEFT).all()
