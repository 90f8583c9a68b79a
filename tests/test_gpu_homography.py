"""Projective camera motion on the GPU (pwc_homography.hip, the projective entry points of pwc_motion.hip and pwc_plate.hip,
pwcnet_amd.homography, infer_continuous.py --motion homography) against the numpy restatement of tests/homography_ref.py (checked
on the CPU by tests/test_host_homography.py).

The kernels' operations are IEEE double + - x /, floor, rint and comparisons in a fixed order, with no fused multiply-add and no
library function, and the restatement performs the same operations in the same order -- the partition, the tree and the part
order of the sums included: the yardstick is BIT EQUALITY, no tolerance.  It rests on the device's double division being
correctly rounded.  Every case prints its figures before it asserts."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import homography as HO  # the feature: without it nothing here can be collected
from tests import homography_ref as R
from tests import motion_ref as MR
from tests import plate_ref as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_SHAPES = ((1, 3), (2, 2), (3, 5), (17, 33), (64, 128), (260, 256))
KEYS = ("matrices", "ok", "count", "weight_sum")


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.fit_homography is HO.fit_homography
    return pwcnet_amd


def _up(a):
    return a if a is None or not isinstance(a, np.ndarray) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fit(P, flows, valid=None, **kw):
    m, ok, info = P.fit_homography(_up(flows), _up(valid), **kw)
    assert m.dtype == torch.float64 and ok.dtype == torch.bool and info["count"].dtype == torch.int32
    return dict(matrices=m.cpu().numpy(), ok=ok.cpu().numpy(), count=info["count"].cpu().numpy(),
                weight_sum=info["weight_sum"].cpu().numpy())


def _same(tag, got, want):
    diff = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in KEYS}
    print(f"homography {tag}: ok {want['ok'].astype(int).tolist()} count {want['count'].tolist()} elements that differ {diff}")
    for k in KEYS:
        assert _eq(got[k], want[k]), (tag, k)


def _flows(H, W, N=2):
    """N flows of a shape: the exact flow of a homography, 0.05 px of noise and (from 17 x 33 up) the block of outliers."""
    return np.stack([R.scene(H, W, seed=n, outliers=H * W >= 500, noise=0.05)[0] for n in range(N)])


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fit_equals_the_restatement_bit_for_bit(P, shape):
    H, W = shape
    flows = _flows(H, W)
    valid = np.random.RandomState(H + W).uniform(size=(2, H, W)) > 0.2 if H * W >= 500 else None
    for iters in (0, 1, 4):
        for v in ((None, valid) if valid is not None else (None,)):
            want = R.fit(flows, v, iters, 1.0)
            _same(f"fit {H}x{W} iters {iters} mask {v is not None}", _fit(P, flows, v, iters=iters), want)
    want = R.fit(flows, None, 4, 1.0)
    if shape == (1, 3):
        assert not want["ok"].any() and (want["count"] == 3).all() and np.array_equal(want["matrices"][0], np.eye(3))
    else:
        assert want["ok"].all() and (want["count"] == H * W).all()
    if H * W >= 500:                                                           # the block is voted out (tests/test_host_homography.py)
        assert R.corner_error(want["matrices"][0], R.scene(H, W, 0, True, 0.05)[1], H, W) < 0.5


def test_a_batch_of_three_masks_and_unknown_pixels(P):
    """Three different motions, the middle image fully masked; every image equals its single-image call; a uint8 and a bool
    mask; NaN, Inf and sentinel pixels under the mask and in the open."""
    H, W = 17, 33
    flows = _flows(H, W, 3)
    valid = np.random.RandomState(3).uniform(size=(3, H, W)) > 0.2
    valid[1] = False
    want = R.fit(flows, valid, 4, 1.0)
    assert want["ok"].tolist() == [True, False, True] and want["count"][1] == 0
    _same("batch of 3, bool mask", _fit(P, flows, valid, iters=4), want)
    _same("batch of 3, uint8 mask", _fit(P, flows, valid.astype(np.uint8) * 255, iters=4), want)
    for n in range(3):
        _same(f"image {n} alone", _fit(P, flows[n:n + 1], valid[n:n + 1], iters=4), {k: want[k][n:n + 1] for k in KEYS})
    shown = flows.copy()
    idx = np.argwhere(~valid)
    for (n, y, x), bad in zip(idx, [np.nan, np.inf, -np.inf, 1e10, -2e9] * len(idx)):
        shown[n, y, x, (y + x) % 2] = bad
    _same("nan, inf, sentinel in the open", _fit(P, shown, None, iters=4), want)
    again = _fit(P, flows, valid, iters=4)
    _same("two calls", again, _fit(P, flows, valid, iters=4))


def test_a_pass_that_leaves_pixels_behind_the_horizon_out(P):
    """A strong perspective (g6 = 1.3 in normalised coordinates) and a few known pixels where its D is negative: from pass 2 on
    six pixels are left out of the sums; the fit ends with the horizon inside the frame: ok False, the identity."""
    H, W = 17, 33
    xh, yh, _, _, s = MR.normalised(H, W)
    g = [1.0, 0.05, 0.1, -0.03, 1.0, 0.05, 1.3, 0.2]
    D = g[6] * xh + g[7] * yh + 1
    xp, yp = (g[0] * xh + g[1] * yh + g[2]) / D, (g[3] * xh + g[4] * yh + g[5]) / D
    flow = np.stack([(xp - xh) * s, (yp - yh) * s], 1).reshape(H, W, 2)
    valid = (D > 0.35).reshape(H, W)
    flow[~valid] = 0.0
    valid[::4, 0] = True
    valid[3, 1] = True
    flow = flow.astype(np.float32)[None]
    for iters in (0, 2, 4):
        want = R.fit(flow, valid[None], iters, 1.0)
        print(f"homography horizon in a pass: iters {iters} left out per pass {want['left_out'][0]}")
        _same(f"D <= 0 in a pass, iters {iters}", _fit(P, flow, valid[None], iters=iters), want)
        if iters >= 2:
            assert want["left_out"][0][-1] > 0 and not want["ok"][0] and np.array_equal(want["matrices"][0], np.eye(3))


def test_channel_slices_cover_both_load_forms(P):
    """Channels 2:4 of a 4-channel buffer (stride 4, an 8-byte boundary: one 8-byte load) and channels 1:3 of a 3-channel one
    (stride 3, a 4-byte boundary: two 4-byte loads)."""
    H, W = 17, 33
    flows = _flows(H, W)
    want = R.fit(flows, None, 4, 1.0)
    wres = R.residual(flows, want["matrices"])
    for width, lo, mod in ((4, 2, 0), (4, 0, 0), (3, 1, 4), (4, 1, 4)):
        buf = torch.full(flows.shape[:3] + (width,), float("nan"), dtype=torch.float32, device="cuda")
        buf[..., lo:lo + 2] = _up(flows)
        view = buf[..., lo:lo + 2]
        assert view.data_ptr() % 8 == mod
        m, ok, info = P.fit_homography(view, iters=4)
        got = dict(matrices=m.cpu().numpy(), ok=ok.cpu().numpy(), count=info["count"].cpu().numpy(), weight_sum=info["weight_sum"].cpu().numpy())
        _same(f"stride {width} offset {lo}", got, want)
        res, inl = P.motion_residual(view, m, projective=True)
        assert _eq(res.cpu().numpy(), wres[0]) and np.array_equal(inl.cpu().numpy(), wres[1])


def _matrices(N, H, W, seed=0):
    """N pixel homographies near the identity, then three special ones in front: a horizon that crosses the frame, a non-finite
    entry, an exactly affine matrix."""
    M = np.stack([R.true_matrix(H, W, 3e-3 / max(H, W) * (n + 1), -2e-3 / max(H, W), seed + n) for n in range(N)])
    if N >= 3:
        M[0, 2] = (-2.0 / W, 0.1 / H, 1.0)                                     # D < 0 in the right half
        M[1, 0, 1] = np.inf
        M[2, 2] = (0.0, 0.0, 1.0)
    return M


@pytest.mark.parametrize("shape", [(3, 4), (33, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_residual_and_warp_equal_the_restatement_bit_for_bit(P, shape):
    H, W = shape
    N = 4
    M = _matrices(N, H, W)
    rs = np.random.RandomState(H)
    flows = rs.normal(0, 3, size=(N, H, W, 2)).astype(np.float32)
    flows[rs.uniform(size=(N, H, W)) < 0.05] = np.nan
    valid = rs.uniform(size=(N, H, W)) > 0.1
    want = R.residual(flows, M, valid, 3.0)
    res, inl = P.motion_residual(_up(flows), _up(M), _up(valid), threshold=3.0, projective=True)
    print(f"homography residual {H}x{W}: inliers {want[1].sum(axis=(1, 2)).tolist()}, sentinels "
          f"{(want[0][..., 0] == R.SENTINEL).sum(axis=(1, 2)).tolist()}, bits differ at {int((_bits(res.cpu().numpy()) != _bits(want[0])).sum())}")
    assert _eq(res.cpu().numpy(), want[0]) and np.array_equal(inl.cpu().numpy(), want[1])
    assert (want[0][1] == R.SENTINEL).all() and 0 < (want[0][0, ..., 0] == R.SENTINEL).sum() < H * W
    assert (want[0][0][:, W - 1] == R.SENTINEL).all()                          # behind the horizon
    # the exactly affine matrix: the affine entry point's bits
    ares, ainl = P.motion_residual(_up(flows[2:3]), _up(M[2:3]), _up(valid[2:3]), threshold=3.0)
    assert torch.equal(ares.view(torch.int32), res[2:3].view(torch.int32)) and torch.equal(ainl, inl[2:3])
    mres = MR.residual(flows[2:3], M[2:3], valid[2:3], 3.0)
    assert _eq(mres[0], want[0][2:3]) and np.array_equal(mres[1], want[1][2:3])
    for dtype in (np.uint8, np.float32):
        for C in (1, 2, 3, 4):
            frames = MR.random_frames(N, H, W, C, dtype, seed=C)
            wout, wcov = R.warp(frames, M)
            out, cov = P.warp_frames(_up(frames), _up(M), projective=True)
            assert out.dtype == _up(frames).dtype and cov.dtype == torch.bool
            print(f"homography warp {np.dtype(dtype).name} C {C} {H}x{W}: covered {wcov.sum(axis=(1, 2)).tolist()}, bits differ at "
                  f"{int((_bits(out.cpu().numpy()) != _bits(wout)).sum())}")
            assert _eq(out.cpu().numpy(), wout) and np.array_equal(cov.cpu().numpy(), wcov)
            assert not wcov[1].any() and not wcov[0][:, W - 1].any() and wcov[3].any()
            aout, acov = P.warp_frames(_up(frames[2:3]), _up(M[2:3]))
            assert torch.equal(aout, out[2:3]) and torch.equal(acov, cov[2:3])
            # an output pointer off the 16-byte (floats) / 4-byte (bytes) boundary: the same values one by one
            flat = torch.zeros(out.numel() + 1, dtype=out.dtype, device="cuda")
            covered = torch.zeros(N * H * W + 1, dtype=torch.uint8, device="cuda")
            fr, mm = _up(frames), _up(M)
            rc = _lib.lib().pwc_warp_projective(ctypes.c_void_p(fr.data_ptr()), _lib.MOTION_U8 if dtype == np.uint8 else _lib.MOTION_F32,
                                                C, ctypes.c_void_p(mm.data_ptr()), N, H, W,
                                                ctypes.c_void_p(flat.data_ptr() + out.element_size()),
                                                ctypes.c_void_p(covered.data_ptr() + 1), _lib.current_stream())
            assert rc == 0
            assert torch.equal(flat[1:].view(out.shape), out) and torch.equal(covered[1:].view(N, H, W).bool(), cov)


def test_residual_past_the_grid_cap(P):
    """3 x 592 x 592 = 1 051 392 pixels, more than 4096 workgroups of 256 lanes: the grid-stride pass."""
    N, H, W = 3, 592, 592
    rs = np.random.RandomState(11)
    flows = rs.normal(0, 4, size=(N, H, W, 2)).astype(np.float32)
    flows[rs.uniform(size=(N, H, W)) < 0.01] = np.nan
    valid = rs.uniform(size=(N, H, W)) > 0.1
    M = _matrices(N, H, W)
    want = R.residual(flows, M, valid, 3.0)
    got = P.motion_residual(_up(flows), _up(M), _up(valid), threshold=3.0, projective=True)
    gres, ginl = got[0].cpu().numpy(), got[1].cpu().numpy()
    print(f"homography residual grid cap: {N * H * W} pixels, inliers {int(want[1].sum())}, bits differ at "
          f"{int((_bits(gres) != _bits(want[0])).sum())}, inlier differs at {int((ginl != want[1]).sum())}")
    assert (want[0][1] == R.SENTINEL).all() and want[1][2].sum() > 1000
    assert _eq(gres, want[0]) and np.array_equal(ginl, want[1])


def _plate_case(T, H, W, Hc, Wc, C, dtype):
    """tests/plate_ref.py's clip with perspective terms on every matrix and frame 2 behind the horizon: (case, matrices canvas ->
    frame, frame_matrices frame -> canvas)."""
    c = PR.case(T, H, W, Hc, Wc, C, dtype)
    rs = np.random.RandomState(T)
    M = c["matrices"].copy()
    M[:, 2, 0] = rs.uniform(-2e-3, 2e-3, size=T)
    M[:, 2, 1] = rs.uniform(-2e-3, 2e-3, size=T)
    inv = np.stack([np.linalg.inv(m) for m in M])
    inv = inv / inv[:, 2:3, 2:3]
    M[2] = -M[2]                                                               # the same points, D < 0 everywhere
    inv[2, 2] = (0.0, 0.0, -1.0)
    return c, M, inv


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("mode", [PR.MEDIAN, PR.MEAN])
@pytest.mark.parametrize("geometry", [(3, 8, 12, 13, 19), (64, 16, 16, 21, 37)], ids=["T3", "T64"])
def test_plate_and_difference_equal_the_restatement_bit_for_bit(P, geometry, mode, dtype):
    T, H, W, Hc, Wc = geometry
    C = 3 if T == 3 else 2
    c, M, inv = _plate_case(T, H, W, Hc, Wc, C, dtype)
    frames = _up(c["frames"])
    thr = 12.0 if dtype == np.uint8 else 0.05
    for use, masks in ((None, None), (c["use"], c["masks"])):
        wplate, wcount = R.plate_build(c["frames"], M, (Hc, Wc), mode, use, masks)
        plate, count = P.background_plate(frames, M, (Hc, Wc), mode=mode, use=use, masks=_up(masks), projective=True)
        print(f"homography plate T {T} {mode} {np.dtype(dtype).name} use/masks {use is not None}: count max {int(wcount.max())} "
              f"bits differ at {int((_bits(plate.cpu().numpy()) != _bits(wplate)).sum())}, count differs at {int((count.cpu().numpy() != wcount).sum())}")
        assert _eq(plate.cpu().numpy(), wplate) and np.array_equal(count.cpu().numpy(), wcount)
        assert 1 <= wcount.max() <= T - 1 - (use is not None)                  # frame 2 is behind the horizon: never a sample
        wd = R.plate_difference(c["frames"], wplate, wcount, inv, thr)
        d, fg, known = P.plate_difference(frames, plate, count, inv, thr, projective=True)
        assert _eq(d.cpu().numpy(), wd[0]) and np.array_equal(fg.cpu().numpy(), wd[1]) and np.array_equal(known.cpu().numpy(), wd[2])
        assert not wd[2][2].any() and wd[2][0].any()
    # affine matrices: projective=True gives the affine entries' bits
    a = P.background_plate(frames, c["matrices"], (Hc, Wc), mode=mode, use=c["use"], masks=_up(c["masks"]))
    b = P.background_plate(frames, c["matrices"], (Hc, Wc), mode=mode, use=c["use"], masks=_up(c["masks"]), projective=True)
    assert torch.equal(a[0].view(torch.uint8), b[0].view(torch.uint8)) and torch.equal(a[1], b[1])
    da = P.plate_difference(frames, a[0], a[1], c["frame_matrices"], thr)
    db = P.plate_difference(frames, a[0], a[1], c["frame_matrices"], thr, projective=True)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(da, db))
    want = PR.reference(T, H, W, Hc, Wc, C, np.dtype(dtype).type, mode, True, True)
    assert _eq(b[0].cpu().numpy(), want[0]) and np.array_equal(b[1].cpu().numpy(), want[1])


def test_infer_continuous_homography_cli(P, tmp_path):
    """The CLI in fresh child processes: four 64 x 128 frames, un-learned weights.  --motion homography --motion_residual --plate:
    the files equal the API's restatement on the .flo files read back.  --motion affine with the same flags: the files the affine
    restatements give, as before."""
    from PIL import Image
    from pwcnet_amd import flow_io, plate
    rng = np.random.RandomState(5)
    base = rng.uniform(0, 255, size=(64, 128, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    frames = np.stack([np.roll(base, 2 * i, axis=1) for i in range(4)])
    for i in range(4):
        Image.fromarray(frames[i]).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2",
           "--motion_residual", "--plate"]
    for model in ("homography", "affine"):
        top = tmp_path / model
        run = subprocess.run(cli + ["--out", str(top), "--motion", model], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
        out = top / "seq"
        motion, ok = np.load(top / "motion.npy"), np.load(top / "motion_ok.npy")
        flows = np.stack([flow_io.read_flo(str(out / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)])
        proj = model == "homography"
        want = R.fit(flows, None, 4, 1.0) if proj else MR.fit(flows, None, "affine", 4, 1.0)
        print(f"homography cli --motion {model}: ok {ok.tolist()}, last rows {motion[:, 2].tolist()}, bits differ at "
              f"{int((_bits(motion) != _bits(want['matrices'])).sum())}")
        assert motion.shape == (3, 3, 3) and _eq(motion, want["matrices"]) and np.array_equal(ok, want["ok"])
        wres, winl = R.residual(flows, motion) if proj else MR.residual(flows, motion)
        for i in range(3):
            res = flow_io.read_flo(str(out / f"frame_{i:02d}_residual.flo"))
            inl = np.asarray(Image.open(out / f"frame_{i:02d}_inlier.png"))
            assert _eq(res.astype(np.float32), wres[i]) and np.array_equal(inl == 255, winl[i])
        to_frame, reach = plate.plate_path(motion, ok, projective=proj)
        x0, y0, Hc, Wc = plate.plate_canvas(to_frame, reach, 64, 128, projective=proj)
        mats = plate.canvas_matrices(to_frame, x0, y0, projective=proj)[0]
        chosen = plate.select_frames(reach, 0, 32)
        build = R.plate_build if proj else PR.plate_build
        wplate, wcount = build(frames[chosen], mats[chosen], (Hc, Wc))
        assert np.array_equal(np.asarray(Image.open(top / "plate.png")), wplate)
        assert np.array_equal(np.asarray(Image.open(top / "plate_count.png")), wcount)
