"""Relative pose and depth on the GPU (pwc_pose.hip, pwcnet_amd.pose, infer_continuous.py --intrinsics / --depth) against the
numpy restatement of tests/pose_ref.py (checked on the CPU by tests/test_host_pose.py).

The kernels' operations are IEEE double + - x / sqrt and comparisons in a fixed order, with no fused multiply-add, and the
restatement performs the same operations in the same order; the vote's counts are integers.  The yardstick is BIT EQUALITY, no
tolerance; it rests on the device's double division and square root being correctly rounded.  The one test that is not bit
equality is the geometry on the device: the scene without the block gives its own rotation and translation back within 1e-4
degrees and its depth map within 1e-6 (the restatement's figures: 6.2e-8 degrees at most for the rotation, 3.4e-7 for the
translation, 1.2e-7 for the depth).  Every case prints its figures before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import pose as PO  # the feature: without it nothing here can be collected
from tests import fundamental_ref as FR
from tests import pose_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((2, 48, 64), (1, 40, 136), (3, 17, 19), (1, 64, 520))
KEYS = ("rotation", "translation", "ok", "votes", "voters", "singular", "essential")
_FITS = {}


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.camera_pose is PO.camera_pose and pwcnet_amd.flow_depth is PO.flow_depth
    return pwcnet_amd


def _up(a):
    return a if a is None or not isinstance(a, np.ndarray) else torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _sentinels(flows, seed):
    """The flows with NaN, Inf, the .flo sentinel and a huge value at 3 % of the pixels, one component each."""
    shown = flows.copy()
    idx = np.argwhere(np.random.RandomState(seed).uniform(size=flows.shape[:3]) < 0.03)
    for (n, y, x), bad in zip(idx, [np.nan, np.inf, -np.inf, 1e10, -2e9] * len(idx)):
        shown[n, y, x, (y + x) % 2] = bad
    return shown


def _matrices(N, H, W, block=True):
    """FR.fit(...) at iters = 4 of FR.batch(N, H, W), computed once and left unchanged."""
    key = (N, H, W, block)
    if key not in _FITS:
        m = FR.fit(FR.batch(N, H, W, block), None, 4, 1.0)["matrices"]
        m.setflags(write=False)
        _FITS[key] = m
    return _FITS[key]


def _pose(P, flows, F, K, valid=None, **kw):
    r, t, ok, info = P.camera_pose(_up(flows), _up(np.array(F)), K, _up(valid), **kw)
    assert r.dtype == torch.float64 and t.dtype == torch.float64 and ok.dtype == torch.bool
    assert info["votes"].dtype == torch.int32 and info["voters"].dtype == torch.int32 and info["votes"].shape == (r.shape[0], 4)
    assert info["singular"].shape == (r.shape[0], 2) and info["essential"].shape == (r.shape[0], 3, 3) and t.shape == (r.shape[0], 3)
    return dict(rotation=r.cpu().numpy(), translation=t.cpu().numpy(), ok=ok.cpu().numpy(), **{k: info[k].cpu().numpy() for k in KEYS[3:]})


def _same(tag, got, want):
    diff = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in KEYS}
    print(f"pose {tag}: ok {want['ok'].astype(int).tolist()} votes {want['votes'].tolist()} voters {want['voters'].tolist()} "
          f"elements that differ {diff}")
    for k in KEYS:
        assert _eq(got[k], want[k]), (tag, k)


def _depth(P, flows, p, K, valid=None, min_parallax=0.25):
    d, kn, par = P.triangulate_depth(_up(flows), _up(p["rotation"]), _up(p["translation"]), K, _up(valid), min_parallax=min_parallax,
                                     return_parallax=True)
    assert d.dtype == torch.float32 and kn.dtype == torch.bool and par.dtype == torch.float32
    return d.cpu().numpy(), kn.cpu().numpy(), par.cpu().numpy()


def _same_depth(tag, got, want):
    diff = [int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)]
    print(f"pose depth {tag}: known {want[1].sum(axis=(1, 2)).tolist()} of {want[1][0].size}, elements that differ (depth, known, parallax) {diff}")
    for g, w in zip(got, want):
        assert _eq(g, w), tag


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_camera_pose_equals_the_restatement_bit_for_bit(P, shape):
    N, H, W = shape
    flows, F, K = FR.batch(N, H, W), _matrices(N, H, W), R.scene_intrinsics(H, W)
    valid = np.random.RandomState(H + W).uniform(size=(N, H, W)) > 0.2
    assert FR.MR.parts_of(H, W) == {(48, 64): 12, (40, 136): 22, (17, 19): 2, (64, 520): 130}[(H, W)]
    for tag, f, v in (("plain", flows, None), ("mask", flows, valid), ("sentinels", _sentinels(flows, H), None)):
        want = R.pose(f, F, K, v, 1.0)
        _same(f"{N}x{H}x{W} {tag}", _pose(P, f, F, K, v), want)
        if (H, W) in ((48, 64), (40, 136)):                                     # the test scene's own shapes
            assert want["ok"].all() and (want["votes"][np.arange(N), want["winner"]] == want["voters"]).all() and (want["voters"] > 0).all()
            if tag == "plain":
                assert want["voters"][0] == {(48, 64): 2964, (40, 136): 5224}[(H, W)]
    want = R.pose(flows, F, K, None, 0.05)                                      # a threshold that leaves voters out
    _same(f"{N}x{H}x{W} threshold 0.05", _pose(P, flows, F, K, threshold=0.05), want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_triangulate_depth_equals_the_restatement_bit_for_bit(P, shape):
    N, H, W = shape
    flows, F, K = FR.batch(N, H, W), _matrices(N, H, W), R.scene_intrinsics(H, W)
    p = R.pose(flows, F, K)
    inl = FR.residual(flows, F)[1]
    shown = _sentinels(flows, H)
    counts = {}
    for mp in (0.0, 0.25, 3.0):
        for tag, f, v in (("inliers", flows, inl), ("no mask", flows, None), ("sentinels", shown, None)):
            want = R.depth(f, p["rotation"], p["translation"], K, v, mp)
            _same_depth(f"{N}x{H}x{W} min_parallax {mp} {tag}", _depth(P, f, p, K, v, mp), want)
            counts[mp, tag] = int(want[1].sum())
    if (H, W) == (48, 64):                                                      # the smallest static parallax there is about 2.1 px
        assert counts[3.0, "inliers"] < counts[0.25, "inliers"] == counts[0.0, "inliers"] == int(inl.sum())
    d, kn = P.triangulate_depth(_up(flows), _up(p["rotation"]), _up(p["translation"]), K, _up(inl))      # no parallax output
    want = R.depth(flows, p["rotation"], p["translation"], K, inl, 0.25)
    assert _eq(d.cpu().numpy(), want[0]) and np.array_equal(kn.cpu().numpy(), want[1])


def test_channel_slices_and_an_odd_base_cover_both_load_forms(P):
    """Stride 2 on an 8-byte boundary and channels 2:4 of a 4-channel buffer (one 8-byte load); channels 1:3 of a 3- and a
    4-channel buffer and a dense buffer that starts on an odd 4-byte boundary (two 4-byte loads)."""
    N, H, W = 2, 48, 64
    flows, F, K = FR.batch(N, H, W), _matrices(N, H, W), R.scene_intrinsics(H, W)
    want = _pose(P, flows, F, K)
    wdep = _depth(P, flows, want, K)
    _same("dense", want, R.pose(flows, F, K))
    views = []
    for width, lo, mod in ((2, 0, 0), (4, 2, 0), (3, 1, 4), (4, 1, 4)):
        buf = torch.full(flows.shape[:3] + (width,), float("nan"), dtype=torch.float32, device="cuda")
        buf[..., lo:lo + 2] = _up(flows)
        views.append((f"stride {width} offset {lo}", buf[..., lo:lo + 2], mod))
    flat = torch.zeros(flows.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = _up(flows).reshape(-1)
    views.append(("odd base", flat[1:].view(flows.shape), 4))
    for tag, view, mod in views:
        assert view.data_ptr() % 8 == mod
        r, t, ok, info = P.camera_pose(view, _up(np.array(F)), K)
        got = dict(rotation=r.cpu().numpy(), translation=t.cpu().numpy(), ok=ok.cpu().numpy(), **{k: info[k].cpu().numpy() for k in KEYS[3:]})
        _same(tag, got, want)
        d, kn, par = P.triangulate_depth(view, r, t, K, return_parallax=True)
        _same_depth(tag, (d.cpu().numpy(), kn.cpu().numpy(), par.cpu().numpy()), wdep)


def test_degenerate_images_inside_a_batch(P):
    """The batch convention: a degenerate image gives ok False and zeros, and its neighbours' bits are those of their own
    one-image calls."""
    N, H, W = 3, 48, 64
    flows, K = FR.batch(N, H, W), np.tile(R.scene_intrinsics(H, W), (N, 1))
    F = np.array(_matrices(N, H, W))
    alone = [_pose(P, flows[n:n + 1], F[n:n + 1], K[n:n + 1]) for n in range(N)]
    assert all(a["ok"][0] for a in alone)
    zero_F, no_fx, nan_k, unknown = F.copy(), K.copy(), K.copy(), flows.copy()
    zero_F[1], no_fx[1, 0], nan_k[1, 3], unknown[1] = 0.0, 0.0, np.nan, 1e10
    for tag, f, m, k in (("an all-zero F", flows, zero_F, K), ("fx = 0", flows, F, no_fx), ("a NaN intrinsic", flows, F, nan_k),
                         ("all flows unknown", unknown, F, K)):
        want = R.pose(f, m, k)
        got = _pose(P, f, m, k)
        _same(f"degenerate, {tag}", got, want)
        assert got["ok"].tolist() == [True, False, True] and not got["rotation"][1].any() and not got["translation"][1].any(), tag
        assert got["voters"][1] == 0 and not got["votes"][1].any(), tag
        for n in (0, 2):
            for key in KEYS:
                assert _eq(got[key][n:n + 1], alone[n][key]), (tag, n, key)
        dep = _depth(P, f, got, k, None, 0.25)
        _same_depth(f"degenerate, {tag}", dep, R.depth(f, want["rotation"], want["translation"], k, None, 0.25))
        assert not dep[1][1].any() and (dep[0][1] == R.SENTINEL).all() and dep[1][0].any() and dep[1][2].any(), tag   # an all-zero rotation


def test_two_calls_and_a_batch_against_its_images(P):
    N, H, W = 3, 40, 136
    flows, F, K = FR.batch(N, H, W), _matrices(N, H, W), R.scene_intrinsics(H, W)
    valid = np.random.RandomState(9).uniform(size=(N, H, W)) > 0.2
    a, b = _pose(P, flows, F, K, valid), _pose(P, flows, F, K, valid)
    _same("two calls", a, b)
    da, db = _depth(P, flows, a, K, valid), _depth(P, flows, a, K, valid)
    _same_depth("two calls", da, db)
    for n in range(N):
        one = _pose(P, flows[n:n + 1], F[n:n + 1], K, valid[n:n + 1])
        _same(f"image {n} alone", one, {k: a[k][n:n + 1] for k in KEYS})
        _same_depth(f"image {n} alone", _depth(P, flows[n:n + 1], one, K, valid[n:n + 1]), [x[n:n + 1] for x in da])


def test_flow_depth_equals_the_four_calls_chained_by_hand(P):
    N, H, W = 2, 48, 64
    flows, K = _up(FR.batch(N, H, W)), R.scene_intrinsics(H, W)
    valid = _up(np.random.RandomState(3).uniform(size=(N, H, W)) > 0.1)
    depth, known, rotation, translation, ok, info = P.flow_depth(flows, K, valid=valid, iters=3, scale=0.8, threshold=0.7, min_parallax=2.5)
    m, fok, _ = P.fit_fundamental(flows, valid=valid, iters=3, scale=0.8)
    dist, inl = P.epipolar_residual(flows, m, valid=valid, threshold=0.7)
    r, t, pok, pinfo = P.camera_pose(flows, m, K, valid=valid, threshold=0.7)
    d, kn = P.triangulate_depth(flows, r, t, K, valid=inl, min_parallax=2.5)
    print(f"pose flow_depth: ok {ok.tolist()} known {known.sum(dim=(1, 2)).tolist()} of inliers {inl.sum(dim=(1, 2)).tolist()}")
    assert torch.equal(depth.view(torch.int32), d.view(torch.int32)) and torch.equal(known, kn) and bool(ok.all())
    assert torch.equal(rotation.view(torch.int64), r.view(torch.int64)) and torch.equal(translation.view(torch.int64), t.view(torch.int64))
    assert torch.equal(ok, pok) and torch.equal(info["matrices"].view(torch.int64), m.view(torch.int64)) and torch.equal(info["inlier"], inl)
    for key in ("votes", "voters"):
        assert torch.equal(info[key], pinfo[key])
    assert 0 < int(known.sum()) < int(inl.sum())                                # 2.5 px switches pixels off at 48 x 64
    want = R.flow_depth(flows.cpu().numpy(), K, valid.cpu().numpy(), 3, 0.8, 0.7, 2.5)
    assert _eq(depth.cpu().numpy(), want[0]) and np.array_equal(known.cpu().numpy(), want[1])


@pytest.mark.parametrize("shape", [(48, 64), (40, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry_on_the_device(P, shape):
    """Not bit equality: the scene without the block gives back the pose and the depth map it was rendered with."""
    H, W = shape
    flow = FR.scene(H, W, 0, False, 0.0)[0][None]
    K = [float(W), float(W), (W - 1) / 2.0, (H - 1) / 2.0]
    depth, known, rotation, translation, ok, info = P.flow_depth(_up(flow), K)
    rot = R.rotation_error(rotation[0].cpu().numpy(), R.scene_rotation())
    tra = R.direction_error(translation[0].cpu().numpy(), R.scene_translation())
    rel = np.abs(depth[0].cpu().numpy() / R.scene_depth(H, W) - 1.0)
    print(f"pose geometry {H}x{W}: rotation {rot:.3e} deg, translation {tra:.3e} deg, known {float(known.float().mean()):.4f}, "
          f"relative depth error max {rel.max():.3e}, votes {info['votes'][0].tolist()} of {int(info['voters'][0])}")
    assert bool(ok[0]) and rot <= 1e-4 and tra <= 1e-4
    assert bool(known.all()) and rel.max() <= 1e-6


def test_infer_continuous_pose_and_depth_cli(P, tmp_path):
    """The CLI in fresh child processes, each with its own time limit: four 64 x 128 frames, a random texture carried along the
    scene's flow, un-learned weights.  --motion fundamental --intrinsics ... --depth writes pose.npy, pose_ok.npy, _depth.npy and _depth.png;
    the same command without the new flags writes the files it wrote before with identical bytes; the argument errors come before
    any GPU work."""
    from PIL import Image
    H, W = 64, 128
    rng = np.random.RandomState(5)
    base = rng.uniform(0, 255, size=(H, W, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    flow = FR.scene(H, W, 0, False)[0]
    y, x = np.mgrid[0:H, 0:W]
    for i in range(4):                                                          # frame i: the texture moved i steps along the flow
        ys = np.clip(np.rint(y - i * flow[..., 1]), 0, H - 1).astype(int)
        xs = np.clip(np.rint(x - i * flow[..., 0]), 0, W - 1).astype(int)
        Image.fromarray(base[ys, xs]).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2"]
    K = ["--intrinsics", str(W), str(W), str((W - 1) / 2.0), str((H - 1) / 2.0)]
    for flags, word in ((["--motion", "fundamental", "--depth"], "--depth needs --intrinsics"),
                        (["--motion", "affine"] + K, "--intrinsics needs --motion fundamental")):
        run = subprocess.run(cli + ["--out", str(tmp_path / "refused")] + flags, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and word in run.stderr and not (tmp_path / "refused").exists(), run.stderr[-500:]
    tops = {}
    for tag, flags in (("old", []), ("new", K + ["--depth", "--depth_min_parallax", "0"])):
        tops[tag] = tmp_path / tag
        run = subprocess.run(cli + ["--out", str(tops[tag]), "--motion", "fundamental", "--motion_residual"] + flags,
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    def files(top):
        return sorted(os.path.relpath(os.path.join(d, f), top) for d, _, fs in os.walk(top) for f in fs)
    old, new = files(tops["old"]), files(tops["new"])
    extra = sorted(set(new) - set(old))
    print(f"pose cli: {len(old)} files without the flags, {len(new)} with: {extra}")
    assert set(old) <= set(new)
    for f in old:                                                               # what was written before: identical bytes
        assert open(tops["old"] / f, "rb").read() == open(tops["new"] / f, "rb").read(), f
    assert extra == sorted(["pose.npy", "pose_ok.npy"] + [f"seq/frame_{i:02d}_depth.{e}" for i in range(3) for e in ("npy", "png")])
    pose, ok, motion = np.load(tops["new"] / "pose.npy"), np.load(tops["new"] / "pose_ok.npy"), np.load(tops["new"] / "motion.npy")
    assert pose.shape == (3, 3, 4) and pose.dtype == np.float64 and ok.shape == (3,) and ok.dtype == bool
    from pwcnet_amd import flow_io
    flows = np.stack([flow_io.read_flo(str(tops["new"] / "seq" / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)])
    Kv = [float(k) for k in K[1:]]
    want = R.pose(flows, motion, Kv)
    inl = FR.residual(flows, motion)[1]
    wdep = R.depth(flows, want["rotation"], want["translation"], Kv, inl, 0.0)
    print(f"pose cli: ok {ok.tolist()}, known {wdep[1].sum(axis=(1, 2)).tolist()}")
    assert _eq(pose[:, :, :3], want["rotation"]) and _eq(pose[:, :, 3], want["translation"]) and np.array_equal(ok, want["ok"])
    sys.path.insert(0, ROOT)
    try:
        from infer_continuous import inverse_depth_picture
    finally:
        sys.path.remove(ROOT)
    for i in range(3):
        d = np.load(tops["new"] / "seq" / f"frame_{i:02d}_depth.npy")
        png = np.asarray(Image.open(tops["new"] / "seq" / f"frame_{i:02d}_depth.png"))
        assert d.shape == (H, W) and d.dtype == np.float32 and _eq(d, wdep[0][i])
        assert png.shape == (H, W) and png.dtype == np.uint8 and np.array_equal(png, inverse_depth_picture(d))
        assert not png[~wdep[1][i]].any()
