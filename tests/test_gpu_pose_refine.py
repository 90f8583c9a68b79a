"""Pose refinement on the GPU (pwc_pose_refine.hip, pwcnet_amd.refine_pose, flow_depth(refine=K), infer_continuous.py --pose_refine)
against the numpy restatement of tests/pose_refine_ref.py (checked on the CPU by tests/test_host_pose_refine.py).

The kernels' operations are IEEE double + - x / sqrt and comparisons in a fixed order, with no fused multiply-add, and the
restatement performs the same operations in the same order; the counts are integers.  The yardstick is BIT EQUALITY of every
output, no tolerance; it rests on the device's double division and square root being correctly rounded.  The shapes cover both
flow load forms, an odd width, a last partial workgroup (17 x 19: 2 parts, the second with 67 pixels) and the largest part count
(64 x 520: 130).  Every case prints its figures before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import pose_refine as RP  # the feature: without it nothing here can be collected
from tests import fundamental_ref as FR
from tests import pose_ref as PR
from tests import pose_refine_ref as RR
from tests.test_host_pose import MEASURED as CLOSED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((2, 48, 64), (1, 40, 136), (3, 17, 19), (1, 64, 520))
KEYS = ("rotation", "translation", "ok", "samples", "best_pass", "cost", "weight_sum")
_POSES = {}


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.refine_pose is RP.refine_pose
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


def _start(N, H, W):
    """(flows, K, the closed-form rotation and translation of the restatement) of FR.batch(N, H, W), computed once, left unchanged."""
    key = (N, H, W)
    if key not in _POSES:
        flows, K = FR.batch(N, H, W), PR.scene_intrinsics(H, W)
        p = PR.pose(flows, FR.fit(flows, None, 4, 1.0)["matrices"], K)
        for a in (p["rotation"], p["translation"]):
            a.setflags(write=False)
        _POSES[key] = (flows, K, p["rotation"], p["translation"])
    return _POSES[key]


def _refine(P, flows, R0, t0, K, valid=None, **kw):
    r, t, ok, info = P.refine_pose(_up(flows), _up(np.array(R0)), _up(np.array(t0)), K, _up(valid), **kw)
    N = r.shape[0]
    assert r.dtype == torch.float64 and t.dtype == torch.float64 and ok.dtype == torch.bool and r.shape == (N, 3, 3) and t.shape == (N, 3)
    assert info["samples"].dtype == torch.int32 and info["best_pass"].dtype == torch.int32 and info["cost"].dtype == torch.float64
    assert info["cost"].shape == (N, kw.get("iters", 4) + 1) and info["weight_sum"].shape == (N,)
    return dict(rotation=r.cpu().numpy(), translation=t.cpu().numpy(), ok=ok.cpu().numpy(), **{k: info[k].cpu().numpy() for k in KEYS[3:]})


def _same(tag, got, want):
    diff = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in KEYS}
    print(f"pose refine {tag}: ok {want['ok'].astype(int).tolist()} samples {want['samples'].tolist()} best pass {want['best_pass'].tolist()} "
          f"frozen {want['frozen'].tolist() if 'frozen' in want else '-'} cost first {want['cost'][:, 0].tolist()} best "
          f"{want['cost'][np.arange(len(want['ok'])), want['best_pass']].tolist()} elements that differ {diff}")
    for k in KEYS:
        assert _eq(got[k], want[k]), (tag, k)
    best = got["cost"][np.arange(len(got["ok"])), got["best_pass"]]
    assert (best <= got["cost"][:, 0]).all(), tag                               # never worse than the input, in the op's own cost


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_refine_pose_equals_the_restatement_bit_for_bit(P, shape):
    N, H, W = shape
    flows, K, R0, t0 = _start(N, H, W)
    valid = np.random.RandomState(H + W).uniform(size=(N, H, W)) > 0.2
    assert FR.MR.parts_of(H, W) == {(48, 64): 12, (40, 136): 22, (17, 19): 2, (64, 520): 130}[(H, W)]
    cases = [("plain", flows, None, it, thr) for it in (0, 1, 6) for thr in (1.0, np.inf)]
    cases += [("mask", flows, valid, 6, 1.0), ("mask", flows, valid, 1, np.inf), ("sentinels", _sentinels(flows, H), None, 6, 1.0),
              ("sentinels", _sentinels(flows, H), None, 1, np.inf)]
    for tag, f, v, iters, thr in cases:
        want = RR.refine(f, R0, t0, K, v, iters, 1.0, thr)
        got = _refine(P, f, R0, t0, K, v, iters=iters, threshold=thr)
        _same(f"{N}x{H}x{W} {tag} iters {iters} threshold {thr}", got, want)
        if iters == 0:                                                          # the input pose, bit for bit
            assert _eq(got["rotation"], np.where(want["ok"][:, None, None], R0, 0.0)) and _eq(got["translation"], np.where(want["ok"][:, None], t0, 0.0))
        if (H, W) in ((48, 64), (40, 136)) and tag == "plain":                  # the test scene's own shapes
            assert want["ok"].all() and (want["frozen"] == -1).all()
            if thr == 1.0:
                assert want["samples"][0] == {(48, 64): 2964, (40, 136): 5224}[(H, W)]
            else:
                assert (want["samples"] == H * W).all()
    want = RR.refine(flows, R0, t0, K, None, 2, 0.5, 0.05)                      # another scale, a threshold that leaves pixels out
    _same(f"{N}x{H}x{W} scale 0.5 threshold 0.05", _refine(P, flows, R0, t0, K, iters=2, scale=0.5, threshold=0.05), want)


def test_channel_slices_and_an_odd_base_cover_both_load_forms(P):
    """Stride 2 on an 8-byte boundary and channels 2:4 of a 4-channel buffer (one 8-byte load); channels 1:3 of a 3- and a
    4-channel buffer and a dense buffer that starts on an odd 4-byte boundary (two 4-byte loads)."""
    N, H, W = 2, 48, 64
    flows, K, R0, t0 = _start(N, H, W)
    want = _refine(P, flows, R0, t0, K, iters=3)
    _same("dense", want, RR.refine(flows, R0, t0, K, None, 3))
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
        r, t, ok, info = P.refine_pose(view, _up(np.array(R0)), _up(np.array(t0)), K, iters=3)
        got = dict(rotation=r.cpu().numpy(), translation=t.cpu().numpy(), ok=ok.cpu().numpy(), **{k: info[k].cpu().numpy() for k in KEYS[3:]})
        _same(tag, got, want)


def test_off_and_frozen_images_inside_a_batch(P):
    """The batch convention: an OFF image gives ok False and zeros and a frozen image keeps its best pose, both in the middle of a
    batch, and their neighbours' bits are those of their own one-image calls."""
    N, H, W = 3, 48, 64
    flows, K1, R0, t0 = _start(N, H, W)
    K = np.tile(K1, (N, 1))
    alone = [_refine(P, flows[n:n + 1], R0[n:n + 1], t0[n:n + 1], K[n:n + 1], iters=3) for n in range(N)]
    assert all(a["ok"][0] for a in alone)
    zero_R, no_fx, nan_k, unknown = np.array(R0), K.copy(), K.copy(), flows.copy()
    zero_R[1], no_fx[1, 0], nan_k[1, 3], unknown[1] = 0.0, 0.0, np.nan, 1e10
    everything = np.ones((N, H, W), bool)
    four, five = everything.copy(), everything.copy()
    four[1], five[1] = False, False
    four[1, 3, 4:8] = True
    five[1, 3, 4:8], five[1, 9, 20] = True, True
    for tag, f, r, k, v, ok1 in (("an all-zero rotation", flows, zero_R, K, None, False), ("fx = 0", flows, R0, no_fx, None, False),
                                 ("a NaN intrinsic", flows, R0, nan_k, None, False), ("all flows unknown", unknown, R0, K, None, False),
                                 ("four samples", flows, R0, K, four, False), ("five samples", flows, R0, K, five, True)):
        want = RR.refine(f, r, t0, k, v, 3)
        got = _refine(P, f, r, t0, k, v, iters=3)
        _same(f"degenerate, {tag}", got, want)
        assert got["ok"].tolist() == [True, ok1, True], tag
        if not ok1:
            for key in ("rotation", "translation", "cost", "weight_sum", "best_pass"):
                assert not got[key][1].any(), (tag, key)
        else:                                                                   # five pixels do not carry five parameters here: frozen
            assert want["frozen"][1] >= 0 and got["samples"][1] == 5 and not got["cost"][1, want["frozen"][1] + 1:].any()
            assert _eq(got["rotation"][1], R0[1]) or got["best_pass"][1] > 0
        for n in (0, 2):
            for key in KEYS:
                assert _eq(got[key][n:n + 1], alone[n][key]), (tag, n, key)


def test_two_calls_and_a_batch_against_its_images(P):
    N, H, W = 3, 40, 136
    flows, K, R0, t0 = _start(N, H, W)
    valid = np.random.RandomState(9).uniform(size=(N, H, W)) > 0.2
    a, b = _refine(P, flows, R0, t0, K, valid, iters=6), _refine(P, flows, R0, t0, K, valid, iters=6)
    _same("two calls", a, b)
    for n in range(N):
        one = _refine(P, flows[n:n + 1], R0[n:n + 1], t0[n:n + 1], K, valid[n:n + 1], iters=6)
        _same(f"image {n} alone", one, {k: a[k][n:n + 1] for k in KEYS})


def test_flow_depth_with_and_without_refinement(P):
    N, H, W = 2, 48, 64
    flows, K = _up(FR.batch(N, H, W)), PR.scene_intrinsics(H, W)
    valid = _up(np.random.RandomState(3).uniform(size=(N, H, W)) > 0.1)
    kw = dict(valid=valid, iters=3, scale=0.8, threshold=0.7, min_parallax=2.5)
    plain, zero = P.flow_depth(flows, K, **kw), P.flow_depth(flows, K, refine=0, **kw)
    for a, b in zip(plain[:5], zero[:5]):                                       # refine = 0: the call as it was
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert sorted(plain[5]) == sorted(zero[5]) and "closed_rotation" not in zero[5]
    depth, known, rotation, translation, ok, info = P.flow_depth(flows, K, refine=4, **kw)
    m, fok, _ = P.fit_fundamental(flows, valid=valid, iters=3, scale=0.8)
    dist, inl = P.epipolar_residual(flows, m, valid=valid, threshold=0.7)
    r, t, pok, pinfo = P.camera_pose(flows, m, K, valid=valid, threshold=0.7)
    r2, t2, rok, rinfo = P.refine_pose(flows, r, t, K, valid=valid, iters=4, scale=0.8, threshold=0.7)
    d, kn = P.triangulate_depth(flows, r2, t2, K, valid=inl, min_parallax=2.5)
    print(f"pose refine flow_depth: ok {ok.tolist()} refine ok {rok.tolist()} best pass {rinfo['best_pass'].tolist()} known "
          f"{known.sum(dim=(1, 2)).tolist()} against {plain[1].sum(dim=(1, 2)).tolist()} closed")
    assert bool(rok.all()) and bool(ok.all()) and torch.equal(ok, pok)
    assert torch.equal(depth.view(torch.int32), d.view(torch.int32)) and torch.equal(known, kn)
    assert torch.equal(rotation.view(torch.int64), r2.view(torch.int64)) and torch.equal(translation.view(torch.int64), t2.view(torch.int64))
    assert torch.equal(info["closed_rotation"].view(torch.int64), r.view(torch.int64))
    assert torch.equal(info["closed_translation"].view(torch.int64), t.view(torch.int64))
    assert torch.equal(info["closed_rotation"].view(torch.int64), plain[2].view(torch.int64))
    assert torch.equal(info["refine_ok"], rok) and torch.equal(info["inlier"], inl)
    for key in ("samples", "best_pass", "cost", "weight_sum"):
        assert torch.equal(info[key], rinfo[key]), key
    assert not torch.equal(rotation, plain[2])                                  # the refinement moved the pose
    want = RR.flow_depth(flows.cpu().numpy(), K, valid.cpu().numpy(), 3, 0.8, 0.7, 2.5, 4)
    assert _eq(depth.cpu().numpy(), want[0]) and np.array_equal(known.cpu().numpy(), want[1])
    assert _eq(rotation.cpu().numpy(), want[2][0]) and _eq(translation.cpu().numpy(), want[2][1])
    # flow_trajectory hands refine through: its depth maps are flow_depth's
    td = P.flow_trajectory(flows, K, refine=4, **kw)
    assert torch.equal(td[0].view(torch.int32), depth.view(torch.int32)) and torch.equal(td[5]["rotation"].view(torch.int64), rotation.view(torch.int64))


@pytest.mark.parametrize("shape", [(48, 64), (40, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_accuracy_on_the_device(P, shape):
    """Not bit equality: on the block scene with 0.02 px of noise flow_depth(refine=6) brings the rotation, the translation and the
    median relative depth error to a quarter of the closed form's or less (tests/test_host_pose_refine.py has the figures)."""
    H, W = shape
    flow, rect = FR.scene(H, W, 0, True, 0.02)
    K = PR.scene_intrinsics(H, W)
    fig = []
    for refine in (0, 6):
        depth, known, rotation, translation, ok, info = P.flow_depth(_up(flow[None]), K, refine=refine)
        kn = known[0].cpu().numpy() & ~rect
        rel = np.abs(depth[0].cpu().numpy() / PR.scene_depth(H, W) - 1.0)[kn]
        fig.append((PR.rotation_error(rotation[0].cpu().numpy(), PR.scene_rotation()),
                    PR.direction_error(translation[0].cpu().numpy(), PR.scene_translation()), float(np.median(rel))))
        assert bool(ok[0])
    print(f"pose refine accuracy {H}x{W}: rotation {fig[0][0]:.4f} -> {fig[1][0]:.6f} deg, translation {fig[0][1]:.4f} -> {fig[1][1]:.6f} deg, "
          f"median relative depth error {fig[0][2]:.5f} -> {fig[1][2]:.6f}")
    for j in range(3):
        assert fig[1][j] <= CLOSED[shape][j] / 4.0, (j, fig)


def test_infer_continuous_pose_refine_cli(P, tmp_path):
    """The CLI in fresh child processes, each with its own time limit: four 64 x 128 frames, a random texture carried along the
    scene's flow, un-learned weights.  --pose_refine 3 writes pose.npy, pose_closed.npy and pose_refine.npy; the same command
    without the flag writes exactly the files it wrote before, and what both write apart from the pose has identical bytes."""
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
    Kf = ["--intrinsics", str(W), str(W), str((W - 1) / 2.0), str((H - 1) / 2.0)]
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2",
           "--motion", "fundamental"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "refused"), "--pose_refine", "3"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and "--pose_refine needs --intrinsics" in run.stderr and not (tmp_path / "refused").exists(), run.stderr[-500:]
    tops = {}
    for tag, flags in (("old", []), ("new", ["--pose_refine", "3"])):
        tops[tag] = tmp_path / tag
        run = subprocess.run(cli + Kf + ["--out", str(tops[tag])] + flags, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    def files(top):
        return sorted(os.path.relpath(os.path.join(d, f), top) for d, _, fs in os.walk(top) for f in fs)
    old, new = files(tops["old"]), files(tops["new"])
    extra = sorted(set(new) - set(old))
    print(f"pose refine cli: {len(old)} files without the flag, {len(new)} with: {extra}")
    assert "pose.npy" in old and "pose_closed.npy" not in old and "pose_refine.npy" not in old
    assert set(old) <= set(new) and extra == ["pose_closed.npy", "pose_refine.npy"]
    for f in old:                                                               # everything but the pose: identical bytes
        if f != "pose.npy":
            assert open(tops["old"] / f, "rb").read() == open(tops["new"] / f, "rb").read(), f
    pose, closed, rows = np.load(tops["new"] / "pose.npy"), np.load(tops["new"] / "pose_closed.npy"), np.load(tops["new"] / "pose_refine.npy")
    ok, motion = np.load(tops["new"] / "pose_ok.npy"), np.load(tops["new"] / "motion.npy")
    assert pose.shape == closed.shape == (3, 3, 4) and pose.dtype == closed.dtype == np.float64 and rows.shape == (3, 4) and rows.dtype == np.float64
    assert _eq(closed, np.load(tops["old"] / "pose.npy"))                       # the closed form is what the old command wrote
    from pwcnet_amd import flow_io
    flows = np.stack([flow_io.read_flo(str(tops["new"] / "seq" / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)])
    Kv = [float(k) for k in Kf[1:]]
    p = PR.pose(flows, motion, Kv)
    want = RR.refine(flows, p["rotation"], p["translation"], Kv, None, 3)
    rot = np.where(want["ok"][:, None, None], want["rotation"], p["rotation"])
    tra = np.where(want["ok"][:, None], want["translation"], p["translation"])
    print(f"pose refine cli: ok {ok.tolist()} refine ok {want['ok'].tolist()} rows {rows.tolist()}")
    assert _eq(closed[:, :, :3], p["rotation"]) and _eq(closed[:, :, 3], p["translation"]) and np.array_equal(ok, p["ok"])
    assert _eq(pose[:, :, :3], rot) and _eq(pose[:, :, 3], tra)
    assert np.array_equal(rows[:, 0], want["samples"]) and np.array_equal(rows[:, 1], want["best_pass"])
    assert _eq(rows[:, 2], want["cost"][:, 0]) and _eq(rows[:, 3], want["cost"][np.arange(3), want["best_pass"]])
    assert (rows[:, 3] <= rows[:, 2]).all()
