"""Scale chain and camera trajectory on the GPU (pwc_trajectory.hip, pwcnet_amd.trajectory, infer_continuous.py --trajectory) against
the numpy restatement of tests/trajectory_ref.py (checked on the CPU by tests/test_host_trajectory.py).

The per-pixel key is IEEE double + - x / and one rounding to float32 in a fixed order, the selection and the counts are integers,
and the chain is IEEE double + - x in a fixed order; the restatement performs the same operations in the same order.  The
yardstick is BIT EQUALITY, no tolerance; it rests on the device's double division being correctly rounded.  The one test that is
not bit equality is the geometry on the device, held to the host test's bound: the chained scale error and the error of the last
camera centre at most one tenth of what unit scales give (0.5 and 0.109; the restatement's figures are 2.9e-5 and 1.2e-5 at
4 x 48 x 64).  Every case prints its figures before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import trajectory as TJ  # the feature: without it nothing here can be collected
from tests import trajectory_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((3, 48, 64), (2, 40, 136), (4, 17, 19), (2, 64, 520))
_SCENES = {}


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.camera_trajectory is TJ.camera_trajectory and pwcnet_amd.flow_trajectory is TJ.flow_trajectory
    return pwcnet_amd


def _up(a):
    return a if a is None or not isinstance(a, np.ndarray) else torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _scene(P, T, H, W):
    """The sequence scene and what pwcnet_amd.flow_depth makes of its exact flows on the device, computed once, left unchanged:
    dict(flows, K, rotation, translation, depth, known) as numpy arrays."""
    key = (T, H, W)
    if key not in _SCENES:
        s = R.sequence(T, H, W)
        depth, known, rotation, translation, ok, _ = P.flow_depth(_up(s["flows"]), s["K"])
        c = dict(flows=s["flows"], K=s["K"], rotation=rotation.cpu().numpy(), translation=translation.cpu().numpy(),
                 depth=depth.cpu().numpy(), known=known.cpu().numpy(), ok=ok.cpu().numpy())
        for v in c.values():
            v.setflags(write=False)
        _SCENES[key] = c
    return _SCENES[key]


def _call(P, flows, rotation, translation, K, depth, known, min_samples=64, state=None):
    tr, sc, sg, info, state = P.camera_trajectory(_up(flows), _up(rotation), _up(translation), K, _up(depth), _up(known),
                                                  min_samples=min_samples, state=state)
    T = tr.shape[0] - 1
    assert tr.dtype == torch.float64 and tr.shape == (T + 1, 3, 4) and sc.dtype == torch.float64 and sc.shape == (T,)
    assert sg.dtype == torch.int32 and info["ratio"].dtype == torch.float32 and info["samples"].dtype == torch.int32
    assert info["linked"].dtype == torch.bool and info["linked"].shape == (T,)
    got = dict(trajectory=tr.cpu().numpy(), scales=sc.cpu().numpy(), segment=sg.cpu().numpy(), ratio=info["ratio"].cpu().numpy(),
               samples=info["samples"].cpu().numpy(), linked=info["linked"].cpu().numpy())
    return got, state


def _same(tag, got, want):
    diff = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in R.KEYS}
    print(f"trajectory {tag}: ratio {want['ratio'].tolist()} samples {want['samples'].tolist()} linked {want['linked'].astype(int).tolist()} "
          f"scales {want['scales'].tolist()} segment {want['segment'].tolist()} elements that differ {diff}")
    for k in R.KEYS:
        assert _eq(got[k], want[k]), (tag, k)


def _random_maps(T, H, W, seed):
    """Random positive depths over forty octaves and a random known mask: the keys spread over many exponents."""
    rng = np.random.RandomState(seed)
    depth = np.exp2(rng.uniform(-20.0, 20.0, size=(T, H, W))).astype(np.float32)
    return depth, rng.uniform(size=(T, H, W)) > 0.3


def _true_pose(T):
    Rm, t = R.scene_poses(T)
    return Rm, t / np.linalg.norm(t, axis=1, keepdims=True)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_camera_trajectory_equals_the_restatement_bit_for_bit(P, shape):
    T, H, W = shape
    c = _scene(P, T, H, W)
    assert R.MR.parts_of(H, W) == {(48, 64): 12, (40, 136): 22, (17, 19): 2, (64, 520): 130}[(H, W)]
    want, _ = R.trajectory(c["flows"], c["rotation"], c["translation"], c["K"], c["depth"], c["known"])
    got, _ = _call(P, c["flows"], c["rotation"], c["translation"], c["K"], c["depth"], c["known"])
    _same(f"{T}x{H}x{W} scene (pose ok {c['ok'].astype(int).tolist()})", got, want)
    if (H, W) in ((48, 64), (40, 136), (64, 520)):                             # the ratios cluster: the low digits decide
        assert c["ok"].all() and want["linked"][1:].all() and (want["samples"][1:] > 64).all()
        assert np.allclose(want["scales"], R.true_scales(T), rtol=1e-3)
    rot, tra = _true_pose(T)                                                   # keys over many exponents: the top digit decides
    depth, known = _random_maps(T, H, W, H + W)
    want, _ = R.trajectory(c["flows"], rot, tra, c["K"], depth, known, 16)
    got, _ = _call(P, c["flows"], rot, tra, c["K"], depth, known, 16)
    _same(f"{T}x{H}x{W} random depths", got, want)
    assert (want["samples"][1:] > 16).all() and want["linked"][1:].all()
    keys = R.seam_keys(c["flows"][0], rot[0], tra[0], c["K"], known[0], rot[1], depth[1], known[1])
    assert np.unique(keys[keys != 0] >> 21).size > 16


def test_channel_slices_and_an_odd_base_cover_both_load_forms(P):
    """Stride 2 on an 8-byte boundary and channels 2:4 of a 4-channel buffer (one 8-byte load); channels 1:3 of a 3- and a
    4-channel buffer and a dense buffer that starts on an odd 4-byte boundary (two 4-byte loads); the state's flow likewise."""
    T, H, W = 3, 48, 64
    c = _scene(P, T, H, W)
    rest = [_up(c[k]) for k in ("rotation", "translation")] + [c["K"], _up(c["depth"]), _up(c["known"])]
    want, _ = R.trajectory(c["flows"], c["rotation"], c["translation"], c["K"], c["depth"], c["known"])
    views = []
    for width, lo, mod in ((2, 0, 0), (4, 2, 0), (3, 1, 4), (4, 1, 4)):
        buf = torch.full(c["flows"].shape[:3] + (width,), float("nan"), dtype=torch.float32, device="cuda")
        buf[..., lo:lo + 2] = _up(c["flows"])
        views.append((f"stride {width} offset {lo}", buf[..., lo:lo + 2], mod))
    flat = torch.zeros(c["flows"].size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = _up(c["flows"]).reshape(-1)
    views.append(("odd base", flat[1:].view(c["flows"].shape), 4))
    for tag, view, mod in views:
        assert view.data_ptr() % 8 == mod
        got, _ = _call(P, view, *rest)
        _same(tag, got, want)
        _, state = _call(P, view[:1], *[r[:1] if isinstance(r, torch.Tensor) else r for r in rest])     # the state's flow is a view of it
        assert state["flow"].data_ptr() == view[0].data_ptr()
        part, _ = _call(P, view[1:], *[r[1:] if isinstance(r, torch.Tensor) else r for r in rest], state=state)
        for k in R.KEYS[:5]:
            assert _eq(part[k], want[k][1:]), (tag, k)
        assert _eq(part["trajectory"], want["trajectory"][1:]), tag


def test_sentinels_and_valid_holes(P):
    T, H, W = 3, 48, 64
    flows = R.sequence(T, H, W)["flows"].copy()
    K = R.scene_intrinsics(H, W)
    idx = np.argwhere(np.random.RandomState(2).uniform(size=flows.shape[:3]) < 0.03)
    for (n, y, x), bad in zip(idx, [np.nan, np.inf, -np.inf, 1e10, -2e9] * len(idx)):
        flows[n, y, x, (y + x) % 2] = bad
    valid = np.random.RandomState(3).uniform(size=(T, H, W)) > 0.2
    depth, known, rotation, translation, ok, _ = P.flow_depth(_up(flows), K, valid=_up(valid))
    args = [a.cpu().numpy() for a in (rotation, translation)] + [K, depth.cpu().numpy(), known.cpu().numpy()]
    want, _ = R.trajectory(flows, *args)
    got, _ = _call(P, flows, *args)
    _same("sentinels and holes", got, want)
    assert ok.all() and 0 < want["samples"][1] < int(valid[0].sum()) and want["linked"][1:].all()
    depth, known = _random_maps(T, H, W, 7)                                    # known where the flow is a sentinel: it is no sample
    want, _ = R.trajectory(flows, args[0], args[1], K, depth, known, 16)
    got, _ = _call(P, flows, args[0], args[1], K, depth, known, 16)
    _same("sentinels under a random known", got, want)


def test_segments_and_thin_seams(P):
    """A pair without a pose in the middle; seams with fewer than min_samples samples, exactly one, none, an even number; all keys
    equal; T = 1."""
    T, H, W = 4, 48, 64
    c = _scene(P, T, H, W)
    rot, tra, known = c["rotation"].copy(), c["translation"].copy(), c["known"].copy()
    rot[1], tra[1], known[1] = 0.0, 0.0, False
    want, _ = R.trajectory(c["flows"], rot, tra, c["K"], c["depth"], known)
    got, _ = _call(P, c["flows"], rot, tra, c["K"], c["depth"], known)
    _same("an all-zero rotation in the middle", got, want)
    assert got["segment"].tolist() == [0, -1, 1, 1] and got["scales"][1] == 0.0 and got["scales"][0] == 1.0 and got["scales"][2] == 1.0
    assert got["linked"].tolist() == [False, False, False, True] and got["samples"][1] == 0 and got["samples"][2] == 0
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    assert np.array_equal(got["trajectory"][0], eye) and np.array_equal(got["trajectory"][2], eye)
    depth, _ = _random_maps(T, H, W, 11)                                       # distinct ratios: the rank matters
    for tag, keep, samples, linked in (("fewer than min_samples", 40, 40, False), ("exactly one sample", 1, 1, False),
                                       ("no sample", 0, 0, False), ("an even number", 6, 6, False), ("enough", 64, 64, True)):
        known = np.ones((T, H, W), bool)
        known[0] = False
        for i in range(keep):                                                  # rows of eight pixels in the middle of the frame
            known[0, 20 + i // 8, 24 + i % 8] = True
        want, _ = R.trajectory(c["flows"], c["rotation"], c["translation"], c["K"], depth, known)
        got, _ = _call(P, c["flows"], c["rotation"], c["translation"], c["K"], depth, known)
        _same(tag, got, want)
        assert got["samples"][1] == samples and bool(got["linked"][1]) == linked, tag
        assert got["segment"].tolist() == ([0, 0, 0, 0] if linked else [0, 1, 1, 1]), tag
        keys = R.seam_keys(c["flows"][0], c["rotation"][0], c["translation"][0], c["K"], known[0], c["rotation"][1], depth[1], known[1])
        v = np.sort(keys[keys != 0].view(np.float32))
        assert v.size == keep and np.unique(v).size == keep
        assert got["ratio"][1] == (v[(keep - 1) // 2] if keep else 0.0), tag  # even: the LOWER of the two middle values
        if keep == 6:
            assert got["ratio"][1] == v[2] < v[3]
    # all keys equal: a sideways camera over a plane -- every pixel's Z1 is 64 / 4 = 16 up to rounding, the next map says 8
    flows = np.zeros((2, H, W, 2), np.float32)
    flows[..., 0] = 4.0
    rot, tra = np.stack([np.eye(3)] * 2), np.array([[1.0, 0.0, 0.0]] * 2)
    depth, known = np.full((2, H, W), 8.0, np.float32), np.ones((2, H, W), bool)
    want, _ = R.trajectory(flows, rot, tra, c["K"], depth, known)
    got, _ = _call(P, flows, rot, tra, c["K"], depth, known)
    _same("all keys equal", got, want)
    keys = R.seam_keys(flows[0], rot[0], tra[0], c["K"], known[0], rot[1], depth[1], known[1])
    assert np.unique(keys[keys != 0]).size == 1 and got["ratio"][1] == 2.0 and got["samples"][1] == H * (W - 4) and got["scales"][1] == 2.0
    want, _ = R.trajectory(c["flows"][:1], c["rotation"][:1], c["translation"][:1], c["K"], c["depth"][:1], c["known"][:1])
    got, _ = _call(P, c["flows"][:1], c["rotation"][:1], c["translation"][:1], c["K"], c["depth"][:1], c["known"][:1])
    _same("T = 1", got, want)
    assert got["ratio"].tolist() == [0.0] and got["samples"].tolist() == [0] and got["scales"].tolist() == [1.0]
    assert _eq(got["trajectory"][1], np.concatenate([c["rotation"][0], c["translation"][0][:, None]], axis=1))


def test_two_calls_and_batches_of_any_size(P):
    T, H, W = 4, 48, 64
    c = _scene(P, T, H, W)
    rot, tra, known = c["rotation"].copy(), c["translation"].copy(), c["known"].copy()
    for tag in ("whole", "broken at pair 2"):
        if tag != "whole":
            rot[2], tra[2], known[2] = 0.0, 0.0, False
        args = (c["flows"], rot, tra, np.tile(c["K"], (T, 1)), c["depth"], known)
        a, _ = _call(P, *args)
        b, _ = _call(P, *args)
        _same(f"two calls, {tag}", a, b)
        _same(f"one call, {tag}", a, R.trajectory(*args)[0])
        for batch in (1, 2, 3):
            _same(f"the restatement in batches of {batch}, {tag}", R.streamed(*args, batch), a)
            got = {k: [] for k in R.KEYS[:5]}
            rows, state = np.zeros((T + 1, 3, 4)), None
            for i in range(0, T, batch):
                part, state = _call(P, *[x[i:i + batch] for x in args], state=state)
                for k in got:
                    got[k].append(part[k])
                rows[i:i + part["trajectory"].shape[0]] = part["trajectory"]
            got = {k: np.concatenate(v) for k, v in got.items()}
            _same(f"batches of {batch}, {tag}", dict(got, trajectory=rows), a)


def test_flow_trajectory_equals_the_calls_chained_by_hand(P):
    T, H, W = 3, 48, 64
    flows, K = _up(R.sequence(T, H, W)["flows"]), R.scene_intrinsics(H, W)
    valid = _up(np.random.RandomState(3).uniform(size=(T, H, W)) > 0.1)
    kw = dict(valid=valid, iters=3, scale=0.8, threshold=0.7, min_parallax=0.5)
    depth, known, tr, sc, sg, info, state = P.flow_trajectory(flows, K, min_samples=100, **kw)
    d, kn, rotation, translation, ok, dinfo = P.flow_depth(flows, K, **kw)
    tr2, sc2, sg2, info2, _ = P.camera_trajectory(flows, rotation, translation, K, d, kn, min_samples=100)
    print(f"flow_trajectory: ok {ok.tolist()} scales {sc.tolist()} samples {info['samples'].tolist()}")
    assert torch.equal(depth.view(torch.int32), d.view(torch.int32)) and torch.equal(known, kn) and bool(ok.all())
    assert torch.equal(tr.view(torch.int64), tr2.view(torch.int64)) and torch.equal(sc.view(torch.int64), sc2.view(torch.int64))
    assert torch.equal(sg, sg2) and all(torch.equal(info[k], info2[k]) for k in ("samples", "linked"))
    assert torch.equal(info["ratio"].view(torch.int32), info2["ratio"].view(torch.int32)) and bool(info["linked"][1:].all())
    assert torch.equal(info["rotation"], rotation) and torch.equal(info["ok"], ok) and torch.equal(info["inlier"], dinfo["inlier"])
    assert sorted(state) == sorted(TJ._STATE)


def test_geometry_on_the_device(P):
    """Not bit equality: the scene's scales and last camera centre come back within the host test's bound."""
    T, H, W = 4, 48, 64
    s = R.sequence(T, H, W)
    _, _, tr, sc, sg, info, _ = P.flow_trajectory(_up(s["flows"]), s["K"])
    scale, centre = R.scale_error(sc.cpu().numpy(), T), R.centre_error(tr[T].cpu().numpy(), T)
    unit_scale, unit_centre = R.scale_error(np.ones(T), T), R.unit_centre_error(T)
    print(f"trajectory geometry {T}x{H}x{W}: scale error {scale:.3e} (unit scales {unit_scale:.3f}), last centre {centre:.3e} "
          f"(unit scales {unit_centre:.3f}), samples {info['samples'].tolist()}")
    assert sg.tolist() == [0] * T and unit_scale >= 0.33
    assert scale <= 0.1 * unit_scale and centre <= 0.1 * unit_centre


def test_infer_continuous_trajectory_cli(P, tmp_path):
    """The CLI in fresh child processes, each with its own time limit: four 64 x 128 frames, a random texture carried along the
    scene's flow, un-learned weights, batches of two pairs, so the chain crosses a batch boundary.  --trajectory writes the four
    files with the values of the ops chained by hand over the .flo files; without the flag the command writes the files it wrote
    before with identical bytes; the flag without --intrinsics is refused before any GPU work."""
    from PIL import Image
    from pwcnet_amd import flow_io
    H, W = 64, 128
    base = np.random.RandomState(5).uniform(0, 255, size=(H, W, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    flow = R.sequence(1, H, W)["flows"][0]
    y, x = np.mgrid[0:H, 0:W]
    for i in range(4):                                                          # frame i: the texture moved i steps along the flow
        ys = np.clip(np.rint(y - i * flow[..., 1]), 0, H - 1).astype(int)
        xs = np.clip(np.rint(x - i * flow[..., 0]), 0, W - 1).astype(int)
        Image.fromarray(base[ys, xs]).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2",
           "--motion", "fundamental"]
    K = ["--intrinsics", str(W), str(W), str((W - 1) / 2.0), str((H - 1) / 2.0)]
    run = subprocess.run(cli + ["--out", str(tmp_path / "refused"), "--trajectory"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and "--trajectory needs" in run.stderr and not (tmp_path / "refused").exists(), run.stderr[-500:]
    tops = {}
    for tag, flags in (("old", []), ("new", ["--trajectory", "--trajectory_min_samples", "32"])):
        tops[tag] = tmp_path / tag
        run = subprocess.run(cli + ["--out", str(tops[tag])] + K + ["--depth"] + flags, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]

    def files(top):
        return sorted(os.path.relpath(os.path.join(d, f), top) for d, _, fs in os.walk(top) for f in fs)
    old, new = files(tops["old"]), files(tops["new"])
    extra = sorted(set(new) - set(old))
    print(f"trajectory cli: {len(old)} files without the flag, {len(new)} with: {extra}")
    assert set(old) <= set(new) and "pose.npy" in old and "seq/frame_00_depth.npy" in old
    for f in old:                                                               # what was written before: identical bytes
        assert open(tops["old"] / f, "rb").read() == open(tops["new"] / f, "rb").read(), f
    assert extra == ["scale.npy", "scale_links.npy", "segment.npy", "trajectory.npy"]
    flows = np.stack([flow_io.read_flo(str(tops["new"] / "seq" / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)])
    Kv = [float(k) for k in K[1:]]
    depth, known, tr, sc, sg, info, _ = P.flow_trajectory(_up(flows), Kv, min_samples=32)     # one call over the three pairs
    got = {k: np.load(tops["new"] / f"{k}.npy") for k in ("trajectory", "scale", "segment", "scale_links")}
    print(f"trajectory cli: ok {info['ok'].tolist()} scale {got['scale'].tolist()} segment {got['segment'].tolist()} "
          f"links {got['scale_links'].tolist()}")
    assert got["trajectory"].shape == (4, 3, 4) and got["trajectory"].dtype == np.float64 and got["segment"].dtype == np.int32
    assert _eq(got["trajectory"], tr.cpu().numpy()) and _eq(got["scale"], sc.cpu().numpy()) and np.array_equal(got["segment"], sg.cpu().numpy())
    assert got["scale_links"].shape == (3, 2) and got["scale_links"].dtype == np.float64
    assert np.array_equal(got["scale_links"][:, 0], info["ratio"].cpu().numpy().astype(np.float64))
    assert np.array_equal(got["scale_links"][:, 1], info["samples"].cpu().numpy().astype(np.float64))
    for i in range(3):                                                          # the --depth files stay in per-pair baselines
        assert _eq(np.load(tops["new"] / "seq" / f"frame_{i:02d}_depth.npy"), depth[i].cpu().numpy())
