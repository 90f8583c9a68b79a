"""The numpy restatement of the scale chain and the camera trajectory (tests/trajectory_ref.py) on the CPU: the selection by digits
against a sort on hand-made key sets, the segment rule on hand-made patterns, orthonormality over the chain, streaming against one
call, the sequence scene's truth, the header / SIGNATURES / SOURCES / __all__ surface, argument errors and the CLI's parsing.
tests/test_gpu_trajectory.py holds the kernels to the restatement bit for bit.

The geometric bound: doing what there was before the chain -- every scale 1 -- is wrong by 0.5 in scale (the baselines are 0.30,
0.45, 0.20, 0.36; |1 / 0.667 - 1|) and by 0.109 of its length in the last camera's centre.  The chained result has to be within
ONE TENTH of each.  Measured on the restatement of flow_depth over the scene's exact flows:
    4 x 48 x 64    scale error 2.9e-5, last centre 1.2e-5
    4 x 40 x 136   scale error 1.5e-5, last centre 6.5e-6
(the bilinear sample of a curved depth map is what is left; the poses are right to 1e-7 degrees, the depths to 2e-7)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import pose_ref as PR
from tests import trajectory_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHAINS = {}


def _keys(values):
    return np.asarray(values, np.float32).view(np.uint32)


def _chained(T, H, W):
    """The scene through the restatements, computed once, left unchanged: (scene, depth, known, pose dict, trajectory dict)."""
    if (T, H, W) not in _CHAINS:
        s = R.sequence(T, H, W)
        _CHAINS[T, H, W] = (s,) + R.flow_trajectory(s["flows"], s["K"])
    return _CHAINS[T, H, W]


def test_the_selection_is_the_lower_median():
    rng = np.random.RandomState(0)
    hand = ([], [3.5], [2.0, 1.0], [1.0, 2.0, 3.0, 4.0], [5.0, 1.0, 3.0], [7.25] * 9, [1.0, 2.0, 2.0, 2.0, 3.0, 9.0],
            [1e-30, 1e30, 1.0, 2.0], [1e-45, 1.0], [3.4028234663852886e38, 1.0, 2.0])
    for values in hand:
        key, n = R.select_key(_keys(values))
        want, m = R.lower_median(values)
        assert n == m == len(values) and key == (_keys([want])[0] if n else 0), values
    assert R.select_key(_keys([1.0, 2.0]))[0] == _keys([1.0])[0]              # even: the LOWER of the two
    assert R.select_key(_keys([1.0, 2.0, 3.0, 4.0]))[0] == _keys([2.0])[0]
    assert R.select_key(_keys([1.0, 2.0, 2.0, 2.0, 3.0, 9.0]))[0] == _keys([2.0])[0]        # ties at the median
    assert R.select_key(np.array([0, 0, _keys([4.0])[0], 0], np.uint32)) == (_keys([4.0])[0], 1)   # 0 is no sample
    for n in (1, 2, 7, 64, 1000, 4097):
        for values in (np.exp2(rng.uniform(-60, 60, n)), 1.5 + 1e-6 * rng.uniform(-1, 1, n), np.full(n, 0.75)):
            values = values.astype(np.float32)                                # exponents apart; within a few ulps; all equal
            key, m = R.select_key(_keys(values))
            assert m == n and key == _keys([R.lower_median(values)[0]])[0]


def test_the_segment_rule_on_hand_made_patterns():
    Rz = PR.scene_rotation()
    t = np.array([0.6, 0.0, 0.8])
    def run(ok, samples, ratio, min_samples=64, state=None):
        T = len(ok)
        rot = np.stack([Rz if o else np.zeros((3, 3)) for o in ok])
        tra = np.stack([t if o else np.zeros(3) for o in ok])
        return R.chain(rot, tra, np.asarray(ratio, np.float32), np.asarray(samples, np.int32), min_samples, state)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    out = run([1, 1, 1, 1], [0, 100, 64, 63], [0, 2.0, 0.25, 3.0])
    assert out["linked"].tolist() == [False, True, True, False] and out["segment"].tolist() == [0, 0, 0, 1]
    assert out["scales"].tolist() == [1.0, 2.0, 0.5, 1.0] and out["segment_state"].tolist() == [1, 2]
    assert np.array_equal(out["trajectory"][0], eye) and np.array_equal(out["trajectory"][3], eye)      # every segment start
    assert np.array_equal(out["trajectory"][4], np.concatenate([Rz, t[:, None]], axis=1))
    out = run([1, 0, 1, 1, 0, 0, 1], [0, 100, 100, 100, 100, 100, 100], [0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0])
    assert out["segment"].tolist() == [0, -1, 1, 1, -1, -1, 2] and out["scales"].tolist() == [1.0, 0.0, 1.0, 2.0, 0.0, 0.0, 1.0]
    assert out["linked"].tolist() == [False, False, False, True, False, False, False]
    for i in (0, 2, 5, 6):                                                     # starts, and the frame after a pair that is not ok
        assert np.array_equal(out["trajectory"][i], eye), i
    assert not np.array_equal(out["trajectory"][1], eye) and not np.array_equal(out["trajectory"][4], eye)
    for ratio in (0.0, -1.0, np.inf, np.nan):                                  # a ratio that is not usable
        out = run([1, 1], [0, 100], [0, ratio])
        assert out["linked"].tolist() == [False, False] and out["segment"].tolist() == [0, 1] and out["scales"].tolist() == [1.0, 1.0]
    assert run([1, 1], [0, 5], [0, 2.0], min_samples=5)["linked"].tolist() == [False, True]
    out = run([0], [0], [0])
    assert out["segment"].tolist() == [-1] and out["segment_state"].tolist() == [-1, 0] and np.array_equal(out["trajectory"][1], eye)


def test_the_chain_stays_orthonormal_and_composes():
    T = 40
    Rm, t = R.scene_poses(T)
    unit = t / np.linalg.norm(t, axis=1, keepdims=True)
    ratio = np.concatenate([[0.0], R.true_scales(T)[1:] / R.true_scales(T)[:-1]]).astype(np.float32)
    out = R.chain(Rm, unit, ratio, np.full(T, 1000, np.int32))
    A, c = R.scene_cameras(T)
    for i in range(T + 1):
        Ai = out["trajectory"][i, :, :3]
        assert np.abs(Ai @ Ai.T - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(Ai) - 1.0) <= 1e-13
    assert np.abs(out["trajectory"][:, :, :3] - A).max() <= 1e-13
    assert np.abs(out["trajectory"][:, :, 3] - c / R.BASELINES[0]).max() <= 1e-5          # (the ratios are float32)
    assert out["segment"].tolist() == [0] * T and np.allclose(out["scales"], R.true_scales(T), rtol=1e-5)


@pytest.mark.parametrize("shape", [(4, 48, 64), (4, 40, 136)], ids=lambda s: "x".join(map(str, s)))
def test_the_scene_comes_back_within_a_tenth_of_the_unit_scale_error(shape):
    T, H, W = shape
    s, dep, kn, p, out = _chained(T, H, W)
    assert p["ok"].all() and kn.mean() > 0.9
    for j in range(T):                                                         # the scene itself: the poses and depths are exact
        assert PR.rotation_error(p["rotation"][j], s["R"][j]) <= 1e-5
        assert PR.direction_error(p["translation"][j], s["t"][j]) <= 1e-4
        assert np.abs(dep[j][kn[j]] * R.BASELINES[j] / s["depths"][j][kn[j]] - 1.0).max() <= 1e-5
    want = np.array([R.BASELINES[j] / R.BASELINES[j - 1] for j in range(1, T)])
    scale, centre = R.scale_error(out["scales"], T), R.centre_error(out["trajectory"][T], T)
    unit_scale, unit_centre = R.scale_error(np.ones(T), T), R.unit_centre_error(T)
    print(f"trajectory scene {T}x{H}x{W}: ratio {out['ratio'].tolist()} (truth {want.tolist()}) samples {out['samples'].tolist()}, "
          f"scale error {scale:.3e} against {unit_scale:.3f} with unit scales, last centre {centre:.3e} against {unit_centre:.3f}")
    assert out["linked"].tolist() == [False] + [True] * (T - 1) and out["segment"].tolist() == [0] * T
    assert (out["samples"][1:] > 0.5 * H * W).all()
    assert unit_scale >= 0.33 and unit_centre >= 0.05
    assert scale <= 0.1 * unit_scale and centre <= 0.1 * unit_centre
    assert np.abs(out["ratio"][1:] / want - 1.0).max() <= 0.1 * unit_scale
    keys = R.seam_keys(s["flows"][0], p["rotation"][0], p["translation"][0], s["K"], kn[0], p["rotation"][1], dep[1], kn[1])
    v = keys[keys != 0].view(np.float32)
    assert out["ratio"][1] == R.lower_median(v)[0] and out["samples"][1] == v.size     # the digits against a sort


def test_streaming_in_batches_of_one_and_two_equals_one_call():
    T, H, W = 4, 48, 64
    s, dep, kn, p, out = _chained(T, H, W)
    rot, tra, known = p["rotation"].copy(), p["translation"].copy(), kn.copy()
    for tag in ("whole", "broken at pair 2", "thin seam 1"):
        if tag == "broken at pair 2":
            rot[2], tra[2], known[2] = 0.0, 0.0, False
        if tag == "thin seam 1":
            known[0] = False
            known[0, 20:26, 24:32] = True
        one, _ = R.trajectory(s["flows"], rot, tra, s["K"], dep, known)
        for batch in (1, 2, 3):
            got = R.streamed(s["flows"], rot, tra, s["K"], dep, known, batch)
            for k in R.KEYS:
                assert np.array_equal(got[k], one[k]), (tag, batch, k)
    assert one["segment"].tolist() == [0, 1, -1, 2] and one["samples"][1] < 64


def test_the_surface_header_signatures_sources_and_all():
    import pwcnet_amd
    from pwcnet_amd import _lib, trajectory
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert "scale chain and camera trajectory" in header and "WHICH WAY ROUND" in header and "ALL FOUR" in header
    for name in ("pwc_scale_links_workspace_bytes", "pwc_scale_links_f32", "pwc_camera_trajectory_f64"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    decl = re.search(r"int pwc_scale_links_f32\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["pwc_scale_links_f32"][1]) == 21
    decl = re.search(r"int pwc_camera_trajectory_f64\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["pwc_camera_trajectory_f64"][1]) == 16
    assert "pwc_trajectory.hip" in _lib.SOURCES
    source = open(os.path.join(_lib.CSRC, "pwc_trajectory.hip")).read()
    assert "#pragma clang fp contract(off)" in source and "two_view_triangulate" in source and "fma" not in source
    for f in ("two_view.h", "flow_record.h"):                              # the project headers its numerics come from
        text = open(os.path.join(_lib.CSRC, f)).read()
        assert "#pragma clang fp contract(off)" in text and "fma" not in text
    assert "pwc_flow_load2<VEC>" in source and "pwc_flow_known(" in source
    L = _lib.lib()
    assert L.pwc_scale_links_workspace_bytes(3, 8, 8, 0) == 4 * (2 * 5124 + 2 * 64) + 16
    assert L.pwc_scale_links_workspace_bytes(3, 8, 8, 1) == 4 * (3 * 5124 + 3 * 64) + 16
    assert L.pwc_scale_links_workspace_bytes(1, 8, 8, 0) == 16 and L.pwc_scale_links_workspace_bytes(0, 8, 8, 0) == 0
    assert L.pwc_scale_links_workspace_bytes(2, 8192, 8193, 0) == 0 and L.pwc_scale_links_workspace_bytes(65536, 8, 8, 0) == 0
    for name in ("camera_trajectory", "flow_trajectory"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(trajectory, name)
        assert "tuned" in getattr(trajectory, name).__doc__ and "baseline" in getattr(trajectory, name).__doc__.lower()
    doc = trajectory.__doc__
    for word in ("epipolar line", "only rotates", "loop closure", "min_samples = 64", "depth[j] * scales[j]", "Segments"):
        assert word in doc, word
    assert "trajectory" in pwcnet_amd.__all__


def test_entry_points_refuse_before_any_launch():
    """Null pointers, sizes, a previous pair given in part, the range, the alignment and a small workspace: every row fails a
    check, so nothing is launched and no GPU is needed."""
    import ctypes
    from pwcnet_amd import _lib
    L = _lib.lib()
    al, mis, mis2 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    big = 1 << 20
    def links(flows=al, cs=2, rot=al, tra=al, K=al, depth=al, known=al, T=2, H=8, W=8, pf=None, pcs=2, pr=None, pt=None, pk=None, pkn=None,
              ws=al, wsb=big, ratio=al, samples=al):
        return L.pwc_scale_links_f32(flows, cs, rot, tra, K, depth, known, T, H, W, pf, pcs, pr, pt, pk, pkn, ws, wsb, ratio, samples, None)
    def chain(rot=al, tra=al, ratio=al, samples=al, T=2, ms=64, pr=None, prow=None, ps=None, pseg=None, traj=al, scales=al, seg=al, linked=al,
              st=al):
        return L.pwc_camera_trajectory_f64(rot, tra, ratio, samples, T, ms, pr, prow, ps, pseg, traj, scales, seg, linked, st, None)
    for bad in (dict(flows=None), dict(rot=None), dict(tra=None), dict(K=None), dict(depth=None), dict(known=None), dict(ws=None),
                dict(ratio=None), dict(samples=None), dict(T=0), dict(H=0), dict(W=-1), dict(cs=1), dict(wsb=64), dict(pf=al),
                dict(pf=al, pr=al, pt=al, pk=al), dict(pf=al, pr=al, pt=al, pk=al, pkn=al, pcs=1)):
        assert links(**bad) == -1, bad
    for bad in (dict(flows=mis2), dict(depth=mis2), dict(ratio=mis2), dict(samples=mis2), dict(rot=mis), dict(tra=mis), dict(K=mis),
                dict(ws=mis), dict(pf=mis2, pr=al, pt=al, pk=al, pkn=al), dict(pf=al, pr=mis, pt=al, pk=al, pkn=al)):
        assert links(**bad) == -2, bad
    assert links(H=8192, W=8193) == -3 and links(T=65536) == -3
    for bad in (dict(rot=None), dict(tra=None), dict(ratio=None), dict(samples=None), dict(traj=None), dict(scales=None), dict(seg=None),
                dict(linked=None), dict(st=None), dict(T=0), dict(ms=0), dict(pr=al), dict(pr=al, prow=al, ps=al)):
        assert chain(**bad) == -1, bad
    for bad in (dict(rot=mis), dict(tra=mis), dict(traj=mis), dict(scales=mis), dict(ratio=mis2), dict(samples=mis2), dict(seg=mis2),
                dict(st=mis2), dict(pr=al, prow=mis, ps=al, pseg=al)):
        assert chain(**bad) == -2, bad
    assert chain(T=65536) == -3


def test_argument_errors():
    import torch
    import pwcnet_amd
    flows = torch.zeros((2, 4, 4, 2))
    rot = torch.eye(3, dtype=torch.float64)[None].repeat(2, 1, 1)
    tra = torch.zeros((2, 3), dtype=torch.float64)
    depth, known = torch.ones((2, 4, 4)), torch.ones((2, 4, 4), dtype=torch.bool)
    K = [4.0, 4.0, 1.5, 1.5]
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known)         # on the CPU: the GPU only
    with pytest.raises(ValueError):
        pwcnet_amd.flow_trajectory(flows, K)
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError):
            pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known, min_samples=bad)
    with pytest.raises(TypeError):
        pwcnet_amd.camera_trajectory(flows.double(), rot, tra, K, depth, known)
    with pytest.raises(TypeError):
        pwcnet_amd.camera_trajectory(flows, rot.float(), tra, K, depth, known)
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot[:1], tra, K, depth, known)
    with pytest.raises(TypeError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth.double(), known)
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth[:1], known)
    with pytest.raises(TypeError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known.float())
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, torch.ones((2, 4, 5), dtype=torch.bool))
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, [4.0, 4.0, 1.5], depth, known)
    with pytest.raises(TypeError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known, state={"flow": flows[0]})
    with pytest.raises(TypeError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known, state=3)
    state = {"flow": flows[0], "rotation": rot[0], "translation": tra[0], "intrinsics": torch.tensor(K, dtype=torch.float64),
             "depth": depth[0], "known": known[0], "row": torch.zeros((3, 4), dtype=torch.float64),
             "scale": torch.ones(1, dtype=torch.float64), "segment": torch.zeros(2, dtype=torch.int32)}
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known, state=dict(state, flow=torch.zeros((4, 5, 2))))
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known, state=dict(state, row=torch.zeros((4, 4), dtype=torch.float64)))
    with pytest.raises(TypeError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known, state=dict(state, segment=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError):
        pwcnet_amd.camera_trajectory(flows, rot, tra, K, depth, known, state=state)        # every check passes: the device, last of all


def test_cli_refuses_trajectory_without_its_flags(tmp_path):
    """--trajectory needs --motion fundamental --intrinsics: an argparse error that says so, before anything touches the GPU or
    the frames."""
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    for flags, word in ((["--trajectory"], "--trajectory needs --motion fundamental --intrinsics"),
                        (["--motion", "fundamental", "--trajectory"], "--trajectory needs --motion fundamental --intrinsics"),
                        (["--motion", "affine", "--trajectory"], "--trajectory needs"),
                        (["--motion", "fundamental", "--intrinsics", "64", "64", "31.5", "23.5", "--trajectory",
                          "--trajectory_min_samples", "0"], "--trajectory_min_samples")):
        run = subprocess.run(cli + flags, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stderr[-500:])
    run = subprocess.run(cli + ["--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "trajectory.npy" in run.stdout and "scale_links.npy" in run.stdout
