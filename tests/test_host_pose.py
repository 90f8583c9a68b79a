"""The pose path on the CPU: the numpy restatement of the essential-matrix decomposition, the cheirality vote and the depth kernel
(tests/pose_ref.py) against numpy.linalg.svd and the test scene's own rotation, translation and depth map; the header /
SIGNATURES / SOURCES / __all__ surface, argument errors and the CLI's parsing.  tests/test_gpu_pose.py holds the kernels to the
restatement bit for bit.

Bounds that are reasoning: a proper rotation to 1e-12 and [t]x R against the projected E to 1e-9 (a dozen double operations on
values of size 1).  singular[:, 1] = s3 / s1 is the ROOT of an eigenvalue of E^T E: when F is exact that eigenvalue is a few
rounding errors of the largest one, k 2.2e-16 with k up to about 45 for the ten sweeps at size 3, so the ratio is below
sqrt(45 x 2.2e-16) = 1e-7, not 1e-16.
Bounds that are measurements (the restatement's own figures, which move with the last bits of the Jacobi route and with nothing
else; each is asserted at twice the measured value): with the block, 0.02 px of noise and iters = 4,

    shape      rotation error   translation error   median relative depth error   maximum (known static pixels)
    48 x 64       0.1933 deg        0.8220 deg             0.03004                      0.11487
    64 x 96       0.1101 deg        0.2584 deg             0.01762                      0.06930
    40 x 136      0.4787 deg        0.3313 deg             0.06691                      0.19855

and every static pixel is known at min_parallax = 0.25 (the condition asks for 99 %), no block pixel votes, and the winner holds
every voter: 2964 / 2964, 5916 / 5916, 5224 / 5224."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fundamental_ref as FR
from tests import pose_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ((48, 64), (64, 96), (40, 136))
# (rotation deg, translation deg, median, maximum relative depth error): the module's docstring
MEASURED = {(48, 64): (0.1933, 0.8220, 0.03004, 0.11487), (64, 96): (0.1101, 0.2584, 0.01762, 0.06930),
            (40, 136): (0.4787, 0.3313, 0.06691, 0.19855)}


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _exact_F(H, W, translation=FR.TRANSLATION):
    """The scene's fundamental matrix from its own pose: K^-T [t]x R K^-1, Frobenius norm 1."""
    fx, fy, cx, cy = R.scene_intrinsics(H, W)
    Kinv = np.linalg.inv(np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]))
    F = Kinv.T @ _skew(R.scene_translation(translation)) @ R.scene_rotation() @ Kinv
    return F / np.linalg.norm(F)


def _projected(E):
    """The closest essential matrix by numpy.linalg.svd, and its U, V^T with determinant + 1."""
    U, _, Vt = np.linalg.svd(E)
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    return U @ np.diag([1.0, 1.0, 0.0]) @ Vt, U, Vt


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_decomposition_against_svd(shape):
    H, W = shape
    K = R.scene_intrinsics(H, W)
    Wm = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for tag, F in (("exact", _exact_F(H, W)), ("fitted", FR.reference_fit(H, W, 4)["matrices"][0])):
        d = R.decompose(F, K)
        assert d["good"]
        E = np.array(d["essential"]).reshape(3, 3)
        Kmat = np.array([[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]])
        assert np.abs(E - Kmat.T @ F @ Kmat).max() <= 1e-12 * np.abs(E).max()
        Ep, U, Vt = _projected(E)
        textbook = [U @ Wm @ Vt, U @ Wm.T @ Vt]
        worst = dict(ortho=0.0, det=0.0, essential=0.0, textbook=0.0)
        for j, (Rc, t) in enumerate(R.candidates(d)):
            worst["ortho"] = max(worst["ortho"], np.abs(Rc.T @ Rc - np.eye(3)).max())
            worst["det"] = max(worst["det"], abs(np.linalg.det(Rc) - 1.0))
            got = _skew(t) @ Rc
            worst["essential"] = max(worst["essential"], min(np.abs(got - Ep).max(), np.abs(got + Ep).max()))
            worst["textbook"] = max(worst["textbook"], min(np.abs(Rc - T).max() for T in textbook))
            assert abs(np.linalg.norm(t) - 1.0) <= 1e-15
            assert min(np.abs(t - U[:, 2]).max(), np.abs(t + U[:, 2]).max()) <= 1e-9
        cand = R.candidates(d)
        assert np.array_equal(cand[0][0], cand[1][0]) and np.array_equal(cand[2][0], cand[3][0])
        assert np.array_equal(cand[0][1], -cand[1][1]) and np.array_equal(cand[0][1], cand[2][1])
        assert np.abs(cand[0][0] - cand[2][0]).max() > 0.1                     # the two rotations are the two textbook ones
        print(f"pose decomposition {H}x{W} {tag}: {worst}, singular {d['singular']}")
        assert worst["ortho"] <= 1e-12 and worst["det"] <= 1e-12 and worst["essential"] <= 1e-9 and worst["textbook"] <= 1e-9
        if tag == "exact":                                                     # (the docstring: the root of a rounding error)
            assert abs(d["singular"][0] - 1.0) <= 1e-7 and d["singular"][1] <= 1e-7


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_vote_picks_the_pose_the_scene_was_rendered_with(shape):
    H, W = shape
    K = R.scene_intrinsics(H, W)
    winners = {}
    for translation in (FR.TRANSLATION, tuple(-q for q in FR.TRANSLATION)):
        flow = FR.scene(H, W, 0, False, 0.0, translation)[0][None]
        F = FR.fit(flow, None, 4, 1.0)["matrices"]
        p = R.pose(flow, F, K)
        dep, kn, par = R.depth(flow, p["rotation"], p["translation"], K, None, 0.25)
        rot = R.rotation_error(p["rotation"][0], R.scene_rotation())
        tra = R.direction_error(p["translation"][0], R.scene_translation(translation))
        rel = np.abs(dep[0] / R.scene_depth(H, W, translation) - 1.0)
        print(f"pose vote {H}x{W} t {translation}: votes {p['votes'][0].tolist()} of {int(p['voters'][0])}, rotation {rot:.3e} deg, "
              f"translation {tra:.3e} deg, known {kn.mean():.4f}, relative depth error max {rel.max():.3e}, parallax min {par.min():.3f} px")
        assert p["ok"][0] and p["voters"][0] == H * W
        assert p["votes"][0, p["winner"][0]] == H * W and p["votes"][0].sum() == H * W      # all to one, none to the other three
        assert rot <= 1e-4 and tra <= 1e-4 and kn.all() and rel.max() <= 1e-6
        winners[translation] = int(p["winner"][0])
    assert winners[FR.TRANSLATION] != winners[tuple(-q for q in FR.TRANSLATION)], winners


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_block_and_noise_figures_of_the_restatement(shape):
    """The module's docstring: measured with the restatement (not the kernel), asserted at twice the measured value."""
    H, W = shape
    flow, rect = FR.scene(H, W, 0, True, 0.02)
    dep, kn, par, p, fit, inl = R.flow_depth(flow[None], R.scene_intrinsics(H, W), None, 4, 1.0, 1.0, 0.25)
    static = ~rect
    rot = R.rotation_error(p["rotation"][0], R.scene_rotation())
    tra = R.direction_error(p["translation"][0], R.scene_translation())
    rel = np.abs(dep[0] / R.scene_depth(H, W) - 1.0)[static & kn[0]]
    print(f"pose figures {H}x{W}: rotation {rot:.4f} deg, translation {tra:.4f} deg, relative depth error median {np.median(rel):.5f} "
          f"max {rel.max():.5f}, static known {kn[0][static].mean():.4f}, votes {p['votes'][0].tolist()} of {int(p['voters'][0])}, "
          f"block voters {int(p['voting'][0][rect].sum())}, static parallax min {par[0][static].min():.3f} px")
    want = MEASURED[shape]
    assert p["ok"][0] and fit["ok"][0]
    assert rot <= 2 * want[0] and tra <= 2 * want[1] and np.median(rel) <= 2 * want[2] and rel.max() <= 2 * want[3]
    assert not p["voting"][0][rect].any() and not kn[0][rect].any()            # no block pixel votes or gets a depth
    assert kn[0][static].mean() >= 0.99
    assert p["votes"][0, p["winner"][0]] == p["voters"][0] == int(static.sum())


def test_a_pure_rotation_gives_ok_false_and_an_unknown_map():
    H, W = 48, 64
    flow = FR.scene(H, W, 0, False, 0.0, (0.0, 0.0, 0.0))[0][None]
    dep, kn, par, p, fit, inl = R.flow_depth(flow, R.scene_intrinsics(H, W))
    print(f"pose pure rotation: fit ok {fit['ok'].tolist()} eigen {fit['eigen'][0].tolist()}, pose ok {p['ok'].tolist()}")
    assert not fit["ok"][0] and not fit["matrices"].any()
    assert not p["ok"][0] and not p["rotation"].any() and not p["translation"].any() and p["voters"][0] == 0 and not p["votes"].any()
    assert not kn.any() and (dep == R.SENTINEL).all() and not par.any()


def test_degenerate_images_of_the_restatement():
    H, W = 24, 32
    K = R.scene_intrinsics(H, W)
    flow = FR.scene(H, W, 0, False)[0][None]
    F = FR.fit(flow, None, 4, 1.0)["matrices"]
    assert R.pose(flow, F, K)["ok"][0]
    for tag, f, m, k in (("zero F", flow, np.zeros_like(F), K), ("fx = 0", flow, F, K * [0, 1, 1, 1]), ("fy < 0", flow, F, K * [1, -1, 1, 1]),
                         ("NaN intrinsic", flow, F, K + [0, 0, np.nan, 0]), ("Inf intrinsic", flow, F, K + [np.inf, 0, 0, 0]),
                         ("nothing known", np.full_like(flow, 1e10), F, K)):
        p = R.pose(f, m, k)
        assert not p["ok"][0] and not p["rotation"].any() and not p["translation"].any() and p["voters"][0] == 0, tag
        dep, kn, par = R.depth(f, p["rotation"], p["translation"], k)
        assert not kn.any() and (dep == R.SENTINEL).all(), tag
    # an ambiguous vote: half the pixels rendered with the translation negated
    other = FR.scene(H, W, 0, False, 0.0, tuple(-q for q in FR.TRANSLATION))[0]
    mixed = flow.copy()
    mixed[0, :, :W // 2] = other[:, :W // 2]
    p = R.pose(mixed, F, K, threshold=1e9)
    print(f"pose ambiguous: votes {p['votes'][0].tolist()} of {int(p['voters'][0])}")
    assert p["voters"][0] == H * W and 2 * p["votes"][0].max() <= p["voters"][0] and not p["ok"][0] and not p["rotation"].any()
    # good intrinsics with a usable rotation but bad intrinsics at the depth call: the image is off
    good = R.pose(flow, F, K)
    assert not R.depth(flow, good["rotation"], good["translation"], K * [0, 1, 1, 1])[1].any()


def test_raising_min_parallax_only_removes_pixels():
    H, W = 48, 64
    flow, rect = FR.scene(H, W, 0, True, 0.02)
    K = R.scene_intrinsics(H, W)
    _, _, par, p, _, inl = R.flow_depth(flow[None], K)
    before, counts = None, []
    for mp in (0.0, 0.25, 2.0, 3.0, 6.0, 1e3):
        dep, kn, par2 = R.depth(flow[None], p["rotation"], p["translation"], K, inl, mp)
        counts.append(int(kn.sum()))
        assert np.array_equal(par2, R.depth(flow[None], p["rotation"], p["translation"], K, inl, 0.0)[2])      # parallax itself does not move
        assert not (kn & ~inl).any() and (dep[~kn] == R.SENTINEL).all()
        if before is not None:
            assert not (kn & ~before).any()
        before = kn
    print(f"pose min_parallax 0, 0.25, 2, 3, 6, 1000: known {counts}, static parallax min {par[0][~rect].min():.3f} px")
    assert counts[0] == counts[1] == int(inl.sum()) and counts[3] < counts[1] and counts[-1] == 0


def test_the_surface_header_signatures_sources_and_all():
    import pwcnet_amd
    from pwcnet_amd import _lib, pose
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert "relative pose and depth" in header and "TRIANGULATE" in header
    for name in ("pwc_camera_pose_workspace_bytes", "pwc_camera_pose_f64", "pwc_triangulate_depth_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    decl = re.search(r"int pwc_camera_pose_f64\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["pwc_camera_pose_f64"][1]) == 19
    decl = re.search(r"int pwc_triangulate_depth_f32\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["pwc_triangulate_depth_f32"][1]) == 14
    assert "pwc_pose.hip" in _lib.SOURCES and "two_view.h" in _lib.HEADERS
    source = ""
    for f in ("pwc_pose.hip", "two_view.h", "flow_record.h"):
        text = open(os.path.join(_lib.CSRC, f)).read()
        assert "#pragma clang fp contract(off)" in text and "fma" not in text.replace("fmax", ""), f
        source += text
    assert "pwc_flow_known(" in source.split("// two_view.h")[0] and "pwc_flow_load2<VEC>" in source.split("// two_view.h")[0]
    assert "#pragma clang fp contract(off)" in source and "motion_jacobi<3>" in source and "fma" not in source.replace("fmax", "")
    L = _lib.lib()
    assert L.pwc_camera_pose_workspace_bytes(3) == 8 * 22 * 3 and L.pwc_camera_pose_workspace_bytes(0) == 0
    assert L.pwc_camera_pose_workspace_bytes(65536) == 0
    for name in ("camera_pose", "triangulate_depth", "flow_depth"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(pose, name)
        doc = getattr(pose, name).__doc__
        assert "tuned" in doc and "only rotates" in doc and "its own" in doc, name           # untuned, rotation-only, per-pair scale
        assert "baseline" in doc.lower(), name                                                 # the units
    assert "NOT tested" in pose.triangulate_depth.__doc__ and "valid=inlier" in pose.triangulate_depth.__doc__
    assert "half" in pose.camera_pose.__doc__ and "half" in pose.flow_depth.__doc__
    assert "pose" in pwcnet_amd.__all__ and "BASELINES" in pose.__doc__


def test_entry_points_refuse_before_any_launch():
    """Null pointers, sizes, a negative or NaN threshold / min_parallax, the range and the alignment: every row fails a check, so
    nothing is launched and no GPU is needed."""
    import ctypes
    from pwcnet_amd import _lib
    L = _lib.lib()
    al, mis, mis2 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    def pose_call(flows=al, cs=2, F=al, K=al, N=1, H=8, W=8, thr=1.0, ws=al, wsb=8 * 22, rot=al, tra=al, ok=al, votes=al, voters=al, sing=al,
                  ess=al):
        return L.pwc_camera_pose_f64(flows, cs, None, F, K, N, H, W, thr, ws, wsb, rot, tra, ok, votes, voters, sing, ess, None)
    def depth_call(flows=al, cs=2, rot=al, tra=al, K=al, N=1, H=8, W=8, mp=0.25, depth=al, known=al, par=None):
        return L.pwc_triangulate_depth_f32(flows, cs, None, rot, tra, K, N, H, W, mp, depth, known, par, None)
    for bad in (dict(flows=None), dict(F=None), dict(K=None), dict(ws=None), dict(rot=None), dict(votes=None), dict(ess=None), dict(N=0),
                dict(H=0), dict(W=-1), dict(cs=1), dict(thr=-1.0), dict(thr=float("nan")), dict(wsb=8 * 22 - 1), dict(N=2)):
        assert pose_call(**bad) == -1, bad
    for bad in (dict(flows=mis2), dict(F=mis), dict(K=mis), dict(ws=mis), dict(rot=mis), dict(tra=mis), dict(votes=mis2), dict(voters=mis2),
                dict(sing=mis), dict(ess=mis)):
        assert pose_call(**bad) == -2, bad
    assert pose_call(H=65536, W=65536) == -3 and pose_call(N=65536, wsb=1 << 30) == -3
    for bad in (dict(flows=None), dict(rot=None), dict(tra=None), dict(K=None), dict(depth=None), dict(known=None), dict(N=0), dict(H=0),
                dict(cs=1), dict(mp=-0.5), dict(mp=float("nan"))):
        assert depth_call(**bad) == -1, bad
    for bad in (dict(flows=mis2), dict(rot=mis), dict(tra=mis), dict(K=mis), dict(depth=mis2), dict(par=mis2)):
        assert depth_call(**bad) == -2, bad
    assert depth_call(H=65536, W=65536) == -3


def test_argument_errors():
    import torch
    import pwcnet_amd
    flows = torch.zeros((2, 4, 4, 2))
    mats = torch.eye(3, dtype=torch.float64)[None].repeat(2, 1, 1)
    K = [4.0, 4.0, 1.5, 1.5]
    trans = torch.zeros((2, 3), dtype=torch.float64)
    with pytest.raises(ValueError):
        pwcnet_amd.camera_pose(flows, mats, K)                                 # on the CPU: the GPU only
    with pytest.raises(ValueError):
        pwcnet_amd.triangulate_depth(flows, mats, trans, K)
    with pytest.raises(ValueError):
        pwcnet_amd.flow_depth(flows, K)
    for thr in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            pwcnet_amd.camera_pose(flows, mats, K, threshold=thr)
        with pytest.raises(ValueError):
            pwcnet_amd.triangulate_depth(flows, mats, trans, K, min_parallax=thr)
    with pytest.raises(TypeError):
        pwcnet_amd.camera_pose(flows.double(), mats, K)
    with pytest.raises(ValueError):
        pwcnet_amd.camera_pose(torch.zeros((2, 4, 4, 3)), mats, K)
    with pytest.raises(ValueError):
        pwcnet_amd.camera_pose(flows, mats, K, valid=torch.ones((2, 4, 5), dtype=torch.bool))
    with pytest.raises(TypeError):
        pwcnet_amd.camera_pose(flows, mats.float(), K)
    with pytest.raises(ValueError):
        pwcnet_amd.camera_pose(flows, mats[:1], K)
    for bad in ([4.0, 4.0, 1.5], np.zeros((3, 4)), torch.zeros((2, 5)), np.zeros((2, 2, 4))):
        with pytest.raises(ValueError):
            pwcnet_amd.camera_pose(flows, mats, bad)
        with pytest.raises(ValueError):
            pwcnet_amd.triangulate_depth(flows, mats, trans, bad)
    with pytest.raises(TypeError):
        pwcnet_amd.camera_pose(flows, mats, "fx fy cx cy")
    with pytest.raises(TypeError):
        pwcnet_amd.triangulate_depth(flows, mats.float(), trans, K)
    with pytest.raises(TypeError):
        pwcnet_amd.triangulate_depth(flows, mats, trans.float(), K)
    with pytest.raises(ValueError):
        pwcnet_amd.triangulate_depth(flows, mats, torch.zeros((2, 4), dtype=torch.float64), K)
    with pytest.raises(ValueError):
        pwcnet_amd.triangulate_depth(flows, mats[:1], trans, K)


def test_cli_refuses_intrinsics_and_depth_without_their_flags(tmp_path):
    """--intrinsics is valid only with --motion fundamental and --depth needs --intrinsics: an argparse error that says so, before
    anything touches the GPU or the frames."""
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    K = ["--intrinsics", "64", "64", "31.5", "23.5"]
    for flags, word in ((["--motion", "fundamental", "--depth"], "--depth needs --intrinsics"),
                        (["--motion", "affine"] + K, "--intrinsics needs --motion fundamental"),
                        (K, "--intrinsics needs --motion fundamental"),
                        (["--motion", "homography"] + K + ["--depth"], "--intrinsics needs --motion fundamental"),
                        (["--motion", "fundamental"] + K + ["--depth", "--depth_min_parallax", "-1"], "--depth_min_parallax"),
                        (["--motion", "fundamental", "--intrinsics", "64", "64", "31.5"], "expected 4 arguments")):
        run = subprocess.run(cli + flags, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stderr[-500:])
    run = subprocess.run(cli + ["--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "camera_pose" in run.stdout and "pose.npy" in run.stdout and "_depth.png" in run.stdout
    assert "need no scaling" in " ".join(run.stdout.split())


def test_inverse_depth_picture():
    sys.path.insert(0, ROOT)
    try:
        from infer_continuous import inverse_depth_picture
    finally:
        sys.path.remove(ROOT)
    depth = np.array([[2.0, 4.0, 1e10], [8.0, 1e10, 2.0]], np.float32)
    assert inverse_depth_picture(depth).tolist() == [[255, 128, 0], [64, 0, 255]] and inverse_depth_picture(depth).dtype == np.uint8
    assert not inverse_depth_picture(np.full((2, 2), 1e10, np.float32)).any()
