"""Pose refinement on the CPU: the numpy restatement of csrc/pwc_pose_refine.hip (tests/pose_refine_ref.py) against the test scene's
own rotation, translation and depth map, its properties by construction, its degenerate cases, the tangent basis, the 5 x 5
elimination against numpy.linalg.solve; the header / SIGNATURES / SOURCES / __all__ surface, argument errors and the CLI's
parsing.  tests/test_gpu_pose_refine.py holds the kernels to the restatement bit for bit.

Why the feature is worth having: on the scene of tests/test_host_pose.py (the block, 0.02 px of noise, iters = 4 upstream) the
closed form's rotation, translation direction and median relative depth error of the known static pixels are that file's MEASURED
table; refine_pose at iters = 6 has to bring EACH to one quarter of it or less.  The restatement's own figures (they move with the
last bits of the upstream Jacobi route and with nothing else; each is also asserted at twice the measured value):

    shape      rotation error            translation error         median relative depth error   maximum      best pass
    48 x 64    0.1933 -> 0.002368 deg    0.8220 -> 0.004856 deg    0.03004 -> 0.002302           0.02772      2
    64 x 96    0.1101 -> 0.001669 deg    0.2584 -> 0.005014 deg    0.01762 -> 0.001551           0.01915      2
    40 x 136   0.4787 -> 0.008180 deg    0.3313 -> 0.040044 deg    0.06691 -> 0.001338           0.01536      5

The smallest gain is the translation at 40 x 136, 8.3 times.  Reported, not asserted: at 0.1 px of noise the gain is about two and
not uniform (64 x 96: translation 0.209 -> 0.241 deg); with threshold = inf on the block scene the block pulls the fit away.
Bounds that are reasoning: the exact flow gives the pose back within 1e-4 degrees (camera_pose's own bound there); R^T R - I and
|t| - 1 within 1e-12 after 64 passes (each pass multiplies by a Cayley matrix that is orthogonal to a few 1e-16 and renormalises
t); the tangent basis orthonormal within 1e-14 (a dozen double operations on values of size 1, the given t itself a unit vector
only to an ulp); the elimination against numpy.linalg.solve within 1e-10 of the largest entry of the solution (the systems'
condition numbers are below 1e5 on these scenes, times 2.2e-16)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fundamental_ref as FR
from tests import pose_ref as PR
from tests import pose_refine_ref as RR
from tests.test_host_pose import MEASURED as CLOSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ((48, 64), (64, 96), (40, 136))
# (rotation deg, translation deg, median, maximum relative depth error) at iters = 6: the module's docstring
MEASURED = {(48, 64): (0.002368, 0.004856, 0.002302, 0.02772), (64, 96): (0.001669, 0.005014, 0.001551, 0.01915),
            (40, 136): (0.008180, 0.040044, 0.001338, 0.01536)}
_CACHE = {}


def _closed(H, W, block=True, noise=0.02, translation=FR.TRANSLATION):
    """(flow (1,H,W,2), the block's mask, K, the closed-form pose dict, inlier) of the scene, computed once and left unchanged."""
    key = (H, W, block, noise, translation)
    if key not in _CACHE:
        flow, rect = FR.scene(H, W, 0, block, noise, translation)
        K = PR.scene_intrinsics(H, W)
        fit = FR.fit(flow[None], None, 4, 1.0)
        inl = FR.residual(flow[None], fit["matrices"], None, 1.0)[1]
        p = PR.pose(flow[None], fit["matrices"], K, None, 1.0)
        for a in (p["rotation"], p["translation"], inl):
            a.setflags(write=False)
        _CACHE[key] = (flow[None], rect, K, p, inl)
    return _CACHE[key]


def _figures(H, W, rect, flow, K, rotation, translation, inl):
    dep, kn, _ = PR.depth(flow, rotation, translation, K, inl, 0.25)
    rel = np.abs(dep[0] / PR.scene_depth(H, W) - 1.0)[~rect & kn[0]]
    return (PR.rotation_error(rotation[0], PR.scene_rotation()), PR.direction_error(translation[0], PR.scene_translation()),
            float(np.median(rel)), float(rel.max()))


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_refinement_brings_every_error_to_a_quarter_of_the_closed_form(shape):
    """The module's docstring: each figure at most one quarter of the closed form's MEASURED one, and at most twice its own."""
    H, W = shape
    flow, rect, K, p, inl = _closed(H, W)
    ref = RR.refine(flow, p["rotation"], p["translation"], K, None, 6, 1.0, 1.0)
    before = _figures(H, W, rect, flow, K, p["rotation"], p["translation"], inl)
    after = _figures(H, W, rect, flow, K, ref["rotation"], ref["translation"], inl)
    print(f"pose refine figures {H}x{W}: rotation {before[0]:.4f} -> {after[0]:.6f} deg, translation {before[1]:.4f} -> {after[1]:.6f} deg, "
          f"relative depth error median {before[2]:.5f} -> {after[2]:.6f} max {before[3]:.5f} -> {after[3]:.5f}, samples {int(ref['samples'][0])}, "
          f"best pass {int(ref['best_pass'][0])}, cost {ref['cost'][0].tolist()}")
    assert ref["ok"][0] and ref["frozen"][0] == -1
    for j in range(3):
        assert after[j] <= CLOSED[shape][j] / 4.0, (j, after[j], CLOSED[shape][j])
    for j in range(4):
        assert after[j] <= 2 * MEASURED[shape][j], (j, after[j], MEASURED[shape][j])
    # the chained restatement uses the same pose
    dep, kn, pose, _, ref2, _ = RR.flow_depth(flow, K, None, 4, 1.0, 1.0, 0.25, 6)
    assert np.array_equal(pose[0], ref["rotation"]) and np.array_equal(pose[1], ref["translation"]) and ref2["ok"][0]


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_figures_at_a_tenth_of_a_pixel_of_noise_are_reported(shape):
    H, W = shape
    flow, rect, K, p, inl = _closed(H, W, True, 0.1)
    ref = RR.refine(flow, p["rotation"], p["translation"], K, None, 6, 1.0, 1.0)
    before = _figures(H, W, rect, flow, K, p["rotation"], p["translation"], inl)
    after = _figures(H, W, rect, flow, K, ref["rotation"], ref["translation"], inl)
    print(f"pose refine figures {H}x{W} at 0.1 px (reported only): rotation {before[0]:.4f} -> {after[0]:.4f} deg, translation {before[1]:.4f} -> "
          f"{after[1]:.4f} deg, median {before[2]:.5f} -> {after[2]:.5f}, max {before[3]:.5f} -> {after[3]:.5f}, best pass {int(ref['best_pass'][0])}")
    assert ref["ok"][0] and ref["cost"][0, ref["best_pass"][0]] <= ref["cost"][0, 0]


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_flow_stays_at_the_truth(shape):
    H, W = shape
    flow, rect, K, p, inl = _closed(H, W, False, 0.0)
    ref = RR.refine(flow, p["rotation"], p["translation"], K, None, 6, 1.0, 1.0)
    rot, tra = PR.rotation_error(ref["rotation"][0], PR.scene_rotation()), PR.direction_error(ref["translation"][0], PR.scene_translation())
    print(f"pose refine exact {H}x{W}: rotation {rot:.3e} deg, translation {tra:.3e} deg, best pass {int(ref['best_pass'][0])}, "
          f"cost {ref['cost'][0].tolist()}")
    assert ref["ok"][0] and ref["samples"][0] == H * W and rot <= 1e-4 and tra <= 1e-4


@pytest.mark.parametrize("shape", SCENES + ((17, 19),), ids=lambda s: f"{s[0]}x{s[1]}")
def test_properties_by_construction(shape):
    H, W = shape
    flow, rect, K, p, inl = _closed(H, W)
    assert p["ok"][0]
    zero = RR.refine(flow, p["rotation"], p["translation"], K, None, 0, 1.0, 1.0)
    assert zero["rotation"].tobytes() == p["rotation"].tobytes() and zero["translation"].tobytes() == p["translation"].tobytes()
    assert zero["ok"][0] and zero["best_pass"][0] == 0 and zero["cost"].shape == (1, 1) and zero["cost"][0, 0] > 0.0
    for thr in (1.0, np.inf):
        for iters in (1, 6):
            ref = RR.refine(flow, p["rotation"], p["translation"], K, None, iters, 1.0, thr)
            assert ref["cost"][0, 0] == RR.refine(flow, p["rotation"], p["translation"], K, None, 0, 1.0, thr)["cost"][0, 0]
            assert ref["cost"][0, ref["best_pass"][0]] <= ref["cost"][0, 0], (thr, iters)
            assert ref["cost"][0, ref["best_pass"][0]] == ref["cost"][0].min()
    long = RR.refine(flow, p["rotation"], p["translation"], K, None, 64, 1.0, 1.0)
    # the pose in work after 64 passes is not an output; the best one is, and both went through the same updates: run the updates
    R, t = [np.float64(q) for q in p["rotation"][0].reshape(9)], [np.float64(q) for q in p["translation"][0]]
    for A, rhs, tol in long["systems"][0]:
        x, _ = RR.MR.ldlt(A, [rhs], tol)
        R, t = RR.update(R, t, x[0])
    Rm, tv = np.array(R).reshape(3, 3), np.array(t)
    ortho, unit = np.abs(Rm.T @ Rm - np.eye(3)).max(), abs(np.linalg.norm(tv) - 1.0)
    best = long["rotation"][0]
    print(f"pose refine 64 passes {H}x{W}: steps {len(long['systems'][0])}, |R^T R - I| {ortho:.2e}, ||t| - 1| {unit:.2e}, best pass "
          f"{int(long['best_pass'][0])}, frozen {int(long['frozen'][0])}")
    assert len(long["systems"][0]) == 64 and long["frozen"][0] == -1
    assert ortho <= 1e-12 and unit <= 1e-12 and abs(np.linalg.det(Rm) - 1.0) <= 1e-12
    assert np.abs(best.T @ best - np.eye(3)).max() <= 1e-12 and abs(np.linalg.norm(long["translation"][0]) - 1.0) <= 1e-12


def test_a_bad_start_stays_bad_at_17x19():
    """What it cannot do: the closed form at 17 x 19 is 80 degrees off in translation, and the refinement does not repair it."""
    H, W = 17, 19
    flow, rect, K, p, inl = _closed(H, W)
    ref = RR.refine(flow, p["rotation"], p["translation"], K, None, 6, 1.0, 1.0)
    tra0, tra1 = PR.direction_error(p["translation"][0], PR.scene_translation()), PR.direction_error(ref["translation"][0], PR.scene_translation())
    print(f"pose refine 17x19: translation {tra0:.2f} -> {tra1:.2f} deg, best pass {int(ref['best_pass'][0])}, cost {ref['cost'][0].tolist()}")
    assert tra0 > 45.0 and tra1 > 45.0 and ref["cost"][0, ref["best_pass"][0]] <= ref["cost"][0, 0]


def test_degenerate_images_of_the_restatement():
    H, W = 24, 32
    flow, rect, K, p, inl = _closed(H, W, False, 0.0)
    Rg, tg = p["rotation"], p["translation"]
    good = RR.refine(flow, Rg, tg, K, None, 3)
    assert good["ok"][0] and good["samples"][0] == H * W
    few = np.zeros((1, H, W), bool)
    few[0, 3, 4:8] = True                                                      # four pixels: one short
    five = few.copy()
    five[0, 9, 20] = True
    for tag, f, r, t, k, v, samples in (("zero rotation", flow, np.zeros_like(Rg), tg, K, None, 0), ("fx = 0", flow, Rg, tg, K * [0, 1, 1, 1], None, 0),
                                        ("NaN intrinsic", flow, Rg, tg, K + [0, 0, np.nan, 0], None, 0),
                                        ("nothing known", np.full_like(flow, 1e10), Rg, tg, K, None, 0),
                                        ("valid all zeros", flow, Rg, tg, K, np.zeros((1, H, W), bool), 0), ("four samples", flow, Rg, tg, K, few, 4)):
        ref = RR.refine(f, r, t, k, v, 3)
        assert not ref["ok"][0] and ref["samples"][0] == samples, tag
        for key in ("rotation", "translation", "cost", "weight_sum", "best_pass"):
            assert not ref[key].any(), (tag, key)
    ref = RR.refine(flow, Rg, tg, K, five, 3)
    print(f"pose refine five samples: ok {ref['ok'].tolist()} frozen {ref['frozen'].tolist()} cost {ref['cost'].tolist()}")
    assert ref["ok"][0] and ref["samples"][0] == 5 and ref["cost"][0, ref["best_pass"][0]] <= ref["cost"][0, 0]
    # a line of pixels does not determine five parameters: the pivot fails, the image freezes and keeps the input
    line = np.zeros((1, H, W), bool)
    line[0, 5, 2:10] = True
    noisy = _closed(H, W, False, 0.02)
    ref = RR.refine(noisy[0], noisy[3]["rotation"], noisy[3]["translation"], K, line, 3)
    print(f"pose refine a line of 8 pixels: frozen {ref['frozen'].tolist()} best {ref['best_pass'].tolist()} cost {ref['cost'].tolist()}")
    assert ref["ok"][0] and ref["samples"][0] == 8
    if ref["frozen"][0] >= 0:
        assert not ref["cost"][0, ref["frozen"][0] + 1:].any()


def test_a_pure_rotation_gives_ok_false_and_zeros():
    H, W = 48, 64
    flow = FR.scene(H, W, 0, False, 0.0, (0.0, 0.0, 0.0))[0][None]
    K = PR.scene_intrinsics(H, W)
    dep, kn, pose, p, ref, inl = RR.flow_depth(flow, K, None, 4, 1.0, 1.0, 0.25, 4)
    assert not p["ok"][0] and not p["rotation"].any()
    assert not ref["ok"][0] and ref["samples"][0] == 0
    for key in ("rotation", "translation", "cost", "weight_sum", "best_pass"):
        assert not ref[key].any(), key
    assert not pose[0].any() and not pose[1].any() and not kn.any() and (dep == PR.SENTINEL).all()


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_without_the_gate_the_block_takes_part(shape):
    """threshold = inf on the block scene: every known pixel is in the set.  Recorded, not asserted to improve."""
    H, W = shape
    flow, rect, K, p, inl = _closed(H, W)
    ref = RR.refine(flow, p["rotation"], p["translation"], K, None, 6, 1.0, np.inf)
    gated = RR.refine(flow, p["rotation"], p["translation"], K, None, 6, 1.0, 1.0)
    before = _figures(H, W, rect, flow, K, p["rotation"], p["translation"], inl)
    after = _figures(H, W, rect, flow, K, ref["rotation"], ref["translation"], inl)
    print(f"pose refine no gate {H}x{W} (recorded only): rotation {before[0]:.4f} -> {after[0]:.4f} deg, translation {before[1]:.4f} -> {after[1]:.4f} "
          f"deg, samples {int(ref['samples'][0])} against {int(gated['samples'][0])} gated")
    assert ref["samples"][0] == H * W and ref["inset"][0][rect].all()
    assert gated["samples"][0] == int((~rect).sum()) and not gated["inset"][0][rect].any()      # the gate keeps the block out
    assert ref["ok"][0] and ref["cost"][0, ref["best_pass"][0]] <= ref["cost"][0, 0]


def test_the_tangent_basis_is_orthonormal():
    s = np.sqrt(0.5)
    cases = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 0.0), (s, s, 0.0), (s, 0.0, s), (0.0, s, -s),
             tuple(np.full(3, np.sqrt(1.0 / 3.0))), tuple(PR.scene_translation()), (0.6, -0.8, 0.0)]
    for t in cases:
        b1, b2 = RR.basis(t)
        M = np.array([t, b1, b2], np.float64)
        assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-14, t
        assert abs(np.linalg.det(M) - 1.0) <= 1e-14, t                            # t, b1, b2 right-handed
    # the index rule: the smallest entry in magnitude, ties to the lowest index
    assert RR.basis((1.0, 0.0, 0.0))[0][1] == 0.0 and RR.basis((1.0, 0.0, 0.0))[0][2] == -1.0      # entries 1 and 2 tie: index 1
    assert RR.basis((0.0, 0.0, 1.0))[0][0] == 0.0 and RR.basis((s, s, 0.0))[0][2] == 0.0
    third = np.sqrt(1.0 / 3.0)
    assert RR.basis((third, third, third))[0][0] == 0.0                         # a three-way tie: index 0


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_elimination_against_numpy_solve(shape):
    H, W = shape
    flow, rect, K, p, inl = _closed(H, W)
    ref = RR.refine(flow, p["rotation"], p["translation"], K, None, 6, 1.0, 1.0)
    worst, cond = 0.0, 0.0
    for A, rhs, tol in ref["systems"][0]:
        L = np.array(A, np.float64)
        full = L + L.T - np.diag(np.diag(L))
        x, d = RR.MR.ldlt(A, [rhs], tol)
        want = np.linalg.solve(full, np.array(rhs, np.float64))
        worst = max(worst, float(np.abs(np.array(x[0]) - want).max() / np.abs(want).max()))
        cond = max(cond, float(np.linalg.cond(full)))
        assert all(q > tol for q in d)
    print(f"pose refine elimination {H}x{W}: {len(ref['systems'][0])} systems, relative difference {worst:.2e}, condition {cond:.2e}")
    assert len(ref["systems"][0]) == 6 and worst <= 1e-10


def test_the_surface_header_signatures_sources_and_all():
    import pwcnet_amd
    from pwcnet_amd import _lib, pose, pose_refine, trajectory
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert "pose refinement" in header and "EPIPOLAR" in header and "BASIS" in header and "Cayley" in header
    for name in ("pwc_pose_refine_workspace_bytes", "pwc_pose_refine_f64"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    decl = re.search(r"int pwc_pose_refine_f64\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["pwc_pose_refine_f64"][1]) == 22
    assert "pwc_pose_refine.hip" in _lib.SOURCES and "two_view.h" in _lib.HEADERS and "motion_ldlt.h" in _lib.HEADERS
    source = open(os.path.join(_lib.CSRC, "pwc_pose_refine.hip")).read()
    assert '#include "two_view.h"' in source and "#pragma clang fp contract(off)" in source and "motion_ldlt<5, 1>" in source
    assert "fma" not in source and "atomic" not in source.replace("No atomic", "")
    shared = open(os.path.join(_lib.CSRC, "two_view.h")).read()
    for f in ("two_view.h", "robust_fit.h", "flow_record.h"):              # the project headers its numerics come from
        text = open(os.path.join(_lib.CSRC, f)).read()
        assert f in _lib.HEADERS and "#pragma clang fp contract(off)" in text and "fma" not in text and "atomic" not in text
    assert '#include "robust_fit.h"' in source and "pwc_fit_write_part<REFINE_SUMS>" in source and "pwc_fit_gather<REFINE_SUMS>" in source
    assert "two_view_epipolar" in shared and "two_view_tangent_basis" in shared and "two_view_epipolar" in source
    L = _lib.lib()
    assert L.pwc_pose_refine_workspace_bytes(3, 48, 64) == 8 * (3 * 12 * 22 + 3 * 19) + 4 * 3 * 12
    assert L.pwc_pose_refine_workspace_bytes(1, 17, 19) == 8 * (2 * 22 + 19) + 8
    assert L.pwc_pose_refine_workspace_bytes(0, 8, 8) == 0 and L.pwc_pose_refine_workspace_bytes(65536, 8, 8) == 0
    assert "refine_pose" in pwcnet_amd.__all__ and "pose_refine" in pwcnet_amd.__all__ and pwcnet_amd.refine_pose is pose_refine.refine_pose
    doc = pose_refine.refine_pose.__doc__
    for word in ("scale", "threshold", "iters", "pivot", "Jacobian", "tuned", "only rotates", "BASELINES", "No autograd"):
        assert word in doc, word
    words = " ".join(pose_refine.__doc__.split())
    assert "bundle adjustment" in words and "bad start" in words
    import inspect
    assert inspect.signature(pose.flow_depth).parameters["refine"].default == 0
    assert inspect.signature(trajectory.flow_trajectory).parameters["refine"].default == 0
    assert "refine_pose" in pose.flow_depth.__doc__ and "closed_rotation" in pose.flow_depth.__doc__


def test_the_entry_point_refuses_before_any_launch():
    """Null pointers, sizes, iters, scale, threshold, the channel stride, the range, the alignment and the workspace: every row fails
    a check, so nothing is launched and no GPU is needed."""
    import ctypes
    from pwcnet_amd import _lib
    L = _lib.lib()
    al, mis, mis2 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    need = L.pwc_pose_refine_workspace_bytes(1, 8, 8)
    def call(flows=al, cs=2, K=al, R0=al, t0=al, N=1, H=8, W=8, iters=4, scale=1.0, thr=1.0, ws=al, wsb=need, rot=al, tra=al, ok=al, samples=al,
             best=al, cost=al, wsum=al):
        return L.pwc_pose_refine_f64(flows, cs, None, K, R0, t0, N, H, W, iters, scale, thr, ws, wsb, rot, tra, ok, samples, best, cost, wsum, None)
    for bad in (dict(flows=None), dict(K=None), dict(R0=None), dict(t0=None), dict(ws=None), dict(rot=None), dict(tra=None), dict(ok=None),
                dict(samples=None), dict(best=None), dict(cost=None), dict(wsum=None), dict(N=0), dict(H=0), dict(W=-1), dict(iters=-1),
                dict(iters=65), dict(scale=0.0), dict(scale=float("nan")), dict(thr=-1.0), dict(thr=float("nan")), dict(cs=1),
                dict(wsb=need - 1), dict(N=2)):
        assert call(**bad) == -1, bad
    for bad in (dict(flows=mis2), dict(K=mis), dict(R0=mis), dict(t0=mis), dict(ws=mis), dict(rot=mis), dict(tra=mis), dict(samples=mis2),
                dict(best=mis2), dict(cost=mis), dict(wsum=mis)):
        assert call(**bad) == -2, bad
    assert call(H=65536, W=65536) == -3 and call(N=65536, wsb=1 << 40) == -3


def test_argument_errors():
    import torch
    import pwcnet_amd
    flows = torch.zeros((2, 4, 4, 2))
    rot = torch.eye(3, dtype=torch.float64)[None].repeat(2, 1, 1)
    tra = torch.zeros((2, 3), dtype=torch.float64)
    K = [4.0, 4.0, 1.5, 1.5]
    with pytest.raises(ValueError):
        pwcnet_amd.refine_pose(flows, rot, tra, K)                             # on the CPU: the GPU only
    for kw in (dict(iters=-1), dict(iters=65), dict(iters=1.5), dict(iters=True), dict(scale=0.0), dict(scale=float("nan")),
               dict(threshold=-1.0), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            pwcnet_amd.refine_pose(flows, rot, tra, K, **kw)
    with pytest.raises(TypeError):
        pwcnet_amd.refine_pose(flows.double(), rot, tra, K)
    with pytest.raises(TypeError):
        pwcnet_amd.refine_pose(flows, rot.float(), tra, K)
    with pytest.raises(TypeError):
        pwcnet_amd.refine_pose(flows, rot, tra.float(), K)
    with pytest.raises(ValueError):
        pwcnet_amd.refine_pose(flows, rot[:1], tra, K)
    with pytest.raises(ValueError):
        pwcnet_amd.refine_pose(flows, rot, torch.zeros((2, 4), dtype=torch.float64), K)
    with pytest.raises(ValueError):
        pwcnet_amd.refine_pose(flows, rot, tra, K, valid=torch.ones((2, 4, 5), dtype=torch.bool))
    with pytest.raises(ValueError):
        pwcnet_amd.refine_pose(flows, rot, tra, [4.0, 4.0, 1.5])
    with pytest.raises(TypeError):
        pwcnet_amd.refine_pose(flows, rot, tra, "fx fy cx cy")
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            pwcnet_amd.flow_depth(flows, K, refine=bad)
        with pytest.raises(ValueError):
            pwcnet_amd.flow_trajectory(flows, K, refine=bad)


def test_cli_refuses_pose_refine_without_intrinsics(tmp_path):
    """--pose_refine needs --intrinsics: an argparse error that says so, before anything touches the GPU or the frames."""
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    K = ["--intrinsics", "64", "64", "31.5", "23.5"]
    for flags, word in ((["--motion", "fundamental", "--pose_refine", "4"], "--pose_refine needs --intrinsics"),
                        (["--pose_refine", "4"], "--pose_refine needs --intrinsics"),
                        (["--motion", "affine", "--pose_refine", "2"] + K, "--intrinsics needs --motion fundamental"),
                        (["--motion", "fundamental", "--pose_refine", "-1"] + K, "--pose_refine must be in 0 .. 64"),
                        (["--motion", "fundamental", "--pose_refine", "65"] + K, "--pose_refine must be in 0 .. 64"),
                        (["--motion", "fundamental", "--pose_refine", "two"] + K, "invalid int value")):
        run = subprocess.run(cli + flags, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stderr[-500:])
    run = subprocess.run(cli + ["--help"], capture_output=True, text=True, timeout=120)
    out = " ".join(run.stdout.split())
    assert run.returncode == 0 and "--pose_refine" in out and "pose_closed.npy" in out and "pose_refine.npy" in out and "refine_pose" in out
