"""The epipolar path on the CPU: the numpy restatement of the fundamental-matrix fit (tests/fundamental_ref.py) against
numpy.linalg.eigh and numpy.linalg.svd on the test scene, the conditions the scene was chosen for, the header / SIGNATURES /
SOURCES / __all__ surface, argument errors and the CLI's parsing.  tests/test_gpu_fundamental.py holds the kernels to the
restatement bit for bit.

Bounds: the restatement's Jacobi eigenvalues agree with numpy.linalg.eigh to 1e-12 of the trace and its F with the one built from
eigh and svd to 1e-9, up to sign (F has Frobenius norm 1).  On the test scene at iters = 4, scale = 1 the static pixels stay
below 0.25 px of Sampson distance (the restatement's own: 0.059 .. 0.076 px), every block pixel is above 1 px (2.46 .. 2.48 px)
and the second eigenvalue is above 1e-5 of the trace (6.0e-5 .. 1.8e-4)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fundamental_ref as R
from tests import homography_ref as HR
from tests import motion_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ((48, 64), (64, 96), (40, 136))


def _independent(flow, F_prev, first, H, W):
    """One pass by an independent route: the weighted rows themselves, numpy.linalg.eigh of their moment matrix, the rank by
    numpy.linalg.svd: (eigenvalues ascending, trace, F^ rank 2 with Frobenius norm as it comes)."""
    known = MR.known_mask(flow[None])[0]
    xh, yh, _, _, s = MR.normalised(H, W)
    xp, yp = xh + flow[..., 0].reshape(-1).astype(np.float64) / s, yh + flow[..., 1].reshape(-1).astype(np.float64) / s
    w = R.pixel_terms(flow, known, F_prev, first, 1.0)[2]
    rows = np.stack([xp * xh, xp * yh, xp, yp * xh, yp * yh, yp, xh, yh, np.ones_like(xh)], axis=1)
    A = (rows * w[:, None]).T @ rows
    lam, vec = np.linalg.eigh(A)
    U, sv, Vt = np.linalg.svd(vec[:, 0].reshape(3, 3))
    return lam, np.trace(A), (U * np.array([sv[0], sv[1], 0.0])) @ Vt


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_pass_equals_eigh_and_svd_on_the_same_weighted_rows(shape):
    H, W = shape
    flow, _ = R.scene(H, W)
    known = MR.known_mask(flow[None])[0]
    F = [0.0] * 9
    for first in (True, False):
        S, cnt = R.image_sums(flow, known, F, first, 1.0)
        A = np.array(R.moment_matrix(S))
        d, V = R.jacobi(A)
        off = np.array(R.jacobi(A)[1])
        lam, tr, want = _independent(flow, F, first, H, W)
        sol, v, eig = R.solve(S, cnt)
        got = np.array(sol).reshape(3, 3)
        err_l = np.abs(np.sort(np.array(d)) - lam).max() / tr
        err_f = min(np.abs(got - want).max(), np.abs(got + want).max())
        ortho = np.abs(off.T @ off - np.eye(9)).max()
        print(f"fundamental eigh {H}x{W} {'pass 0' if first else 'reweighted'}: eigenvalues off by {err_l:.3e} of the trace, F by "
              f"{err_f:.3e}, V^T V - I {ortho:.3e}, eigen {eig[0]:.3e} {eig[1]:.3e}")
        assert np.allclose(A, A.T) and cnt == H * W
        assert err_l <= 1e-12 and err_f <= 1e-9 and ortho <= 1e-12
        assert abs(eig[0] - lam[0] / tr) <= 1e-12 and abs(eig[1] - lam[1] / tr) <= 1e-12
        F = sol


def test_ten_sweeps_are_enough_and_four_are_not():
    H, W = 48, 64
    flow, _ = R.scene(H, W)
    S, _ = R.image_sums(flow, MR.known_mask(flow[None])[0], [0.0] * 9, True, 1.0)
    A = np.array(R.moment_matrix(S))
    left = {}
    for sweeps in (4, 6, R.SWEEPS):
        d, V = R.jacobi(A, sweeps)
        V = np.array(V)
        B = V.T @ A @ V
        left[sweeps] = np.abs(B - np.diag(np.diag(B))).max() / np.trace(A)
    print(f"fundamental jacobi: off-diagonal part over the trace after 4, 6, {R.SWEEPS} sweeps: {left}")
    assert R.SWEEPS == 10 and left[4] > 1e-13 and left[6] <= 1e-13 and left[10] <= 1e-13
    d3, V3 = R.jacobi([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 5.0]])    # size 3, a zero entry skipped
    assert np.allclose(sorted(d3), [1.0, 3.0, 5.0], atol=1e-15) and R.smallest(d3) == 0 and R.smallest([1.0, 1.0, 3.0]) == 0
    assert R.smallest([1.0, 1.0, 3.0], skip=0) == 1


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_test_scene_separates_the_block_from_the_parallax(shape):
    H, W = shape
    flow, rect = R.scene(H, W)
    out = R.reference_fit(H, W, 4)
    F, e = out["matrices"][0], out["epipole"][0]
    dist, inl = R.residual(flow[None], out["matrices"])
    sv = np.linalg.svd(F)[1]
    print(f"fundamental scene {H}x{W}: static max {dist[0][~rect].max():.4f} px, block min {dist[0][rect].min():.4f} px, eigen "
          f"{out['eigen'][0].tolist()}, |F e| {np.abs(F @ e).max():.3e} |e| {np.abs(e).max():.3e}, singular values {sv.tolist()}")
    assert out["ok"][0] and out["count"][0] == H * W and out["left_out"][0] == [0] * 5
    assert dist[0][~rect].max() <= 0.25 and (dist[0][rect] > 1.0).all() and out["eigen"][0, 1] > 1e-5
    assert inl[0][~rect].all() and not inl[0][rect].any()
    assert np.abs(F @ e).max() <= 1e-12 * np.abs(e).max()                      # F e = 0
    assert sv[2] <= 1e-15 and sv[1] > 1e-3 and np.linalg.matrix_rank(F, tol=1e-12) == 2
    assert abs(np.sqrt((F * F).sum()) - 1.0) <= 1e-15 and F.reshape(-1)[np.abs(F).argmax()] > 0.0
    # without the block the rigid scene fits to the float32 rounding of the flow
    clean = R.scene(H, W, block=False)[0][None]
    d0 = R.residual(clean, R.reference_fit(H, W, 4, block=False)["matrices"])[0]
    print(f"fundamental scene {H}x{W} without the block: static max {d0.max():.3e} px")
    assert d0.max() <= 1e-5
    # the homography cannot explain the parallax (the GPU test's bounds come from these figures)
    hres = HR.residual(flow[None], HR.fit(flow[None], None, 4)["matrices"])[1]
    print(f"fundamental scene {H}x{W}: static pixels that are no inliers of the fitted homography at 3 px: {(~hres[0][~rect]).mean():.4f}")


def test_degenerate_inputs_give_ok_false_and_zeros():
    H, W = 24, 32
    flow = R.scene(H, W)[0][None]
    exact = HR.exact_flow(HR.true_matrix(H, W), H, W)[None]
    seven = np.zeros((1, H, W), bool)
    seven[0, [1, 5, 9, 12, 17, 20, 23], [2, 11, 4, 30, 15, 8, 31]] = True
    for tag, f, v in (("a homography's flow", exact, None), ("7 known pixels", flow, seven), ("all sentinel", np.full_like(flow, 1e10), None),
                      ("zero flow", np.zeros_like(flow), None)):
        for iters in (0, 3):
            out = R.fit(f, v, iters)
            print(f"fundamental degenerate, {tag}, iters {iters}: ok {out['ok'].tolist()} count {out['count'].tolist()} eigen {out['eigen'][0].tolist()}")
            assert not out["ok"][0] and not out["matrices"].any() and not out["epipole"].any(), tag
            d, inl = R.residual(f, out["matrices"])
            assert (d == R.SENTINEL).all() and not inl.any()
    nan = flow.copy()
    nan[0, 4, 4, 0] = np.nan                                                   # a NaN flow is one unknown pixel, not a failure
    out = R.fit(nan, None, 4)
    assert out["ok"][0] and out["count"][0] == H * W - 1


def test_the_surface_header_signatures_sources_and_all():
    import pwcnet_amd
    from pwcnet_amd import _lib, fundamental
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert "epipolar motion" in header and "exactly 10 sweeps" in header
    for name in ("pwc_fundamental_fit_workspace_bytes", "pwc_fundamental_fit_f64", "pwc_epipolar_residual_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    decl = re.search(r"int pwc_fundamental_fit_f64\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["pwc_fundamental_fit_f64"][1]) == 17
    decl = re.search(r"int pwc_epipolar_residual_f32\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["pwc_epipolar_residual_f32"][1]) == 11
    assert "pwc_fundamental.hip" in _lib.SOURCES and "pwc_homography.hip" in _lib.SOURCES and "motion_jacobi.h" in _lib.HEADERS
    for f in ("pwc_fundamental.hip", "motion_jacobi.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, f))
    source = ""
    for f in ("pwc_fundamental.hip", "motion_jacobi.h", "two_view.h", "robust_fit.h", "flow_record.h"):   # the file and the project
        text = open(os.path.join(_lib.CSRC, f)).read()                                                   # headers its numerics come from
        assert ("#pragma clang fp contract(off)" in text or f == "motion_jacobi.h") and "fma" not in text.replace("fmax", ""), f
        source += text
    assert "two_view_sampson(" in source and "pwc_fit_gather<FUNDAMENTAL_SUMS>" in source and "pwc_flow_known(" in source
    assert "#pragma clang fp contract(off)" in source and "MOTION_JACOBI_SWEEPS 10" in source and "fma" not in source.replace("fmax", "")
    for name in ("fit_fundamental", "epipolar_residual", "epipolar_regions"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(fundamental, name)
        doc = getattr(fundamental, name).__doc__
        assert "epipolar line" in doc and "tuned" in doc or name == "epipolar_regions"
    assert "fundamental" in pwcnet_amd.__all__ and "only rotates" in fundamental.__doc__ and "along" in fundamental.__doc__.lower()


def test_argument_errors():
    import torch
    import pwcnet_amd
    flows = torch.zeros((1, 4, 4, 2))
    for kw in (dict(iters=-1), dict(iters=65), dict(iters=1.5), dict(iters=True), dict(scale=0.0), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            pwcnet_amd.fit_fundamental(flows, **kw)
    with pytest.raises(ValueError):
        pwcnet_amd.fit_fundamental(flows)                                      # on the CPU: the GPU only
    with pytest.raises(ValueError):
        pwcnet_amd.fit_fundamental(torch.zeros((1, 4, 4, 3)))
    with pytest.raises(TypeError):
        pwcnet_amd.fit_fundamental(flows.double())
    with pytest.raises(ValueError):
        pwcnet_amd.fit_fundamental(flows, valid=torch.ones((1, 4, 5), dtype=torch.bool))
    mats = torch.eye(3, dtype=torch.float64)[None]
    with pytest.raises(TypeError):
        pwcnet_amd.epipolar_residual(flows, mats.float())
    with pytest.raises(ValueError):
        pwcnet_amd.epipolar_residual(flows, mats.repeat(2, 1, 1))
    for thr in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            pwcnet_amd.epipolar_residual(flows, mats, threshold=thr)
    with pytest.raises(ValueError):
        pwcnet_amd.epipolar_residual(flows, mats)                              # on the CPU: the GPU only
    with pytest.raises(TypeError):
        pwcnet_amd.epipolar_regions(flows, mats, projective=True)              # no point map: not a keyword here
    with pytest.raises(TypeError):
        pwcnet_amd.epipolar_regions(flows, mats, min_aera=3)


def test_cli_refuses_stabilize_and_plate_with_motion_fundamental(tmp_path):
    """--motion fundamental is a choice; --stabilize and --plate need a point map and end in an argparse error that says so,
    before anything touches the GPU or the frames."""
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    for flags in (["--stabilize", "2"], ["--plate"], ["--plate", "--plate_foreground", "10"]):
        run = subprocess.run(cli + ["--motion", "fundamental"] + flags, capture_output=True, text=True, timeout=120)
        assert run.returncode == 2 and "point map" in run.stderr and "fundamental" in run.stderr, run.stderr[-500:]
    run = subprocess.run(cli + ["--motion", "essential"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and "fundamental" in run.stderr and "invalid choice" in run.stderr
    run = subprocess.run(cli + ["--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "fit_fundamental" in run.stdout and "epipoles.npy" in run.stdout
