"""The projective path on the CPU: the numpy restatement of the homography fit (tests/homography_ref.py) against known
homographies, outliers, numpy.linalg.lstsq and the degenerate inputs; projective.h's position against the affine sums; the host
helpers plate_path, plate_canvas, canvas_matrices and smooth_path with projective=True against hand-made chains; argument errors
and the CLI's parsing.  tests/test_gpu_homography.py holds the kernels to the restatement bit for bit.

Bounds: corners within 1e-3 px (the project's flow tolerance; the restatement's worst on exact float32 flows is 1.6e-8 px) and,
with a block of 15 % of the pixels moved by 9 px, below 0.5 px at iters = 4 and below a tenth of the same fit's error at
iters = 0 (the restatement's own: 0.032 .. 0.033 px at iters = 4 against 2.1 .. 2.4 px at iters = 0)."""
import subprocess
import sys
import os

import numpy as np
import pytest

from tests import homography_ref as R
from tests import motion_ref as MR
from tests import plate_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("iters", [0, 4])
def test_exact_flows_of_a_homography_are_recovered(shape, iters):
    H, W = shape
    _, truth, _ = R.scene(H, W)
    out = R.reference_fit(H, W, iters)
    err = R.corner_error(out["matrices"][0], truth, H, W)
    print(f"homography exact {H}x{W} iters {iters}: corner error {err:.3e} px, smallest pivot / weight sum {min(out['pivots'][0]):.3e}")
    assert out["ok"][0] and out["count"][0] == H * W and out["matrices"][0][2, 2] == 1.0
    assert err <= 1e-3
    assert min(out["pivots"][0]) > 1e-3                                        # six orders above the pivot rule: no pivoting needed


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_block_of_outliers_is_voted_out(shape):
    H, W = shape
    _, truth, rect = R.scene(H, W, outliers=True)
    assert 0.14 <= rect.mean() <= 0.17
    e0 = R.corner_error(R.reference_fit(H, W, 0, outliers=True)["matrices"][0], truth, H, W)
    e4 = R.corner_error(R.reference_fit(H, W, 4, outliers=True)["matrices"][0], truth, H, W)
    print(f"homography outliers {H}x{W}: block {rect.mean():.3f} of the pixels, corner error {e0:.3f} px at iters 0, {e4:.4f} px at iters 4")
    assert e4 < 0.5 and e4 < 0.1 * e0


def test_a_pass_equals_lstsq_on_the_same_weighted_rows():
    """The 23 sums, the assembly and the elimination against numpy.linalg.lstsq on the 2 K weighted rows themselves: pass 0
    (unit weights) and a reweighted pass against the parameters pass 0 gave."""
    H, W = 17, 33
    flow, _, _ = R.scene(H, W, outliers=True, noise=0.05)
    known = MR.known_mask(flow[None])[0]
    xh, yh, _, _, s = MR.normalised(H, W)
    xp, yp = xh + flow[..., 0].reshape(-1).astype(np.float64) / s, yh + flow[..., 1].reshape(-1).astype(np.float64) / s
    g = list(R.IDENTITY)
    for first in (True, False):
        S, cnt = R.image_sums(flow, known, g, first, 1.0)
        sol, _ = R.solve(S, cnt)
        w = R.pixel_terms(flow, known, g, first, 1.0)[0][:, 0]
        z, o = np.zeros_like(xh), np.ones_like(xh)
        rows = np.concatenate([np.stack([xh, yh, o, z, z, z, -xp * xh, -xp * yh], 1), np.stack([z, z, z, xh, yh, o, -yp * xh, -yp * yh], 1)])
        rhs, sw = np.concatenate([xp, yp]), np.sqrt(np.concatenate([w, w]))
        ref = np.linalg.lstsq(rows * sw[:, None], rhs * sw, rcond=None)[0]
        a, b = R.pixel_matrix(sol, H, W)[0], R.pixel_matrix(ref, H, W)[0]
        err = R.corner_error(a, b, H, W)
        print(f"homography lstsq {'pass 0' if first else 'reweighted'}: corner distance {err:.3e} px")
        assert err < 1e-6
        g = sol


def test_degenerate_inputs_give_ok_false_and_the_identity():
    H, W = 13, 19
    flow = R.scene(H, W)[0][None]
    few = np.zeros((1, H, W), bool)
    few[0, [1, 5, 9], [2, 11, 4]] = True                                       # three known pixels
    row = np.zeros((1, H, W), bool)
    row[0, 6] = True                                                           # a collinear mask: one row
    diag = np.zeros((1, H, W), bool)
    diag[0, np.arange(13), np.arange(13)] = True                               # ... and a diagonal
    nan = flow.copy()
    nan[0, 4, 4, 0] = np.nan
    cases = [("three pixels", flow, few), ("a row", flow, row), ("a diagonal", flow, diag), ("a 1 x 19 image", R.scene(1, 19)[0][None], None),
             ("a 19 x 1 image", R.scene(19, 1)[0][None], None), ("nothing known", np.full_like(flow, np.nan), None)]
    for tag, f, v in cases:
        for iters in (0, 3):
            out = R.fit(f, v, iters)
            print(f"homography degenerate, {tag}, iters {iters}: ok {out['ok'].tolist()} count {out['count'].tolist()}")
            assert not out["ok"][0] and np.array_equal(out["matrices"][0], np.eye(3)), tag
    out = R.fit(nan, None, 4)                                                  # a NaN flow is one unknown pixel, not a failure ...
    assert out["ok"][0] and out["count"][0] == H * W - 1
    assert R.corner_error(out["matrices"][0], R.scene(H, W)[1], H, W) < 1e-3
    # the horizon-in-frame rule: the exact flows (where they exist) of a homography whose D changes sign inside the frame
    M = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0 / 12.0, 0.0, 1.0]])  # D = 0 at x = 12
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        D = 1.0 - x / 12.0
        f = np.stack([x / D - x, y / D - y], -1).astype(np.float32)[None]
    out = R.fit(f, (x < 9)[None], 0)
    print(f"homography horizon in the frame: ok {out['ok'].tolist()}, m6 of the normalised fit {out['params'][0][6]:.4f}")
    assert not out["ok"][0] and np.array_equal(out["matrices"][0], np.eye(3)) and out["count"][0] == 9 * H
    assert not R.pixel_matrix(out["params"][0], H, W)[1]


def test_an_affine_field_and_affine_matrices():
    H, W = 48, 64
    flow = MR.scene(H, W, noise=0.0, outliers=False)[0]
    truth = MR.pixel_matrix(MR.TRUE_PARAMS, H, W)
    out = R.fit(flow[None], None, 4)
    err = R.corner_error(out["matrices"][0], truth, H, W)
    print(f"homography on an affine field: corner error {err:.3e} px, last row {out['matrices'][0][2].tolist()}")
    assert out["ok"][0] and err <= 1e-3
    # projective.h's position on affine matrices: the affine sums' bits; the consumers' restatements agree bit for bit
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    there, sx, sy = R.position(truth, x, y)
    ax, ay = ((truth[0, 0] * x) + (truth[0, 1] * y)) + truth[0, 2], ((truth[1, 0] * x) + (truth[1, 1] * y)) + truth[1, 2]
    assert there.all() and np.array_equal(sx.view(np.int64), ax.view(np.int64)) and np.array_equal(sy.view(np.int64), ay.view(np.int64))
    a, b = MR.residual(flow[None], truth[None]), R.residual(flow[None], truth[None])
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    frames = MR.random_frames(1, H, W, 3, np.float32)
    a, b = MR.warp(frames, truth[None]), R.warp(frames, truth[None])
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    # no position: D <= 0, a NaN
    bad = truth.copy()
    bad[2] = (0.0, 0.0, -1.0)
    assert not R.position(bad, x, y)[0].any()
    bad[2] = (np.nan, 0.0, 1.0)
    assert not R.position(bad, x, y)[0].any() and not R.finite(bad)


# ------------------------------------------------------------------ the host helpers
def _chain(T=4):
    rs = np.random.RandomState(8)
    M = np.tile(np.eye(3), (T, 1, 1))
    M[:, :2] += rs.normal(0, 0.02, size=(T, 2, 3))
    M[:, :2, 2] += rs.uniform(-4, 4, size=(T, 2))
    M[:, 2, :2] = rs.uniform(-3e-4, 3e-4, size=(T, 2))
    return M


def test_plate_path_chains_and_inverts_full_matrices():
    from pwcnet_amd import plate
    M = _chain()
    P, reach = plate.plate_path(M, anchor=2, projective=True)
    assert reach.all() and np.array_equal(P[2], np.eye(3))
    want3 = M[2] / M[2][2, 2]
    want4 = (M[3] @ want3)
    want1 = np.linalg.inv(M[1])
    want0 = np.linalg.inv(M[0]) @ (want1 / want1[2, 2])
    for got, want in ((P[3], want3), (P[4], want4), (P[1], want1), (P[0], want0)):
        assert got[2, 2] == 1.0 and np.allclose(got, want / want[2, 2], rtol=1e-12, atol=1e-12)
    assert np.abs(P[4][2, :2]).max() > 1e-5                                    # the last row is carried, not reset
    # a point followed pair by pair lands where the chained matrix sends it
    p = np.array([7.0, 5.0, 1.0])
    q = p.copy()
    for t in (2, 3):
        q = M[t] @ q
        q = q / q[2]
    r = P[4] @ p
    assert np.allclose(r / r[2], q, atol=1e-9)
    # breaks: ok False, a non-finite matrix, a step that lands behind the horizon
    assert plate.plate_path(M, [True, False, True, True], anchor=0, projective=True)[1].tolist() == [True, True, False, False, False]
    bad = M.copy()
    bad[3, 2, 2] = -1.0
    assert plate.plate_path(bad, anchor=2, projective=True)[1].tolist() == [True, True, True, True, False]
    bad[3, 0, 0] = np.nan
    assert plate.plate_path(bad, anchor=2, projective=True)[1].tolist() == [True, True, True, True, False]
    # projective=False: the present results on affine inputs
    A = M.copy()
    A[:, 2] = (0.0, 0.0, 1.0)
    a, b = plate.plate_path(A, anchor=1), PR.plate_path(A, anchor=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.allclose(plate.plate_path(A, anchor=1, projective=True)[0], a[0], atol=1e-12)
    with pytest.raises(TypeError):
        plate.plate_path(M, projective=1)


def test_plate_canvas_divides_and_skips_a_frame_behind_the_horizon():
    from pwcnet_amd import plate
    H, W = 20, 30
    P = np.tile(np.eye(3), (3, 1, 1))
    P[1] = [[1.0, 0.0, -5.0], [0.0, 1.0, 2.0], [1e-3, 0.0, 1.0]]
    reach = np.ones(3, bool)
    x0, y0, Hc, Wc = plate.plate_canvas(P, reach, H, W, projective=True)
    xs, ys = [], []
    for t in range(3):
        qx, qy, D = R.project(np.linalg.inv(P[t]), R.corners_of(H, W))
        assert (D > 0).all()
        xs, ys = xs + list(qx), ys + list(qy)
    assert (x0, y0) == (int(np.floor(min(xs))), int(np.floor(min(ys))))
    assert (Hc, Wc) == (int(np.ceil(max(ys))) - y0 + 1, int(np.ceil(max(xs))) - x0 + 1)
    assert (x0, y0, Hc, Wc) != plate.plate_canvas(P, reach, H, W)              # (the affine rule ignores the division)
    # frame 2 puts a corner behind the horizon: it counts as not reached
    P2 = P.copy()
    P2[2] = np.linalg.inv(np.array([[1.0, 0.0, 40.0], [0.0, 1.0, 0.0], [-1.0 / 15.0, 0.0, 1.0]]))
    assert not (R.project(np.linalg.inv(P2[2]), R.corners_of(H, W))[2] > 0).all()
    assert plate.plate_canvas(P2, reach, H, W, projective=True) == plate.plate_canvas(P, np.array([True, True, False]), H, W, projective=True)
    with pytest.raises(ValueError):
        plate.plate_canvas(P2[2:], np.ones(1, bool), H, W, projective=True)
    A = np.tile(np.eye(3), (2, 1, 1))
    A[1, :2, 2] = (3.5, -2.25)
    assert plate.plate_canvas(A, np.ones(2, bool), H, W) == PR.plate_canvas(A, np.ones(2, bool), H, W)
    assert plate.plate_canvas(A, np.ones(2, bool), H, W, projective=True) == PR.plate_canvas(A, np.ones(2, bool), H, W)


def test_canvas_matrices_keep_the_last_row():
    from pwcnet_amd import plate
    P, _ = plate.plate_path(_chain(), anchor=0, projective=True)
    mats, inv = plate.canvas_matrices(P, -3, 4, projective=True)
    shift = np.array([[1.0, 0.0, -3.0], [0.0, 1.0, 4.0], [0.0, 0.0, 1.0]])
    for t in range(len(P)):
        want = P[t] @ shift
        assert np.allclose(mats[t], want / want[2, 2], atol=1e-12) and mats[t][2, 2] == 1.0 and inv[t][2, 2] == 1.0
        prod = inv[t] @ mats[t]
        assert np.allclose(prod / prod[2, 2], np.eye(3), atol=1e-9)
    assert np.abs(mats[-1][2, :2]).max() > 1e-5
    bad = P.copy()
    bad[1, 2, 2] = 0.0
    bad[1, 2, :2] = 0.0
    m2, i2 = plate.canvas_matrices(bad, 0, 0, projective=True)
    assert np.isnan(m2[1]).all() and np.isnan(i2[1]).all() and np.isfinite(m2[0]).all()
    A = P.copy()
    A[:, 2] = (0.0, 0.0, 1.0)
    a, b = plate.canvas_matrices(A, -3, 4), PR.canvas_matrices(A, -3, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_smooth_path_averages_the_eight_normalised_entries():
    from pwcnet_amd import motion
    M = _chain(5)
    ident = motion.smooth_path(M, 0, projective=True)
    assert np.allclose(ident, np.tile(np.eye(3), (6, 1, 1)), atol=1e-12)
    A = motion.smooth_path(M, 1, projective=True)
    P = [np.eye(3)]
    for t in range(5):
        nxt = M[t] @ P[-1]
        P.append(nxt / nxt[2, 2])
    for t in range(6):
        mean = np.mean(P[max(0, t - 1):min(5, t + 1) + 1], axis=0)
        assert mean[2, 2] == 1.0
        want = P[t] @ np.linalg.inv(mean)
        assert np.allclose(A[t], want / want[2, 2], atol=1e-12) and A[t][2, 2] == 1.0
    assert np.abs(A[:, 2, :2]).max() > 1e-6
    Aff = M.copy()
    Aff[:, 2] = (0.0, 0.0, 1.0)
    before = motion.smooth_path(Aff, 2)
    assert (before[:, 2] == (0.0, 0.0, 1.0)).all() and np.allclose(motion.smooth_path(Aff, 2, projective=True), before, atol=1e-12)
    with pytest.raises(TypeError):
        motion.smooth_path(M, 1, projective="yes")


# ------------------------------------------------------------------ errors and the CLI
def test_argument_errors():
    import torch
    import pwcnet_amd
    from pwcnet_amd import motion, plate, regions
    assert pwcnet_amd.fit_homography is pwcnet_amd.homography.fit_homography and "fit_homography" in pwcnet_amd.__all__
    flows = torch.zeros((1, 4, 4, 2))
    with pytest.raises(ValueError):
        motion.fit_motion(flows, model="homography")                           # as before: the affine family only
    for kw in (dict(iters=-1), dict(iters=65), dict(iters=1.5), dict(iters=True), dict(scale=0.0), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            pwcnet_amd.fit_homography(flows, **kw)
    with pytest.raises(ValueError):
        pwcnet_amd.fit_homography(flows)                                       # on the CPU: the GPU only
    with pytest.raises(ValueError):
        pwcnet_amd.fit_homography(torch.zeros((1, 4, 4, 3)))
    with pytest.raises(TypeError):
        pwcnet_amd.fit_homography(flows.double())
    with pytest.raises(ValueError):
        pwcnet_amd.fit_homography(flows, valid=torch.ones((1, 4, 5), dtype=torch.bool))
    mats = torch.eye(3, dtype=torch.float64)[None]
    frames = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        motion.motion_residual(flows, mats, projective=1)
    with pytest.raises(TypeError):
        motion.warp_frames(frames, mats, projective=None)
    with pytest.raises(TypeError):
        plate.background_plate(frames, mats, (4, 4), projective="on")
    with pytest.raises(TypeError):
        plate.plate_difference(frames, frames[0], torch.zeros((4, 4), dtype=torch.uint8), mats, 1.0, projective=0)
    with pytest.raises(TypeError):
        regions.moving_regions(flows, mats, projective=2)
    with pytest.raises(TypeError):
        regions.moving_regions(flows, mats, projectiv=True)


def test_cli_parses_motion_homography(tmp_path):
    """--motion homography is a choice; a fifth name is not; the flags' rules are reported before anything touches the GPU."""
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(tmp_path / "none_*.png")]
    run = subprocess.run(cli + ["--motion", "projective"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and "homography" in run.stderr and "invalid choice" in run.stderr
    run = subprocess.run(cli + ["--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "fit_homography" in run.stdout
    run = subprocess.run(cli + ["--motion", "homography", "--motion_iters", "65"], capture_output=True, text=True, timeout=120)
    assert run.returncode != 0 and "invalid choice" not in run.stderr
