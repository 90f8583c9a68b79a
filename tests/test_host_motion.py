"""CPU tests of the dominant-motion feature: the numpy restatement of csrc/pwc_motion.hip (tests/motion_ref.py) against
independent routes and cases done by hand, the conditions the GPU tests rely on, smooth_path, the argument checks and the C ABI
surface.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import motion_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _design(H, W, model):
    """The design matrix of the stacked (u, v) observations in the model's own unknowns, and the map to the six parameters."""
    xh, yh, _, _, _ = R.normalised(H, W)
    one, zero = np.ones_like(xh), np.zeros_like(xh)
    if model == "translation":
        Du, Dv = np.stack([one, zero], 1), np.stack([zero, one], 1)
        to6 = lambda q: [q[0], 0, 0, q[1], 0, 0]                                   # noqa: E731
    elif model == "similarity":
        Du, Dv = np.stack([one, zero, xh, -yh], 1), np.stack([zero, one, yh, xh], 1)
        to6 = lambda q: [q[0], q[2], -q[3], q[1], q[3], q[2]]                      # noqa: E731
    else:
        Du = np.stack([one, xh, yh, zero, zero, zero], 1)
        Dv = np.stack([zero, zero, zero, one, xh, yh], 1)
        to6 = lambda q: list(q)                                                    # noqa: E731
    return Du, Dv, to6


def _irls_lstsq(flow, known, model, iters, scale):
    """The same estimator by another route: np.linalg.lstsq on the weighted design matrix, the weights from the pass before."""
    H, W = known.shape
    Du, Dv, to6 = _design(H, W, model)
    k = known.reshape(-1)
    u, v = flow[..., 0].reshape(-1).astype(np.float64), flow[..., 1].reshape(-1).astype(np.float64)
    xh, yh, _, _, _ = R.normalised(H, W)
    p = np.zeros(6)
    for it in range(iters + 1):
        if it == 0:
            w = np.ones_like(u)
        else:
            ru, rv = u - (p[0] + p[1] * xh + p[2] * yh), v - (p[3] + p[4] * xh + p[5] * yh)
            w = 1.0 / (1.0 + (ru * ru + rv * rv) / scale ** 2)
        sw = np.sqrt(w[k])
        D = np.concatenate([Du[k] * sw[:, None], Dv[k] * sw[:, None]])
        q = np.linalg.lstsq(D, np.concatenate([u[k] * sw, v[k] * sw]), rcond=None)[0]
        p = np.array(to6(q), np.float64)
    return p


@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("iters", [0, 1, 4])
def test_restatement_equals_weighted_lstsq(model, iters):
    for (H, W), seed in zip(R.SHAPES + ((260, 256),), range(4)):
        flow, _ = R.scene(H, W, seed)
        valid = np.random.RandomState(seed).uniform(size=(H, W)) > 0.2
        got = R.fit(flow[None], valid[None], model, iters, 1.0)
        want = _irls_lstsq(flow, valid, model, iters, 1.0)
        err = np.abs(got["params"][0] - want).max() / max(1.0, np.abs(want).max())
        print(f"motion host lstsq {model} iters {iters} {H}x{W}: relative difference {err:.2e}")
        assert got["ok"][0] and got["count"][0] == valid.sum()
        assert err < 1e-9


def test_pure_translation_by_hand():
    flow = np.zeros((1, 5, 7, 2), np.float32)
    flow[..., 0], flow[..., 1] = 3.0, -2.0
    for model in R.MODELS:
        got = R.fit(flow, None, model, 2, 1.0)
        assert got["ok"][0] and got["count"][0] == 35 and got["weight_sum"][0] == 35.0
        assert np.allclose(got["matrices"][0], [[1, 0, 3], [0, 1, -2], [0, 0, 1]], atol=1e-12), model
    got = R.fit(flow, None, "translation", 2, 1.0)
    assert np.array_equal(got["matrices"][0], [[1, 0, 3], [0, 1, -2], [0, 0, 1]])          # 105 / 35 and -70 / 35 are exact
    res, inl = R.residual(flow, got["matrices"])
    assert np.array_equal(res, np.zeros_like(res)) and inl.all()


def test_rotation_about_the_centre_by_hand():
    """A rotation by theta about the frame's centre is the similarity alpha = s' (cos - 1), beta = s' sin, a0 = b0 = 0."""
    H, W, th = 9, 12, 0.05
    y, x = np.meshgrid(np.arange(H) - (H - 1) / 2, np.arange(W) - (W - 1) / 2, indexing="ij")
    flow = np.stack([np.cos(th) * x - np.sin(th) * y - x, np.sin(th) * x + np.cos(th) * y - y], -1).astype(np.float32)[None]
    for model in ("similarity", "affine"):
        got = R.fit(flow, None, model, 3, 1.0)
        M = got["matrices"][0]
        assert got["ok"][0]
        assert np.allclose(M[:2, :2], [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]], atol=1e-6)
        centre = np.array([(W - 1) / 2, (H - 1) / 2, 1.0])
        assert np.allclose(M @ centre, centre, atol=1e-5)
    s = max(H, W) / 2
    p = R.fit(flow, None, "similarity", 3, 1.0)["params"][0]
    assert np.allclose(p, [0, s * (np.cos(th) - 1), -s * np.sin(th), 0, s * np.sin(th), s * (np.cos(th) - 1)], atol=1e-5)


def test_irls_rejects_the_moving_rectangle():
    """The conditions the GPU tests' inputs rely on, on the restatement alone: plain least squares is pulled more than 1 px by
    the rectangle, four reweighting passes at scale 1 land within 0.1 px, the pivots stay far from the refusal threshold."""
    for (H, W), seed in zip(R.SHAPES, range(3)):
        flow, rect = R.scene(H, W, seed)
        frac = rect.mean()
        plain = R.fit(flow[None], None, "affine", 0, 1.0)
        robust = R.fit(flow[None], None, "affine", 4, 1.0)
        more = R.fit(flow[None], None, "affine", 12, 1.0)
        e0 = np.abs(plain["params"][0] - R.TRUE_PARAMS).max()
        e4 = np.abs(robust["params"][0] - R.TRUE_PARAMS).max()
        e12 = np.abs(more["params"][0] - R.TRUE_PARAMS).max()
        piv = [p for r in (plain, robust) for p in r["pivots"][0]]
        print(f"motion host irls {H}x{W}: rectangle {frac:.3f}, error iters 0 {e0:.3f} px, iters 4 {e4:.4f} px, iters 12 "
              f"{e12:.4f} px, pivots / Sw {min(piv):.3f} .. {max(piv):.3f}")
        assert 0.26 <= frac <= 0.29
        assert e0 > 1.0 and e4 < 0.1 and e12 < 0.1
        assert min(piv) > 1e-3
        res, inl = R.residual(flow[None], robust["matrices"], None, 3.0)
        assert (inl[0] == ~rect).mean() > 0.99


def test_a_row_of_pixels_is_degenerate_for_the_affine_model():
    """1 x 19: yh = 0 everywhere, so Sy = Sxy = Syy = 0 and the affine system's last pivot is exactly zero -- degenerate.  The
    translation is fine.  The similarity is fine as well, and that is arithmetic, not a choice: on a row its model is
    u = a0 + alpha xh, v = b0 + beta xh, four unknowns that two components along a line determine; the 4 x 4 system's pivots
    are Sw, Sw and twice Sxx - Sx Sx / Sw, the spread of xh, which is not small.  (The issue this feature answers expected a
    zero pivot for the similarity too; the system it specifies does not have one.  DESIGN.md 20 says so.)"""
    flow = R.batch(1, 19, seed=5, outliers=False)
    for model, ok in (("translation", True), ("similarity", True), ("affine", False)):
        got = R.fit(flow, None, model, 2, 1.0)
        assert bool(got["ok"][0]) is ok, model
        if not ok:
            assert np.array_equal(got["matrices"][0], np.eye(3)) and not got["params"][0].any()
            assert got["pivots"][0][-1] == 0.0                                      # yh = 0 everywhere: a pivot of exactly zero
        else:
            assert min(got["pivots"][0]) > 1e-3
    exact = R.batch(1, 19, seed=5, outliers=False, noise=0.0, params=(1.5, 0.25, -0.5, -0.5, 0.5, 0.25))
    assert np.allclose(R.fit(exact, None, "similarity", 2, 1.0)["params"][0], (1.5, 0.25, -0.5, -0.5, 0.5, 0.25), atol=1e-6)
    column = R.batch(19, 1, seed=5, outliers=False)
    assert not R.fit(column, None, "affine", 2, 1.0)["ok"][0] and R.fit(column, None, "similarity", 2, 1.0)["ok"][0]
    one = R.fit(np.zeros((1, 1, 1, 2), np.float32), None, "affine", 1, 1.0)
    assert not one["ok"][0] and one["count"][0] == 1
    assert R.fit(np.ones((1, 1, 1, 2), np.float32), None, "translation", 1, 1.0)["matrices"][0][0, 2] == 1.0
    few = np.zeros((1, 4, 4), bool)
    few[0, 1, 1] = few[0, 2, 3] = True
    assert not R.fit(R.batch(4, 4), few, "affine", 1, 1.0)["ok"][0] and R.fit(R.batch(4, 4), few, "similarity", 1, 1.0)["ok"][0]


def test_unknown_pixels_reach_nothing():
    flow = R.batch(13, 19, seed=2)
    valid = np.random.RandomState(1).uniform(size=(1, 13, 19)) > 0.3
    want = R.fit(flow, valid, "affine", 2, 1.0)
    dirty = flow.copy()
    dirty[~valid] = np.nan
    open_bad = flow.copy()
    idx = np.argwhere(~valid[0])
    for (y, x), bad in zip(idx, [np.nan, np.inf, -np.inf, 1e10, 2e9] * len(idx)):
        open_bad[0, y, x, (y + x) % 2] = bad
    for got in (R.fit(dirty, valid, "affine", 2, 1.0), R.fit(open_bad, None, "affine", 2, 1.0)):
        assert np.array_equal(got["matrices"].view(np.int64), want["matrices"].view(np.int64)) and got["count"][0] == valid.sum()
    res, inl = R.residual(open_bad, want["matrices"], None, 3.0)
    assert (res[~valid] == R.SENTINEL).all() and not inl[~valid].any() and (res[valid] != R.SENTINEL).all()
    bad = want["matrices"].copy()
    bad[0, 2, 0] = 1e-300
    assert (R.residual(flow, bad)[0] == R.SENTINEL).all()


def test_integer_shift_warp_equals_slicing():
    for dtype in (np.uint8, np.float32):
        fr = R.random_frames(2, 7, 9, 3, dtype, seed=3)
        M = np.tile(np.eye(3), (2, 1, 1))
        M[0, 0, 2], M[0, 1, 2] = 2.0, -1.0                                          # out(x, y) = frame(x + 2, y - 1)
        out, cov = R.warp(fr, M)
        assert np.array_equal(out[1], fr[1]) and cov[1].all()
        assert np.array_equal(out[0, 1:, :7], fr[0, :6, 2:]) and cov[0, 1:, :7].all()
        assert not cov[0, 0].any() and not cov[0, :, 7:].any() and not out[0, 0].any() and not out[0, :, 7:].any()
        M[1, 2, 2] = 2.0
        out, cov = R.warp(fr, M)
        assert not cov[1].any() and not out[1].any()


def test_mutations_are_told_apart_by_the_shared_inputs():
    """On the restatement only: the faults DESIGN.md 20 names change bits on the inputs the GPU tests use."""
    flow = R.batch(13, 19, seed=0)
    a, b = R.fit(flow, None, "affine", 4, 1.0), R.fit(flow, None, "affine", 4, 1.0, mutate="no_cross")
    assert not np.array_equal(a["matrices"], b["matrices"])
    fr = R.random_frames(1, 6, 8, 1, np.uint8)
    M = np.eye(3)[None].copy()
    M[0, 0, 2] = 1.0                                                                 # the column x = W - 2 samples x = W - 1 exactly
    assert R.warp(fr, M)[1][0, :, 6].all() and not R.warp(fr, M, mutate="strict_last_column")[1][0, :, 6].any()


def test_smooth_path():
    from pwcnet_amd.motion import smooth_path
    rs = np.random.RandomState(0)
    M = np.tile(np.eye(3), (5, 1, 1))
    M[:, :2, :2] += rs.normal(0, 0.01, size=(5, 2, 2))
    M[:, :2, 2] = rs.normal(0, 3.0, size=(5, 2))
    A = smooth_path(M, 0)
    assert A.shape == (6, 3, 3) and A.dtype == np.float64
    assert np.allclose(A, np.eye(3), atol=1e-12) and np.array_equal(A[:, 2], np.tile([0.0, 0.0, 1.0], (6, 1)))
    steady = np.tile(np.eye(3), (4, 1, 1))
    steady[:, 0, 2] = 2.0                                                            # a steady pan: only the ends are pulled in
    A = smooth_path(steady, 1)
    assert np.allclose(A[1:4], np.eye(3), atol=1e-12) and np.allclose(A[0, :2, 2], [-1.0, 0.0]) and np.allclose(A[4, :2, 2], [1.0, 0.0])
    shaky = steady.copy()
    shaky[1, 1, 2], shaky[2, 1, 2] = 3.0, -3.0                                       # frame 2 alone is 3 px low
    A = smooth_path(shaky, 1)
    assert np.allclose(A[2, :2, 2], [0.0, 2.0]) and "not a geodesic" in " ".join(smooth_path.__doc__.split())
    assert np.array_equal(smooth_path(torch.from_numpy(shaky), 1), A)
    with pytest.raises(ValueError, match="matrices"):
        smooth_path(np.eye(3), 1)
    with pytest.raises(ValueError, match="radius"):
        smooth_path(steady, -1)


def test_argument_checks_come_before_the_device():
    import pwcnet_amd
    from pwcnet_amd import motion
    for name in ("fit_motion", "motion_residual", "warp_frames", "smooth_path"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(motion, name)
    flows = torch.zeros((2, 4, 5, 2))
    mats = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(TypeError, match="flows"):
        motion.fit_motion(flows.double())
    with pytest.raises(ValueError, match="flows"):
        motion.fit_motion(flows[..., :1])
    with pytest.raises(ValueError, match="valid"):
        motion.fit_motion(flows, valid=torch.ones((2, 4, 4), dtype=torch.bool))
    with pytest.raises(TypeError, match="valid"):
        motion.fit_motion(flows, valid=torch.ones((2, 4, 5)))
    with pytest.raises(ValueError, match="model"):
        motion.fit_motion(flows, model="homography")
    for bad in (-1, 65, 1.5, True):
        with pytest.raises(ValueError, match="iters"):
            motion.fit_motion(flows, iters=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            motion.fit_motion(flows, scale=bad)
    with pytest.raises(ValueError, match="GPU only"):
        motion.fit_motion(flows)
    with pytest.raises(TypeError, match="matrices"):
        motion.motion_residual(flows, mats.float())
    with pytest.raises(ValueError, match="matrices"):
        motion.motion_residual(flows, mats[:1])
    with pytest.raises(ValueError, match="threshold"):
        motion.motion_residual(flows, mats, threshold=-1.0)
    with pytest.raises(ValueError, match="GPU only"):
        motion.motion_residual(flows, mats)
    with pytest.raises(TypeError, match="frames"):
        motion.warp_frames(torch.zeros((2, 4, 5, 3), dtype=torch.float64), mats)
    with pytest.raises(ValueError, match="frames"):
        motion.warp_frames(torch.zeros((2, 4, 5, 5)), mats)
    with pytest.raises(TypeError, match="matrices"):
        motion.warp_frames(torch.zeros((2, 4, 5, 3)), np.eye(3, dtype=np.float32)[None])
    with pytest.raises(ValueError, match="GPU only"):
        motion.warp_frames(torch.zeros((2, 4, 5, 3)), mats)


def test_c_abi_surface():
    import ctypes
    from pwcnet_amd import _lib
    assert "pwc_motion.hip" in _lib.SOURCES
    for name in ("pwc_motion_fit_workspace_bytes", "pwc_motion_fit_f64", "pwc_motion_residual_f32", "pwc_warp_affine"):
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    for N, H, W in ((1, 1, 1), (3, 13, 19), (2, 260, 256), (8, 448, 1024)):
        parts = R.parts_of(H, W)
        want = 8 * (N * parts * 12 + N * 6) + (4 * N * parts + 7) // 8 * 8
        assert L.pwc_motion_fit_workspace_bytes(N, H, W) == want
    assert L.pwc_motion_fit_workspace_bytes(0, 4, 4) == 0 and L.pwc_motion_fit_workspace_bytes(65536, 4, 4) == 0
    assert L.pwc_motion_fit_workspace_bytes(1, 1 << 16, 1 << 15) == 0
    # refusals that need no device: the checks come before any launch
    assert L.pwc_motion_fit_f64(None, 2, None, 1, 4, 4, 2, 4, 1.0, None, 0, None, None, None, None, None) == -1
    assert L.pwc_warp_affine(None, 0, 3, None, 1, 4, 4, None, None, None) == -1
    assert L.pwc_motion_residual_f32(None, 2, None, None, 1, 4, 4, 3.0, None, None, None) == -1
    assert isinstance(ctypes.c_double, type)
    from infer_continuous import build_parser
    ap = build_parser()
    args = ap.parse_args(["-i", "a", "b"])
    assert args.motion is None and args.stabilize == 0 and not args.motion_residual and args.motion_iters == 4 and args.motion_scale == 1.0
    args = ap.parse_args(["-i", "a", "b", "--motion", "similarity", "--motion_iters", "2", "--motion_scale", "0.5", "--stabilize", "3",
                          "--motion_residual"])
    assert (args.motion, args.motion_iters, args.motion_scale, args.stabilize, args.motion_residual) == ("similarity", 2, 0.5, 3, True)


def test_shared_rules_are_written_once():
    """The known-flow rule and the finite test stand in flow_record.h alone, the host's misalignment test in pwc_common.h alone,
    the Sampson terms in two_view.h alone."""
    from pwcnet_amd import _lib
    texts = {f: open(os.path.join(_lib.CSRC, f), errors="replace").read() for f in _lib.SOURCES + _lib.HEADERS}
    for literal, home in (("<= 1e9f", "flow_record.h"), ("1.7976931348623157e308", "flow_record.h"),
                          ("reinterpret_cast<uintptr_t>(p) & mask", "pwc_common.h")):
        assert [f for f, t in texts.items() if literal in t] == [home], literal
    assert not [f for f, t in texts.items() if "1e9f" in t and f != "flow_record.h"]
    assert not [f for f, t in texts.items() if "fundamental_sampson" in t]
    assert [f for f, t in texts.items() if "void two_view_sampson(" in t] == ["two_view.h"]
