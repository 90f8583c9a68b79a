"""Frame interpolation without a GPU: the numpy restatement of tests/interp_ref.py against cases computed by hand and against an
independent scalar loop, the argument checks of pwcnet_amd.interpolate_frames (raised before any device is touched), and the
conditions the GPU tests (tests/test_gpu_interp.py) rely on, asserted on the restatement alone."""
import math

import numpy as np
import pytest
import torch

from pwcnet_amd import interp as IP  # the feature: without it nothing here can be collected
from tests import interp_ref as R


def _frames(H, W, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 1, size=(1, H, W, 3)).astype(np.float32), rs.uniform(0, 1, size=(1, H, W, 3)).astype(np.float32)


def test_zero_flows_give_the_cross_fade_everywhere():
    f0, f1 = _frames(4, 5, 0)
    z = np.zeros((1, 4, 5, 2), np.float32)
    for t in (0.0, 0.25, 0.5, 1.0):
        ref = R.interpolate(f0, f1, z, z, [t])
        assert (ref["source"] == 3).all() and (ref["cnt"] == 1).all()
        fade = (1.0 - t) * f0.astype(np.float64) + t * f1.astype(np.float64)
        # one source per target with b = 1: c_k = rint(w x 2^36) / rint(w 2^36), within 2^-37 (1 + |x|) / (w - 2^-37) of x
        w = np.exp(-10.0)
        assert np.abs(ref["value"][0, 0] - fade[0]).max() <= 2.0 ** -36 / (w - 2.0 ** -37)
        assert np.array_equal(ref["frames_t"][0, 0], ref["value"][0, 0].astype(np.float32))


def test_integer_translation_moves_the_content_by_half_of_it():
    """frame_1 is frame_0 moved 4 px to the right; flows (+4, 0) and (-4, 0); t = 0.5: the content sits 2 px to the right."""
    H, W = 3, 12
    f0, _ = _frames(H, W, 1)
    f1 = np.roll(f0, 4, axis=2)
    fw = np.zeros((1, H, W, 2), np.float32)
    bw = np.zeros((1, H, W, 2), np.float32)
    fw[..., 0], bw[..., 0] = 4.0, -4.0
    ref = R.interpolate(f0, f1, fw, bw, [0.5])
    src = ref["source"][0, 0]
    # direction 0 reaches x = 2 .. 13 -> columns 2 .. 11; direction 1 reaches x = -2 .. 9 -> columns 0 .. 9
    assert (src[:, :2] == 2).all() and (src[:, 2:10] == 3).all() and (src[:, 10:] == 1).all()
    want = np.roll(f0, 2, axis=2).astype(np.float64)[0]
    # columns 2 .. 11 hold frame 0's content moved by exactly 2 px (frame 1's agrees where both arrive)
    assert np.abs(ref["value"][0, 0][:, 2:] - want[:, 2:]).max() <= 2.0 ** -36 / (np.exp(-10.0) - 2.0 ** -37)
    # columns 0, 1: frame 1's columns 2, 3 moved left by 2 = frame 0's columns 10, 11 wrapped, i.e. roll by 2 again
    assert np.abs(ref["value"][0, 0][:, :2] - want[:, :2]).max() <= 2.0 ** -36 / (np.exp(-10.0) - 2.0 ** -37)


def test_the_better_match_dominates_by_the_weight_ratio():
    """Two sources of frame 0 sent to one target; their matches in frame 1 differ from them by 0.05 and by 0.25."""
    H, W = 1, 8
    f0 = np.zeros((1, H, W, 3), np.float32)
    f1 = np.zeros((1, H, W, 3), np.float32)
    f0[0, 0, 1], f0[0, 0, 5] = 0.75, 0.25                       # the two sources
    fw = np.full((1, H, W, 2), np.float32(1e10))                # every other pixel of direction 0: unknown
    bw = np.full((1, H, W, 2), np.float32(1e10))                # direction 1: nothing at all
    fw[0, 0, 1], fw[0, 0, 5] = (4.0, 0.0), (-4.0, 0.0)          # t = 0.5: both land on x = 3; their matches: x = 5 and x = 1
    f1[0, 0, 5] = 0.75 - 0.05                                   # source 1's match: e = 0.05
    f1[0, 0, 1] = 0.25 + 0.25                                   # source 5's match: e = 0.25
    ref = R.interpolate(f0, f1, fw, bw, [0.5], alpha=20.0)
    e1 = abs(np.float64(np.float32(0.75)) - np.float64(np.float32(0.75 - 0.05)))
    e5 = abs(np.float64(np.float32(0.25)) - np.float64(np.float32(0.25 + 0.25)))
    w1, w5 = math.exp(-20.0 * e1), math.exp(-20.0 * e5)
    assert abs(w1 / w5 - math.exp(20.0 * 0.2)) < 1e-5 * math.exp(4.0)
    assert ref["source"][0, 0, 0, 3] == 1 and ref["cnt"][0, 0, 0, 3].tolist() == [2, 0]
    want = (w1 * 0.75 + w5 * 0.25) / (w1 + w5)
    assert abs(ref["value"][0, 0, 0, 3, 0] - want) < 1e-9 and abs(ref["den"][0, 0, 0, 3, 0] - (w1 + w5)) < 2.0 ** -35
    # with alpha = 0 they count alike
    assert abs(R.interpolate(f0, f1, fw, bw, [0.5], alpha=0.0)["value"][0, 0, 0, 3, 0] - 0.5) < 1e-9


def test_a_target_nothing_reaches_is_a_hole_with_the_cross_fade():
    f0, f1 = _frames(3, 6, 2)
    fw = np.zeros((1, 3, 6, 2), np.float32)
    bw = np.zeros((1, 3, 6, 2), np.float32)
    fw[0, 1, 2], bw[0, 1, 2] = (0.0, 1.0), (0.0, -1.0)          # (2, 1) moves away in both directions
    ref = R.interpolate(f0, f1, fw, bw, [0.25])
    # t = 0.25: direction 0 leaves b = 0.75 at (2, 1): still covered; direction 1 (s = 0.75) leaves 0.25 < 0.5
    assert ref["source"][0, 0, 1, 2] == 1
    fw[0, 1, 2] = (0.0, 4.0)                                    # now 1 px away at t = 0.25: b = 0 at (2, 1)
    ref = R.interpolate(f0, f1, fw, bw, [0.25])
    assert ref["source"][0, 0, 1, 2] == 0 and (np.delete(ref["source"][0, 0].ravel(), 1 * 6 + 2) != 0).all()
    fade = 0.75 * f0[0, 1, 2].astype(np.float64) + 0.25 * f1[0, 1, 2].astype(np.float64)
    assert np.array_equal(ref["value"][0, 0, 1, 2], fade)


def test_masked_and_sentinel_flows_contribute_nothing():
    f0, f1 = _frames(2, 4, 3)
    z = np.zeros((1, 2, 4, 2), np.float32)
    fw = z.copy()
    fw[0, 0, 1] = (1e10, 0.0)
    fw[0, 1, 3] = (0.0, np.nan)
    fw[0, 1, 0] = (-np.inf, 0.0)
    vbw = np.ones((1, 2, 4), np.uint8)
    vbw[0, 0, 2] = 0
    ref = R.interpolate(f0, f1, fw, z, [0.5], valid_bw=vbw)
    want = np.full((2, 4), 3)
    want[0, 1] = want[1, 3] = want[1, 0] = 2
    want[0, 2] = 1
    assert np.array_equal(ref["source"][0, 0], want)
    assert ref["cnt"][0, 0, 0, 1].tolist() == [0, 1] and ref["cnt"][0, 0, 0, 2].tolist() == [1, 0]
    assert np.isfinite(ref["value"]).all()


def test_a_match_out_of_frame_gets_the_lowest_weight():
    f0, f1 = _frames(1, 6, 4)
    fw = np.zeros((1, 1, 6, 2), np.float32)
    bw = np.full((1, 1, 6, 2), np.float32(1e10))
    fw[0, 0, 5] = (1.0, 0.0)                                    # q = (6, 0): out of frame; at t = 0.5 half of it stays on x = 5
    f1[0, 0] = f0[0, 0]                                         # every other match is perfect: w = 1
    ref = R.interpolate(f0, f1, fw, bw, [0.5])
    assert abs(ref["den"][0, 0, 0, 5, 0] - 0.5 * math.exp(-10.0)) < 2.0 ** -36
    assert abs(ref["den"][0, 0, 0, 4, 0] - 1.0) < 2.0 ** -36
    assert ref["exp_args"].min() == -10.0 and (ref["exp_args"] == -10.0).sum() == 1


# ---------------------------------------------------------------- an independent scalar loop
def _scalar(frames_0, frames_1, flows_fw, flows_bw, times, alpha, min_range, valid_fw, valid_bw):
    N, H, W, _ = flows_fw.shape
    M = len(times)
    alpha, min_range = float(np.float32(alpha)), float(np.float32(min_range))
    cols = [R.to_double(frames_0), R.to_double(frames_1)]
    acc = np.zeros((N, M, H, W, 2, 5), dtype=object)
    acc[...] = 0
    for k, (flow, valid) in enumerate(((flows_fw, valid_fw), (flows_bw, valid_bw))):
        own, other = cols[k], cols[1 - k]
        for n in range(N):
            for y in range(H):
                for x in range(W):
                    if valid is not None and not valid[n, y, x]:
                        continue
                    u, v = float(flow[n, y, x, 0]), float(flow[n, y, x, 1])
                    if not (abs(u) <= 1e9 and abs(v) <= 1e9):
                        continue
                    qx, qy = x + u, y + v
                    if 0 <= qx <= W - 1 and 0 <= qy <= H - 1:
                        x0, y0 = int(math.floor(qx)), int(math.floor(qy))
                        x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
                        ax, ay = qx - x0, qy - y0
                        e = 0.0
                        for c in range(3):
                            top = (1.0 - ax) * other[n, y0, x0, c] + ax * other[n, y0, x1, c]
                            bot = (1.0 - ax) * other[n, y1, x0, c] + ax * other[n, y1, x1, c]
                            e = e + abs(own[n, y, x, c] - ((1.0 - ay) * top + ay * bot))
                        w = float(np.exp(-min(alpha * (e / 3.0), 10.0)))
                    else:
                        w = float(np.exp(-10.0))
                    for m, t in enumerate(times):
                        s = t if k == 0 else 1.0 - t
                        px, py = x + s * u, y + s * v
                        if not (-1 < px < W and -1 < py < H):
                            continue
                        x0, y0 = int(math.floor(px)), int(math.floor(py))
                        ax, ay = px - x0, py - y0
                        for dy in (0, 1):
                            for dx in (0, 1):
                                cx, cy = x0 + dx, y0 + dy
                                if not (0 <= cx < W and 0 <= cy < H):
                                    continue
                                b = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
                                cell = acc[n, m, cy, cx, k]
                                for c in range(3):
                                    cell[c] += int(np.rint((b * w) * own[n, y, x, c] * 2.0 ** 36))
                                cell[3] += int(np.rint((b * w) * 2.0 ** 36))
                                cell[4] += int(np.rint(b * 2.0 ** 36))
    value = np.zeros((N, M, H, W, 3))
    source = np.zeros((N, M, H, W), np.uint8)
    for n in range(N):
        for m, t in enumerate(times):
            for y in range(H):
                for x in range(W):
                    cov = [acc[n, m, y, x, k][4] * 2.0 ** -36 >= min_range and acc[n, m, y, x, k][3] > 0 for k in range(2)]
                    c = [[float(acc[n, m, y, x, k][j]) / float(acc[n, m, y, x, k][3]) for j in range(3)] if cov[k] else None
                         for k in range(2)]
                    source[n, m, y, x] = cov[0] + 2 * cov[1]
                    for j in range(3):
                        if cov[0] and cov[1]:
                            value[n, m, y, x, j] = (1.0 - t) * c[0][j] + t * c[1][j]
                        elif cov[0] or cov[1]:
                            value[n, m, y, x, j] = c[0][j] if cov[0] else c[1][j]
                        else:
                            value[n, m, y, x, j] = (1.0 - t) * cols[0][n, y, x, j] + t * cols[1][n, y, x, j]
    return value, source


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_a_scalar_loop_agrees_with_the_vectorised_restatement(dtype):
    inp, kw, ref = R.case((2, 13, 19, 3), dtype)
    value, source = _scalar(**inp, times=kw["times"], alpha=R.ALPHA, min_range=R.MIN_RANGE)
    assert np.array_equal(source, ref["source"])
    assert np.array_equal(value, ref["value"])                                # the same IEEE operations: the same bits


# ---------------------------------------------------------------- what the GPU tests rely on
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_the_seeded_inputs_exercise_every_case(dtype):
    inp, kw, ref = R.case((2, 13, 19, 3), dtype)
    share = [float((ref["source"] == code).mean()) for code in range(4)]
    many = float((ref["cnt"] >= 3).any(axis=-1).mean())
    near = float(R.near_threshold(ref).mean())
    print(f"interp seeded (2,13,19,3) {np.dtype(dtype).name}: source shares {share}, >= 3 contributions {many:.3f}, near the "
          f"threshold {near:.4f}")
    assert min(share) >= 0.05 and many >= 0.02 and near <= 0.01


@pytest.mark.parametrize("shape", R.SHAPES)
def test_every_shape_keeps_the_near_threshold_share_small(shape):
    for given in (False, True):
        ref = R.case(shape, np.float32, given_weights=given)[2]
        assert R.near_threshold(ref).mean() <= 0.01
        assert np.isfinite(ref["value"]).all()


# ---------------------------------------------------------------- argument checks, no device
def _cpu_args(N=1, H=3, W=4, dtype=torch.float32):
    return dict(frames_0=torch.zeros((N, H, W, 3), dtype=dtype), frames_1=torch.zeros((N, H, W, 3), dtype=dtype),
                flows_fw=torch.zeros((N, H, W, 2)), flows_bw=torch.zeros((N, H, W, 2)), times=0.5)


@pytest.mark.parametrize("change, exc", [
    (dict(times=[]), ValueError), (dict(times=[0.1] * 17), ValueError), (dict(times=1.5), ValueError),
    (dict(times=[0.5, float("nan")]), ValueError), (dict(times="half"), TypeError), (dict(times=None), TypeError),
    (dict(alpha=-1.0), ValueError), (dict(alpha=float("nan")), ValueError), (dict(min_range=-0.1), ValueError),
    (dict(frames_1=torch.zeros((1, 3, 4, 3), dtype=torch.uint8)), TypeError),
    (dict(frames_0=torch.zeros((1, 3, 4, 3), dtype=torch.float64)), TypeError),
    (dict(frames_0=torch.zeros((1, 3, 4, 4))), ValueError), (dict(frames_1=torch.zeros((1, 3, 5, 3))), ValueError),
    (dict(flows_bw=torch.zeros((1, 3, 5, 2))), ValueError), (dict(flows_fw=torch.zeros((1, 3, 4, 3))), ValueError),
    (dict(flows_fw=torch.zeros((1, 3, 4, 2), dtype=torch.float64)), TypeError),
    (dict(valid_fw=torch.zeros((1, 3, 4))), TypeError), (dict(valid_bw=torch.zeros((1, 3, 5), dtype=torch.bool)), ValueError),
    (dict(weights_fw=torch.zeros((1, 3, 4), dtype=torch.float64)), TypeError),
    (dict(weights_bw=torch.zeros((1, 4, 3))), ValueError),
    (dict(max_workspace_bytes=0), ValueError), (dict(max_workspace_bytes=1.5), ValueError),
])
def test_argument_checks_come_before_the_device(change, exc):
    with pytest.raises(exc):
        IP.interpolate_frames(**dict(_cpu_args(), **change))


def test_the_device_check_comes_last():
    with pytest.raises(ValueError, match="GPU only"):
        IP.interpolate_frames(**_cpu_args())
    with pytest.raises(ValueError, match="GPU only"):
        IP.interpolate_frames(**_cpu_args(dtype=torch.uint8))


def test_plan_slices_cuts_along_n_then_along_m():
    per = IP.workspace_bytes(1, 1, 5, 7)
    assert per == 8 * (5 * 7 * 10 + 1) and IP.workspace_bytes(3, 4, 5, 7) == 8 * (3 * 4 * 5 * 7 * 10 + 1)
    assert IP.plan_slices(3, 4, 5, 7, 1 << 30) == [(0, 3, 0, 4)]
    assert IP.plan_slices(3, 4, 5, 7, IP.workspace_bytes(2, 4, 5, 7)) == [(0, 2, 0, 4), (2, 3, 0, 4)]
    assert IP.plan_slices(2, 4, 5, 7, IP.workspace_bytes(1, 3, 5, 7)) == [(0, 1, 0, 3), (0, 1, 3, 4), (1, 2, 0, 3), (1, 2, 3, 4)]
    assert IP.plan_slices(2, 2, 5, 7, per) == [(0, 1, 0, 1), (0, 1, 1, 2), (1, 2, 0, 1), (1, 2, 1, 2)]
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        IP.plan_slices(2, 2, 5, 7, per - 1)
