"""The background plate without a GPU: the numpy restatement (tests/plate_ref.py) against clips whose result is known by hand, the
host helpers plate_path, plate_canvas and canvas_matrices against their definitions and against known pans, the argument checks
of every Python entry point and of the --plate flags, and the error codes of the C entries (dummy addresses, nothing is launched)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import plate as PL  # the feature: without it nothing here can be collected
from tests import plate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3
_AL, _MIS = 4096, 4098
EYE = np.eye(3)


def shift(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def square_clip(dtype=np.uint8, T=5, H=12, W=16):
    """A constant background of 100 (three channels 100, 110, 120) and a 3 x 3 square of 250 that sits elsewhere in every frame."""
    frames = np.empty((T, H, W, 3), np.float64)
    frames[...] = (100.0, 110.0, 120.0)
    where = []
    for t in range(T):
        y, x = 1 + 2 * t, 2 + 3 * (t % 4)
        frames[t, y:y + 3, x:x + 3] = 250.0
        where.append((y, x))
    if np.dtype(dtype) == np.float32:
        return (frames / 255.0).astype(np.float32), where
    return frames.astype(np.uint8), where


# ------------------------------------------------------------------ the restatement against hand-made truths
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_the_median_votes_the_square_out_and_the_mean_does_not(dtype):
    frames, _ = square_clip(dtype)
    mats = np.tile(EYE, (5, 1, 1))
    plate, count = R.plate_build(frames, mats, (12, 16), R.MEDIAN)
    assert (count == 5).all() and (plate == frames[0, 0, 15]).all()        # the background, exactly
    mean, count = R.plate_build(frames, mats, (12, 16), R.MEAN)
    assert (count == 5).all() and (mean != frames[0, 0, 15]).any() and (mean[0, 15] == frames[0, 0, 15]).all()
    if dtype == np.uint8:
        assert (mean[1, 2] == (130, 138, 146)).all()                       # (4 x 100 + 250) / 5 = 130, ...


def test_an_even_count_picks_the_lower_middle_value():
    frames = np.array([40, 10, 30, 20], np.uint8).reshape(4, 1, 1, 1)
    mats = np.tile(EYE, (4, 1, 1))
    plate, count = R.plate_build(frames, mats, (1, 1), R.MEDIAN)
    assert count[0, 0] == 4 and plate[0, 0, 0] == 20
    assert R.plate_build(frames[:2], mats[:2], (1, 1), R.MEDIAN)[0][0, 0, 0] == 10
    assert R.plate_build(frames[:3], mats[:3], (1, 1), R.MEDIAN)[0][0, 0, 0] == 30
    assert R.plate_build(frames, mats, (1, 1), R.MEAN)[0][0, 0, 0] == 25
    f = np.array([0.0, -0.0, 1.0, -1.0], np.float32).reshape(4, 1, 1, 1)
    got = R.plate_build(f, mats, (1, 1), R.MEDIAN)[0]
    assert got.view(np.uint32)[0, 0, 0] == 0x80000000                      # -1 < -0 < +0 < 1: the lower middle one is -0
    assert R.plate_build(f[[0, 1]], mats[:2], (1, 1), R.MEDIAN)[0].view(np.uint32)[0, 0, 0] == 0x80000000
    # mean of 0.1 three times: ((0 + a) + a) + a in double, / 3, rounded once
    a = np.full((3, 1, 1, 1), 0.1, np.float32)
    want = np.float32(((0.0 + float(a[0, 0, 0, 0])) + float(a[0, 0, 0, 0]) + float(a[0, 0, 0, 0])) / 3.0)
    assert R.plate_build(a, mats[:3], (1, 1), R.MEAN)[0][0, 0, 0] == want


def test_integer_translations_paste_the_union():
    rs = np.random.RandomState(0)
    H, W, Hc, Wc = 6, 8, 9, 14
    scene = rs.randint(0, 256, size=(Hc, Wc, 3)).astype(np.uint8)
    offsets = [(0, 0), (3, 2), (6, 3), (1, 1)]                               # where each frame's corner sits on the canvas (x, y)
    frames = np.stack([scene[oy:oy + H, ox:ox + W] for ox, oy in offsets])
    mats = np.stack([shift(-ox, -oy) for ox, oy in offsets])                 # canvas -> frame
    overlap = np.zeros((Hc, Wc), np.uint8)
    for ox, oy in offsets:
        overlap[oy:oy + H, ox:ox + W] += 1
    for mode in (R.MEDIAN, R.MEAN):
        plate, count = R.plate_build(frames, mats, (Hc, Wc), mode)
        assert (count == overlap).all()
        assert (plate[overlap > 0] == scene[overlap > 0]).all() and (plate[overlap == 0] == 0).all()
    assert overlap.min() == 0 and overlap.max() == 4


def test_masks_use_and_min_count_remove_what_they_should():
    frames, _ = square_clip()
    mats = np.tile(EYE, (5, 1, 1))
    use = np.array([1, 0, 1, 1, 0], np.uint8)
    plate, count = R.plate_build(frames, mats, (12, 16), R.MEAN, use=use)
    want, _ = R.plate_build(frames[[0, 2, 3]], mats[:3], (12, 16), R.MEAN)
    assert (count == 3).all() and (plate == want).all()
    masks = np.ones((5, 12, 16), np.uint8)
    masks[0, 4, 5] = 0                                                     # the samples whose corners touch (5, 4): x in 4..5, y in 3..4 ...
    masks[1] = 0
    plate, count = R.plate_build(frames, mats, (12, 16), R.MEDIAN, masks=masks)
    lost = np.zeros((12, 16), bool)
    lost[3:5, 4:6] = True                                                  # ... since the corners of pixel (x, y) are x..x+1, y..y+1
    assert (count[lost] == 3).all() and (count[~lost] == 4).all()
    plate, count = R.plate_build(frames, mats, (12, 16), R.MEDIAN, masks=masks, min_count=4)
    assert (count[lost] == 3).all() and (plate[lost] == 0).all() and (plate[~lost] != 0).all()
    plate, count = R.plate_build(frames, mats, (12, 16), R.MEDIAN, use=np.zeros(5, np.uint8))
    assert (count == 0).all() and (plate == 0).all()


def test_a_broken_matrix_removes_that_frame_only():
    frames, _ = square_clip()
    good = np.tile(EYE, (5, 1, 1))
    want = R.plate_build(frames[[0, 2, 4]], good[:3], (12, 16), R.MEAN)
    for bad in (np.nan, np.inf):
        mats = good.copy()
        mats[1, 0, 2] = bad
        mats[3, 2, 0] = 1e-9                                               # last row not exactly 0 0 1
        got = R.plate_build(frames, mats, (12, 16), R.MEAN)
        assert (got[0] == want[0]).all() and (got[1] == 3).all()
    assert not R.affine_finite(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 2.0]])) and R.affine_finite(EYE)


def test_an_inf_loses_exactly_the_samples_that_touch_it():
    frames, _ = square_clip(np.float32)
    frames[2, 6, 9, 1] = np.inf
    mats = np.tile(EYE, (5, 1, 1))
    mats[2] = shift(0.5, 0.0)                                              # frame 2 is read half a pixel to the right
    plate, count = R.plate_build(frames, mats, (12, 16), R.MEDIAN)
    lost = np.zeros((12, 16), bool)
    lost[5:7, 8:10] = True                                                 # x + 0.5 has the corners x, x + 1; y has y, y + 1
    lost[:, 15] = True                                                     # 15.5 is outside the frame
    assert (count[lost] == 4).all() and (count[~lost] == 5).all() and np.isfinite(plate).all()
    diff, fg, known = R.plate_difference(frames, plate, count, np.tile(EYE, (5, 1, 1)), 0.1)
    assert not known[2, 6, 9] and known[2, 6, 8] and known.sum() == known.size - 1


# ------------------------------------------------------------------ the difference
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_difference_of_the_frames_that_built_the_plate(dtype):
    frames, where = square_clip(dtype)
    one = frames[:1]
    plate, count = R.plate_build(one, EYE[None], (12, 16), R.MEDIAN)
    diff, fg, known = R.plate_difference(one, plate, count, EYE[None], 0.0)
    assert known.all() and (diff == 0).all() and not fg.any()
    mats = np.tile(EYE, (5, 1, 1))
    plate, count = R.plate_build(frames, mats, (12, 16), R.MEDIAN)
    threshold = 10.0 if dtype == np.uint8 else 10.0 / 255.0
    diff, fg, known = R.plate_difference(frames, plate, count, mats, threshold)
    want = np.zeros((5, 12, 16), bool)
    for t, (y, x) in enumerate(where):
        want[t, y:y + 3, x:x + 3] = True
    assert known.all() and (fg == want).all()
    assert diff.max() == np.float32(150.0 if dtype == np.uint8 else float(frames.max()) - float(plate[0, 0, 0]))
    # unknown: a shifted frame looks beyond the canvas; min_count above the count
    diff, fg, known = R.plate_difference(frames, plate, count, np.tile(shift(2.0, 0.0), (5, 1, 1)), threshold)
    assert not known[:, :, 14:].any() and known[:, :, :14].all() and (diff[:, :, 14:] == 0).all()
    assert not R.plate_difference(frames, plate, count, mats, threshold, min_count=6)[2].any()


# ------------------------------------------------------------------ the host helpers
def _motions(rs, T):
    out = []
    for _ in range(T):
        ang, sc = np.deg2rad(rs.uniform(-2, 2)), rs.uniform(0.97, 1.03)
        out.append(np.array([[sc * np.cos(ang), -sc * np.sin(ang), rs.uniform(-5, 5)],
                             [sc * np.sin(ang), sc * np.cos(ang), rs.uniform(-5, 5)], [0.0, 0.0, 1.0]]))
    return np.stack(out)


def test_plate_path_rebased_and_cut():
    M = _motions(np.random.RandomState(2), 7)
    base, reach = PL.plate_path(M)
    want, want_reach = R.plate_path(M)
    assert reach.all() and (base == want).all() and (base[0] == EYE).all() and base.shape == (8, 3, 3) and base.dtype == np.float64
    assert np.allclose(base[3], M[2] @ M[1] @ M[0], rtol=1e-14, atol=0)
    mid, reach = PL.plate_path(torch.from_numpy(M), anchor=4)
    assert reach.all() and (mid[4] == EYE).all() and (mid == R.plate_path(M, anchor=4)[0]).all()
    rebased = base @ np.linalg.inv(base[4])                                # to_frame[t] seen from frame 4
    scale = np.abs(rebased).max(axis=(1, 2), keepdims=True)
    assert (np.abs(mid - rebased) <= 1e-12 * scale).all()
    ok = np.ones(7, bool)
    ok[5] = False                                                          # between frames 5 and 6
    cut, reach = PL.plate_path(M, ok, anchor=2)
    assert reach.tolist() == [True] * 6 + [False] * 2 and (cut[6:] == EYE).all() and (cut[:6] == R.plate_path(M, ok, 2)[0][:6]).all()
    assert (cut[:6] == PL.plate_path(M, anchor=2)[0][:6]).all()            # the left side is untouched
    ok[0] = False
    reach = PL.plate_path(M, torch.from_numpy(ok), anchor=2)[1]
    assert reach.tolist() == [False] + [True] * 5 + [False] * 2
    assert PL.plate_path(M, ok, anchor=0)[1].tolist() == [True] + [False] * 7
    nan = M.copy()
    nan[3, 0, 0] = np.nan
    assert PL.plate_path(nan)[1].tolist() == [True] * 4 + [False] * 4
    assert PL.plate_path(np.zeros((0, 3, 3)))[1].tolist() == [True]


def test_plate_canvas_on_known_pans():
    H, W = 48, 64
    pan = np.tile(shift(-3.0, 0.0), (6, 1, 1))                             # the content moves 3 px left per frame: the camera pans right
    to_frame, reach = PL.plate_path(pan)
    assert PL.plate_canvas(to_frame, reach, H, W) == (0, 0, 48, 64 + 18) == R.plate_canvas(to_frame, reach, H, W)
    assert PL.plate_canvas(to_frame, reach, H, W, margin=2) == (-2, -2, 52, 86)
    to_frame, reach = PL.plate_path(pan, anchor=3)
    assert PL.plate_canvas(to_frame, reach, H, W) == (-9, 0, 48, 82)
    reach[5:] = False
    assert PL.plate_canvas(to_frame, reach, H, W) == (-9, 0, 48, 64 + 12)
    diag = np.tile(shift(1.5, -2.25), (2, 1, 1))
    to_frame, reach = PL.plate_path(diag)
    assert PL.plate_canvas(to_frame, reach, H, W) == (-3, 0, 48 + 5, 64 + 3) == R.plate_canvas(to_frame, reach, H, W)
    with pytest.raises(ValueError, match=r"48 x 82 .* max_side = 80"):
        PL.plate_canvas(*PL.plate_path(pan), H, W, max_side=80)
    with pytest.raises(ValueError, match="no frame is reachable"):
        PL.plate_canvas(to_frame, np.zeros(3, bool), H, W)


def test_canvas_matrices_and_a_panned_plate():
    """The helpers end to end on the restatement: frames cut from one scene by a pan give back the scene."""
    rs = np.random.RandomState(3)
    H, W = 10, 12
    scene = rs.randint(0, 256, size=(H, W + 15, 3)).astype(np.uint8)
    frames = np.stack([scene[:, 3 * i:3 * i + W] for i in range(6)])
    to_frame, reach = PL.plate_path(np.tile(shift(-3.0, 0.0), (5, 1, 1)), anchor=2)
    x0, y0, Hc, Wc = PL.plate_canvas(to_frame, reach, H, W)
    assert (x0, y0, Hc, Wc) == (-6, 0, H, W + 15)
    mats, back = PL.canvas_matrices(to_frame, x0, y0)
    rm, rb = R.canvas_matrices(to_frame, x0, y0)
    assert (mats == rm).all() and (back == rb).all() and (mats[:, 2] == (0, 0, 1)).all() and (back[:, 2] == (0, 0, 1)).all()
    assert (mats[0] == shift(0.0, 0.0)).all() and (mats[5] == shift(-15.0, 0.0)).all() and (back[5] == shift(15.0, 0.0)).all()
    plate, count = R.plate_build(frames, mats, (Hc, Wc))
    assert (plate == scene).all() and count.min() == 1 and count.max() == 4
    diff, fg, known = R.plate_difference(frames, plate, count, back, 0.0)
    assert known.all() and not fg.any()
    singular = to_frame.copy()
    singular[1] = [[1, 2, 0], [2, 4, 0], [0, 0, 1]]
    assert np.isnan(PL.canvas_matrices(singular, 0, 0)[1][1, :2]).all()
    assert PL.select_frames(reach, 2, 64) == [0, 1, 2, 3, 4, 5] and PL.select_frames(reach, 2, 3) == [0, 2, 5]
    picked = PL.select_frames(np.ones(100, bool), 37, 32)
    assert len(picked) == 32 and 37 in picked and picked == sorted(set(picked)) and picked[0] == 0 and picked[-1] == 99


# ------------------------------------------------------------------ argument checks
def test_host_helper_argument_errors():
    M = np.tile(EYE, (3, 1, 1))
    with pytest.raises(ValueError, match=r"matrices: expected shape \(T, 3, 3\)"):
        PL.plate_path(np.zeros((3, 2, 3)))
    with pytest.raises(ValueError, match="ok: expected shape"):
        PL.plate_path(M, np.ones(4, bool))
    for anchor in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match="anchor: expected an integer in 0 .. 3"):
            PL.plate_path(M, anchor=anchor)
    P, reach = PL.plate_path(M)
    with pytest.raises(ValueError, match="reach: expected shape"):
        PL.plate_canvas(P, reach[:2], 4, 4)
    with pytest.raises(ValueError, match=r"to_frame: expected shape \(T, 3, 3\)"):
        PL.plate_canvas(P[0], reach, 4, 4)
    for kw, what in ((dict(H=0, W=4), "H"), (dict(H=4, W=0), "W"), (dict(H=4, W=4, margin=-1), "margin"),
                     (dict(H=4, W=4, max_side=0), "max_side")):
        with pytest.raises(ValueError, match=f"{what}: expected an integer"):
            PL.plate_canvas(P, reach, **kw)
    with pytest.raises(ValueError, match="x0: expected a finite number"):
        PL.canvas_matrices(P, float("nan"), 0)
    with pytest.raises(ValueError, match="y0: expected a finite number"):
        PL.canvas_matrices(P, 0, None)


def test_background_plate_argument_errors():
    f = torch.zeros((3, 4, 5, 3), dtype=torch.uint8)
    M = np.tile(EYE, (3, 1, 1))
    with pytest.raises(TypeError, match="frames: expected a torch.uint8 or torch.float32 tensor"):
        PL.background_plate(f.double(), M, (4, 5))
    with pytest.raises(TypeError, match="frames: expected a torch.uint8 or torch.float32 tensor"):
        PL.background_plate(f.numpy(), M, (4, 5))
    for bad in (torch.zeros((4, 5, 3), dtype=torch.uint8), torch.zeros((3, 4, 5, 5), dtype=torch.uint8), torch.zeros((3, 0, 5, 3))):
        with pytest.raises(ValueError, match=r"frames: expected a \(T, H, W, C\) tensor with 1 to 4 channels"):
            PL.background_plate(bad, M, (4, 5))
    with pytest.raises(ValueError, match="frames: expected at most 64 frames, got 65"):
        PL.background_plate(torch.zeros((65, 1, 1, 1)), np.tile(EYE, (65, 1, 1)), (1, 1))
    with pytest.raises(TypeError, match="matrices: expected a float64 array"):
        PL.background_plate(f, M.astype(np.float32), (4, 5))
    with pytest.raises(ValueError, match=r"matrices: expected shape \(3, 3, 3\)"):
        PL.background_plate(f, M[:2], (4, 5))
    with pytest.raises(TypeError, match="matrices: expected a torch.float64 tensor"):
        PL.background_plate(f, torch.from_numpy(M).float(), (4, 5))
    for canvas in (5, (4, 5, 6), "ab"):
        with pytest.raises(ValueError, match="canvas: expected"):
            PL.background_plate(f, M, canvas)
    for canvas in ((0, 5), (4, 2.0), (4, -1)):
        with pytest.raises(ValueError, match="canvas: expected an integer"):
            PL.background_plate(f, M, canvas)
    with pytest.raises(ValueError, match=r"mode: expected one of \['mean', 'median'\]"):
        PL.background_plate(f, M, (4, 5), mode="mode")
    for use in (np.ones(2, bool), np.ones(3, np.float32), np.ones((3, 1), bool)):
        with pytest.raises(ValueError, match="use: expected 3 booleans"):
            PL.background_plate(f, M, (4, 5), use=use)
    with pytest.raises(TypeError, match="masks: expected a torch.bool or torch.uint8 tensor"):
        PL.background_plate(f, M, (4, 5), masks=torch.ones((3, 4, 5)))
    with pytest.raises(ValueError, match="masks: expected shape"):
        PL.background_plate(f, M, (4, 5), masks=torch.ones((3, 4, 4), dtype=torch.bool))
    for mc in (0, 256, 1.0, True):
        with pytest.raises(ValueError, match="min_count: expected an integer in 1 .. 255"):
            PL.background_plate(f, M, (4, 5), min_count=mc)
    with pytest.raises(ValueError, match="frames: the tensor is on cpu"):
        PL.background_plate(f, M, (4, 5))


def test_plate_difference_argument_errors():
    f = torch.zeros((3, 4, 5, 3), dtype=torch.uint8)
    plate, count = torch.zeros((6, 7, 3), dtype=torch.uint8), torch.zeros((6, 7), dtype=torch.uint8)
    M = np.tile(EYE, (3, 1, 1))
    with pytest.raises(TypeError, match="frames: expected a torch.uint8 or torch.float32 tensor"):
        PL.plate_difference(f.int(), plate, count, M, 1.0)
    with pytest.raises(TypeError, match="plate: expected a torch.uint8 tensor, the frames' dtype"):
        PL.plate_difference(f, plate.float(), count, M, 1.0)
    for bad in (plate[..., :2], plate[0], plate[:0]):
        with pytest.raises(ValueError, match=r"plate: expected an \(Hc, Wc, 3\) tensor"):
            PL.plate_difference(f, bad, count, M, 1.0)
    with pytest.raises(TypeError, match="count: expected a torch.uint8 tensor"):
        PL.plate_difference(f, plate, count.bool(), M, 1.0)
    with pytest.raises(ValueError, match=r"count: expected shape \(6, 7\)"):
        PL.plate_difference(f, plate, count[:5], M, 1.0)
    with pytest.raises(ValueError, match=r"matrices: expected shape \(3, 3, 3\)"):
        PL.plate_difference(f, plate, count, M[:1], 1.0)
    for thr in (-1.0, float("nan"), None, True):
        with pytest.raises(ValueError, match="threshold: expected a non-negative number"):
            PL.plate_difference(f, plate, count, M, thr)
    with pytest.raises(ValueError, match="min_count: expected an integer in 1 .. 255"):
        PL.plate_difference(f, plate, count, M, 1.0, min_count=0)
    with pytest.raises(ValueError, match="frames: the tensor is on cpu"):
        PL.plate_difference(f, plate, count, M, 1.0)


def test_package_exports_and_constants():
    import pwcnet_amd
    for name in ("plate_path", "plate_canvas", "canvas_matrices", "background_plate", "plate_difference"):
        assert getattr(pwcnet_amd, name) is getattr(PL, name) and name in pwcnet_amd.__all__
    assert (_lib.PLATE_MEDIAN, _lib.PLATE_MEAN, _lib.PLATE_MAX_FRAMES) == (0, 1, 64) and "pwc_plate.hip" in _lib.SOURCES
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert "enum { PWC_PLATE_MEDIAN = 0, PWC_PLATE_MEAN = 1 };" in header and "#define PWC_PLATE_MAX_FRAMES 64" in header


# ------------------------------------------------------------------ the C entries' checks (nothing is launched)
def test_c_abi_error_codes_without_a_gpu():
    L = _lib.lib()
    U8, F32 = _lib.MOTION_U8, _lib.MOTION_F32

    def build(frames=_AL, dtype=U8, C=3, matrices=_AL, T=2, H=4, W=5, Hc=6, Wc=7, mode=0, min_count=1, plate=_AL, count=_AL):
        return L.pwc_plate_build(frames, dtype, C, matrices, None, None, T, H, W, Hc, Wc, mode, min_count, plate, count, None)

    def diff(frames=_AL, dtype=U8, C=3, plate=_AL, count=_AL, matrices=_AL, T=2, H=4, W=5, Hc=6, Wc=7, min_count=1, threshold=1.0,
             difference=_AL, foreground=_AL, known=_AL):
        return L.pwc_plate_difference(frames, dtype, C, plate, count, matrices, T, H, W, Hc, Wc, min_count, threshold, difference,
                                      foreground, known, None)

    for kw in (dict(frames=None), dict(matrices=None), dict(plate=None), dict(count=None), dict(T=0), dict(H=0), dict(W=-1), dict(Hc=0),
               dict(Wc=0), dict(T=65), dict(C=0), dict(C=5), dict(dtype=2), dict(mode=2), dict(min_count=0),
               dict(T=65, H=1 << 16, W=1 << 15), dict(mode=3, matrices=_MIS)):      # EINVAL wins over ERANGE and EALIGN
        assert build(**kw) == EINVAL, kw
    for kw in (dict(frames=None), dict(plate=None), dict(count=None), dict(matrices=None), dict(difference=None), dict(foreground=None),
               dict(known=None), dict(T=0), dict(H=0), dict(W=0), dict(Hc=-3), dict(Wc=0), dict(C=0), dict(C=5), dict(dtype=7),
               dict(min_count=0), dict(threshold=-0.5), dict(threshold=float("nan")), dict(threshold=-1.0, T=1 << 20)):
        assert diff(**kw) == EINVAL, kw
    edge = dict(H=46340, W=46340)                                          # 2147395600 <= 2^31 - 65537 = 2147418111: in range
    assert build(H=1 << 16, W=1 << 15) == ERANGE and build(Hc=1 << 16, Wc=1 << 15) == ERANGE
    assert build(H=46341, W=46341, matrices=_MIS) == ERANGE                # 2147488281 is above; ERANGE wins over EALIGN
    assert build(matrices=_MIS, **edge) == EALIGN                          # ... and this size passed the range check
    assert diff(H=1 << 16, W=1 << 15) == ERANGE and diff(Hc=1 << 16, Wc=1 << 15) == ERANGE and diff(T=65536) == ERANGE
    assert diff(T=65536, matrices=_MIS) == ERANGE
    assert build(matrices=_AL + 4) == EALIGN and diff(matrices=_AL + 4) == EALIGN
    assert build(dtype=F32, frames=_MIS) == EALIGN and build(dtype=F32, plate=_MIS) == EALIGN
    assert diff(dtype=F32, frames=_MIS) == EALIGN and diff(dtype=F32, plate=_MIS) == EALIGN and diff(difference=_MIS) == EALIGN


# ------------------------------------------------------------------ the command line
def _cli(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", "a.png", "b.png", *flags],
                          capture_output=True, text=True, timeout=120)


def test_cli_flag_rules():
    import infer_continuous
    args = infer_continuous.build_parser().parse_args(["-i", "a.png", "b.png"])
    assert args.plate is False and args.plate_mode == "median" and args.plate_anchor == 0 and args.plate_frames == 32
    assert args.plate_margin == 0 and args.plate_max_side == 4096 and args.plate_inliers is False and args.plate_foreground is None
    for flags, message in ((["--plate"], "--plate needs --motion MODEL"),
                           (["--plate", "--motion", "affine", "--plate_anchor", "2"], "--plate_anchor must be a frame of the sequence, 0 .. 1"),
                           (["--plate", "--motion", "affine", "--plate_frames", "65"], "--plate_frames must be in 1 .. 64"),
                           (["--plate", "--motion", "affine", "--plate_frames", "0"], "--plate_frames must be in 1 .. 64"),
                           (["--plate", "--motion", "affine", "--plate_margin", "-1"], "--plate_margin must be at least 0"),
                           (["--plate", "--motion", "affine", "--plate_max_side", "0"], "--plate_max_side must be at least 1"),
                           (["--plate", "--motion", "affine", "--plate_foreground", "-1"], "--plate_foreground must be non-negative"),
                           (["--plate", "--motion", "affine", "--plate_mode", "mode"], "invalid choice")):
        run = _cli(*flags)
        assert run.returncode == 2 and message in run.stderr, (flags, run.stderr[-500:])
    doc = infer_continuous.__doc__
    for flag in ("--plate ", "--plate_mode", "--plate_anchor", "--plate_frames", "--plate_margin", "--plate_max_side", "--plate_inliers",
                 "--plate_foreground"):
        assert flag in doc
