"""The training augmentation without a GPU: the float64 reference of tests/augment_ref.py (the yardstick of
tests/test_gpu_augment.py) checked against a closed form that shares no code with its gather, against the crop the host path
forms today, and on sparse labels; pwcnet_amd.augment.draw_params / crop_params; the margins of the GPU test's geometries and
the planted float32 fault at each of them; the library's argument checks (they return before any launch) and train.py's flags.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pwcnet_amd import _lib, augment  # noqa: E402
from tests import augment_ref as R  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _apply(m, x, y):
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


# ---------------------------------------------------------------------------------------------- closed form
CLOSED_FORM = {
    "zoom": dict(zoom=1.4),
    "rotation": dict(deg=23.0),
    "mirror": dict(mirror=True),
    "relative": dict(zoom=1.2, deg=-11.0, mirror=True),
}


@pytest.mark.parametrize("case", sorted(CLOSED_FORM))
def test_affine_flow_in_closed_form(case):
    """For flow(q) = B q + c bilinear sampling is exact, so out_flow(p) = I1 ((I + B) M0 p + c) - p, to 1e-9 px.  The right-hand
    side is 3 x 3 matrix algebra on the records: no gather, no taps, none of the reference's code.  B and c are dyadic, so the
    float32 input field holds the affine field exactly."""
    H, W, OH, OW = 40, 56, 16, 24
    c, pc = ((W - 1) / 2.0, (H - 1) / 2.0), ((OW - 1) / 2.0, (OH - 1) / 2.0)
    m0 = R.similarity(c, pc, shift=(0.8, -0.3), **CLOSED_FORM[case])
    m1 = R.similarity(c, pc, shift=(2.1, 0.9), zoom=1.2 * 1.03, deg=-9.0, mirror=True) if case == "relative" else m0
    B = np.array([[0.03125, -0.015625], [0.0078125, 0.046875]])
    cc = np.array([1.5, -2.25])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flow = np.stack([B[0, 0] * xs + B[0, 1] * ys + cc[0], B[1, 0] * xs + B[1, 1] * ys + cc[1]], axis=-1)[None]
    assert np.array_equal(flow, flow.astype(np.float32).astype(np.float64))
    im = np.zeros((1, H, W, 3), np.uint8)
    got = R.augment(im, im, R.record(m0, m1)[None], (OH, OW), flow.astype(np.float32))
    assert got["valid"].all()                                               # the crop lies inside the frame
    hom = lambda m: np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0.0, 0.0, 1.0]])
    F = np.eye(3)
    F[:2, :2] += B
    F[:2, 2] = cc
    T = np.linalg.inv(hom(m1)) @ F @ hom(m0)                                # p -> p1, in one matrix
    py, px = np.meshgrid(np.arange(OH, dtype=np.float64), np.arange(OW, dtype=np.float64), indexing="ij")
    want = np.stack([T[0, 0] * px + T[0, 1] * py + T[0, 2] - px, T[1, 0] * px + T[1, 1] * py + T[1, 2] - py], axis=-1)[None]
    err = float(np.abs(got["flow"] - want).max())
    print(f"{case}: max |out_flow - closed form| = {err:.3e} px, max |out_flow| = {float(np.abs(want).max()):.2f} px")
    assert err <= 1e-9, (case, err)
    if case == "mirror":
        assert float(np.abs(want[..., 0] + 1.5).max()) > 1.0               # u changes sign under the mirror: not the input field


# ---------------------------------------------------------------------------------------------- the crop of today's path
def test_crop_params_is_the_host_crop():
    """crop_params through the reference: frame[y0:y0 + ch, x0:x0 + cw], float32(v) / 255 for uint8, all 256 values; the flow
    and a sparse mask cut the same way; every bit."""
    rng = np.random.RandomState(3)
    N, H, W, ch, cw = 2, 20, 32, 9, 16
    u8 = np.arange(N * H * W * 3, dtype=np.int64).reshape(N, H, W, 3) * 7 % 256
    u8 = u8.astype(np.uint8)
    assert len(np.unique(u8[:, 3:12, 5:21])) == 256
    f32 = rng.uniform(-3, 3, size=(N, H, W, 3)).astype(np.float32)           # float32 frames pass through whatever their range
    flow = rng.uniform(-5, 5, size=(N, H, W, 2)).astype(np.float32)
    valid = rng.uniform(size=(N, H, W)) >= 0.3
    flow[~valid] = 1e10
    y0, x0 = np.array([3, 11]), np.array([5, 16])
    P = augment.crop_params(N, y0, x0)
    assert np.array_equal(P, np.stack([R.crop_record(3, 5), R.crop_record(11, 16)]))
    sl = lambda a, n: a[n, y0[n]:y0[n] + ch, x0[n]:x0[n] + cw]
    for frames, want in ((u8, u8.astype(np.float32) / 255.0), (f32, f32)):
        got = R.augment(frames, frames[::-1].copy(), P, (ch, cw), flow, valid)
        for n in range(N):
            assert np.array_equal(bits(got["out0"][n]), bits(sl(want, n)))
            assert np.array_equal(bits(got["out1"][n]), bits(sl(want[::-1], n)))
            assert np.array_equal(got["valid"][n], sl(valid, n))
            assert np.array_equal(bits(got["flow"][n]), bits(np.where(sl(valid, n)[..., None], sl(flow, n), 0)))
    assert np.array_equal(augment.crop_params(3, 2, 4), np.stack([R.crop_record(2, 4)] * 3))
    with pytest.raises(ValueError, match="integers"):
        augment.crop_params(1, 0.5, 0)


# ---------------------------------------------------------------------------------------------- draw_params
FULL = dict(scale=(0.9, 1.4), rotate_deg=12.0, translate_frac=0.1, flip=0.5, rel_scale=1.03, rel_rotate_deg=1.5,
            rel_translate_px=2.0, color=True)


@pytest.mark.parametrize("frame,crop", [((436, 1024), (384, 448)), ((96, 128), (64, 96))])
def test_draw_params_keeps_every_crop_inside_both_frames(frame, crop):
    H, W = frame
    ch, cw = crop
    P = augment.draw_params(200, frame, crop, np.random.RandomState(5), **FULL)
    assert P.shape == (200, 32) and P.dtype == np.float64 and np.all(P[:, 30:] == 0)
    assert np.array_equal(P, augment.draw_params(200, frame, crop, np.random.RandomState(5), **FULL))      # the same seed
    assert not np.array_equal(P, augment.draw_params(200, frame, crop, np.random.RandomState(6), **FULL))
    moved = 0
    for rec in P:
        for m in (rec[0:6], rec[6:12]):
            for x in (0.0, cw - 1.0):
                for y in (0.0, ch - 1.0):
                    qx, qy = _apply(m, x, y)
                    assert 0.0 <= qx <= W - 1.0 and 0.0 <= qy <= H - 1.0, (m, x, y, qx, qy)
        # I1 M1 = identity
        A = lambda m: np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0.0, 0.0, 1.0]])
        assert float(np.abs(A(rec[12:18]) @ A(rec[6:12]) - np.eye(3)).max()) <= 1e-12
        moved += int(not np.array_equal(rec[0:6], np.round(rec[0:6])))
        assert 0.79 <= rec[18:21].min() and rec[18:21].max() <= 1.26 and 0.66 <= rec[21] <= 1.51 and rec[27] == rec[21]
    assert moved > 100                                                       # the fall-back is the exception, not the rule


def test_draw_params_switches():
    rng = lambda: np.random.RandomState(1)
    # everything off: the centred crop, the identity colour record
    P = augment.draw_params(4, (96, 128), (64, 96), rng(), flip=0.0, color=False)
    assert np.array_equal(P, augment.crop_params(4, 16, 16))
    # geometry only
    P = augment.draw_params(4, (96, 128), (64, 96), rng(), **{**FULL, "color": False})
    assert np.all(P[:, 18:24] == R.PHOTO_IDENTITY) and np.all(P[:, 24:30] == R.PHOTO_IDENTITY)
    # no relative transform: one map for both frames
    P = augment.draw_params(8, (96, 128), (64, 96), rng(), scale=(0.9, 1.4), rotate_deg=12.0)
    assert np.array_equal(P[:, 0:6], P[:, 6:12]) and not np.array_equal(P[0, 0:6], P[1, 0:6])
    # mirror always: a negative determinant
    P = augment.draw_params(8, (96, 128), (64, 96), rng(), flip=1.0)
    assert np.all(P[:, 0] * P[:, 4] - P[:, 1] * P[:, 3] < 0)
    # a crop with no room to rotate falls back to the centred identity crop after the rejections
    P = augment.draw_params(3, (64, 96), (64, 96), rng(), rotate_deg=30.0, flip=0.0, color=False)
    assert np.array_equal(P, augment.crop_params(3, 0, 0))


def test_draw_params_refusals():
    rng = np.random.RandomState(0)
    with pytest.raises(ValueError, match="larger than the frame"):
        augment.draw_params(1, (64, 96), (65, 96), rng)
    with pytest.raises(ValueError, match="larger than the frame"):
        augment.draw_params(1, (64, 96), (64, 128), rng)
    with pytest.raises(ValueError, match="positive"):
        augment.draw_params(0, (64, 96), (64, 96), rng)
    with pytest.raises(ValueError, match="RandomState"):
        augment.draw_params(1, (64, 96), (64, 96), 7)
    with pytest.raises(ValueError, match="scale"):
        augment.draw_params(1, (64, 96), (64, 96), rng, scale=(1.2, 0.8))
    with pytest.raises(ValueError, match="probability"):
        augment.draw_params(1, (64, 96), (64, 96), rng, flip=1.5)
    with pytest.raises(ValueError, match="non-negative"):
        augment.draw_params(1, (64, 96), (64, 96), rng, rotate_deg=-1.0)


# ---------------------------------------------------------------------------------------------- sparse labels
@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
def test_sparse_labels_never_reach_an_output(nearest):
    """30 % of the labels removed and 1e10 written there: no output exceeds what the labelled input allows, and out_valid is 0
    wherever a tap the sample used was unlabelled (taps and weights recomputed here, pixel by pixel)."""
    g = R.GEOM_IDS.index("2x37x53-16x24-sparse")
    im0, im1, flow, valid = R.inputs(g)
    _, N, (H, W), (OH, OW), _ = R.GEOMETRIES[g]
    P = R.records(g)
    ref = R.reference(g, nearest)
    assert 0.25 < 1.0 - valid.mean() < 0.35 and np.all(flow[~valid] == 1e10)
    # |out_flow| <= |I1| (|q0 - q0'| ...) is bounded by the labelled flow's range carried through the maps: far below 1e3
    assert np.isfinite(ref["flow"]).all() and float(np.abs(ref["flow"]).max()) < 1e3
    assert np.all(ref["flow"][~ref["valid"]] == 0)
    assert 0.05 < ref["valid"].mean() < 0.95
    for n in range(N):
        for y in range(OH):
            for x in range(OW):
                qx, qy = _apply(P[n, 0:6], float(x), float(y))
                assert 0 <= qx <= W - 1 and 0 <= qy <= H - 1
                if nearest:
                    used = [(int(np.floor(qy + 0.5)), int(np.floor(qx + 0.5)))]
                else:
                    x0, y0 = int(np.floor(qx)), int(np.floor(qy))
                    used = [(yy, xx) for yy, wy in ((y0, 1 - (qy - y0)), (y0 + 1, qy - y0)) for xx, wx in ((x0, 1 - (qx - x0)), (x0 + 1, qx - x0))
                            if wy * wx != 0]
                assert bool(ref["valid"][n, y, x]) == all(valid[n, yy, xx] for yy, xx in used), (n, y, x, used)
    # a dense mask of ones is the path without a mask
    dense = R.augment(im0, im1, P, (OH, OW), np.where(valid[..., None], flow, 0).astype(np.float32), None, nearest)
    full = R.augment(im0, im1, P, (OH, OW), np.where(valid[..., None], flow, 0).astype(np.float32), np.ones_like(valid), nearest)
    assert np.array_equal(dense["flow"], full["flow"]) and dense["valid"].all()


# ---------------------------------------------------------------------------------------------- the GPU test's geometries
@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("g", range(len(R.GEOMETRIES)), ids=R.GEOM_IDS)
def test_gpu_geometries_keep_their_margin_and_catch_the_planted_fault(g, nearest):
    """Every geometry of tests/test_gpu_augment.py: the sample coordinates stay MIN_MARGIN away from every decision boundary (so
    out_valid and the nearest taps can be compared exactly), the float64 value rounded once meets the bound, and the same
    arithmetic in float32 misses it somewhere."""
    ref = R.reference(g, nearest)
    name, N, hw, chw, sparse = R.GEOMETRIES[g]
    assert ref["out0"].shape == (N, *chw, 3) and ref["flow"].shape == (N, *chw, 2) and ref["valid"].shape == (N, *chw)
    print(f"{name} {'nearest' if nearest else 'bilinear'}: margin {ref['margin']:.3e} px, valid {ref['valid'].mean():.3f}")
    assert ref["margin"] >= R.MIN_MARGIN
    if "outside" in name:
        assert 0.05 < ref["valid"].mean() < 0.95 and np.all(ref["flow"][~ref["valid"]] == 0)
    elif not sparse:
        assert ref["valid"].all()
    once = {k: ref[k].astype(np.float32) for k in ("out0", "out1", "flow")}
    once["valid"] = ref["valid"]
    good = R.violations(once, ref)
    assert all(c == 0 for c, _ in good.values()), good
    bad32 = R.reference(g, nearest, np.float32)
    bad = R.violations({k: bad32[k] for k in ("out0", "out1", "flow", "valid")}, ref)
    print(f"    float32 arithmetic: " + ", ".join(f"{k} {c} off (worst excess {w:.2e})" for k, (c, w) in bad.items()))
    assert sum(c for c, _ in bad.values()) > 0, bad


def test_uint8_and_float32_frames_hold_the_same_values():
    for g in range(len(R.GEOMETRIES)):
        im0, im1, flow, valid = R.inputs(g)
        a = R.reference(g, False)
        b = R.augment(R.to_float32(im0), R.to_float32(im1), R.records(g), R.GEOMETRIES[g][3], flow, valid)
        assert np.array_equal(a["out0"], b["out0"]) and np.array_equal(a["out1"], b["out1"])


# ---------------------------------------------------------------------------------------------- the library and the wrapper
def test_library_argument_checks_return_before_any_launch():
    L = _lib.lib()
    al = ctypes.c_void_p(4096)          # an aligned non-null address: argument checks only
    f = L.pwc_augment_pairs_f32
    ok = dict(im0=al, im1=al, u8=1, flow=al, valid=al, params=al, out0=al, out1=al, oflow=al, ovalid=al, N=1, H=8, W=8, OH=4, OW=4,
              nearest=0)
    call = lambda **kw: f(*{**ok, **kw}.values(), None)
    for k in ("im0", "im1", "params", "out0", "out1", "oflow", "ovalid"):
        assert call(**{k: None}) == -1, k
    for k in ("N", "H", "W", "OH", "OW"):
        assert call(**{k: 0}) == -1 and call(**{k: -3}) == -1, k
    assert call(im0=ctypes.c_void_p(4098), u8=0) == -2 and call(im1=ctypes.c_void_p(4097), u8=0) == -2
    assert call(out0=ctypes.c_void_p(4098)) == -2 and call(out1=ctypes.c_void_p(4099)) == -2
    assert call(params=ctypes.c_void_p(4100)) == -2
    assert call(flow=ctypes.c_void_p(4100)) == -2 and call(oflow=ctypes.c_void_p(4100)) == -2
    assert call(N=1 << 10, H=1 << 11, W=1 << 10) == -3 and call(N=1 << 10, OH=1 << 11, OW=1 << 10) == -3
    assert call(N=65536) == -3 and call(OH=16 * 65535 + 1, OW=1) == -3


def test_python_layer_rejects_what_the_kernel_cannot_take():
    P = augment.crop_params(1, 0, 0)
    with pytest.raises(ValueError, match="CUDA"):
        augment.augment_pairs(torch.zeros((1, 8, 8, 3)), torch.zeros((1, 8, 8, 3)), P, (4, 4))
    with pytest.raises(ValueError, match="torch tensor"):
        augment.augment_pairs(np.zeros((1, 8, 8, 3), np.float32), np.zeros((1, 8, 8, 3), np.float32), P, (4, 4))


def test_train_cli_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0
    for flag in ("--augment", "--aug_scale", "--aug_rotate", "--aug_translate", "--aug_flip", "--aug_rel_rotate",
                 "--aug_rel_translate", "--aug_seed"):
        assert flag in out.stdout, flag
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "--augment", "heavy"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert bad.returncode == 2 and "--augment" in bad.stderr
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "--augment", "full", "--aug_scale", "1.2",
                          "0.8"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert bad.returncode == 2 and "--aug_scale" in bad.stderr


def test_train_batches_refuse_frames_of_different_sizes():
    sys.path.insert(0, ROOT)
    import train as cli
    a = (np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 2), np.float32), np.ones((8, 8), bool))
    b = (np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9, 2), np.float32), np.ones((8, 9), bool))
    got = list(cli.batches([a, a], [0, 1], 2, same_size=True))
    assert len(got) == 1 and got[0][0].dtype == torch.uint8 and tuple(got[0][0].shape) == (2, 8, 8, 3)
    with pytest.raises(ValueError, match="differ in size"):
        list(cli.batches([a, b], [0, 1], 2, same_size=True))
