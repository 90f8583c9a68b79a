"""The temporal filter without a GPU: the numpy restatement (tests/temporal_ref.py) against tests/track_ref.py's step and against
clips whose result is known by hand, plan_windows, the argument checks of pwcnet_amd.temporal_filter and of the --denoise flags,
and the error codes of the C entry (aligned dummy addresses, nothing is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import temporal as TP  # the feature: without it nothing here can be collected
from tests import temporal_ref as R
from tests import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3
_AL, _MIS = 4096, 4098


# ------------------------------------------------------------------ the restatement
def test_step_equals_track_refs_step():
    """On the flows, masks and queries of the tracker's main case, every point VISIBLE going in: the same status as
    track_ref.step, and where the point comes through VISIBLE the same float32 position, bit for bit -- with and without the check."""
    flows, points, _ = track_ref.main_inputs()
    x, y = points[:, 0].copy(), points[:, 1].copy()
    live = np.ones(x.shape, bool)
    seen = set()
    for t in range(flows["fw"].shape[0]):
        for check in (True, False):
            for F, Fm, G, Gm in ((flows["fw"][t], flows["valid_fw"][t], flows["bw"][t], flows["valid_bw"][t]),
                                 (flows["bw"][t], None, flows["fw"][t], None)):
                G_, Gm_ = (G, Gm) if check else (None, None)
                want = track_ref.step(F, Fm, G_, Gm_, x, y, np.full(x.shape, track_ref.VISIBLE, np.uint8), 0.01, 0.5, True)
                got = R.step(F, Fm, G_, Gm_, x, y, live, 0.01, 0.5)
                assert (got[2] == want[2]).all()
                vis = want[2] == track_ref.VISIBLE
                assert (got[0][vis].view(np.uint32) == want[0][vis].view(np.uint32)).all()
                assert (got[1][vis].view(np.uint32) == want[1][vis].view(np.uint32)).all()
                assert (got[0][~vis].view(np.uint32) == x[~vis].view(np.uint32)).all()
                seen.update(got[2].tolist())
    assert seen == {R.VISIBLE, R.LEFT, R.OCCLUDED, R.UNKNOWN}
    dead = R.step(flows["fw"][0], None, None, None, x, y, ~live, 0.01, 0.5)
    assert (dead[2] == 0).all() and (dead[0].view(np.uint32) == x.view(np.uint32)).all()


def _picture(rs, H, W, C):
    return rs.randint(0, 256, size=(H, W, C)).astype(np.uint8)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("R_,P_", [(1, 0), (2, 1), (3, 2)])
def test_identical_frames_zero_flows_return_the_input(dtype, R_, P_):
    rs = np.random.RandomState(1)
    T, H, W, C = 2 * R_ + 3, 9, 11, 3
    pic = _picture(rs, H, W, C)
    frames = np.repeat(pic[None], T, axis=0)
    if dtype == np.float32:
        frames = (frames.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    zero = np.zeros((T - 1, H, W, 2), np.float32)
    out, sup = R.temporal_filter(frames, zero, zero, radius=R_, patch=P_)
    assert out.dtype == frames.dtype and sup.dtype == np.uint8
    if dtype == np.uint8:
        assert (out == frames).all()
    else:                                                                      # (255 v) / 255 may round: at most one ulp
        assert np.abs(out.astype(np.float64) - frames).max() <= 2.0 ** -24
    assert (sup[R_:T - R_] == 2 * R_).all()
    for i in range(T):
        assert (sup[i] == min(i, R_) + min(T - 1 - i, R_)).all()


@pytest.mark.parametrize("P_", [0, 1])
def test_integer_translations_return_the_input(P_):
    rs = np.random.RandomState(2)
    T, H, W, C, R_ = 5, 12, 16, 1, 2
    dx, dy = 2, -1
    big = _picture(rs, H + 16, W + 16, C)
    frames = np.stack([big[8 - t * dy:8 - t * dy + H, 8 - t * dx:8 - t * dx + W] for t in range(T)])   # frame t (y, x) = frame 0 (y - t dy, x - t dx)
    fw = np.broadcast_to(np.array([dx, dy], np.float32), (T - 1, H, W, 2)).copy()
    out, sup, info = R.temporal_filter(frames, fw, -fw, radius=R_, patch=P_, details=True)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for i in range(T):
        whole = np.ones((H, W), bool)
        for k in range(-min(i, R_), min(T - 1 - i, R_) + 1):
            whole &= (xs + k * dx >= P_) & (xs + k * dx <= W - 1 - P_) & (ys + k * dy >= P_) & (ys + k * dy <= H - 1 - P_)
        assert whole.any()
        assert (sup[i][whole] == min(i, R_) + min(T - 1 - i, R_)).all()
        assert (out[i][whole] == frames[i][whole]).all()
        if P_ == 0:
            assert (out[i] == frames[i]).all()
        w = info["weight"][i]
        assert (w[:, :, whole][info["status"][i][:, :, whole] == R.VISIBLE] == 1.0).all()
    assert (sup < 2 * R_).any()                                                # some walks do leave the frame


def test_one_frame_is_returned():
    rs = np.random.RandomState(3)
    frames = _picture(rs, 6, 7, 3)[None]
    empty = np.zeros((0, 6, 7, 2), np.float32)
    out, sup = R.temporal_filter(frames, empty, empty, radius=2, patch=1)
    assert (out == frames).all() and (sup == 0).all() and sup.shape == (1, 6, 7)


def test_failing_fb_check_gives_the_input_back():
    rs = np.random.RandomState(4)
    T, H, W = 4, 10, 12
    frames = np.stack([_picture(rs, H, W, 3) for _ in range(T)])
    fw = np.full((T - 1, H, W, 2), 1.5, np.float32)
    out, sup, info = R.temporal_filter(frames, fw, fw, radius=2, patch=1, details=True)      # f + b = 2 f: inconsistent everywhere
    assert (out == frames).all() and (sup == 0).all()
    assert set(np.unique(info["status"])) <= {0, R.LEFT, R.OCCLUDED} and (info["status"] == R.OCCLUDED).any()
    out2, sup2, info2 = R.temporal_filter(frames, fw, fw, radius=2, patch=1, fb_check=False, details=True)
    assert (info2["status"] == R.VISIBLE).any() and (sup2 > 0).any() and (out2 != frames).any()
    # the same flows are walked: a frame's first step forwards lands where the flow says
    assert (sup2[0][:H - 3, :W - 3] == 2).all() and (sup2[0][H - 1] == 0).all()


def test_a_sentinel_drops_the_walks_that_touch_its_corners():
    rs = np.random.RandomState(5)
    H, W, y, x = 8, 9, 4, 5
    frames = np.stack([_picture(rs, H, W, 1) for _ in range(2)])
    fw, bw = np.zeros((1, H, W, 2), np.float32), np.zeros((1, H, W, 2), np.float32)
    fw[0, y, x, 1] = R.SENTINEL
    hit = np.zeros((H, W), bool)
    hit[y - 1:y + 1, x - 1:x + 1] = True                                      # the pixels with (y, x) among their four corners
    sup, info = R.temporal_filter(frames, fw, bw, radius=1, patch=0, details=True)[1:]
    assert (sup[0] == np.where(hit, 0, 1)).all() and (sup[1] == np.where(hit, 0, 1)).all()     # frame 1 meets it in the check
    assert (info["status"][0, 0, 0][hit] == R.UNKNOWN).all() and (info["status"][1, 1, 0][hit] == R.UNKNOWN).all()
    sup = R.temporal_filter(frames, fw, bw, radius=1, patch=0, fb_check=False)[1]
    assert (sup[0] == np.where(hit, 0, 1)).all() and (sup[1] == 1).all()
    valid = np.ones((1, H, W), np.uint8)
    valid[0, y, x] = 0
    fw[0, y, x] = np.nan                                                       # a masked corner's flow is not read
    sup = R.temporal_filter(frames, fw, bw, radius=1, patch=0, fb_check=False, valids_fw=valid)[1]
    assert (sup[0] == np.where(hit, 0, 1)).all() and (sup[1] == 1).all()


def test_noise_is_reduced_on_a_static_clip():
    """A static 24 x 40 clip of 5 frames, zero flows, Gaussian noise of sigma = 10 grey levels, R = 2, P = 1: the output is
    closer to the clean clip than the input is.  The ratio is printed (and recorded in DESIGN.md 24), not fixed in advance."""
    rs = np.random.RandomState(7)
    clean = np.stack([R.smooth_field(rs, (24, 40), 80.0, cells=5) + 128.0 for _ in range(3)], axis=-1)
    noisy = np.clip(np.rint(clean[None] + rs.normal(0.0, 10.0, size=(5, 24, 40, 3))), 0, 255).astype(np.uint8)
    zero = np.zeros((4, 24, 40, 2), np.float32)
    out, sup = R.temporal_filter(noisy, zero, zero, radius=2, patch=1, sigma=10.0)
    mse_in = ((noisy.astype(np.float64) - clean[None]) ** 2).mean()
    mse_out = ((out.astype(np.float64) - clean[None]) ** 2).mean()
    print(f"temporal filter, static clip: MSE in {mse_in:.2f}, out {mse_out:.2f}, ratio {mse_out / mse_in:.3f}")
    assert mse_out < mse_in
    assert (sup[2] == 4).all()


# ------------------------------------------------------------------ windows
@pytest.mark.parametrize("T", [1, 2, 5, 17])
@pytest.mark.parametrize("batch", [1, 4, 8])
def test_plan_windows_covers_every_frame_once(T, batch):
    for radius in (1, 2, 8):
        pieces = TP.plan_windows(T, radius, batch)
        assert pieces == R.plan_windows(T, radius, batch)
        produced = [i for _, _, o0, o1 in pieces for i in range(o0, o1)]
        assert produced == list(range(T))
        for cs, ce, o0, o1 in pieces:
            assert 0 < o1 - o0 <= batch
            assert cs == max(o0 - radius, 0) and ce == min(o1 + radius, T)


def test_plan_windows_arguments():
    for bad in (dict(T=0), dict(T=2.0), dict(T=True), dict(radius=0), dict(radius=9), dict(batch=0), dict(batch="4")):
        kw = dict(dict(T=5, radius=2, batch=4), **bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            TP.plan_windows(**kw)


@pytest.mark.parametrize("batch", [1, 3])
def test_pieces_equal_one_call(batch):
    c = R.case(5, 24, 40, 3, np.uint8)
    whole = R.reference(5, 24, 40, 3, np.uint8, 2, 1, True, True, None)
    parts = R.by_pieces(c["frames"], c["fw_s"], c["bw_s"], 2, batch, valids_fw=c["valid_fw"], valids_bw=c["valid_bw"], patch=1)
    assert (parts[0] == whole[0]).all() and (parts[1] == whole[1]).all()


def test_the_main_case_meets_every_status():
    """What the GPU tests rely on: in the main case every outcome of a step occurs, supports from 0 to 2 R occur, and
    max_distance changes the result."""
    ref = R.reference(5, 24, 40, 3, np.uint8, 2, 1, True, True, None)
    assert set(np.unique(ref[2]["status"])) == {0, R.VISIBLE, R.LEFT, R.OCCLUDED, R.UNKNOWN}
    assert set(np.unique(ref[1])) == {0, 1, 2, 3, 4}
    cut = R.reference(5, 24, 40, 3, np.uint8, 2, 1, True, True, 8.0)
    assert (cut[1] < ref[1]).any() and (cut[0] != ref[0]).any()
    nomask = R.reference(5, 24, 40, 3, np.uint8, 2, 1, False, True, None)
    assert (nomask[1] != ref[1]).any()


# ------------------------------------------------------------------ argument checks
def _args(T=3, H=6, W=8, C=3, dtype=torch.uint8):
    return dict(frames=torch.zeros((T, H, W, C), dtype=dtype), flows_fw=torch.zeros((T - 1, H, W, 2)), flows_bw=torch.zeros((T - 1, H, W, 2)))


def test_python_argument_errors_come_before_any_device_work():
    a = _args()
    cases = [
        (TypeError, "frames", dict(frames=a["frames"].to(torch.int32))), (TypeError, "frames", dict(frames=np.zeros((3, 6, 8, 3), np.uint8))),
        (ValueError, "frames", dict(frames=torch.zeros((3, 6, 8, 2), dtype=torch.uint8))), (ValueError, "frames", dict(frames=torch.zeros((3, 6, 8), dtype=torch.uint8))),
        (ValueError, "frames", dict(frames=torch.zeros((0, 6, 8, 3), dtype=torch.uint8))),
        (TypeError, "flows_fw", dict(flows_fw=a["flows_fw"].double())), (TypeError, "flows_fw", dict(flows_fw=None)),
        (ValueError, "flows_fw", dict(flows_fw=torch.zeros((3, 6, 8, 2)))), (ValueError, "flows_fw", dict(flows_fw=torch.zeros((2, 6, 8, 3)))),
        (TypeError, "flows_bw", dict(flows_bw=None)), (ValueError, "flows_bw", dict(flows_bw=torch.zeros((2, 6, 7, 2)))),
        (TypeError, "valids_fw", dict(valids_fw=torch.zeros((2, 6, 8)))), (ValueError, "valids_fw", dict(valids_fw=torch.zeros((3, 6, 8), dtype=torch.bool))),
        (ValueError, "valids_bw", dict(valids_bw=torch.zeros((2, 8, 6), dtype=torch.uint8).permute(0, 2, 1))),
        (ValueError, "radius", dict(radius=0)), (ValueError, "radius", dict(radius=9)), (ValueError, "radius", dict(radius=2.0)), (ValueError, "radius", dict(radius=True)),
        (ValueError, "patch", dict(patch=-1)), (ValueError, "patch", dict(patch=3)), (ValueError, "patch", dict(patch=1.0)),
        (ValueError, "sigma", dict(sigma=0.0)), (ValueError, "sigma", dict(sigma=-1.0)), (ValueError, "sigma", dict(sigma=float("nan"))),
        (ValueError, "sigma", dict(sigma=float("inf"))), (ValueError, "sigma", dict(sigma="10")), (ValueError, "sigma", dict(sigma=1e-200)),
        (ValueError, "max_distance", dict(max_distance=0.0)), (ValueError, "max_distance", dict(max_distance=float("nan"))),
        (ValueError, "max_distance", dict(max_distance=float("inf"))),
        (ValueError, "alpha1", dict(alpha1=-0.1)), (ValueError, "alpha2", dict(alpha2=float("nan"))),
        (ValueError, "out_range", dict(out_range=(1, 1))), (ValueError, "out_range", dict(out_range=(-1, 2))), (ValueError, "out_range", dict(out_range=(0, 4))),
        (ValueError, "out_range", dict(out_range=3)), (ValueError, "out_range", dict(out_range=(0.0, 2.0))),
        (ValueError, "frames: the tensor is on cpu", dict()),                  # the device, last of all
    ]
    for exc, match, change in cases:
        with pytest.raises(exc, match=match):
            TP.temporal_filter(**dict(a, **change))
    one = _args(T=1)
    with pytest.raises(ValueError, match="GPU only"):                          # T = 1 needs no flows
        TP.temporal_filter(one["frames"], None, None)
    with pytest.raises(ValueError, match="flows_fw"):
        TP.temporal_filter(one["frames"], torch.zeros((1, 6, 8, 2)), None)


def test_cli_flag_errors(capsys):
    sys.path.insert(0, ROOT)
    try:
        import infer_continuous as IC
    finally:
        sys.path.remove(ROOT)
    ap = IC.build_parser()
    base = ["-i", "a.png", "b.png"]
    args = ap.parse_args(base)
    assert args.denoise == 0 and TP.check_cli_arguments(ap, args) is None
    args = ap.parse_args(base + ["--denoise", "3", "--denoise_sigma", "4.5", "--denoise_patch", "2", "--denoise_no_fb"])
    assert TP.check_cli_arguments(ap, args) == dict(radius=3, sigma=4.5, patch=2, fb_check=False)
    assert TP.check_cli_arguments(ap, ap.parse_args(base + ["--denoise", "1"])) == dict(radius=1, sigma=10.0, patch=1, fb_check=True)
    for flags, word in ((["--denoise", "9"], "--denoise must"), (["--denoise", "-1"], "--denoise must"),
                        (["--denoise", "1", "--denoise_sigma", "0"], "--denoise_sigma"), (["--denoise_sigma", "nan"], "--denoise_sigma"),
                        (["--denoise", "1", "--denoise_patch", "3"], "--denoise_patch"), (["--denoise_patch", "-1"], "--denoise_patch")):
        with pytest.raises(SystemExit):
            TP.check_cli_arguments(ap, ap.parse_args(base + flags))
        assert word in capsys.readouterr().err


def test_c_abi_surface_and_refusals_that_need_no_launch():
    assert "pwc_temporal.hip" in _lib.SOURCES and "pwc_temporal_filter" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "pwc_hip.h")) as f:
        header = f.read()
    assert "pwc_temporal_filter(" in header and "temporal filter" in header
    assert (_lib.TEMPORAL_MAX_RADIUS, _lib.TEMPORAL_MAX_PATCH, _lib.TEMPORAL_U8, _lib.TEMPORAL_F32) == (8, 2, 0, 1)
    assert "#define PWC_TEMPORAL_MAX_RADIUS 8" in header and "#define PWC_TEMPORAL_MAX_PATCH 2" in header
    assert "PWC_TEMPORAL_U8 = 0, PWC_TEMPORAL_F32 = 1" in header
    lib = _lib.lib()
    p = lambda v: None if v is None else ctypes.c_void_p(v)                    # noqa: E731

    def call(**change):
        a = dict(frames=_AL, dtype=0, C=3, fw=_AL, fw_cs=2, bw=_AL, bw_cs=2, vfw=None, vbw=None, T=5, H=8, W=8, R=2, P=1, sigma=10.0,
                 md=0.0, fb=1, a1=0.01, a2=0.5, i0=0, i1=5, out=_AL, support=_AL)
        a.update(change)
        return lib.pwc_temporal_filter(p(a["frames"]), a["dtype"], a["C"], p(a["fw"]), a["fw_cs"], p(a["bw"]), a["bw_cs"], p(a["vfw"]),
                                       p(a["vbw"]), a["T"], a["H"], a["W"], a["R"], a["P"], a["sigma"], a["md"], a["fb"], a["a1"], a["a2"],
                                       a["i0"], a["i1"], p(a["out"]), p(a["support"]), None)

    nan, inf = float("nan"), float("inf")
    refused = [(EINVAL, dict(frames=None)), (EINVAL, dict(out=None)), (EINVAL, dict(support=None)), (EINVAL, dict(fw=None)), (EINVAL, dict(bw=None)),
               (EINVAL, dict(T=0)), (EINVAL, dict(H=0)), (EINVAL, dict(W=-1)), (EINVAL, dict(fw_cs=1)), (EINVAL, dict(bw_cs=0)),
               (EINVAL, dict(dtype=2)), (EINVAL, dict(C=2)), (EINVAL, dict(C=4)), (EINVAL, dict(C=0)),
               (EINVAL, dict(R=0)), (EINVAL, dict(R=9)), (EINVAL, dict(P=-1)), (EINVAL, dict(P=3)),
               (EINVAL, dict(sigma=0.0)), (EINVAL, dict(sigma=-2.0)), (EINVAL, dict(sigma=nan)), (EINVAL, dict(sigma=inf)),
               (EINVAL, dict(sigma=1e-200)), (EINVAL, dict(sigma=1e200)), (EINVAL, dict(md=nan)),
               (EINVAL, dict(a1=-1.0)), (EINVAL, dict(a2=nan)),
               (EINVAL, dict(i0=-1)), (EINVAL, dict(i1=6)), (EINVAL, dict(i0=2, i1=2)), (EINVAL, dict(i0=3, i1=2)),
               (EINVAL, dict(T=1, fw=None, bw=None, i1=2)),
               (ERANGE, dict(H=1 << 15, W=1 << 16)), (ERANGE, dict(H=(1 << 24) + 1, W=1)), (ERANGE, dict(H=1, W=(1 << 24) + 1)),
               (ERANGE, dict(T=65536, i1=1)), (ERANGE, dict(H=8 * 65535 + 1, W=1)),
               (EINVAL, dict(H=1 << 15, W=1 << 16, R=0)),                                         # EINVAL comes before ERANGE
               (ERANGE, dict(H=1 << 15, W=1 << 16, fw=_MIS)),                                     # ERANGE before EALIGN
               (EALIGN, dict(fw=_MIS)), (EALIGN, dict(bw=_MIS)), (EALIGN, dict(dtype=1, frames=_MIS)), (EALIGN, dict(dtype=1, out=_MIS))]
    for code, change in refused:
        assert call(**change) == code, change
