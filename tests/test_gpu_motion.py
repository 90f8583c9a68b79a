"""Dominant motion on the GPU (pwc_motion.hip, pwcnet_amd.motion, infer_continuous.py --motion) against the numpy restatement of
tests/motion_ref.py (checked on the CPU by tests/test_host_motion.py).

The kernels' operations are IEEE double + - x /, floor, rint and comparisons in a fixed order, with no fused multiply-add and no
library function, and the restatement performs the same operations in the same order -- the partition, the tree and the part
order of the sums included: the yardstick is BIT EQUALITY of matrices, ok, count, weight_sum, residual, inlier, the warped frames
and covered, no tolerance.  It rests on the device's double division being correctly rounded.  Every case prints its figures
before it asserts (profiles/motion_gpu_test_figures.txt)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import motion as MO  # the feature: without it nothing here can be collected
from tests import motion_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3
SHAPES = ((1, 1), (1, 19), (13, 19), (16, 16), (17, 16), (260, 256))


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.fit_motion is MO.fit_motion
    return pwcnet_amd


def _up(a):
    return a if a is None or not isinstance(a, np.ndarray) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _fit(P, flows, valid=None, **kw):
    m, ok, info = P.fit_motion(_up(flows), _up(valid), **kw)
    assert m.dtype == torch.float64 and ok.dtype == torch.bool and info["count"].dtype == torch.int32
    return dict(matrices=m.cpu().numpy(), ok=ok.cpu().numpy(), count=info["count"].cpu().numpy(),
                weight_sum=info["weight_sum"].cpu().numpy())


def _same(tag, got, want, keys=("matrices", "ok", "count", "weight_sum")):
    diff = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in keys}
    print(f"motion {tag}: ok {want['ok'].astype(int).tolist()} count {want['count'].tolist()} elements that differ {diff}")
    for k in keys:
        assert got[k].shape == want[k].shape and np.array_equal(_bits(got[k]), _bits(want[k])), (tag, k)


@pytest.fixture(scope="module")
def scenes():
    """The flows and masks of every shape, made once: two images per shape, a mask that drops a fifth of the pixels."""
    out = {}
    for k, (H, W) in enumerate(SHAPES):
        flows = R.batch(H, W, N=2, seed=10 * k)
        valid = np.random.RandomState(k).uniform(size=(2, H, W)) > 0.2
        out[(H, W)] = (flows, valid)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("model", R.MODELS)
def test_fit_equals_the_restatement_bit_for_bit(P, scenes, shape, model):
    flows, valid = scenes[shape]
    for iters in (0, 1, 4):
        for v in (None, valid):
            want = R.fit(flows, v, model, iters, 1.0)
            _same(f"fit {shape[0]}x{shape[1]} {model} iters {iters} mask {v is not None}", _fit(P, flows, v, model=model, iters=iters), want)
    want = R.fit(flows, None, model, 4, 1.0)
    if shape == (1, 1):
        assert want["ok"].tolist() == [model == "translation"] * 2
    elif shape == (1, 19):
        assert want["ok"].tolist() == [model != "affine"] * 2              # (a row holds a similarity: tests/test_host_motion.py)
    else:
        assert want["ok"].all()
        if model == "affine" and shape in R.SHAPES:                            # the rectangle is rejected (tests/test_host_motion.py)
            assert np.abs(want["params"] - R.TRUE_PARAMS).max() < 0.1


def test_masks_that_leave_too_little(P, scenes):
    flows, _ = scenes[(13, 19)]
    for left in (0, 1, 2, 3):
        valid = np.zeros((2, 13, 19), bool)
        valid[1] = True
        for y, x in ((2, 3), (7, 11), (12, 0))[:left]:
            valid[0, y, x] = True
        for model in R.MODELS:
            want = R.fit(flows, valid, model, 2, 1.0)
            assert bool(want["ok"][0]) is (left >= R.MIN_COUNT[model]) and want["ok"][1] and want["count"][0] == left
            _same(f"mask leaves {left} {model}", _fit(P, flows, valid, model=model, iters=2), want)
            if not want["ok"][0]:
                assert np.array_equal(want["matrices"][0], np.eye(3))


def test_unknown_flows_under_the_mask_and_in_the_open(P, scenes):
    flows, valid = scenes[(17, 16)]
    want = R.fit(flows, valid, "affine", 4, 1.0)
    hidden = flows.copy()
    hidden[~valid] = np.nan
    hidden[tuple(np.argwhere(~valid)[::2].T)] = np.inf
    shown = flows.copy()
    idx = np.argwhere(~valid)
    for (n, y, x), bad in zip(idx, [np.nan, np.inf, -np.inf, 1e10, -2e9] * len(idx)):
        shown[n, y, x, (y + x) % 2] = bad
    _same("nan under the mask", _fit(P, hidden, valid, model="affine", iters=4), want)
    _same("nan, inf, sentinel in the open", _fit(P, shown, None, model="affine", iters=4), want)
    res, inl = P.motion_residual(_up(shown), _up(want["matrices"]))
    wres, winl = R.residual(shown, want["matrices"])
    assert np.array_equal(_bits(res.cpu().numpy()), _bits(wres)) and np.array_equal(inl.cpu().numpy(), winl)
    assert (wres[~valid] == R.SENTINEL).all() and not winl[~valid].any()


def test_channel_slices_and_odd_offsets_give_the_same_bits(P, scenes):
    """Flows at channel stride 3, and as channels 1:3 of a 4-channel buffer (off the 8-byte boundary): two 4-byte loads a record."""
    flows, valid = scenes[(17, 16)]
    want = R.fit(flows, valid, "similarity", 4, 1.0)
    wres = R.residual(flows, want["matrices"], valid)
    for width, lo in ((3, 0), (3, 1), (4, 1), (4, 2)):
        buf = torch.full(flows.shape[:3] + (width,), float("nan"), dtype=torch.float32, device="cuda")
        buf[..., lo:lo + 2] = _up(flows)
        view = buf[..., lo:lo + 2]
        m, ok, info = P.fit_motion(view, _up(valid), model="similarity", iters=4)
        got = dict(matrices=m.cpu().numpy(), ok=ok.cpu().numpy(), count=info["count"].cpu().numpy(), weight_sum=info["weight_sum"].cpu().numpy())
        _same(f"stride {width} offset {lo} (address % 8 = {view.data_ptr() % 8})", got, want)
        res, inl = P.motion_residual(view, m, _up(valid))
        assert np.array_equal(_bits(res.cpu().numpy()), _bits(wres[0])) and np.array_equal(inl.cpu().numpy(), wres[1])


@pytest.mark.parametrize("shape", [(13, 19), (260, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_an_image_alone_gives_the_bits_it_gives_in_a_batch(P, scenes, shape):
    flows, valid = scenes[shape]
    alone = _fit(P, flows[:1], valid[:1], model="affine", iters=4)
    rs = np.random.RandomState(7)
    for tag, other in (("nan", np.full_like(flows[0], np.nan)), ("random", rs.normal(0, 30, size=flows[0].shape).astype(np.float32))):
        three = _fit(P, np.stack([other, flows[0], other]), np.stack([valid[1], valid[0], valid[1]]), model="affine", iters=4)
        middle = {k: v[1:2] for k, v in three.items()}
        _same(f"seam {shape} {tag} neighbours", middle, alone)
    again = _fit(P, flows[:1], valid[:1], model="affine", iters=4)
    _same(f"two calls {shape}", again, alone)


def test_residual_past_the_grid_cap(P):
    """3 x 592 x 592 = 1 051 392 pixels, more than 4096 workgroups of 256 lanes: the grid-stride pass; one matrix is not affine."""
    N, H, W = 3, 592, 592
    rs = np.random.RandomState(11)
    flows = rs.normal(0, 4, size=(N, H, W, 2)).astype(np.float32)
    flows[rs.uniform(size=(N, H, W)) < 0.01] = np.nan
    valid = rs.uniform(size=(N, H, W)) > 0.1
    M = np.tile(np.eye(3), (N, 1, 1))
    M[:, :2] += rs.normal(0, 0.01, size=(N, 2, 3))
    M[1, 2, 1] = 1e-3
    want = R.residual(flows, M, valid, 3.0)
    got = P.motion_residual(_up(flows), _up(M), _up(valid), threshold=3.0)
    gres, ginl = got[0].cpu().numpy(), got[1].cpu().numpy()
    print(f"motion residual grid cap: {N * H * W} pixels, inliers {int(want[1].sum())}, sentinels {int((want[0][..., 0] == R.SENTINEL).sum())}, "
          f"bits differ at {int((_bits(gres) != _bits(want[0])).sum())}, inlier differs at {int((ginl != want[1]).sum())}")
    assert (want[0][1] == R.SENTINEL).all() and want[1][0].sum() > 1000
    assert np.array_equal(_bits(gres), _bits(want[0])) and np.array_equal(ginl, want[1])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("C", [1, 3])
def test_warp_equals_the_restatement_bit_for_bit(P, dtype, C):
    """13 x 19 (247 pixels: the last run of four is partial) and 16 x 16, three images: a similarity that moves part of the frame
    out, an integer shift (exact ties at the last column and row), a matrix that is not affine."""
    for H, W in ((13, 19), (16, 16)):
        frames = R.random_frames(3, H, W, C, dtype, seed=H)
        M = np.tile(np.eye(3), (3, 1, 1))
        M[0, :2] = [[0.98, -0.07, 1.75], [0.07, 0.98, -2.5]]
        M[1, 0, 2], M[1, 1, 2] = 3.0, -2.0
        M[2, 2, 0] = 1e-6
        want = R.warp(frames, M)
        out, cov = P.warp_frames(_up(frames), _up(M))
        assert out.dtype == _up(frames).dtype and cov.dtype == torch.bool
        got = (out.cpu().numpy(), cov.cpu().numpy())
        print(f"motion warp {np.dtype(dtype).name} C {C} {H}x{W}: covered {want[1].sum(axis=(1, 2)).tolist()}, bits differ at "
              f"{int((_bits(got[0]) != _bits(want[0])).sum())}, covered differs at {int((got[1] != want[1]).sum())}")
        assert 0 < want[1][0].sum() < H * W and want[1][1].sum() == (H - 2) * (W - 3) and not want[1][2].any()
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
        out2, _ = P.warp_frames(_up(frames), M)                                     # a numpy array of matrices, smooth_path's
        assert torch.equal(out2, out)
        # off the vector boundaries: the same values one by one
        flat = torch.zeros(out.numel() + 1, dtype=out.dtype, device="cuda")
        covered = torch.zeros(3 * H * W + 1, dtype=torch.uint8, device="cuda")
        fr, mm = _up(frames), _up(M)
        esize = out.element_size()
        rc = _lib.lib().pwc_warp_affine(ctypes.c_void_p(fr.data_ptr()), _lib.MOTION_U8 if dtype == np.uint8 else _lib.MOTION_F32, C,
                                        ctypes.c_void_p(mm.data_ptr()), 3, H, W, ctypes.c_void_p(flat.data_ptr() + esize),
                                        ctypes.c_void_p(covered.data_ptr() + 1), _lib.current_stream())
        assert rc == 0
        assert torch.equal(flat[1:].view(out.shape), out) and torch.equal(covered[1:].view(3, H, W).bool(), cov)


def test_refusals_by_their_codes(P):
    flows = torch.zeros((2, 4, 4, 4), dtype=torch.float32, device="cuda")
    nbytes = _lib.lib().pwc_motion_fit_workspace_bytes(2, 4, 4)
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    mats = torch.full((2, 3, 3), 7.0, dtype=torch.float64, device="cuda")
    ok = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    count = torch.full((4,), -5, dtype=torch.int32, device="cuda")
    wsum = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda v: None if v is None else ctypes.c_void_p(v)                        # noqa: E731
    L = _lib.lib()

    def fit(**change):
        a = dict(flows=flows.data_ptr(), cs=4, valid=None, N=2, H=4, W=4, model=_lib.MOTION_AFFINE, iters=4, scale=1.0,
                 ws=ws.data_ptr(), nbytes=nbytes, mats=mats.data_ptr(), ok=ok.data_ptr(), count=count.data_ptr(), wsum=wsum.data_ptr())
        a.update(change)
        return L.pwc_motion_fit_f64(p(a["flows"]), a["cs"], p(a["valid"]), a["N"], a["H"], a["W"], a["model"], a["iters"], a["scale"],
                                    p(a["ws"]), a["nbytes"], p(a["mats"]), p(a["ok"]), p(a["count"]), p(a["wsum"]), _lib.current_stream())

    refused = [(EINVAL, dict(flows=None)), (EINVAL, dict(ws=None)), (EINVAL, dict(mats=None)), (EINVAL, dict(ok=None)),
               (EINVAL, dict(count=None)), (EINVAL, dict(wsum=None)), (EINVAL, dict(N=0)), (EINVAL, dict(H=0)), (EINVAL, dict(W=-1)),
               (EINVAL, dict(iters=-1)), (EINVAL, dict(iters=65)), (EINVAL, dict(scale=0.0)), (EINVAL, dict(scale=-1.0)),
               (EINVAL, dict(scale=float("nan"))), (EINVAL, dict(model=3)), (EINVAL, dict(model=-1)), (EINVAL, dict(cs=1)),
               (EINVAL, dict(nbytes=nbytes - 1)), (ERANGE, dict(H=1 << 16, W=1 << 15)), (ERANGE, dict(N=65536)),
               (EALIGN, dict(flows=flows.data_ptr() + 2)), (EALIGN, dict(ws=ws.data_ptr() + 4)), (EALIGN, dict(mats=mats.data_ptr() + 4)),
               (EALIGN, dict(wsum=wsum.data_ptr() + 4)), (EALIGN, dict(count=count.data_ptr() + 2))]
    for code, change in refused:
        assert fit(**change) == code, change

    res = torch.full((2, 4, 4, 2), 7.0, dtype=torch.float32, device="cuda")
    inl = torch.full((2, 4, 4), 0xEE, dtype=torch.uint8, device="cuda")

    def residual(**change):
        a = dict(flows=flows.data_ptr(), cs=4, valid=None, mats=mats.data_ptr(), N=2, H=4, W=4, thr=3.0, res=res.data_ptr(), inl=inl.data_ptr())
        a.update(change)
        return L.pwc_motion_residual_f32(p(a["flows"]), a["cs"], p(a["valid"]), p(a["mats"]), a["N"], a["H"], a["W"], a["thr"], p(a["res"]),
                                         p(a["inl"]), _lib.current_stream())

    refused_r = [(EINVAL, dict(flows=None)), (EINVAL, dict(mats=None)), (EINVAL, dict(res=None)), (EINVAL, dict(inl=None)),
                 (EINVAL, dict(N=0)), (EINVAL, dict(H=0)), (EINVAL, dict(W=0)), (EINVAL, dict(cs=1)), (EINVAL, dict(thr=-1.0)),
                 (EINVAL, dict(thr=float("nan"))), (ERANGE, dict(H=1 << 16, W=1 << 15)), (EALIGN, dict(flows=flows.data_ptr() + 1)),
                 (EALIGN, dict(res=res.data_ptr() + 2)), (EALIGN, dict(mats=mats.data_ptr() + 4))]
    for code, change in refused_r:
        assert residual(**change) == code, change

    frames = torch.zeros((2, 4, 4, 3), dtype=torch.float32, device="cuda")
    out = torch.full((2, 4, 4, 3), 7.0, dtype=torch.float32, device="cuda")

    def warp(**change):
        a = dict(frames=frames.data_ptr(), dtype=_lib.MOTION_F32, C=3, mats=mats.data_ptr(), N=2, H=4, W=4, out=out.data_ptr(), cov=inl.data_ptr())
        a.update(change)
        return L.pwc_warp_affine(p(a["frames"]), a["dtype"], a["C"], p(a["mats"]), a["N"], a["H"], a["W"], p(a["out"]), p(a["cov"]),
                                 _lib.current_stream())

    refused_w = [(EINVAL, dict(frames=None)), (EINVAL, dict(mats=None)), (EINVAL, dict(out=None)), (EINVAL, dict(cov=None)),
                 (EINVAL, dict(N=0)), (EINVAL, dict(H=-1)), (EINVAL, dict(W=0)), (EINVAL, dict(C=0)), (EINVAL, dict(C=5)), (EINVAL, dict(dtype=2)),
                 (ERANGE, dict(H=1 << 16, W=1 << 15)), (EALIGN, dict(mats=mats.data_ptr() + 4)), (EALIGN, dict(frames=frames.data_ptr() + 2)),
                 (EALIGN, dict(out=out.data_ptr() + 1))]
    for code, change in refused_w:
        assert warp(**change) == code, change
    torch.cuda.synchronize()
    assert bool((mats == 7.0).all()) and bool((ok == 0xEE).all()) and bool((count == -5).all()) and bool((wsum == 7.0).all())
    assert bool((res == 7.0).all()) and bool((inl == 0xEE).all()) and bool((out == 7.0).all())
    print(f"motion refusals: {len(refused) + len(refused_r) + len(refused_w)} calls refused, outputs untouched")
    mats.copy_(torch.eye(3, dtype=torch.float64, device="cuda").repeat(2, 1, 1))
    assert fit() == 0 and residual() == 0 and warp() == 0 and warp(out=out.data_ptr(), frames=frames.data_ptr(), dtype=_lib.MOTION_U8) == 0
    torch.cuda.synchronize()
    assert bool((ok != 0xEE).all()) and bool((res != 7.0).all()) and bool((out != 7.0).all()) and bool((count[:2] == 16).all())


def test_infer_continuous_motion_cli(P, tmp_path):
    """The CLI in a fresh child process: five 64 x 128 frames, un-learned weights, --motion affine --motion_residual --stabilize 1
    --batch 2.  The files' shapes; motion.npy equals fit_motion on the .flo files read back; and a second child without the flags
    writes the same .flo files byte for byte."""
    from PIL import Image
    from pwcnet_amd import flow_io
    rng = np.random.RandomState(5)
    base = rng.uniform(0, 255, size=(64, 128, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(5):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o"), "--motion", "affine", "--motion_residual", "--stabilize", "1"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    out = tmp_path / "o" / "seq"
    motion, ok = np.load(tmp_path / "o" / "motion.npy"), np.load(tmp_path / "o" / "motion_ok.npy")
    assert motion.shape == (4, 3, 3) and motion.dtype == np.float64 and ok.shape == (4,) and ok.dtype == bool
    flows = np.stack([flow_io.read_flo(str(out / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(4)])
    want = R.fit(flows, None, "affine", 4, 1.0)
    print(f"motion cli: translations {np.round(motion[:, :2, 2], 3).tolist()}, bits differ at {int((_bits(motion) != _bits(want['matrices'])).sum())}")
    assert np.array_equal(_bits(motion), _bits(want["matrices"])) and np.array_equal(ok, want["ok"])
    wres, winl = R.residual(flows, motion)
    for i in range(4):
        res = flow_io.read_flo(str(out / f"frame_{i:02d}_residual.flo"))
        inl = np.asarray(Image.open(out / f"frame_{i:02d}_inlier.png"))
        assert res.shape == (64, 128, 2) and inl.shape == (64, 128) and inl.dtype == np.uint8
        assert np.array_equal(_bits(res.astype(np.float32)), _bits(wres[i])) and np.array_equal(inl == 255, winl[i])
    for i in range(5):
        stab = np.asarray(Image.open(out / f"frame_{i:02d}_stab.png"))
        assert stab.shape == (64, 128, 3) and stab.dtype == np.uint8
    run = subprocess.run(cli + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert not (tmp_path / "plain" / "motion.npy").exists() and not (tmp_path / "plain" / "seq" / "frame_00_stab.png").exists()
    for i in range(4):                                                         # the flags change nothing else
        for ext in (".flo", ".png"):
            assert (tmp_path / "plain" / "seq" / f"frame_{i:02d}{ext}").read_bytes() == (out / f"frame_{i:02d}{ext}").read_bytes()
