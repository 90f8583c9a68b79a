"""The temporal filter on the GPU (pwc_temporal.hip, pwcnet_amd.temporal, infer_continuous.py --denoise) against the numpy
restatement of its definition (tests/temporal_ref.py): `filtered` and `support` BIT for bit, no pixel excluded -- the kernel forms
no fused multiply-add and calls no library function, so nothing is left to a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import temporal as TP  # the feature: without it nothing here can be collected
from tests import temporal_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.temporal_filter is TP.temporal_filter and pwcnet_amd.plan_windows is TP.plan_windows
    return pwcnet_amd


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _run(P, frames, fw, bw, valids_fw=None, valids_bw=None, **kw):
    """pwcnet_amd.temporal_filter on numpy arrays (or tensors already on the GPU), back as numpy."""
    up = lambda a: a if isinstance(a, torch.Tensor) else _up(a)                # noqa: E731
    filtered, support = P.temporal_filter(up(frames), up(fw), up(bw), valids_fw=up(valids_fw), valids_bw=up(valids_bw), **kw)
    assert support.dtype == torch.uint8 and filtered.is_contiguous() and support.is_contiguous() and not filtered.requires_grad
    return filtered.cpu().numpy(), support.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    assert got[0].dtype == want[0].dtype and got[0].shape == want[0].shape and got[1].shape == want[1].shape
    bad = int((_bits(got[0]) != _bits(want[0])).sum())
    bad_s = int((got[1] != want[1]).sum())
    print(f"temporal {what}: {got[0].size} values, {bad} differ; {got[1].size} supports, {bad_s} differ")
    assert bad == 0 and bad_s == 0


# (H, W, C, dtype, R, P, masks, fb_check, max_distance), T = 5 throughout
_MAIN = [(24, 40, C, dt, 2, Pp, True, True, None) for C in (1, 3) for dt in (np.uint8, np.float32) for Pp in (0, 1, 2)]
_MORE = [
    (24, 40, 3, np.uint8, 1, 1, True, True, None), (24, 40, 3, np.uint8, 8, 1, True, True, None),          # R = 8: both clip ends cut the walk
    (24, 40, 1, np.float32, 1, 2, True, True, None), (24, 40, 1, np.float32, 8, 2, False, True, None),
    (24, 40, 3, np.uint8, 2, 1, True, True, 8.0), (24, 40, 3, np.float32, 2, 0, False, True, 8.0),         # max_distance on
    (24, 40, 3, np.uint8, 2, 1, False, True, None), (24, 40, 3, np.uint8, 2, 1, True, False, None),        # no masks; no fb check
    (33, 65, 3, np.uint8, 2, 0, False, True, None), (33, 65, 3, np.uint8, 2, 1, True, True, None),         # straddling tile seams
    (33, 65, 3, np.uint8, 2, 2, False, True, None), (33, 65, 1, np.float32, 8, 1, True, True, 8.0),
    (1, 1, 3, np.uint8, 2, 2, False, True, None), (1, 1, 1, np.float32, 1, 1, True, True, None),
    (1, 7, 3, np.uint8, 2, 2, True, True, None), (1, 7, 1, np.float32, 1, 1, False, False, None),
]


def _id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{np.dtype(c[3]).name}-R{c[4]}-P{c[5]}-{'masks' if c[6] else 'nomasks'}-{'fb' if c[7] else 'nofb'}-md{c[8]}"


@pytest.mark.parametrize("cfg", _MAIN + _MORE, ids=_id)
def test_bits_equal_the_restatement(P, cfg):
    H, W, C, dtype, radius, patch, masks, fb, md = cfg
    c = R.case(5, H, W, C, dtype)
    want = R.reference(5, H, W, C, dtype, radius, patch, masks, fb, md)
    got = _run(P, c["frames"], c["fw_s"], c["bw_s"], c["valid_fw"] if masks else None, c["valid_bw"] if masks else None,
               radius=radius, patch=patch, fb_check=fb, max_distance=md)
    _same(got, want[:2], _id(cfg))
    assert int(got[1].max()) <= min(2 * radius, 4)


def test_masked_flows_are_not_read_and_a_nan_frame_value_reads_as_zero(P):
    c = R.case(5, 24, 40, 3, np.float32)
    want = R.reference(5, 24, 40, 3, np.float32, 2, 1, True, True, None)
    _same(_run(P, c["frames"], c["fw_nan"], c["bw_nan"], c["valid_fw"], c["valid_bw"], radius=2, patch=1), want[:2], "NaN behind the masks")
    frames = c["frames"].copy()
    frames[1, 5, 6, 1] = np.nan
    frames[3, 0, 39, 2] = np.nan
    want = R.temporal_filter(frames, c["fw_s"], c["bw_s"], radius=2, patch=1)
    got = _run(P, frames, c["fw_s"], c["bw_s"], radius=2, patch=1)
    _same(got, want, "NaN in a frame")
    assert np.isfinite(got[0]).all()


def test_channel_slices_pieces_and_repeats(P):
    """Flows passed as channel slices of one wider buffer (channel stride 6, the first on a 4-byte boundary only); out_range
    pieces from plan_windows against one call; two calls give the same bits."""
    c = R.case(5, 33, 65, 3, np.uint8)
    want = R.reference(5, 33, 65, 3, np.uint8, 2, 1, True, True, None)
    wide = torch.full((4, 33, 65, 6), float("nan"), device="cuda")
    wide[..., 1:3] = _up(c["fw_s"])
    wide[..., 3:5] = _up(c["bw_s"])
    kw = dict(valids_fw=c["valid_fw"], valids_bw=c["valid_bw"], radius=2, patch=1)
    first = _run(P, c["frames"], wide[..., 1:3], wide[..., 3:5], **kw)
    _same(first, want[:2], "channel slices")
    again = _run(P, c["frames"], wide[..., 1:3], wide[..., 3:5], **kw)
    _same(again, first, "a second call")
    for batch in (1, 2, 4):
        assert P.plan_windows(5, 2, batch) == R.plan_windows(5, 2, batch)
        parts = R.by_pieces(c["frames"], c["fw_s"], c["bw_s"], 2, batch, valids_fw=c["valid_fw"], valids_bw=c["valid_bw"], patch=1,
                            run=lambda *a, **k: _run(P, *a, **k))
        _same(parts, want[:2], f"plan_windows pieces of {batch}")
    part = _run(P, c["frames"], c["fw_s"], c["bw_s"], out_range=(1, 3), **kw)
    assert part[0].shape == (2, 33, 65, 3)
    _same(part, (want[0][1:3], want[1][1:3]), "out_range (1, 3)")


def test_one_frame(P):
    for dtype in (np.uint8, np.float32):
        frames = R.case(1, 24, 40, 3, dtype)["frames"]
        got = _run(P, frames, None, None, radius=2, patch=2)
        want = R.temporal_filter(frames, np.zeros((0, 24, 40, 2), np.float32), np.zeros((0, 24, 40, 2), np.float32), radius=2, patch=2)
        _same(got, want, "T = 1")
        assert (got[1] == 0).all()
        if dtype == np.uint8:
            assert (got[0] == frames).all()


def test_support_counts_the_frames_track_points_sees(P):
    """The positions walked are track_points': with max_distance off every reached neighbour has a weight above 0, so support is
    the number of frames within R of i in which the pixel, tracked both ways from frame i with the check, is VISIBLE."""
    T, H, W, radius = 5, 24, 40, 2
    c = R.case(T, H, W, 3, np.uint8)
    support = _run(P, c["frames"], c["fw_s"], c["bw_s"], c["valid_fw"], c["valid_bw"], radius=radius, patch=0)[1]
    points = P.grid_points(H, W, 1).cuda()
    seen = set()
    for i in range(T):
        start = torch.full((H * W,), i, dtype=torch.int32, device="cuda")
        status = P.track_points(_up(c["fw_s"]), points, flows_bw=_up(c["bw_s"]), start=start, valids_fw=_up(c["valid_fw"]),
                                valids_bw=_up(c["valid_bw"]), direction="both")[1].cpu().numpy()
        near = [t for t in range(max(i - radius, 0), min(i + radius, T - 1) + 1) if t != i]
        visible = (status[near] == P.track.VISIBLE).sum(axis=0).reshape(H, W)
        assert (support[i] == visible).all()
        seen.update(np.unique(status).tolist())
    assert seen == {P.track.VISIBLE, P.track.LEFT, P.track.OCCLUDED, P.track.UNKNOWN}


def test_infer_continuous_denoise_cli(P, tmp_path):
    """The CLI in a fresh child process: four 64 x 64 frames, un-learned weights, --denoise 1 --batch 2.  One _denoised.png per
    frame, the last one included, equal to temporal_filter on the same flows (computed here by the same model on the same frames,
    both ways, in the CLI's batches); the .flo files and montages are those of a run without the flag, byte for byte."""
    from PIL import Image
    rng = np.random.RandomState(3)
    base = rng.uniform(0, 255, size=(64, 64, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    frames = [np.roll(base, 2 * i, axis=1) for i in range(4)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o"), "--denoise", "1"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    plain = subprocess.run(cli + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]
    out = tmp_path / "o" / "seq"
    for i in range(3):
        for ext in (".flo", ".png"):
            assert (tmp_path / "plain" / "seq" / f"frame_{i:02d}{ext}").read_bytes() == (out / f"frame_{i:02d}{ext}").read_bytes()
    assert not list((tmp_path / "plain" / "seq").glob("*_denoised.png"))
    assert sorted(p.name for p in out.glob("*_denoised.png")) == [f"frame_{i:02d}_denoised.png" for i in range(4)]
    model = P.ForwardPipeline(depth=1)
    stack = np.stack(frames)
    seq_f = torch.from_numpy(stack.astype(np.float32) / 255.0).cuda()
    first, second = seq_f[:-1].contiguous(), seq_f[1:].contiguous()
    fws, bws = [], []
    for lo, hi in ((0, 2), (2, 3)):                                               # the CLI's batches
        fw_t, bw_t = model.submit(first[lo:hi], second[lo:hi]), model.submit(second[lo:hi], first[lo:hi])
        model.synchronize()
        fws.append(fw_t.result()[0].clone())
        bws.append(bw_t.result()[0].clone())
    want = P.temporal_filter(torch.from_numpy(stack).cuda(), torch.cat(fws), torch.cat(bws), radius=1)[0].cpu().numpy()
    differing = 0
    for i in range(4):
        got = np.asarray(Image.open(out / f"frame_{i:02d}_denoised.png"))
        assert got.shape == (64, 64, 3) and got.dtype == np.uint8
        differing += int((got != want[i]).sum())
    print(f"denoise cli: four pictures, {differing} bytes differ from temporal_filter on the same flows")
    assert differing == 0
