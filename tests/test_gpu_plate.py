"""The background plate on the GPU (pwc_plate.hip, pwcnet_amd.plate, infer_continuous.py --plate) against the numpy restatement
of its definition (tests/plate_ref.py): plate, count, difference, foreground and known BIT for bit, no pixel excluded -- the
kernels form no fused multiply-add and call no library function, so nothing is left to a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import plate as PL  # the feature: without it nothing here can be collected
from tests import plate_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.background_plate is PL.background_plate and pwcnet_amd.plate_difference is PL.plate_difference
    return pwcnet_amd


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    """Every array of `got` against `want`, bit for bit; prints the figures first."""
    bad = []
    want = [w.cpu().numpy() if isinstance(w, torch.Tensor) else w for w in want]
    for g, w in zip(got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
        bad.append(int((_bits(np.ascontiguousarray(g)) != _bits(np.ascontiguousarray(w))).sum()))
    print(f"plate {what}: {[w.size for w in want]} values, {bad} differ")
    assert not any(bad)


def _build(P, c, canvas, mode, masks=False, use=False, min_count=1, matrices=None):
    plate, count = P.background_plate(_up(c["frames"]), c["matrices"] if matrices is None else matrices, canvas, mode=mode,
                                      use=c["use"] if use else None, masks=_up(c["masks"]) if masks else None, min_count=min_count)
    assert count.dtype == torch.uint8 and plate.is_contiguous() and count.is_contiguous() and not plate.requires_grad
    return plate, count


# (T, H, W, Hc, Wc, C, dtype, mode, masks, use, min_count)
_U8, _F32 = np.uint8, np.float32
_CASES = [(T, 24, 40, 30, 52, C, dt, mode, T == 5, False, 1)
          for T, C in ((1, 3), (2, 1), (5, 3), (5, 4), (64, 1), (64, 3)) for dt in (_U8, _F32) for mode in (R.MEDIAN, R.MEAN)]
_CASES += [
    (5, 33, 65, 41, 70, 3, _U8, R.MEDIAN, False, False, 1), (5, 33, 65, 41, 70, 3, _F32, R.MEDIAN, True, True, 1),    # tile seams
    (64, 33, 65, 41, 70, 4, _U8, R.MEDIAN, True, True, 3), (2, 33, 65, 41, 70, 1, _F32, R.MEAN, False, False, 1),
    (5, 1, 1, 1, 1, 3, _U8, R.MEDIAN, False, False, 1), (5, 1, 1, 1, 1, 1, _F32, R.MEDIAN, False, False, 1),
    (5, 1, 7, 1, 7, 3, _U8, R.MEAN, False, False, 1), (2, 1, 7, 1, 7, 4, _F32, R.MEDIAN, True, False, 1),
    (5, 24, 40, 30, 52, 3, _U8, R.MEDIAN, True, True, 3), (5, 24, 40, 30, 52, 3, _F32, R.MEAN, True, True, 3),        # min_count 3
    (64, 24, 40, 30, 52, 4, _F32, R.MEDIAN, True, True, 1), (2, 24, 40, 30, 52, 2, _U8, R.MEDIAN, False, False, 1),
]


def _id(c):
    return (f"T{c[0]}-{c[1]}x{c[2]}on{c[3]}x{c[4]}x{c[5]}-{np.dtype(c[6]).name}-{c[7]}-{'masks' if c[8] else 'nomasks'}-"
            f"{'use' if c[9] else 'all'}-min{c[10]}")


@pytest.mark.parametrize("cfg", _CASES, ids=_id)
def test_bits_equal_the_restatement(P, cfg):
    T, H, W, Hc, Wc, C, dtype, mode, masks, use, min_count = cfg
    threshold = 10.0 if dtype == _U8 else 10.0 / 255.0
    c = R.case(T, H, W, Hc, Wc, C, dtype)
    want = R.reference(T, H, W, Hc, Wc, C, dtype, mode, masks, use, min_count, threshold=threshold)
    plate, count = _build(P, c, (Hc, Wc), mode, masks, use, min_count)
    _same((plate, count), want[:2], _id(cfg) + " build")
    got = P.plate_difference(_up(c["frames"]), plate, count, c["frame_matrices"], threshold, min_count=min_count)
    _same(got, want[2:], _id(cfg) + " difference")
    if H >= 24:                                                            # the case reaches what it is meant to reach
        n = want[1]
        assert n.min() == 0 and n.max() == (T - 1 if use and T > 1 else T) and len(np.unique(n)) >= min(T, 3)
        assert want[4].any() and (want[3].any() or T == 1)


@pytest.mark.parametrize("mode", [R.MEDIAN, R.MEAN])
@pytest.mark.parametrize("T", [5, 64])
def test_float_specials(P, T, mode):
    """-0.0 against +0.0, a block of duplicates, an Inf, a -Inf and a NaN in the frames: the samples that touch a non-finite value
    are gone, the median carries one of the samples' bit patterns."""
    c = R.case(T, 24, 40, 30, 52, 3, _F32, special=True)
    want = R.reference(T, 24, 40, 30, 52, 3, _F32, mode, special=True, threshold=0.04)
    plate, count = _build(P, c, (30, 52), mode)
    _same((plate, count), want[:2], f"specials T{T} {mode} build")
    assert np.isfinite(want[0]).all() and (want[1] < R.reference(T, 24, 40, 30, 52, 3, _F32, mode)[1]).any()
    if mode == R.MEDIAN:                                                   # half the frames show -0.0, half +0.0: the lower one
        assert (want[0].view(np.uint32) == 0x80000000).any()
    _same(P.plate_difference(_up(c["frames"]), plate, count, c["frame_matrices"], 0.04), want[2:], f"specials T{T} {mode} difference")
    assert not want[4][0, 3, 4] and want[4][0, 3, 6]                         # the Inf pixel of frame 0 is unknown, a neighbour is not


def test_nothing_used_and_broken_matrices(P):
    c = R.case(5, 24, 40, 30, 52, 3, _U8)
    for dtype in (_U8, _F32):
        c = R.case(5, 24, 40, 30, 52, 3, dtype)
        plate, count = P.background_plate(_up(c["frames"]), c["matrices"], (30, 52), use=np.zeros(5, bool))
        assert int(count.max()) == 0 and float(plate.abs().max() if dtype == _F32 else plate.max()) == 0
    broken = c["matrices"].copy()
    broken[0, 2, 2] = 1.0 + 2.0 ** -52                                     # not affine
    broken[2, 0, 2] = np.nan
    broken[3, 1, 1] = np.inf
    for mode in (R.MEDIAN, R.MEAN):
        want = R.plate_build(c["frames"], broken, (30, 52), mode)
        _same(_build(P, c, (30, 52), mode, matrices=broken), want, f"broken matrices {mode}")
        only = R.plate_build(c["frames"], c["matrices"], (30, 52), mode, use=np.array([0, 1, 0, 0, 1]))
        _same(want, only, "the same as switching those frames off")
    back = c["frame_matrices"].copy()
    back[1, 2, 0] = 1e-300
    back[4, 0, 0] = -np.inf
    plate, count = R.plate_build(c["frames"], c["matrices"], (30, 52))
    got = P.plate_difference(_up(c["frames"]), _up(plate), _up(count), back, 0.05)
    _same(got, R.plate_difference(c["frames"], plate, count, back, 0.05), "broken frame matrices")
    assert not got[2][1].any() and not got[2][4].any() and got[2][0].any()


def test_matrices_as_array_and_tensor_repeats_and_views(P):
    """A numpy array and a float64 tensor give the same bits; so do two calls; a uint8 frames view that starts one byte into its
    buffer gives the bits of the contiguous copy (the wrapper makes its input contiguous: the kernel reads dense frames)."""
    T, H, W, Hc, Wc, C = 5, 33, 65, 41, 70, 3
    c = R.case(T, H, W, Hc, Wc, C, _U8)
    want = R.reference(T, H, W, Hc, Wc, C, _U8, R.MEDIAN, True, True, 1, threshold=10.0)
    first = _build(P, c, (Hc, Wc), R.MEDIAN, True, True)
    _same(first, want[:2], "array matrices")
    _same(_build(P, c, (Hc, Wc), R.MEDIAN, True, True, matrices=_up(c["matrices"])), first, "tensor matrices")
    _same(_build(P, c, (Hc, Wc), R.MEDIAN, True, True), first, "a second call")
    raw = torch.zeros(c["frames"].size + 1, dtype=torch.uint8, device="cuda")
    raw[1:] = _up(c["frames"]).reshape(-1)
    view = raw[1:].view(T, H, W, C)
    assert view.data_ptr() % 2 == 1
    got = P.background_plate(view, c["matrices"], (Hc, Wc), use=c["use"], masks=_up(c["masks"]))
    _same(got, first, "frames one byte into their buffer")
    strided = _up(np.concatenate([c["frames"], c["frames"]], axis=3))[..., :C]
    assert not strided.is_contiguous()
    _same(P.background_plate(strided, c["matrices"], (Hc, Wc), use=c["use"], masks=_up(c["masks"])), first, "a channel slice")
    d1 = P.plate_difference(view, first[0], first[1], _up(c["frame_matrices"]), 10.0)
    _same(d1, want[2:], "difference, tensor matrices, frames one byte into their buffer")
    _same(P.plate_difference(_up(c["frames"]), first[0], first[1], c["frame_matrices"], 10.0), d1, "a second call")


def test_unaligned_byte_pointers_through_the_c_entry(P):
    """uint8 frames and plate need no alignment: the C entry on pointers one byte into their buffers."""
    T, H, W, Hc, Wc, C = 5, 24, 40, 30, 52, 3
    c = R.case(T, H, W, Hc, Wc, C, _U8)
    want = R.reference(T, H, W, Hc, Wc, C, _U8, R.MEDIAN)
    raw = torch.zeros(c["frames"].size + 1, dtype=torch.uint8, device="cuda")
    raw[1:] = _up(c["frames"]).reshape(-1)
    plate = torch.zeros(Hc * Wc * C + 1, dtype=torch.uint8, device="cuda")
    count = torch.zeros(Hc * Wc + 1, dtype=torch.uint8, device="cuda")
    mats = _up(c["matrices"])
    rc = _lib.lib().pwc_plate_build(raw.data_ptr() + 1, _lib.MOTION_U8, C, mats.data_ptr(), None, None, T, H, W, Hc, Wc,
                                    _lib.PLATE_MEDIAN, 1, plate.data_ptr() + 1, count.data_ptr() + 1, _lib.current_stream())
    assert rc == 0
    _same((plate[1:].view(Hc, Wc, C), count[1:].view(Hc, Wc)), want, "unaligned byte pointers")
    assert int(plate[0]) == 0 and int(count[0]) == 0


def test_c_abi_error_codes(P):
    L = _lib.lib()
    T, H, W, Hc, Wc, C = 2, 4, 5, 6, 7, 3
    fr = torch.zeros(T * H * W * C * 4 + 8, dtype=torch.uint8, device="cuda")
    mats = torch.eye(3, dtype=torch.float64, device="cuda").repeat(T + 1, 1, 1)
    plate = torch.zeros(Hc * Wc * C * 4 + 8, dtype=torch.uint8, device="cuda")
    count = torch.zeros(Hc * Wc, dtype=torch.uint8, device="cuda")
    out = torch.zeros(T * H * W * 4 + 8, dtype=torch.uint8, device="cuda")
    by = torch.zeros(2 * T * H * W, dtype=torch.uint8, device="cuda")
    s = _lib.current_stream()
    U8, F32, MED = _lib.MOTION_U8, _lib.MOTION_F32, _lib.PLATE_MEDIAN

    def build(frames=fr.data_ptr(), dtype=U8, C=C, matrices=mats.data_ptr(), T=T, H=H, W=W, Hc=Hc, Wc=Wc, mode=MED, min_count=1,
              plate=plate.data_ptr(), count=count.data_ptr()):
        return L.pwc_plate_build(frames, dtype, C, matrices, None, None, T, H, W, Hc, Wc, mode, min_count, plate, count, s)

    def diff(frames=fr.data_ptr(), dtype=U8, C=C, plate=plate.data_ptr(), count=count.data_ptr(), matrices=mats.data_ptr(), T=T, H=H,
             W=W, Hc=Hc, Wc=Wc, min_count=1, threshold=1.0, difference=out.data_ptr(), foreground=by.data_ptr(),
             known=by.data_ptr() + T * H * W):
        return L.pwc_plate_difference(frames, dtype, C, plate, count, matrices, T, H, W, Hc, Wc, min_count, threshold, difference,
                                      foreground, known, s)

    assert build() == 0 and diff() == 0 and build(dtype=F32, mode=_lib.PLATE_MEAN) == 0 and diff(dtype=F32) == 0
    for kw in (dict(frames=None), dict(matrices=None), dict(plate=None), dict(count=None), dict(T=0), dict(H=0), dict(W=0), dict(Hc=0),
               dict(Wc=0), dict(T=_lib.PLATE_MAX_FRAMES + 1), dict(C=0), dict(C=5), dict(dtype=2), dict(mode=2), dict(mode=-1),
               dict(min_count=0)):
        assert build(**kw) == EINVAL, kw
    for kw in (dict(frames=None), dict(plate=None), dict(count=None), dict(matrices=None), dict(difference=None), dict(foreground=None),
               dict(known=None), dict(T=0), dict(H=0), dict(W=0), dict(Hc=0), dict(Wc=0), dict(C=0), dict(C=5), dict(dtype=-1),
               dict(min_count=0), dict(threshold=-1.0), dict(threshold=float("nan"))):
        assert diff(**kw) == EINVAL, kw
    big = (1 << 16, 1 << 15)                                               # 2^31 pixels: refused before anything is read
    assert build(H=big[0], W=big[1]) == ERANGE and build(Hc=big[0], Wc=big[1]) == ERANGE
    assert diff(H=big[0], W=big[1]) == ERANGE and diff(Hc=big[0], Wc=big[1]) == ERANGE and diff(T=65536) == ERANGE
    assert build(matrices=mats.data_ptr() + 4) == EALIGN and diff(matrices=mats.data_ptr() + 4) == EALIGN
    assert build(dtype=F32, frames=fr.data_ptr() + 2) == EALIGN and build(dtype=F32, plate=plate.data_ptr() + 1) == EALIGN
    assert diff(dtype=F32, frames=fr.data_ptr() + 2) == EALIGN and diff(dtype=F32, plate=plate.data_ptr() + 1) == EALIGN
    assert diff(difference=out.data_ptr() + 2) == EALIGN
    assert build(frames=fr.data_ptr() + 1, plate=plate.data_ptr() + 1) == 0    # bytes need no alignment
    torch.cuda.synchronize()


def test_infer_continuous_plate_cli(P, tmp_path):
    """The CLI in a fresh child process: six 64 x 128 frames cut from one wide picture by a pan of 3 px per frame, un-learned
    weights.  With --motion translation --plate --plate_foreground 10 the plate, its count and one _fg.png per reachable frame are
    there, with the shapes plate_canvas predicts from the motion.npy the run wrote; every other file equals, byte for byte, the
    files of a run with --motion translation alone, which writes none of the new ones."""
    from PIL import Image
    rng = np.random.RandomState(4)
    wide = rng.uniform(0, 255, size=(64, 160, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(6):
        Image.fromarray(np.ascontiguousarray(wide[:, 3 * i:3 * i + 128])).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "4",
           "--motion", "translation"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o"), "--plate", "--plate_foreground", "10"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    plain = subprocess.run(cli + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]

    def listing(root):
        return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}
    new, old = listing(tmp_path / "o"), listing(tmp_path / "plain")
    motions, ok = np.load(tmp_path / "o" / "motion.npy"), np.load(tmp_path / "o" / "motion_ok.npy")
    to_frame, reach = P.plate_path(motions, ok)
    x0, y0, Hc, Wc = P.plate_canvas(to_frame, reach, 64, 128)
    added = {"plate.png", "plate_count.png"} | {os.path.join("seq", f"frame_{i:02d}_fg.png") for i in range(6) if reach[i]}
    assert set(new) == set(old) | added and not added & set(old)
    assert all(new[name] == old[name] for name in old)
    plate, count = np.asarray(Image.open(tmp_path / "o" / "plate.png")), np.asarray(Image.open(tmp_path / "o" / "plate_count.png"))
    assert plate.shape == (Hc, Wc, 3) and plate.dtype == np.uint8 and count.shape == (Hc, Wc) and count.dtype == np.uint8
    assert count.max() <= int(reach.sum())
    for name in added - {"plate.png", "plate_count.png"}:
        fg = np.asarray(Image.open(tmp_path / "o" / name))
        assert fg.shape == (64, 128) and set(np.unique(fg).tolist()) <= {0, 128, 255}
    print(f"plate cli: canvas {Hc} x {Wc} at ({x0}, {y0}), {int(reach.sum())} of 6 frames reachable, count up to {int(count.max())}")
