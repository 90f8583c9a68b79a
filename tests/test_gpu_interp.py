"""Frame interpolation on the GPU (pwc_interp.hip, pwcnet_amd.interp, infer_continuous.py --interp) against the numpy restatement of
tests/interp_ref.py (checked on the CPU by tests/test_host_interp.py).

The kernel's operations are IEEE double operations in a fixed order with no fused multiply-add, its sums are integers, and the
restatement performs the same operations in the same order: the only operation whose result may differ is exp.

THE BOUND of a float32 element, from the terms DESIGN.md 11 uses for a normalised splat, per covered direction k and weighted by
its share a_k of the output (1 - t and t where both cover, 1 where one does, none in a hole, whose value is the restatement's):
    2^-24 |ref|                                   the one float32 rounding of the output,
    e_k (1 + |c_k|) / (den_k - e_k)               the fixed point: e_k = cnt_k 2^-37 (1 + 2^-20), cnt_k contributions of at most half
                                                  a step each to a numerator (|colour| <= 1) and to the denominator,
    d4 (1 + |c_k|) / (1 - d4)                     exp: weights off by a relative d move a weighted mean of colours in [0, 1] by at
                                                  most d max|colour - c_k| / (1 - d),
    2^-50                                         the blend's and the quotient's own double roundings, where a direction covers;
                                                  a hole's value is the restatement's own sequence of operations: bound 0.
d4 = 4 max(d, 2^-52): d is the largest relative difference this test measures between the device's double exp (torch.exp on the
GPU) and numpy's on the weights' own arguments, and 2^-52, one unit in the last place of a double, is the floor where it
measures none.  Measured on an MI355X: d = 2.22e-16 (one unit in the last place; 926 arguments in [-10, -0.079] of the largest
case), so d4 = 8.9e-16.  With given weights there is no exp and no exp term.  Figures: profiles/interp_gpu_test_figures.txt.
uint8 frames: bytes equal except where the restatement's 255 v lies within 255 times that bound (without the float32 term) of
a half-integer; there they may differ by one level; such elements are under 1 % of the test's inputs.
`source` codes are compared outside the set tests/interp_ref.near_threshold leaves out (under 1 %, asserted on the CPU)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import interp as IP  # the feature: without it nothing here can be collected
from tests import interp_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.interpolate_frames is IP.interpolate_frames
    return pwcnet_amd


def _up(a):
    return torch.from_numpy(np.array(a)).cuda() if isinstance(a, np.ndarray) else a


def _gpu(inp, kw):
    return {k: _up(v) for k, v in dict(inp, **kw).items()}


def _run(P, inp, kw):
    frames_t, source = P.interpolate_frames(**_gpu(inp, kw))
    assert source.dtype == torch.uint8 and frames_t.is_contiguous() and source.is_contiguous()
    return frames_t.cpu().numpy(), source.cpu().numpy()


_EXP = {}


def _exp_term(ref):
    """d4 of the docstring for the arguments exp saw in `ref`."""
    args = ref["exp_args"]
    if args.size == 0:
        return 0.0
    key = id(ref)
    if key not in _EXP:
        dev = torch.exp(torch.from_numpy(args).cuda()).cpu().numpy()
        d = float(np.abs(dev / np.exp(args) - 1.0).max())
        print(f"interp exp: {args.size} arguments in [{args.min():.3f}, {args.max():.3f}], device against numpy: largest relative "
              f"difference {d:.3e}")
        _EXP[key] = 4.0 * max(d, 2.0 ** -52)
    return _EXP[key]


def _bound(ref, d4, fp32):
    """The docstring's bound per element (N,M,H,W,3)."""
    t = ref["times"][None, :, None, None]
    code = ref["source"]
    share = np.stack([np.where(code == 3, 1.0 - t, (code == 1) * 1.0), np.where(code == 3, t, (code == 2) * 1.0)], axis=-1)
    e = ref["cnt"] * 2.0 ** -37 * (1.0 + 2.0 ** -20)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(ref["covered"][..., None], np.abs(ref["c"]), 0.0)                   # (N,M,H,W,2,3)
        per = (e / (ref["den"] - e))[..., None] * (1.0 + c) + d4 * (1.0 + c) / (1.0 - d4)
    per = np.where(ref["covered"][..., None], per, 0.0)
    assert (ref["den"] > e)[ref["covered"]].all()
    bound = (share[..., None] * per).sum(axis=-2) + np.where(code != 0, 2.0 ** -50, 0.0)[..., None]
    return bound + (2.0 ** -24 * np.abs(ref["value"]) if fp32 else 0.0)


def _check_source(tag, got, ref):
    out = R.near_threshold(ref)
    differ = got != ref["source"]
    print(f"interp {tag}: source codes {np.bincount(ref['source'].ravel(), minlength=4).tolist()}, left out {int(out.sum())} of "
          f"{out.size}, differing {int(differ.sum())} ({int((differ & ~out).sum())} outside the set left out)")
    assert out.mean() <= 0.01 and not (differ & ~out).any(), tag


def _check_f32(tag, got, ref, d4):
    bound = _bound(ref, d4, True)
    err = np.abs(got.astype(np.float64) - ref["value"])
    k = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"interp {tag}: largest error {err.max():.3e}, largest error / bound {float(err[k] / bound[k]):.3e} "
          f"(error {err[k]:.3e}, bound {bound[k]:.3e}); bits equal to the restatement's at "
          f"{float((got.view(np.int32) == ref['frames_t'].view(np.int32)).mean()):.4f} of the elements")
    assert np.isfinite(got).all() and (err <= bound).all(), tag


def _check_u8(tag, got, ref, d4):
    x = 255.0 * ref["value"]
    near = np.abs(np.abs(x - np.floor(x)) - 0.5) < 255.0 * _bound(ref, d4, False)         # (a hole's bound is 0: never near)
    diff = np.abs(got.astype(np.int64) - ref["frames_t"].astype(np.int64))
    print(f"interp {tag}: bytes differing {int((diff != 0).sum())} of {diff.size}, largest difference {int(diff.max())}, near a "
          f"half-integer {int(near.sum())} ({float(near.mean()):.5f})")
    assert near.mean() < 0.01 and (diff[~near] == 0).all() and (diff <= 1).all(), tag


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("masks", [False, True])
def test_float32_frames_and_source_codes_against_the_restatement(P, shape, masks):
    inp, kw, ref = R.case(shape, np.float32, masks=masks)
    frames_t, source = _run(P, inp, kw)
    assert frames_t.dtype == np.float32 and frames_t.shape == tuple(shape[:1]) + (shape[3],) + tuple(shape[1:3]) + (3,)
    tag = f"f32 {shape} masks {masks}"
    _check_source(tag, source, ref)
    _check_f32(tag, frames_t, ref, _exp_term(ref))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_uint8_frames_against_the_restatement(P, shape):
    inp, kw, ref = R.case(shape, np.uint8)
    frames_t, source = _run(P, inp, kw)
    assert frames_t.dtype == np.uint8
    _check_source(f"u8 {shape}", source, ref)
    _check_u8(f"u8 {shape}", frames_t, ref, _exp_term(ref))


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_given_weights_need_no_exp_term(P, shape, dtype):
    inp, kw, ref = R.case(shape, dtype, given_weights=True)
    assert ref["exp_args"].size == 0
    frames_t, source = _run(P, inp, kw)
    tag = f"given weights {np.dtype(dtype).name} {shape}"
    _check_source(tag, source, ref)
    (_check_f32 if dtype == np.float32 else _check_u8)(tag, frames_t, ref, 0.0)


def test_256_sources_on_one_target(P):
    """Every pixel of a 16 x 16 frame 0 is sent to (8, 8) at t = 0.5 with weight 1; frame 1 sends nothing."""
    rs = np.random.RandomState(5)
    H = W = 16
    f0 = rs.uniform(0, 1, size=(1, H, W, 3)).astype(np.float32)
    f1 = rs.uniform(0, 1, size=(1, H, W, 3)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fw = np.stack([2.0 * (8 - xs), 2.0 * (8 - ys)], axis=-1)[None].astype(np.float32)
    bw = np.full((1, H, W, 2), np.float32(1e10))
    inp = dict(frames_0=f0, frames_1=f1, flows_fw=fw, flows_bw=bw)
    kw = dict(times=[0.5], weights_fw=np.ones((1, H, W), np.float32))
    ref = R.interpolate(**inp, **kw)
    assert ref["cnt"][0, 0, 8, 8].tolist() == [256, 0] and ref["source"][0, 0, 8, 8] == 1 and ref["den"][0, 0, 8, 8, 0] == 256.0
    assert (np.delete(ref["source"].ravel(), 8 * W + 8) == 0).all()
    frames_t, source = _run(P, inp, kw)
    assert np.array_equal(source, ref["source"])
    _check_f32("collision", frames_t, ref, 0.0)
    mean = f0.astype(np.float64).reshape(-1, 3).mean(axis=0)
    bound = _bound(ref, 0.0, True)[0, 0, 8, 8]
    err = np.abs(frames_t[0, 0, 8, 8].astype(np.float64) - mean)
    print(f"interp collision: against the exact mean, error {err.max():.3e}, bound {bound.max():.3e}")
    assert (err <= bound + 2.0 ** -50).all()                                      # (the mean's own double roundings)
    fade = 0.5 * f0.astype(np.float64) + 0.5 * f1.astype(np.float64)
    holes = ref["source"][0, 0] == 0
    assert np.array_equal(frames_t[0, 0][holes], fade[0][holes].astype(np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_reproducible_and_the_pieces_give_the_whole_calls_bits(P, dtype):
    inp, kw, _ = R.case((2, 13, 19, 3), dtype)
    g = _gpu(inp, kw)
    whole = P.interpolate_frames(**g)
    again = P.interpolate_frames(**g)
    assert torch.equal(whole[0].view(torch.uint8), again[0].view(torch.uint8)) and torch.equal(whole[1], again[1])
    tensors = ("frames_0", "frames_1", "flows_fw", "flows_bw", "valid_fw", "valid_bw")
    for n in range(2):                                                            # a batch equals its images run singly
        one = P.interpolate_frames(**dict(g, **{k: g[k][n:n + 1] for k in tensors}))
        assert torch.equal(one[0].view(torch.uint8), whole[0][n:n + 1].view(torch.uint8)) and torch.equal(one[1], whole[1][n:n + 1])
    for m, t in enumerate(kw["times"]):                                           # M = 3 equals three calls with M = 1
        one = P.interpolate_frames(**dict(g, times=t))
        assert torch.equal(one[0].view(torch.uint8), whole[0][:, m:m + 1].view(torch.uint8)) and torch.equal(one[1], whole[1][:, m:m + 1])
    for cap, pieces in ((IP.workspace_bytes(1, 3, 13, 19), 2), (IP.workspace_bytes(1, 2, 13, 19), 4)):   # cut along N; along M
        assert len(IP.plan_slices(2, 3, 13, 19, cap)) == pieces
        cut = P.interpolate_frames(**dict(g, max_workspace_bytes=cap))
        assert torch.equal(cut[0].view(torch.uint8), whole[0].view(torch.uint8)) and torch.equal(cut[1], whole[1])
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        P.interpolate_frames(**dict(g, max_workspace_bytes=IP.workspace_bytes(1, 1, 13, 19) - 8))


def test_channel_slices_are_read_in_place(P):
    """Flows as channels 1:3 of a 5-channel buffer and float32 frames as channels 2:5 of a 7-channel one (odd strides, NaN
    around them), with the masks: the bits of the dense call, and the restatement's within the bound."""
    inp, kw, ref = R.case((2, 13, 19, 3), np.float32)
    g = _gpu(inp, kw)
    dense = P.interpolate_frames(**g)
    wide = {}
    for k, (lo, c, total) in dict(flows_fw=(1, 2, 5), flows_bw=(1, 2, 5), frames_0=(2, 3, 7), frames_1=(2, 3, 7)).items():
        buf = torch.full(tuple(g[k].shape[:3]) + (total,), float("nan"), dtype=torch.float32, device="cuda")
        buf[..., lo:lo + c] = g[k]
        wide[k] = buf[..., lo:lo + c]
        assert not wide[k].is_contiguous()
    sliced = P.interpolate_frames(**dict(g, **wide))
    assert torch.equal(sliced[0].view(torch.int32), dense[0].view(torch.int32)) and torch.equal(sliced[1], dense[1])
    _check_source("slices", sliced[1].cpu().numpy(), ref)
    _check_f32("slices", sliced[0].cpu().numpy(), ref, _exp_term(ref))
    nomask = P.interpolate_frames(**dict(g, valid_fw=None, valid_bw=None))
    assert not torch.equal(nomask[1], dense[1])                                   # the masks are honoured


def test_past_the_grid_caps(P):
    """N H W = 3 * 592 * 592 = 1 051 392 source pixels, past the scatter's 4096 * 256 = 1 048 576 lanes, and N M H W =
    4 205 568 output pixels, past the resolve's 4096 * 256 * 4 = 4 194 304: against its images run singly, each under both caps."""
    N, H, W, M = 3, 592, 592, 4
    assert N * H * W > 4096 * 256 > H * W and N * M * H * W > 4096 * 1024 > M * H * W
    gen = torch.Generator(device="cuda").manual_seed(11)
    f0 = (torch.rand((N, H, W, 3), device="cuda", generator=gen) * 255).to(torch.uint8)
    f1 = (torch.rand((N, H, W, 3), device="cuda", generator=gen) * 255).to(torch.uint8)
    fw = (torch.rand((N, H, W, 2), device="cuda", generator=gen) - 0.5) * 6
    bw = (torch.rand((N, H, W, 2), device="cuda", generator=gen) - 0.5) * 6
    fw[:, ::7, ::5] = float("nan")
    times = [0.0, 0.3, 0.5, 1.0]
    whole = P.interpolate_frames(f0, f1, fw, bw, times)
    codes = torch.bincount(whole[1].flatten().long(), minlength=4).tolist()
    print(f"interp grid caps: {N * H * W} sources, {N * M * H * W} outputs, source codes {codes}")
    assert min(codes) > 0
    for n in range(N):
        one = P.interpolate_frames(f0[n:n + 1], f1[n:n + 1], fw[n:n + 1], bw[n:n + 1], times)
        assert torch.equal(one[0], whole[0][n:n + 1]) and torch.equal(one[1], whole[1][n:n + 1]), n


def _call(f0, f1, fw, bw, N, H, W, times, ws, ws_bytes, out, source, dtype_0=1, dtype_1=1, cs_0=3, cs_1=3, fw_cs=2, bw_cs=2, M=None,
          alpha=20.0, min_range=0.5, wfw=None, wbw=None):
    """pwc_interp_frames on raw addresses (integers or None)."""
    p = lambda v: None if v is None else ctypes.c_void_p(v)                        # noqa: E731
    table = None if times is None else (ctypes.c_double * max(len(times), 1))(*times)
    return _lib.lib().pwc_interp_frames(p(f0), dtype_0, cs_0, p(f1), dtype_1, cs_1, p(fw), fw_cs, p(bw), bw_cs, None, None, p(wfw),
                                        p(wbw), N, H, W, table, len(times) if M is None else M, alpha, min_range, p(ws), ws_bytes,
                                        p(out), p(source), _lib.current_stream())


def test_refusals_leave_the_outputs_untouched(P):
    N, H, W = 1, 2, 3
    fr = torch.zeros((N, H, W, 4), dtype=torch.float32, device="cuda")
    fl = torch.zeros((N, H, W, 4), dtype=torch.float32, device="cuda")
    nbytes = _lib.lib().pwc_interp_workspace_bytes(N, 2, H, W)
    assert nbytes == 8 * (N * 2 * H * W * 10 + 1) == IP.workspace_bytes(N, 2, H, W)
    assert _lib.lib().pwc_interp_workspace_bytes(N, 0, H, W) == 0 and _lib.lib().pwc_interp_workspace_bytes(N, 17, H, W) == 0
    ws = torch.full((nbytes // 8 + 1,), 0x55, dtype=torch.int64, device="cuda")
    out = torch.full((N, 2, H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    source = torch.full((N, 2, H, W), 0xEE, dtype=torch.uint8, device="cuda")
    f, l, w, o, s = fr.data_ptr(), fl.data_ptr(), ws.data_ptr(), out.data_ptr(), source.data_ptr()
    good = dict(f0=f, f1=f, fw=l, bw=l, N=N, H=H, W=W, times=[0.25, 0.75], ws=w, ws_bytes=nbytes, out=o, source=s, cs_0=4, cs_1=4,
                fw_cs=4, bw_cs=4)
    refused = [
        (EINVAL, dict(M=0)), (EINVAL, dict(times=[0.5] * 17)), (EINVAL, dict(times=[0.25, 1.5])), (EINVAL, dict(times=[float("nan"), 0.5])),
        (EINVAL, dict(times=[-0.1, 0.5])), (EINVAL, dict(alpha=float("nan"))), (EINVAL, dict(alpha=-1.0)),
        (EINVAL, dict(min_range=float("nan"))), (EINVAL, dict(min_range=-0.5)),
        (EINVAL, dict(dtype_1=0)), (EINVAL, dict(dtype_0=0)), (EINVAL, dict(dtype_0=2, dtype_1=2)),
        (EINVAL, dict(out=None)), (EINVAL, dict(source=None)), (EINVAL, dict(f0=None)), (EINVAL, dict(f1=None)),
        (EINVAL, dict(fw=None)), (EINVAL, dict(bw=None)), (EINVAL, dict(ws=None)), (EINVAL, dict(times=None, M=2)),
        (EINVAL, dict(N=0)), (EINVAL, dict(H=0)), (EINVAL, dict(W=-1)),
        (EINVAL, dict(fw_cs=1)), (EINVAL, dict(bw_cs=1)), (EINVAL, dict(cs_0=2)), (EINVAL, dict(cs_1=2)),
        (EINVAL, dict(dtype_0=0, dtype_1=0, cs_0=4, cs_1=4)), (EINVAL, dict(ws_bytes=nbytes - 8)),
        (ERANGE, dict(H=1 << 16, W=1 << 15)), (ERANGE, dict(H=1 << 20, W=1 << 20)),
        (EALIGN, dict(f0=f + 2)), (EALIGN, dict(f1=f + 1)), (EALIGN, dict(fw=l + 2)), (EALIGN, dict(bw=l + 1)), (EALIGN, dict(out=o + 2)),
        (EALIGN, dict(ws=w + 4)), (EALIGN, dict(wfw=l + 2)), (EALIGN, dict(wbw=l + 1)),
    ]
    for code, change in refused:
        assert _call(**dict(good, **change)) == code, change
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((source == 0xEE).all()) and bool((ws == 0x55).all())       # no launch, no memset
    print(f"interp refusals: {len(refused)} calls refused, outputs and workspace untouched")
    assert _call(**good) == 0 and _call(**dict(good, f0=f + 4, fw=l + 8)) == 0    # an accepted call writes every element
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((source == 3).all()) and int(ws[-1]) == 0x55
    # (the sizes that fail the range check are sizes of memory: they are refused through the C ABI above only)


def test_a_weight_beyond_the_fixed_point_poisons_the_call(P):
    """A given weight of 2^26: the flag word, every float NaN, every byte and every source code 0; no fault."""
    inp, kw, _ = R.case((1, 5, 1, 2), np.float32)
    w = np.ones((1, 5, 1), np.float32)
    w[0, 2, 0] = 2.0 ** 26
    got = _run(P, inp, dict(kw, weights_fw=w))
    assert np.isnan(got[0]).all() and (got[1] == 0).all()
    inp8 = R.case((1, 5, 1, 2), np.uint8)[0]
    got = _run(P, inp8, dict(kw, weights_fw=w))
    assert (got[0] == 0).all() and (got[1] == 0).all()
    w[0, 2, 0] = np.inf                                                           # not finite: skipped, nothing is poisoned
    assert np.isfinite(_run(P, inp, dict(kw, weights_fw=w))[0]).all()


def test_infer_continuous_interp_cli(P, tmp_path):
    """The CLI in a fresh child process: four 64 x 64 frames, un-learned weights, --interp 2 --batch 2.  The six in-between
    pictures have the frames' size; the .flo files are those of a run without the flag, byte for byte; and the pictures' bytes
    equal interpolate_frames on the same flows (computed here by the same model on the same frames, both ways)."""
    from PIL import Image
    rng = np.random.RandomState(3)
    base = rng.uniform(0, 255, size=(64, 64, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    frames = [np.roll(base, 2 * i, axis=1) for i in range(4)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o"), "--interp", "2"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    plain = subprocess.run(cli + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]
    out = tmp_path / "o" / "seq"
    for i in range(3):
        for ext in (".flo", ".png"):
            assert (tmp_path / "plain" / "seq" / f"frame_{i:02d}{ext}").read_bytes() == (out / f"frame_{i:02d}{ext}").read_bytes()
        assert not list((tmp_path / "plain" / "seq").glob("*_t*of*.png"))
    model = P.ForwardPipeline(depth=1)
    stack = np.stack(frames)
    seq_f = torch.from_numpy(stack.astype(np.float32) / 255.0).cuda()
    first, second = seq_f[:-1].contiguous(), seq_f[1:].contiguous()
    differing = 0
    for lo, hi in ((0, 2), (2, 3)):                                               # the CLI's batches
        fw_t, bw_t = model.submit(first[lo:hi], second[lo:hi]), model.submit(second[lo:hi], first[lo:hi])
        model.synchronize()
        pictures = torch.from_numpy(stack[lo:hi + 1]).cuda()
        want = P.interpolate_frames(pictures[:-1], pictures[1:], fw_t.result()[0], bw_t.result()[0], [1 / 3, 2 / 3])[0].cpu().numpy()
        for i in range(lo, hi):
            for m in range(2):
                got = np.asarray(Image.open(out / f"frame_{i:02d}_t{m + 1}of3.png"))
                assert got.shape == (64, 64, 3) and got.dtype == np.uint8
                differing += int((got != want[i - lo, m]).sum())
    print(f"interp cli: six pictures, {differing} bytes differ from interpolate_frames on the same flows")
    assert differing == 0
    assert len(list(out.glob("*_t*of3.png"))) == 6
