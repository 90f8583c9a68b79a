"""The training augmentation on the GPU (pwcnet_amd/augment.py over csrc/pwc_augment.hip) against the float64 reference of
tests/augment_ref.py, and train.py --augment end to end.

Bound.  The kernel forms every value in double with the reference's own operations and rounds it to float32 once, so per
element |y - ref64| <= 0.5 ulp32(ref64) + 1e-9 S, S the largest magnitude among the element's corners (for the flow also
max(H, W), the size of the coordinates its value is a difference of): three double operations on coordinates below 2^11 px move
a coordinate by less than 1e-12 px, three orders inside the 1e-9 S slack, which in turn stays 30 x under a float32 half-ulp.
Where a frame's gamma is not 1 the allowance is one ulp instead of half: the GPU's and numpy's double pow may differ in the last
bit.  out_valid and the nearest-mode taps are compared exactly: the geometries are explicit records whose sample coordinates
stay 1e-6 px away from every decision boundary (tests/test_host_augment.py asserts that, and that the same arithmetic in
float32 misses this bound at every geometry).  Every test prints its figures before it asserts
(profiles/augment_gpu_test_figures.txt).
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

from tests import augment_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    torch.cuda.set_device(0)
    return pwcnet_amd


def bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else t
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_inputs(g, frames):
    im0, im1, flow, valid = R.inputs(g)
    if frames == "float32":
        im0, im1 = R.to_float32(im0), R.to_float32(im1)
    cu = lambda a: None if a is None else torch.from_numpy(a).cuda()
    return cu(im0), cu(im1), cu(flow), cu(valid)


@pytest.mark.parametrize("interp", ["bilinear", "nearest"])
@pytest.mark.parametrize("frames", ["uint8", "float32"])
@pytest.mark.parametrize("g", range(len(R.GEOMETRIES)), ids=R.GEOM_IDS)
def test_augment_pairs(pa, g, frames, interp):
    name, N, (H, W), (OH, OW), sparse = R.GEOMETRIES[g]
    ref = R.reference(g, interp == "nearest")
    assert ref["margin"] >= R.MIN_MARGIN
    im0, im1, flow, valid = device_inputs(g, frames)
    P = R.records(g)
    x0, x1, f, v = pa.augment_pairs(im0, im1, P, (OH, OW), flows=flow, valid=valid, flow_interp=interp)
    torch.cuda.synchronize()
    assert tuple(x0.shape) == tuple(x1.shape) == (N, OH, OW, 3) and tuple(f.shape) == (N, OH, OW, 2) and tuple(v.shape) == (N, OH, OW)
    assert x0.dtype == x1.dtype == f.dtype == torch.float32 and v.dtype == torch.bool
    got = {"out0": x0.cpu().numpy(), "out1": x1.cpu().numpy(), "flow": f.cpu().numpy(), "valid": v.cpu().numpy()}
    bad = R.violations(got, ref)
    print(f"augment {name} {frames} {interp}: " + ", ".join(f"{k} {c} off (worst excess {w:.2e})" for k, (c, w) in bad.items())
          + f"; valid {got['valid'].mean():.3f}, margin {ref['margin']:.2e} px, allowed ulps {ref['ulps0'].tolist()} {ref['ulps1'].tolist()}")
    assert all(c == 0 for c, _ in bad.values()), (name, frames, interp, bad)
    assert np.all(got["flow"][~got["valid"]] == 0) and np.isfinite(got["flow"]).all() and float(np.abs(got["flow"]).max()) < 1e3
    # two calls, the same bits; the records as a float64 tensor on the device are the same call
    y0, y1, yf, yv = pa.augment_pairs(im0, im1, torch.from_numpy(P).cuda(), (OH, OW), flows=flow, valid=valid, flow_interp=interp)
    assert torch.equal(x0, y0) and torch.equal(x1, y1) and np.array_equal(bits(f), bits(yf)) and torch.equal(v, yv)


@pytest.mark.parametrize("frames", ["uint8", "float32"])
def test_flows_none_writes_only_the_frames(pa, frames):
    """Through the wrapper (None, None come back) and through the C entry with NULL flow outputs: the frames are those of the
    call with a flow, and guard words behind them stay untouched."""
    from pwcnet_amd import _lib
    g = 0
    name, N, (H, W), (OH, OW), _ = R.GEOMETRIES[g]
    im0, im1, flow, _ = device_inputs(g, frames)
    P = R.records(g)
    x0, x1, f, v = pa.augment_pairs(im0, im1, P, (OH, OW))
    assert f is None and v is None
    y0, y1, _, _ = pa.augment_pairs(im0, im1, P, (OH, OW), flows=flow)
    assert torch.equal(x0, y0) and torch.equal(x1, y1)
    guard, n3 = 12345.0, N * OH * OW * 3
    b0, b1 = torch.full((n3 + 64,), guard, device="cuda"), torch.full((n3 + 64,), guard, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    Pd = torch.from_numpy(P).cuda()
    _lib.check(_lib.lib().pwc_augment_pairs_f32(p(im0), p(im1), int(frames == "uint8"), None, None, p(Pd), p(b0), p(b1), None, None,
                                                N, H, W, OH, OW, 0, _lib.current_stream()))
    torch.cuda.synchronize()
    assert bool((b0[n3:] == guard).all()) and bool((b1[n3:] == guard).all())
    assert torch.equal(b0[:n3].reshape(N, OH, OW, 3), x0) and torch.equal(b1[:n3].reshape(N, OH, OW, 3), x1)


@pytest.mark.parametrize("frames", ["uint8", "float32"])
def test_crop_params_is_the_host_crop(pa, frames):
    """The crop the host path forms today -- frame[y0:y0 + ch, x0:x0 + cw] / 255 in float32 -- the flow and a sparse mask cut
    the same way: torch.equal."""
    rng = np.random.RandomState(21)
    N, H, W, ch, cw = 3, 41, 67, 17, 35                       # more than one workgroup each way, ragged edges
    u8 = rng.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    u8[0, :16, :16, 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)       # all 256 values inside sample 0's window
    host = [torch.from_numpy(u8.astype(np.float32)) / 255.0, torch.from_numpy(u8[::-1].astype(np.float32)) / 255.0]   # train.py's
    flow = rng.uniform(-5, 5, size=(N, H, W, 2)).astype(np.float32)
    valid = rng.uniform(size=(N, H, W)) >= 0.3
    flow[~valid] = 1e10
    y0, x0 = np.array([0, 24, 11]), np.array([0, 32, 5])
    src = [torch.from_numpy(u8), torch.from_numpy(np.ascontiguousarray(u8[::-1]))] if frames == "uint8" else host
    o0, o1, f, v = pa.augment_pairs(src[0].cuda(), src[1].cuda(), pa.crop_params(N, y0, x0), (ch, cw), flows=torch.from_numpy(flow).cuda(),
                                    valid=torch.from_numpy(valid).cuda())
    for n in range(N):
        sl = (n, slice(y0[n], y0[n] + ch), slice(x0[n], x0[n] + cw))
        assert torch.equal(o0[n].cpu(), host[0][sl]) and torch.equal(o1[n].cpu(), host[1][sl])
        assert torch.equal(v[n].cpu(), torch.from_numpy(valid[sl]))
        want = np.where(valid[sl][..., None], flow[sl], np.float32(0))
        assert np.array_equal(bits(f[n]), bits(want))
    # dense labels: the flow itself
    flow = np.where(valid[..., None], flow, np.float32(0.5))
    _, _, f, v = pa.augment_pairs(src[0].cuda(), src[1].cuda(), pa.crop_params(N, y0, x0), (ch, cw), flows=torch.from_numpy(flow).cuda())
    assert bool(v.all())
    for n in range(N):
        assert np.array_equal(bits(f[n]), bits(flow[n, y0[n]:y0[n] + ch, x0[n]:x0[n] + cw]))


def test_argument_errors(pa):
    """The C entry returns its codes without a launch (the outputs keep their fill); the wrapper raises ValueError with the reason."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    im = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    fl = torch.zeros((1, 8, 8, 2), device="cuda")
    va = torch.ones((1, 8, 8), dtype=torch.bool, device="cuda")
    P = torch.from_numpy(pa.crop_params(1, 0, 0)).cuda()
    o0, o1 = torch.full((1, 4, 4, 3), 7.0, device="cuda"), torch.full((1, 4, 4, 3), 7.0, device="cuda")
    of, ov = torch.full((1, 4, 4, 2), 7.0, device="cuda"), torch.full((1, 4, 4), 7, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = _lib.current_stream()
    f = L.pwc_augment_pairs_f32
    assert f(None, p(im), 1, p(fl), p(va), p(P), p(o0), p(o1), p(of), p(ov), 1, 8, 8, 4, 4, 0, s) == -1
    assert f(p(im), p(im), 1, p(fl), p(va), None, p(o0), p(o1), p(of), p(ov), 1, 8, 8, 4, 4, 0, s) == -1
    assert f(p(im), p(im), 1, p(fl), p(va), p(P), p(o0), None, p(of), p(ov), 1, 8, 8, 4, 4, 0, s) == -1
    assert f(p(im), p(im), 1, p(fl), p(va), p(P), p(o0), p(o1), None, p(ov), 1, 8, 8, 4, 4, 0, s) == -1     # a flow needs its outputs
    assert f(p(im), p(im), 1, p(fl), p(va), p(P), p(o0), p(o1), p(of), None, 1, 8, 8, 4, 4, 0, s) == -1
    assert f(p(im), p(im), 1, p(fl), p(va), p(P), p(o0), p(o1), p(of), p(ov), 0, 8, 8, 4, 4, 0, s) == -1
    assert f(p(im), p(im), 1, p(fl), p(va), p(P), p(o0), p(o1), p(of), p(ov), 1, 8, 8, 4, 0, 0, s) == -1
    assert f(p(im), p(im), 1, p(fl), p(va), ctypes.c_void_p(P.data_ptr() + 4), p(o0), p(o1), p(of), p(ov), 1, 8, 8, 4, 4, 0, s) == -2
    assert f(p(im), p(im), 1, p(fl), p(va), p(P), p(o0), p(o1), ctypes.c_void_p(of.data_ptr() + 4), p(ov), 1, 8, 8, 4, 4, 0, s) == -2
    assert f(p(im), p(im), 1, p(fl), p(va), p(P), p(o0), p(o1), p(of), p(ov), 65536, 8, 8, 4, 4, 0, s) == -3
    torch.cuda.synchronize()
    assert bool((o0 == 7.0).all()) and bool((o1 == 7.0).all()) and bool((of == 7.0).all()) and bool((ov == 7).all())
    imf = torch.zeros((1, 8, 8, 3), device="cuda")
    rec = pa.crop_params(1, 0, 0)
    with pytest.raises(ValueError, match="contiguous"):
        pa.augment_pairs(torch.zeros((1, 8, 3, 8), device="cuda").permute(0, 1, 3, 2), imf, rec, (4, 4))
    with pytest.raises(ValueError, match="dtype"):
        pa.augment_pairs(imf.half(), imf.half(), rec, (4, 4))
    with pytest.raises(ValueError, match="shape"):
        pa.augment_pairs(torch.zeros((1, 8, 8, 4), device="cuda"), torch.zeros((1, 8, 8, 4), device="cuda"), rec, (4, 4))
    with pytest.raises(ValueError, match="frames differ"):
        pa.augment_pairs(imf, im, rec, (4, 4))
    with pytest.raises(ValueError, match="CUDA"):
        pa.augment_pairs(imf.cpu(), imf.cpu(), rec, (4, 4))
    with pytest.raises(ValueError, match="params"):
        pa.augment_pairs(imf, imf, rec.astype(np.float32), (4, 4))
    with pytest.raises(ValueError, match="params"):
        pa.augment_pairs(imf, imf, pa.crop_params(2, 0, 0), (4, 4))
    with pytest.raises(ValueError, match="flow_interp"):
        pa.augment_pairs(imf, imf, rec, (4, 4), flows=fl, flow_interp="cubic")
    with pytest.raises(ValueError, match="flows must be"):
        pa.augment_pairs(imf, imf, rec, (4, 4), flows=torch.zeros((1, 8, 9, 2), device="cuda"))
    with pytest.raises(ValueError, match="torch.bool"):
        pa.augment_pairs(imf, imf, rec, (4, 4), flows=fl, valid=va.to(torch.uint8))
    with pytest.raises(ValueError, match="belongs to flows"):
        pa.augment_pairs(imf, imf, rec, (4, 4), valid=va)
    with pytest.raises(ValueError, match="crop_shape"):
        pa.augment_pairs(imf, imf, rec, (0, 4))


# ---------------------------------------------------------------------------------------------- train.py
def run_train(tmp_path, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                           "64", "128", "--synthetic_pairs", "8", "--model_dir", str(tmp_path), *extra],
                          capture_output=True, text=True, timeout=300, cwd=ROOT)


@pytest.mark.parametrize("loss", ["multiscale", "unsup"])
def test_train_cli_with_full_augmentation(tmp_path, loss):
    from pwcnet_amd import PWCDCNet, ckpt
    out = run_train(tmp_path, "--augment", "full", *(("--loss", "unsup") if loss == "unsup" else ()))
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    if loss == "unsup":
        steps = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
        assert len(steps) == 3, steps                   # 8 pairs: 1 for validation, 7 to train on, batch 2, drop_last
        for ln in steps:
            assert np.isfinite(float(ln.split("loss/unsup")[1].split()[0])), ln
    epoch = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch 1:")]
    assert len(epoch) == 1 and "global_step 3" in epoch[0]
    tag = "loss/unsup" if loss == "unsup" else "loss/pwc"
    assert np.isfinite(float(epoch[0].split(tag)[1].split()[0])) and np.isfinite(float(epoch[0].split("EPE/val")[1].split()[0]))
    PWCDCNet().load_weights(ckpt.load_weights(str(tmp_path / "model_1.ckpt")))


def test_train_cli_augment_none_is_the_run_without_the_flag(tmp_path):
    """The step lines of the label-free run (the supervised loop prints none) and everything of the epoch line in front of
    the throughput: equal, character for character."""
    def lines(out):
        keep = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
        keep += [ln.split("global_step")[0] for ln in out.stdout.splitlines() if ln.startswith("epoch ")]
        return keep
    plain = run_train(tmp_path / "a", "--loss", "unsup")
    flagged = run_train(tmp_path / "b", "--loss", "unsup", "--augment", "none")
    print(plain.stdout[-1500:], plain.stderr[-1500:], flagged.stdout[-1500:], flagged.stderr[-1500:])
    assert plain.returncode == 0 and flagged.returncode == 0
    assert len(lines(plain)) == 4 and lines(plain) == lines(flagged)
