"""GPU tests of flow visualisation (csrc/pwc_flowvis.hip through pwcnet_amd.vis) against the float64 restatement tests/vis_ref.py.

Bounds.  flow_max_radius: bit-equal.  flow_error_color and frame tiles: byte-equal.  flow_to_color and a montage's flow tiles: a
channel value equals floor(t), t = 255 * col of the restatement, except where the restatement's own t lies within 1e-9 of an
integer r -- there it may be r or r - 1, because atan2 may differ from numpy's by a few ulp, which moves t by about 1e-11 (one
channel of every pixel has wheel value 255 at both hues, (1 - f) + f may be one ulp below 1: about a third of all values are
near an integer).  The share of values under that allowance is asserted on the restatement before the GPU is looked at: at most
0.35 in the continuous cases, 0.5 in the integer-valued one.  Unknown, masked and zero-flow pixels are exactly white: they get
no allowance (and so do not count as under it).
Measured figures: profiles/vis_gpu_test_figures.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import vis as V  # the feature: without it nothing here can be collected
from tests import vis_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 9, 15), (2, 1, 257), (2, 23, 37)]
SEEDS = {(1, 1, 1): 1, (2, 5, 7): 2, (3, 9, 15): 3, (2, 1, 257): 4, (2, 23, 37): 5}


def _device(flows, sliced):
    """The flows on the GPU: plain, or as channels 1:3 of a NaN-filled 5-channel buffer (odd channel stride, read in place)."""
    t = torch.from_numpy(flows).cuda()
    if not sliced:
        return t
    wide = torch.full(tuple(flows.shape[:3]) + (5,), float("nan"), device="cuda")
    wide[..., 1:3] = t
    return wide[..., 1:3]


def _mask(shape, seed, masked):
    if not masked:
        return None, None
    m = np.random.default_rng(100 + seed).random(shape) < 0.7
    return m, torch.from_numpy(m).cuda()


def _rule(what, got, want, t, exact, limit=0.35):
    """The colour rule of every picture of flow colours.  exact: the pixels that must be exactly white (R.white: unknown, masked,
    zero flow) -- they get no allowance, so they do not count as under it; limit: the largest share of values under it."""
    share = float(R.allowed(t, exact).mean())                              # on the restatement, before the GPU is looked at
    assert share <= limit, (what, share)
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert bool((got[exact] == 255).all()), what
    differ, near = R.check_color(got, want, t, exact)
    print(f"vis {what}: {differ} of {t.size} values differ from the restatement's bytes, {near} under the allowance")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("sliced", [False, True], ids=["plain", "slice"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_color_radius_and_error_against_restatement(shape, sliced, masked):
    seed = SEEDS[shape]
    flows = R.random_flows(*shape, seed=seed)
    if shape != (1, 1, 1):
        flows[0, 0, 0] = 0.0                                               # exactly zero flow: white
    m, dm = _mask(shape, seed, masked)
    d = _device(flows, sliced)
    what = f"{shape} {'slice' if sliced else 'plain'} {'mask' if masked else 'nomask'}"
    # the maximum: bit-equal, with a scale that rounds too
    for scale in (1.0, 0.625 * 1.1):
        want = R.max_radius(flows, m, scale)
        got = V.flow_max_radius(d, dm, scale)
        assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0],)
        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)), (what, scale)
    # each image's own maximum
    want, t = R.color(flows, None, m)
    got = V.flow_to_color(d, valid=dm)
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape + (3,) and got.is_contiguous()
    # (a one-pixel image holds its own maximum: rad / scale is 1 or one ulp below, so the channel whose wheel value is 0 at both
    # hues has t = 255 (1 - rad / scale), within 1e-13 of 0, next to the saturated one: two of its three values, whatever the seed)
    limit = 0.35 if shape != (1, 1, 1) else 2.0 / 3.0
    _rule(f"color {what}", got, want, t, R.white(flows, m), limit)
    assert torch.equal(got, V.flow_to_color(d, valid=dm))                                     # two calls
    assert torch.equal(got, V.flow_to_color(d, V.flow_max_radius(d, dm), dm))                 # None = the op's own maximum
    for n in range(shape[0]):                                                                 # alone and in a batch
        assert torch.equal(got[n:n + 1], V.flow_to_color(d[n:n + 1], valid=None if dm is None else dm[n:n + 1])), n
    # a level scale, as the CLIs pass it
    want, t = R.color(flows, None, m, 0.3125)
    _rule(f"color x 0.3125 {what}", V.flow_to_color(d, valid=dm, flow_scale=0.3125), want, t, R.white(flows, m, 0.3125), limit)
    # half the true maximum: the col * 0.75 branch; a float and a tensor of that value agree; max_rad = 0 runs
    half = 0.5 * float(R.max_radius(flows, m).max())
    want, t = R.color(flows, half, m)
    got = V.flow_to_color(d, half, dm)
    _rule(f"color half radius {what}", got, want, t, R.white(flows, m))
    assert torch.equal(got, V.flow_to_color(d, torch.full((shape[0],), half, dtype=torch.float64, device="cuda"), dm))
    want, t = R.color(flows, 0.0, m)
    _rule(f"color zero radius {what}", V.flow_to_color(d, 0.0, dm), want, t, R.white(flows, m))
    # the error map: exact
    gt = R.random_flows(*shape, seed=50 + seed, sigma=20.0)
    pred = (gt + R.random_flows(*shape, seed=60 + seed, sigma=1.0) * np.exp(np.random.default_rng(seed).uniform(-4, 4, shape))[..., None])
    pred = pred.astype(np.float32)
    gt.reshape(-1, 2)[::7] = 0.0                                           # zero ground truth: the absolute measure alone
    gt.reshape(-1, 2)[3::11] = 1e10                                        # unknown ground truth: black
    pred.reshape(-1, 2)[5::13] = np.nan                                    # unknown prediction: the last bin
    want = R.error_color(pred, gt, m)
    got = V.flow_error_color(_device(pred, sliced), _device(gt, sliced), dm)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), what
    print(f"vis error map {what}: {len(np.unique(want.reshape(-1, 3), axis=0))} colours, exact")


def test_error_map_bin_edges_on_the_gpu():
    planted = []
    for e in R.ERR_EDGES:
        x = np.float32(3.0 * e)
        planted += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))]
    pred = np.zeros((1, 1, len(planted), 2), np.float32)
    pred[0, 0, :, 1] = planted
    gt = np.zeros_like(pred)
    want = R.error_color(pred, gt)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) == 10
    assert np.array_equal(V.flow_error_color(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()).cpu().numpy(), want)
    gt[..., 0] = 64.0                                                      # the relative measure: n_err = (d / 64) / 0.05
    pred[..., 0] = 64.0
    want = R.error_color(pred, gt)
    assert np.array_equal(V.flow_error_color(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()).cpu().numpy(), want)


def test_integer_flows_and_an_unknown_image():
    """Whole-number flows along both axes and the diagonals (fk lands on wheel entries); image 2 is all unknown."""
    flows = R.random_flows(3, 9, 15, seed=7, integer=True)
    flows[0, 0, :8] = [(1, 0), (-1, 0), (0, 1), (0, -1), (2, 2), (-2, 2), (2, -2), (-3, -3)]
    flows[2] = 1e10
    flows[2, 4, 4] = (np.nan, 0.0)
    want, t = R.color(flows)
    d = torch.from_numpy(flows).cuda()
    assert V.flow_max_radius(d).cpu().numpy().tolist() == R.max_radius(flows).tolist() and R.max_radius(flows)[2] == 0.0
    got = V.flow_to_color(d)
    _rule("color integer flows (3, 9, 15)", got, want, t, R.white(flows), limit=0.5)
    assert bool((got[2] == 255).all()) and bool(R.white(flows)[2].all())


@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 1, 257), (2, 23, 37)], ids=str)
def test_special_values_change_nothing_else(shape):
    flows = R.random_flows(*shape, seed=20 + shape[2])
    big = int(np.argmax(np.square(flows[0].astype(np.float64)).sum(-1)))     # (not the pixel that holds the maximum)
    spots = [p for p in range(shape[1] * shape[2]) if p != big][:: max(1, shape[1] * shape[2] // 6)][:6]
    planted, cleared = flows.copy(), flows.copy()
    specials = [(np.nan, 1.0), (np.inf, 0.0), (0.0, -np.inf), (1e10, 1e10), (-1e10, 2.0), (np.nan, np.nan)]
    for p, s in zip(spots, specials):
        planted[0].reshape(-1, 2)[p] = s
        cleared[0].reshape(-1, 2)[p] = 0.0
    a, b = torch.from_numpy(planted).cuda(), torch.from_numpy(cleared).cuda()
    assert torch.equal(V.flow_max_radius(a).view(torch.int64), V.flow_max_radius(b).view(torch.int64))
    assert np.array_equal(V.flow_max_radius(a).cpu().numpy(), R.max_radius(planted))
    got = V.flow_to_color(a)
    assert torch.equal(got, V.flow_to_color(b))
    assert bool((got[0].reshape(-1, 3)[spots[:len(specials)]] == 255).all())


# ------------------------------------------------------------------ montages and frame tiles
MONTAGES = [((24, 40), [(3, 5), (6, 10), (24, 40)], [0.3125, 0.625, 1.25]),
            ((23, 37), [(6, 10), (6, 10)], [0.3125, 1.0]),                 # tile width 38: the next tile starts at an odd byte offset
            ((12, 20), [(24, 40)], [1.25])]                                # a downscale


@pytest.mark.parametrize("float_frames", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("frame,sizes,scales", MONTAGES, ids=["24x40", "23x37", "12x20"])
def test_montage_against_restatement(frame, sizes, scales, float_frames):
    rng = np.random.default_rng(frame[0])
    u8 = rng.integers(0, 256, (2,) + frame + (3,), dtype=np.uint8)
    frames = (u8.astype(np.float32) / np.float32(255.0)) if float_frames else u8
    flows = [R.random_flows(2, a, b, seed=10 * a + b, sigma=3.0) for a, b in sizes]
    flows[0][1, 0, 0] = (np.nan, 1e10)
    want, t = R.montage(frames, flows, scales)
    dflows = [_device(f, sliced=(l % 2 == 1)) for l, f in enumerate(flows)]
    got = V.pyramid_montage(torch.from_numpy(frames).cuda(), dflows, scales)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    w = frame[1]
    assert np.array_equal(got[:, :, :w].cpu().numpy(), u8)                 # the frame tile: exact; u8 / 255 in float32 gives back u8
    _rule(f"montage {frame} {'f32' if float_frames else 'u8'} frames", got, want, t, R.montage_white(frames, flows, scales))
    assert torch.equal(got, V.pyramid_montage(torch.from_numpy(frames).cuda(), dflows, scales))
    for n in range(2):
        alone = V.pyramid_montage(torch.from_numpy(frames[n:n + 1]).cuda(), [f[n:n + 1] for f in dflows], scales)
        assert torch.equal(alone, got[n:n + 1]), n
    # a flow tile of the montage is flow_to_color of that flow, resampled
    ry, rx = R.tile_indices(frame[0], *sizes[0])
    tile = V.flow_to_color(dflows[0], flow_scale=scales[0]).cpu().numpy()[:, ry][:, :, rx]
    assert np.array_equal(got[:, :, w:w + len(rx)].cpu().numpy(), tile)


def test_float_frames_and_seven_flows():
    odd = np.array([np.nan, -1.0, 2.0, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.25, 1.0, 0.0, 0.999], np.float32)
    frames = np.broadcast_to(odd[None, None, :, None], (1, 2, len(odd), 3)).copy()
    flow = np.zeros((1, 2, 3, 2), np.float32)
    d = torch.from_numpy(flow).cuda()
    got = V.pyramid_montage(torch.from_numpy(frames).cuda(), [d] * 7)
    assert tuple(got.shape) == (1, 2, len(odd) + 7 * 3, 3)                  # seven flows accepted
    assert np.array_equal(got[:, :, :len(odd)].cpu().numpy(), R.frame_bytes(frames))
    assert bool((got[:, :, len(odd):] == 255).all())
    with pytest.raises(ValueError, match="flows_list: expected a list of 1 to 7"):
        V.pyramid_montage(torch.from_numpy(frames).cuda(), [d] * 8)         # eight refused
    with pytest.raises(ValueError, match="flows_gt: the tensor is on cpu"):
        V.flow_error_color(d, torch.from_numpy(flow))
    with pytest.raises(ValueError, match="max_rad: the tensor is on cpu"):
        V.flow_to_color(d, torch.zeros(1, dtype=torch.float64))


def test_output_off_a_dword_boundary_is_written_byte_by_byte():
    """The C entry point with an output 1, 2 and 3 bytes off a 4-byte boundary (vis.py's own outputs never are): every run takes
    the byte path, the bytes are those of the dword path and nothing outside the picture is touched."""
    from pwcnet_amd import _lib
    flows = R.random_flows(2, 5, 7, seed=31)
    d = torch.from_numpy(flows).cuda()
    rad = V.flow_max_radius(d)
    want = V.flow_to_color(d, rad)
    size = want.numel()
    tile = _lib.VisTile(src=d.data_ptr(), gt=None, valid=None, max_rad=rad.data_ptr(), kind=_lib.VIS_FLOW, src_cs=2, gt_cs=0, src_h=5,
                        src_w=7, x0=0, tile_w=7, flow_scale=1.0)
    table = (_lib.VisTile * 1)(tile)
    for off in (1, 2, 3):
        buf = torch.full((size + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        _lib.check(_lib.lib().pwc_flow_vis_tiles_u8(_lib.ctypes.cast(table, _lib.ctypes.c_void_p), 1, 2, 5, 7,
                                                    _lib.ctypes.c_void_p(buf.data_ptr() + off), _lib.current_stream()), "tiles")
        assert torch.equal(buf[off:off + size].view(want.shape), want), off
        assert bool((buf[:off] == 0x5A).all()) and bool((buf[off + size:] == 0x5A).all()), off


def test_more_runs_than_the_grid_has_lanes():
    """A picture of more than 16384 x 256 runs of four pixels: the picture kernel's grid-stride loop.  A uint8 frame beside a
    2 x 2 flow blown up to the frame's height; compared on the GPU."""
    h = w = 4104                                                           # 4104 x 8208 pixels = 8.4 M runs, twice the grid
    g = torch.Generator(device="cuda").manual_seed(2)
    frames = torch.randint(0, 256, (1, h, w, 3), device="cuda", generator=g, dtype=torch.uint8)
    flow = torch.tensor([[[[1.0, 0.5], [-2.0, 0.25]], [[0.0, 0.0], [3.0, -1.5]]]], device="cuda")
    got = V.pyramid_montage(frames, [flow])
    assert tuple(got.shape) == (1, h, 2 * w, 3)
    assert torch.equal(got[:, :, :w], frames)
    small = V.flow_to_color(flow)
    idx = torch.arange(h, device="cuda") * 2 // h
    assert torch.equal(got[:, :, w:], small[:, idx][:, :, idx])


# ------------------------------------------------------------------ the CLIs, each in a fresh child process
def _frames(tmp_path, count, size=(64, 128)):
    from PIL import Image
    rng = np.random.RandomState(3)
    base = rng.uniform(0, 255, size=size + (3,)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    paths = []
    for i in range(count):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(seq / f"frame_{i:02d}.png")
        paths.append(str(seq / f"frame_{i:02d}.png"))
    return seq, paths, [np.roll(base, 2 * i, axis=1) for i in range(count)]


def _run(cmd):
    run = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    return run


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_infer_cli_vis(tmp_path):
    """Un-learned model, 64 x 128 frames.  Without --vis and with --vis host: today's bytes, flow_io.flow_to_color on the
    copied-back flows of the same forward.  --vis gpu: the same .flo, PNGs under the colour rule."""
    import pwcnet_amd
    from pwcnet_amd import flow_io
    _, paths, frames = _frames(tmp_path, 2)
    outs = {}
    for tag, extra in (("plain", []), ("host", ["--vis", "host"]), ("gpu", ["--vis", "gpu"])):
        outs[tag] = tmp_path / tag
        _run([os.path.join(ROOT, "infer.py"), "--input_images", *paths, "--out", str(outs[tag])] + extra)
    x = torch.from_numpy(np.array(frames, dtype=np.float32) / 255.0).cuda()
    model = pwcnet_amd.PWCDCNet(range_check="sync")
    flow_final, flows = model(x[0:1], x[1:2])
    names = [f"flow_level{l}.png" for l in range(len(flows))] + ["flow_final.png"]
    fields = [f[0].cpu().numpy() * (20.0 / 2 ** (model.num_levels - l)) for l, f in enumerate(flows)] + [flow_final[0].cpu().numpy()]
    assert np.array_equal(flow_io.read_flo(str(outs["plain"] / "flow_final.flo")), fields[-1])
    for name, field in zip(names, fields):
        assert np.array_equal(_png(outs["plain"] / name), flow_io.flow_to_color(field)), name
        assert (outs["host"] / name).read_bytes() == (outs["plain"] / name).read_bytes(), name
        want, t = R.color(field[None])
        _rule(f"infer.py --vis gpu {name}", _png(outs["gpu"] / name)[None], want, t, R.white(field[None]))
    for tag in ("host", "gpu"):
        assert (outs[tag] / "flow_final.flo").read_bytes() == (outs["plain"] / "flow_final.flo").read_bytes(), tag
    assert sorted(p.name for p in outs["gpu"].iterdir()) == sorted(p.name for p in outs["plain"].iterdir())


def test_infer_continuous_cli_vis(tmp_path):
    """Three frames, one batch of two pairs.  Default and --vis host: infer_continuous.pyramid_montage on the copied-back
    pyramid of the same forward; --vis gpu: the same .flo files, montages under the colour rule."""
    import importlib.util
    import pwcnet_amd
    spec = importlib.util.spec_from_file_location("infer_continuous_under_test", os.path.join(ROOT, "infer_continuous.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    seq, _, frames = _frames(tmp_path, 3)
    outs = {}
    for tag, extra in (("plain", []), ("host", ["--vis", "host"]), ("gpu", ["--vis", "gpu"])):
        outs[tag] = tmp_path / tag / "seq"
        _run([os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--out",
              str(tmp_path / tag)] + extra)
    model = pwcnet_amd.ForwardPipeline(depth=1)
    x = torch.from_numpy(np.stack(frames).astype(np.float32) / 255.0).cuda()
    ticket = model.submit(x[:-1].contiguous(), x[1:].contiguous())
    model.synchronize()
    _, flows = ticket.result()
    levels = model.nets[0].num_levels
    flows = [f.cpu().numpy() for f in flows]
    scales = [20.0 / 2 ** (levels - l) for l in range(len(flows))]
    want, t = R.montage(np.stack(frames[:2]), flows, scales)
    white = R.montage_white(np.stack(frames[:2]), flows, scales)
    for k in range(2):
        name = f"frame_{k:02d}.png"
        host = cli.pyramid_montage(frames[k], [f[k] * (20.0 / 2 ** (levels - l)) for l, f in enumerate(flows)])
        assert np.array_equal(_png(outs["plain"] / name), host), name
        assert (outs["host"] / name).read_bytes() == (outs["plain"] / name).read_bytes(), name
        _rule(f"infer_continuous.py --vis gpu {name}", _png(outs["gpu"] / name)[None], want[k:k + 1], t[k:k + 1], white[k:k + 1])
        for tag in ("host", "gpu"):
            flo = f"frame_{k:02d}.flo"
            assert (outs[tag] / flo).read_bytes() == (outs["plain"] / flo).read_bytes(), (tag, flo)


def test_infer_continuous_cli_vis_with_fit_pad(tmp_path):
    """--fit pad --vis gpu: 70 x 130 frames go up as uint8 and are drawn at their own size beside the pyramid of the padded
    128 x 192 forward (tile widths 105, 105, 105, 105, 105 at height 70 from levels 2 x 3 .. 32 x 48).  The host run's montage
    equals the restatement on the pyramid of the same forward made here; the gpu run's is under the colour rule, same .flo."""
    import pwcnet_amd
    seq, _, frames = _frames(tmp_path, 3, size=(70, 130))
    outs = {}
    for tag in ("host", "gpu"):
        outs[tag] = tmp_path / tag / "seq"
        _run([os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--fit", "pad", "--vis", tag,
              "--out", str(tmp_path / tag)])
    model = pwcnet_amd.ForwardPipeline(depth=1)
    shown = torch.from_numpy(np.stack(frames)).cuda()
    x, _ = pwcnet_amd.fit_frames(shown, "pad")
    ticket = model.submit(x[:-1].contiguous(), x[1:].contiguous())
    model.synchronize()
    flows = [f.cpu().numpy() for f in ticket.result()[1]]
    assert [f.shape[1:3] for f in flows] == [(2, 3), (4, 6), (8, 12), (16, 24), (32, 48)]
    levels = model.nets[0].num_levels
    scales = [20.0 / 2 ** (levels - l) for l in range(len(flows))]
    want, t = R.montage(np.stack(frames[:2]), flows, scales)
    white = R.montage_white(np.stack(frames[:2]), flows, scales)
    assert want.shape == (2, 70, 130 + 5 * 105, 3)
    for k in range(2):
        name = f"frame_{k:02d}.png"
        assert np.array_equal(_png(outs["host"] / name), want[k]), name
        got = _png(outs["gpu"] / name)
        assert np.array_equal(got[:, :130], frames[k])
        _rule(f"infer_continuous.py --fit pad --vis gpu {name}", got[None], want[k:k + 1], t[k:k + 1], white[k:k + 1])
        assert (outs["gpu"] / f"frame_{k:02d}.flo").read_bytes() == (outs["host"] / f"frame_{k:02d}.flo").read_bytes(), k


def test_evaluate_cli_save_vis(tmp_path):
    """Two pairs with a sparse ground truth: three pictures per index; the error map exact, the two flow pictures under the
    colour rule with the ground truth's largest valid magnitude as the radius of both."""
    from pwcnet_amd import flow_io
    _, paths, _ = _frames(tmp_path, 3)
    rng = np.random.default_rng(9)
    lines, gts = [], []
    for i in range(2):
        gt = (rng.standard_normal((64, 128, 2)) * (0.02 + 0.3 * i)).astype(np.float32)
        gt[rng.random((64, 128)) < 0.2] = 1e10
        flow_io.write_flo(str(tmp_path / f"gt_{i}.flo"), gt)
        gts.append(gt)
        lines.append(f"{paths[i]} {paths[i + 1]} {tmp_path / f'gt_{i}.flo'}")
    (tmp_path / "pairs.txt").write_text("\n".join(lines) + "\n")
    out = tmp_path / "saved"
    _run([os.path.join(ROOT, "evaluate.py"), "--list", str(tmp_path / "pairs.txt"), "--save_dir", str(out), "--save_vis"])
    assert sorted(p.name for p in out.iterdir()) == sorted(f"{i:06d}{s}" for i in range(2) for s in (".flo", ".png", "_gt.png", "_err.png"))
    for i, gt in enumerate(gts):
        pred = flow_io.read_flo(str(out / f"{i:06d}.flo"))
        valid = flow_io.flow_valid(gt)
        assert np.array_equal(_png(out / f"{i:06d}_err.png"), R.error_color(pred[None], gt[None], valid[None])[0]), i
        rad = R.max_radius(gt[None], valid[None])
        want, t = R.color(pred[None], rad)
        _rule(f"evaluate.py --save_vis {i:06d}.png", _png(out / f"{i:06d}.png")[None], want, t, R.white(pred[None]))
        want, t = R.color(gt[None], rad, valid[None])
        _rule(f"evaluate.py --save_vis {i:06d}_gt.png", _png(out / f"{i:06d}_gt.png")[None], want, t, R.white(gt[None], valid[None]))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--list", str(tmp_path / "pairs.txt"), "--save_dir",
                          str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["000000.flo", "000001.flo"]
    assert (tmp_path / "plain" / "000000.flo").read_bytes() == (out / "000000.flo").read_bytes()
