"""CPU tests of flow visualisation: the float64 restatement tests/vis_ref.py pinned to the host code that exists
(flow_io.flow_to_color, infer_continuous.pyramid_montage with its float32 level scaling), the error map's table and bin edges at
planted values, the library's colour wheel against flow_io.color_wheel(), every refusal pwcnet_amd.vis raises before it calls the
library, the library's own argument checks (they return before any launch), and the new flags of the three CLIs."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from pwcnet_amd import flow_io
from pwcnet_amd import vis as V  # the feature: without it nothing here can be collected
from tests import vis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_cli(name):
    spec = importlib.util.spec_from_file_location(name + "_under_test", os.path.join(ROOT, name + ".py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ------------------------------------------------------------------ the restatement against the host code
@pytest.mark.parametrize("shape,seed,integer", [((2, 5, 7), 1, False), ((3, 9, 15), 2, False), ((2, 23, 37), 3, False),
                                                ((2, 9, 15), 4, True)])
def test_restatement_bytes_equal_flow_io(shape, seed, integer):
    flows = R.random_flows(*shape, seed=seed, integer=integer)
    flows[0, 0, 0] = (np.nan, 1.0)
    flows[-1, -1, -1] = (1e10, 1e10)
    flows[-1, 0, -1] = (np.inf, -np.inf)
    for scale in (1.0, 0.3125, 2.5):
        got, t = R.color(flows, None, None, scale)
        assert np.array_equal(np.floor(t).astype(np.uint8), got)
        rad = R.max_radius(flows, None, scale)
        for n in range(shape[0]):
            host = flows[n] * scale                                    # a float32 array times a Python float: float32
            assert host.dtype == np.float32
            assert np.array_equal(got[n], flow_io.flow_to_color(host)), (n, scale)
            u, v = host[..., 0].astype(np.float64), host[..., 1].astype(np.float64)
            assert rad[n] == np.sqrt(u * u + v * v)[flow_io.flow_valid(host)].max()
        # a given radius, inside and beyond it
        for max_rad in (0.5 * float(rad.max()), 3.0 * float(rad.max()), 0.0):
            got, _ = R.color(flows, max_rad, None, scale)
            for n in range(shape[0]):
                assert np.array_equal(got[n], flow_io.flow_to_color(flows[n] * scale, max_rad)), (n, scale, max_rad)
    # a mask is the same as unknown flow at the masked pixels
    valid = np.random.default_rng(seed).random(shape) < 0.7
    cleared = flows.copy()
    cleared[~valid] = np.nan
    assert np.array_equal(R.color(flows, None, valid)[0], R.color(cleared)[0])
    assert np.array_equal(R.max_radius(flows, valid), R.max_radius(cleared))
    # unknown, masked and zero flow: white; an image that is all unknown: maximum 0, all white
    got = R.color(cleared)[0]
    assert bool((got[~valid] == 255).all())
    blank = np.full((1, 3, 4, 2), 1e10, np.float32)
    assert R.max_radius(blank).tolist() == [0.0] and bool((R.color(blank)[0] == 255).all())
    assert bool((R.color(np.zeros((1, 3, 4, 2), np.float32))[0] == 255).all())


def test_restatement_montage_equals_infer_continuous():
    cli = _load_cli("infer_continuous")
    rng = np.random.default_rng(11)
    num_levels = 6
    for (h, w), sizes, dtype in (((24, 40), [(3, 5), (6, 10), (24, 40)], np.uint8), ((23, 37), [(6, 10)], np.uint8),
                                 ((12, 20), [(24, 40)], np.float32), ((64, 128), [(1, 2), (2, 4), (4, 8), (8, 16), (16, 32)], np.uint8)):
        u8 = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        frames = u8 if dtype == np.uint8 else (u8.astype(np.float32) / 255.0)
        flows = [(rng.standard_normal((2, a, b, 2)) * 0.4).astype(np.float32) for a, b in sizes]
        scales = [20.0 / 2 ** (num_levels - l) for l in range(len(flows))]
        got, t = R.montage(frames, flows, scales)
        for k in range(2):
            pyr = [f[k] * (20.0 / 2 ** (num_levels - l)) for l, f in enumerate(flows)]      # the CLI's line
            assert all(p.dtype == np.float32 for p in pyr)
            want = cli.pyramid_montage(u8[k], pyr)
            assert got[k].shape == want.shape and np.array_equal(got[k], want)
        assert got.shape[2] == w + sum(h * b // a for a, b in sizes)
        assert bool(np.isnan(t[:, :, :w]).all()) and not bool(np.isnan(t[:, :, w:]).any())
    # the non-divisible map: a 6 x 10 flow at height 23 is 38 columns wide, the next tile starts at an odd byte offset
    ry, rx = R.tile_indices(23, 6, 10)
    assert len(rx) == 38 and ry.max() == 5 and rx.max() == 9 and ((37 + 38) * 3) % 4 == 1


def test_frame_bytes():
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    assert np.array_equal(R.frame_bytes(u8), u8)
    assert np.array_equal(R.frame_bytes(u8.astype(np.float32) / np.float32(255.0)), u8)          # u8 / 255 in float32 gives back u8
    odd = np.array([np.nan, -1.0, 2.0, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 2.5 / 255], np.float32).reshape(1, 1, 8, 1).repeat(3, axis=3)
    want = [0, 0, 255, 255, 0] + [int(np.rint(255.0 * float(np.float32(x)))) for x in (0.5 / 255, 1.5 / 255, 2.5 / 255)]
    assert R.frame_bytes(odd)[0, 0, :, 0].tolist() == want


# ------------------------------------------------------------------ the error map
TABLE = [(0, 0.0625, (49, 54, 149)), (0.0625, 0.125, (69, 117, 180)), (0.125, 0.25, (116, 173, 209)), (0.25, 0.5, (171, 217, 233)),
         (0.5, 1, (224, 243, 248)), (1, 2, (254, 224, 144)), (2, 4, (253, 174, 97)), (4, 8, (244, 109, 67)), (8, 16, (215, 48, 39)),
         (16, float("inf"), (165, 0, 38))]


def _table_color(n_err):
    for lo, hi, rgb in TABLE:
        if lo <= n_err < hi:
            return rgb
    raise AssertionError(n_err)


def test_error_map_table_and_edges():
    assert len(R.ERR_COLORS) == len(TABLE) == len(R.ERR_EDGES) + 1
    for k, (lo, hi, rgb) in enumerate(TABLE):
        assert tuple(R.ERR_COLORS[k].tolist()) == rgb
        assert R.error_bin(lo) == k and R.error_bin(np.nextafter(hi, 0)) == k
        if k:
            assert R.error_bin(np.nextafter(lo, 0)) == k - 1
    # planted through the whole function, on and beside every edge.  Zero ground truth: n_err = d_err / 3, and 3 * edge is a
    # float32 whose third is the edge exactly
    edges = [lo for lo, _, _ in TABLE[1:]]
    planted = []
    for e in edges:
        x = np.float32(3.0 * e)
        planted += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))]
    planted += [np.float32(0.0), np.float32(1e6)]
    pred = np.zeros((1, 1, len(planted), 2), np.float32)
    pred[0, 0, :, 0] = planted
    gt = np.zeros_like(pred)
    got = R.error_color(pred, gt)
    for i, x in enumerate(planted):
        assert tuple(got[0, 0, i].tolist()) == _table_color(float(x) / 3.0), (i, x)
    for j, e in enumerate(edges):                                          # on the edge: the bin it opens; just below: the one before
        assert tuple(got[0, 0, 3 * j + 1].tolist()) == TABLE[j + 1][2] and tuple(got[0, 0, 3 * j].tolist()) == TABLE[j][2]
    # the relative branch, against a scalar statement: a large ground truth makes 5 % of it the smaller measure
    rng = np.random.default_rng(5)
    gt = (rng.standard_normal((2, 9, 15, 2)) * 40).astype(np.float32)
    pred = (gt + rng.standard_normal(gt.shape) * np.exp(rng.uniform(-4, 5, gt.shape[:3]))[..., None]).astype(np.float32)
    gt[0, 0, 0] = 0
    gt[0, 1, 1] = (1e10, 1e10)                                             # unknown ground truth: black
    gt[1, 2, 2] = (np.nan, 0)
    pred[0, 3, 3] = (np.nan, 1.0)                                          # unknown prediction, known ground truth: the last bin
    pred[1, 4, 4] = (1e10, 1e10)
    valid = rng.random(gt.shape[:3]) < 0.8
    valid[0, 3, 3] = valid[1, 4, 4] = valid[0, 0, 0] = True
    got = R.error_color(pred, gt, valid)
    seen = set()
    for n, y, x in np.ndindex(*gt.shape[:3]):
        gu, gv = (float(c) for c in gt[n, y, x])
        pu, pv = (float(c) for c in pred[n, y, x])
        if not valid[n, y, x] or not (abs(gu) <= 1e9 and abs(gv) <= 1e9):
            want = (0, 0, 0)
        elif not (abs(pu) <= 1e9 and abs(pv) <= 1e9):
            want = TABLE[-1][2]
        else:
            d_err = float(np.sqrt(np.float64((pu - gu) * (pu - gu) + (pv - gv) * (pv - gv))))
            d_mag = float(np.sqrt(np.float64(gu * gu + gv * gv)))
            n_err = d_err / 3.0 if d_mag == 0 else min(d_err / 3.0, (d_err / d_mag) / 0.05)
            want = _table_color(n_err)
            seen.add(want)
        assert tuple(got[n, y, x].tolist()) == want, (n, y, x)
    assert len(seen) >= 8
    assert tuple(got[0, 1, 1].tolist()) == (0, 0, 0) and tuple(got[0, 3, 3].tolist()) == TABLE[-1][2]


# ------------------------------------------------------------------ the library's constants
def test_device_wheel_equals_color_wheel():
    w = V.wheel()
    assert w.dtype == np.uint8 and w.shape == (55, 3) == (V.WHEEL_ENTRIES, 3)
    assert np.array_equal(w.astype(np.float64), flow_io.color_wheel())


def test_colour_rule_helper():
    t = np.array([3.0 - 1e-11, 3.0 + 1e-11, 3.5, 7.0 + 1e-6, np.nan, 0.0])
    want = np.floor(np.where(np.isnan(t), 9, t)).astype(np.uint8)
    assert R.check_color(want, want, t) == (0, 3)
    assert R.check_color(np.array([3, 2, 3, 7, 9, 0], np.uint8), want, t) == (2, 3)
    for bad in ([2, 3, 2, 7, 9, 0], [2, 3, 3, 6, 9, 0], [2, 3, 3, 7, 8, 0], [4, 3, 3, 7, 9, 0], [2, 3, 3, 7, 9, 1]):
        with pytest.raises(AssertionError):
            R.check_color(np.array(bad, np.uint8), want, t)


# ------------------------------------------------------------------ pwcnet_amd.vis: refusals before any library call
def test_python_functions_refuse_bad_arguments_on_the_cpu():
    import pwcnet_amd as P
    f = torch.zeros((2, 5, 7, 2))
    ok = torch.ones((2, 5, 7), dtype=torch.bool)
    u8 = torch.zeros((2, 5, 7, 3), dtype=torch.uint8)
    for fn in (P.flow_max_radius, P.flow_to_color, lambda x, **kw: P.flow_error_color(x, f, **kw)):
        with pytest.raises(ValueError, match="flows: expected a torch.float32"):
            fn(f.double())
        with pytest.raises(ValueError, match="flows: expected an NHWC"):
            fn(torch.zeros((2, 5, 7, 3)))
        with pytest.raises(ValueError, match="flows: expected an NHWC"):
            fn(torch.zeros((5, 7, 2)))
        with pytest.raises(ValueError, match="flows: empty"):
            fn(torch.zeros((2, 0, 7, 2)))
        with pytest.raises(ValueError, match="valid: expected a torch.bool"):
            fn(f, valid=torch.zeros((2, 5, 7)))
        with pytest.raises(ValueError, match="valid: expected shape"):
            fn(f, valid=torch.zeros((2, 7, 5), dtype=torch.uint8))
        with pytest.raises(ValueError, match="valid: the mask must be contiguous"):
            fn(f, valid=torch.zeros((2, 7, 5), dtype=torch.bool).transpose(1, 2))
        with pytest.raises(ValueError, match="flows: the tensor is on cpu"):
            fn(f, valid=ok)
    for fn in (P.flow_max_radius, P.flow_to_color):
        for bad in (float("nan"), float("inf"), "2", True):
            with pytest.raises(ValueError, match="flow_scale: expected a finite number"):
                fn(f, flow_scale=bad)
    for bad in (-1.0, float("nan"), float("inf"), -1e-300):
        with pytest.raises(ValueError, match="max_rad: expected a finite radius >= 0"):
            P.flow_to_color(f, bad)
    with pytest.raises(ValueError, match="max_rad: expected None, a number"):
        P.flow_to_color(f, "3")
    for bad in (torch.zeros(2), torch.zeros(3, dtype=torch.float64), torch.zeros((2, 1), dtype=torch.float64)):
        with pytest.raises(ValueError, match="max_rad: expected a contiguous"):
            P.flow_to_color(f, bad)
    with pytest.raises(ValueError, match="flows_gt: expected a torch.float32"):
        P.flow_error_color(f, f.half())
    with pytest.raises(ValueError, match="flows_gt: expected shape"):
        P.flow_error_color(f, torch.zeros((2, 5, 8, 2)))
    with pytest.raises(ValueError, match="frames: expected a torch.uint8 or torch.float32"):
        P.pyramid_montage(u8.double(), [f])
    with pytest.raises(ValueError, match="frames: expected an"):
        P.pyramid_montage(torch.zeros((2, 5, 7, 4), dtype=torch.uint8), [f])
    with pytest.raises(ValueError, match="frames: a dense"):
        P.pyramid_montage(torch.zeros((2, 7, 5, 3), dtype=torch.uint8).transpose(1, 2), [f])
    for bad in ([], [f] * 8, f):
        with pytest.raises(ValueError, match="flows_list: expected a list of 1 to 7"):
            P.pyramid_montage(u8, bad)
    with pytest.raises(ValueError, match=r"flows_list\[1\]: expected a torch.float32"):
        P.pyramid_montage(u8, [f, f.double()])
    with pytest.raises(ValueError, match=r"flows_list\[1\]: expected a batch of 2"):
        P.pyramid_montage(u8, [f, torch.zeros((3, 5, 7, 2))])
    with pytest.raises(ValueError, match=r"flows_list\[0\]: a 40 x 1 flow has no column"):
        P.pyramid_montage(u8, [torch.zeros((2, 40, 1, 2))])
    with pytest.raises(ValueError, match="flow_scales: expected None or 2 numbers"):
        P.pyramid_montage(u8, [f, f], [1.0])
    with pytest.raises(ValueError, match=r"flow_scales\[1\]: expected a finite number"):
        P.pyramid_montage(u8, [f, f], [1.0, float("nan")])
    with pytest.raises(ValueError, match="frames: the tensor is on cpu"):
        P.pyramid_montage(u8, [f] * 7)                                     # seven flows pass every check but the device


def test_library_refuses_before_any_launch():
    from pwcnet_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN, ERANGE = -1, -2, -3
    p, odd, half = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    assert ctypes.sizeof(_lib.VisTile) == 64

    def rad(flow=p, cs=2, N=2, H=5, W=7, out=p):
        return L.pwc_flow_max_radius_f64(flow, cs, None, N, H, W, 1.0, out, None)

    for bad in (dict(flow=None), dict(out=None), dict(N=0), dict(H=0), dict(W=-1), dict(cs=1)):
        assert rad(**bad) == EINVAL, bad
    assert rad(N=65536) == ERANGE and rad(N=1, H=1 << 16, W=1 << 15) == ERANGE
    assert rad(flow=odd) == EALIGN and rad(out=half) == EALIGN and rad(out=None, N=65536) == EINVAL

    def tile(**kw):
        t = dict(src=4096, gt=None, valid=None, max_rad=4096, kind=_lib.VIS_FLOW, src_cs=2, gt_cs=0, src_h=5, src_w=7, x0=0,
                 tile_w=7, flow_scale=1.0)
        t.update(kw)
        return _lib.VisTile(**t)

    def tiles(ts, N=2, out_h=5, out_w=7, out=p, n=None, table=True):
        arr = (_lib.VisTile * max(len(ts), 1))(*ts)
        return L.pwc_flow_vis_tiles_u8(ctypes.cast(arr, ctypes.c_void_p) if table else None, len(ts) if n is None else n, N, out_h,
                                       out_w, out, None)

    assert tiles([tile()], table=False) == EINVAL and tiles([tile()], out=None) == EINVAL
    assert tiles([], n=0) == EINVAL and tiles([tile()] * 9) == EINVAL
    for bad in (dict(N=0), dict(out_h=0), dict(out_w=0)):
        assert tiles([tile()], **bad) == EINVAL, bad
    err = dict(kind=_lib.VIS_ERROR, gt=4096, gt_cs=2, max_rad=None)
    for bad in (dict(src=None), dict(src_h=0), dict(src_w=0), dict(tile_w=0), dict(x0=-1), dict(x0=1), dict(tile_w=8), dict(kind=4),
                dict(kind=-1), dict(max_rad=None), dict(src_cs=1), dict(err, gt=None), dict(err, gt_cs=1), dict(err, src_cs=1)):
        assert tiles([tile(**bad)]) == EINVAL, bad
    assert tiles([tile()], N=65536) == ERANGE and tiles([tile()], N=1, out_h=1 << 16, out_w=1 << 15) == ERANGE
    assert tiles([tile(src_h=1 << 16, src_w=1 << 15)]) == ERANGE
    # an image whose last pixels an int pixel index stepped by up to 65536 cannot pass: the shared range check refuses it
    for wide in ((1 << 31) - 1, (1 << 31) - 65536):
        assert rad(N=1, H=1, W=wide) == ERANGE and tiles([tile()], N=1, out_h=1, out_w=wide) == ERANGE
        assert tiles([tile(src_h=1, src_w=wide)]) == ERANGE
    assert tiles([tile(src=4098)]) == EALIGN and tiles([tile(max_rad=4100)]) == EALIGN and tiles([tile(**dict(err, gt=4098))]) == EALIGN
    assert tiles([tile(kind=_lib.VIS_FRAME_F32, src=4098, max_rad=None)]) == EALIGN
    assert tiles([tile(src=None), tile()], N=65536) == EINVAL                      # the order of the header


# ------------------------------------------------------------------ the CLIs
def test_parsers_accept_the_new_flags():
    for name, argv in (("infer", ["--input_images", "a.png", "b.png"]), ("infer_continuous", ["-i", "a.png", "b.png"])):
        cli = _load_cli(name)
        ap = cli.build_parser()
        assert ap.parse_args(argv).vis == "host"
        assert ap.parse_args(argv + ["--vis", "gpu"]).vis == "gpu" and ap.parse_args(argv + ["--vis", "host"]).vis == "host"
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--vis", "cpu"])
        assert "--vis gpu" in " ".join(cli.__doc__.split())
    cli = _load_cli("evaluate")
    ap = cli.build_parser()
    args = ap.parse_args(["--list", "pairs.txt"])
    assert args.save_vis is False and args.save_dir is None
    assert ap.parse_args(["--list", "pairs.txt", "--save_dir", "d", "--save_vis"]).save_vis is True
    assert "--save_vis" in " ".join(cli.__doc__.split())


def test_evaluate_refuses_save_vis_without_save_dir(monkeypatch, capsys):
    cli = _load_cli("evaluate")
    monkeypatch.setattr("sys.argv", ["evaluate.py", "--list", "pairs.txt", "--save_vis"])
    with pytest.raises(SystemExit) as exit_info:                           # exit status 2, before anything is loaded
        cli.main()
    assert exit_info.value.code == 2 and "--save_vis requires --save_dir" in capsys.readouterr().err
