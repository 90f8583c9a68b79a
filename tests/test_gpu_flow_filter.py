"""The flow filter on the GPU (pwc_flow_filter.hip, pwcnet_amd.flow_filter, infer_continuous.py --flow_filter) against the numpy
restatement of the definition in tests/flow_filter_ref.py (held to a second route, to np.median and to hand-worked cases on the
CPU by tests/test_host_flow_filter.py).

The weights are integers and a median is a selection: the yardstick is BIT EQUALITY of the flow and of the mask, no tolerance.
Every case prints its figures before it asserts."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import flow_filter as FF  # the feature: without it nothing here can be collected
from tests import flow_filter_ref as R
from tests import seam_util as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3

# 19 x 45: two tile rows and two tile columns, both cut; 8 x 32: one tile exactly; 9 x 33: one pixel past it on both axes; a
# pixel, a row, a column; 5 x 3: W <= r for r = 3 and 7 (every window is cut on both sides); batch3: three images in one call.
GEOMETRIES = {"19x45": (1, 19, 45), "8x32": (1, 8, 32), "9x33": (1, 9, 33), "1x1": (1, 1, 1), "1x40": (1, 1, 40), "40x1": (1, 40, 1),
              "5x3": (1, 5, 3), "batch3": (3, 9, 33)}
RADII = (1, 2, 3, 7)
GUIDES = (None, "u8c3", "u8c1", "f32c3", "f32c1")


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.filter_flow is FF.filter_flow and pwcnet_amd.fill_flow is FF.fill_flow
    return pwcnet_amd


def make_flows(N, H, W, seed, unknown=0.12):
    """Flows on a half-pixel lattice (many ties), with +0 and -0, negatives, magnitudes up to exactly 1e9, and unknown pixels of
    every kind: NaN, +-inf, the sentinel 1e10, the first float above 1e9."""
    rs = np.random.RandomState(seed)
    f = (rs.randint(-4, 5, size=(N, H, W, 2)) * 0.5).astype(np.float32)
    pick = rs.uniform(size=f.shape)
    f[pick < 0.08] = -0.0
    f[(pick >= 0.08) & (pick < 0.12)] = 1e9
    f[(pick >= 0.12) & (pick < 0.16)] = -1e9
    f[(pick >= 0.16) & (pick < 0.22)] = rs.normal(0, 1e4, size=int(((pick >= 0.16) & (pick < 0.22)).sum())).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, 1e10, np.nextafter(np.float32(1e9), np.float32(np.inf))], np.float32)
    hole = rs.uniform(size=(N, H, W)) < unknown
    f[hole, rs.randint(0, 2, size=int(hole.sum()))] = bad[rs.randint(0, len(bad), size=int(hole.sum()))]
    return f


def make_guide(kind, N, H, W, seed):
    """Blocky pictures (so that colour differences repeat); the float kind holds values outside [0, 1] and NaN."""
    if kind is None:
        return None
    rs = np.random.RandomState(seed + 77)
    C = 3 if kind.endswith("c3") else 1
    coarse = rs.randint(0, 256, size=(N, -(-H // 3), -(-W // 4), C))
    g = np.kron(coarse, np.ones((1, 3, 4, 1), np.int64))[:, :H, :W] + rs.randint(-6, 7, size=(N, H, W, C))
    if kind.startswith("u8"):
        return np.clip(g, 0, 255).astype(np.uint8)
    g = (g / 255.0).astype(np.float32)                       # (some below 0 and above 1 already)
    pick = rs.uniform(size=g.shape)
    g[pick < 0.03] = np.nan
    g[(pick >= 0.03) & (pick < 0.06)] = 7.5
    g[(pick >= 0.06) & (pick < 0.09)] = -3.0
    g[(pick >= 0.09) & (pick < 0.12)] = (rs.randint(0, 255, size=int(((pick >= 0.09) & (pick < 0.12)).sum())) + 0.5) / 255.0   # near ties of rint
    return g


def make_valid(N, H, W, seed, keep=0.85):
    return np.random.RandomState(seed + 991).uniform(size=(N, H, W)) < keep


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu(P, flows, guide, valid, **kw):
    out, ok = P.filter_flow(_up(flows), guide=_up(guide), valid=_up(valid), **kw)
    assert out.dtype == torch.float32 and ok.dtype == torch.bool and tuple(out.shape) == tuple(flows.shape[:3]) + (2,)
    return out.cpu().numpy(), ok.cpu().numpy()


def _same(tag, got, want):
    flow_diff = int((S.bits(got[0]) != S.bits(want[0])).sum())
    mask_diff = int((got[1].astype(np.uint8) != want[1].astype(np.uint8)).sum())
    print(f"flow filter {tag}: {want[0].shape[:3]} known out {int(want[1].sum())} of {want[1].size}, bits that differ: flow "
          f"{flow_diff} mask {mask_diff}")
    S.assert_same_bits(got[1].astype(np.uint8), want[1].astype(np.uint8), f"{tag}: out_valid")
    S.assert_same_bits(got[0], want[0], f"{tag}: flow")


@functools.lru_cache(maxsize=None)
def tables(r, C, sigma_space=1.5, sigma_color=12.0):
    return FF.filter_tables(r, sigma_space, sigma_color, C)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_geometries_and_radii_equal_the_restatement(P, geometry, radius):
    """Every geometry at every radius, masked, smoothing and filling at once; the guide kind walks with the case."""
    N, H, W = GEOMETRIES[geometry]
    seed = 13 * list(GEOMETRIES).index(geometry) + radius
    kind = GUIDES[seed % 4]
    flows, guide, valid = make_flows(N, H, W, seed), make_guide(kind, N, H, W, seed), make_valid(N, H, W, seed)
    space, color = tables(radius, 1 if kind in ("u8c1", "f32c1") else 3)
    want = R.filter_flow_ref(flows, guide, valid, radius, space, color, True, True, 1, 1)
    got = _gpu(P, flows, guide, valid, radius=radius, sigma_space=1.5, sigma_color=12.0, smooth=True, fill=True)
    _same(f"{geometry} r{radius} guide {kind}", got, want)


@pytest.mark.parametrize("radius", (1, 3))
@pytest.mark.parametrize("kind", GUIDES)
def test_guide_kinds(P, kind, radius):
    """No guide, bytes with three channels and one, floats (beyond [0, 1], NaN, halves that rint takes to even) with both."""
    N, H, W = 1, 11, 37
    flows, guide = make_flows(N, H, W, 40 + radius), make_guide(kind, N, H, W, 41)
    space, color = tables(radius, 1 if kind in ("u8c1", "f32c1") else 3, 2.0, 6.0)
    want = R.filter_flow_ref(flows, guide, None, radius, space, color, True, False, 1, 1)
    got = _gpu(P, flows, guide, None, radius=radius, sigma_space=2.0, sigma_color=6.0)
    _same(f"guide {kind} r{radius}", got, want)
    if kind is not None and kind.startswith("f32"):                                      # the float guide is its bytes
        as_bytes = R.guide_bytes(guide).astype(np.uint8)
        _same(f"guide {kind} r{radius} as bytes", _gpu(P, flows, as_bytes, None, radius=radius, sigma_space=2.0, sigma_color=6.0), want)


@pytest.mark.parametrize("min_count", (1, 4))
@pytest.mark.parametrize("smooth,fill", ((True, False), (False, True), (True, True)))
def test_smooth_fill_and_min_count(P, smooth, fill, min_count):
    N, H, W, r = 1, 9, 33, 2
    flows, guide, valid = make_flows(N, H, W, 50, unknown=0.5), make_guide("u8c3", N, H, W, 50), make_valid(N, H, W, 50, 0.5)
    space, color = FF.filter_tables(r, None, 20.0, 3)
    want = R.filter_flow_ref(flows, guide, valid, r, space, color, smooth, fill, min_count, 1)
    got = _gpu(P, flows, guide, valid, radius=r, sigma_color=20.0, smooth=smooth, fill=fill, min_count=min_count)
    _same(f"smooth {smooth} fill {fill} min_count {min_count}", got, want)
    if not smooth:                                                                        # a known pixel keeps its bits
        kn = R.known(flows, valid)
        S.assert_same_bits(got[0][kn], flows[kn], "known pixels under fill alone")
    if not fill:
        assert np.array_equal(got[1], R.known(flows, valid))


@pytest.mark.parametrize("iters", (1, 2, 3))
@pytest.mark.parametrize("smooth", (False, True))
def test_holes_wider_than_the_radius_close_from_the_rim(P, iters, smooth):
    """A 9 x 11 hole in the mask and a 5 x 5 hole of sentinels under r = 2: a pass closes two pixels of rim, the small one needs
    two passes, the large one three on its short axis.  fill_flow is the same call."""
    N, H, W, r = 2, 19, 45, 2
    flows, valid = make_flows(N, H, W, 60, unknown=0.0), np.ones((N, H, W), bool)
    valid[:, 4:13, 6:17] = False
    flows[:, 10:15, 30:35] = 1e10
    guide = None                                             # (space weights alone: none is zero, so the rim always closes)
    space, color = tables(r, 1)
    want = R.filter_flow_ref(flows, guide, valid, r, space, None, smooth, True, 1, iters)
    got = _gpu(P, flows, guide, valid, radius=r, sigma_space=1.5, smooth=smooth, fill=True, iters=iters)
    _same(f"holes iters {iters} smooth {smooth}", got, want)
    left = int((want[1] == 0).sum())
    print(f"flow filter holes: unknown after {iters} passes {left}")
    assert (left == 0) == (iters == 3) and (iters > 1 or left > 0)
    if not smooth:
        out, ok = P.fill_flow(_up(flows), valid=_up(valid), radius=r, sigma_space=1.5, iters=iters)
        _same(f"fill_flow iters {iters}", (out.cpu().numpy(), ok.cpu().numpy()), want)


def test_tables_with_zeros_and_explicit_tables(P):
    """tables=: a space table with a zero centre and zero corners, a colour table that is zero from d = 40 on, and all-zero
    tables (n = 0 everywhere: known pixels keep their bits, unknown ones stay unknown)."""
    N, H, W, r = 1, 9, 33, 2
    flows, guide, valid = make_flows(N, H, W, 70), make_guide("u8c3", N, H, W, 70), make_valid(N, H, W, 70)
    space = np.arange(1, 26, dtype=np.uint32) * 2500
    space[[0, 4, 12, 20, 24]] = 0
    color = np.where(np.arange(766) < 40, 65535 - 1000 * np.arange(766), 0).astype(np.uint32)
    for tag, sp, co in (("zero centre", space, color), ("zero space", np.zeros(25, np.uint32), color),
                        ("zero colour", space, np.zeros(766, np.uint32)), ("largest entries", np.full(25, 65535, np.uint32), np.full(766, 65535, np.uint32))):
        want = R.filter_flow_ref(flows, guide, valid, r, sp, co, True, True, 1, 1)
        got = _gpu(P, flows, guide, valid, radius=r, tables=(sp, co), smooth=True, fill=True)
        _same(f"tables {tag}", got, want)
        if tag.startswith("zero "):
            kn = R.known(flows, valid)
            assert np.array_equal(got[1], kn) == (tag != "zero centre")
    want = R.filter_flow_ref(flows, None, valid, r, space, None, True, True, 1, 1)
    _same("tables without a guide", _gpu(P, flows, None, valid, radius=r, tables=(torch.from_numpy(space.astype(np.int64)), None), fill=True), want)
    with pytest.raises(ValueError):
        P.filter_flow(_up(flows), radius=r, tables=(np.full(25, 65536), None))
    with pytest.raises(ValueError):
        P.filter_flow(_up(flows), radius=r, tables=(np.full(24, 1), None))
    with pytest.raises(ValueError):
        P.filter_flow(_up(flows), radius=r, tables=(space, color), sigma_space=1.0)


def _raw(flows, valid, guide, r, space, color, smooth, fill, min_count, iters, out, out_valid, flow_cs, out_cs, ws=None, ws_bytes=None,
         dtype=0, C=3, N=None, H=None, W=None):
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else (0 if t is None else t.data_ptr()))
    n, h, w = (N, H, W) if N is not None else flows.shape[:3]
    if ws_bytes is None:
        ws_bytes = 0 if ws is None else (1 << 40 if isinstance(ws, int) else ws.numel() * ws.element_size())
    return L.pwc_flow_filter_f32(p(flows), flow_cs, p(valid), p(guide), dtype, C, n, h, w, r, p(space), p(color), smooth, fill,
                                 min_count, iters, p(ws), ws_bytes, p(out), out_cs, p(out_valid), _lib.current_stream())


def test_channel_strides_of_three(P):
    """flow_cs = out_cs = 3 through the C ABI, iters 1 and 2: the third channel of the input is not read as flow and the third
    channel of out is not written; through Python a channel slice of a wider tensor is read in place."""
    N, H, W, r = 1, 9, 33, 3
    flows, guide, valid = make_flows(N, H, W, 80), make_guide("u8c3", N, H, W, 80), make_valid(N, H, W, 80)
    space, color = tables(r, 3)
    wide = np.concatenate([flows, np.full((N, H, W, 1), np.nan, np.float32)], axis=3)
    d_space, d_color = _up(space.view(np.int32)), _up(color.view(np.int32))
    for iters in (1, 2):
        want = R.filter_flow_ref(flows, guide, valid, r, space, color, True, True, 1, iters)
        out = torch.full((N, H, W, 3), -7.0, device="cuda")
        ok = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
        nbytes = _lib.lib().pwc_flow_filter_workspace_bytes(N, H, W, iters)
        ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device="cuda")
        d_wide, d_valid, d_guide = _up(wide), _up(valid), _up(guide)
        rc = _raw(d_wide, d_valid, d_guide, r, d_space, d_color, 1, 1, 1, iters, out, ok, 3, 3, ws, nbytes)
        assert rc == 0
        out = out.cpu().numpy()
        _same(f"strides of three iters {iters}", (np.ascontiguousarray(out[..., :2]), ok.cpu().numpy()), want)
        assert (out[..., 2] == -7.0).all()
    want = R.filter_flow_ref(flows, guide, valid, r, space, color, True, True, 1, 1)
    got = P.filter_flow(_up(wide)[..., :2], guide=_up(guide), valid=_up(valid), radius=r, sigma_space=1.5, sigma_color=12.0, fill=True)
    _same("a channel slice", (got[0].cpu().numpy(), got[1].cpu().numpy()), want)


@pytest.mark.parametrize("radius", (2, 7))
def test_a_batch_gives_its_images_one_by_one(P, radius):
    """tests/seam_util.py: the subject between random neighbours, copies and poison gives the same bits, and the bits of the
    subject alone; three passes, so that the intermediate field is a batch as well."""
    H, W = 9, 13
    subject = {"flow": make_flows(1, H, W, 90), "valid": make_valid(1, H, W, 90), "guide": make_guide("u8c3", 1, H, W, 90)}
    roles = {"flow": S.FLOW, "valid": S.MASK, "guide": S.FLOAT}

    def op(inp):
        out, ok = _gpu(P, inp["flow"], inp["guide"], inp["valid"], radius=radius, sigma_space=2.0, sigma_color=15.0, fill=True, iters=3)
        return {"flow": out, "valid": ok}
    outs = S.check_isolation(op, subject, roles, what=f"filter_flow r{radius}")
    single = S.check_batch_equals_single(op, subject, outs["random"], what=f"filter_flow r{radius}")
    space, color = FF.filter_tables(radius, 2.0, 15.0, 3)
    want = R.filter_flow_ref(subject["flow"], subject["guide"], subject["valid"], radius, space, color, True, True, 1, 3)
    _same(f"seams r{radius}", (single["flow"], single["valid"]), want)


def test_two_calls_give_the_same_bits(P):
    N, H, W = 2, 40, 70
    flows, guide, valid = make_flows(N, H, W, 100), make_guide("f32c3", N, H, W, 100), make_valid(N, H, W, 100)
    for r in (1, 2, 7):
        a = _gpu(P, flows, guide, valid, radius=r, sigma_space=2.0, sigma_color=10.0, fill=True, iters=2)
        b = _gpu(P, flows, guide, valid, radius=r, sigma_space=2.0, sigma_color=10.0, fill=True, iters=2)
        S.assert_same_bits(a[0], b[0], f"two calls r{r}: flow")
        S.assert_same_bits(a[1].astype(np.uint8), b[1].astype(np.uint8), f"two calls r{r}: mask")


def test_abi_refusals_and_the_workspace_contract(P):
    """Every refusal of include/pwc_hip.h's list by its code, each with everything before it in order; nothing is launched by a
    refused call.  pwc_flow_filter_workspace_bytes: 0 for one pass and for refused sizes, 8 P + P rounded up to 8 otherwise."""
    L = _lib.lib()
    N, H, W, r = 2, 5, 7, 2
    P_ = N * H * W
    assert L.pwc_flow_filter_workspace_bytes(N, H, W, 1) == 0
    assert L.pwc_flow_filter_workspace_bytes(N, H, W, 2) == L.pwc_flow_filter_workspace_bytes(N, H, W, 9) == 8 * P_ + (P_ + 7) // 8 * 8
    for bad in ((0, H, W, 2), (N, 0, W, 2), (N, H, -1, 2), (N, H, W, 0), (65536, H, W, 2), (1, 1 << 16, 1 << 15, 2)):
        assert L.pwc_flow_filter_workspace_bytes(*bad) == 0, bad
    flows = torch.zeros((N, H, W, 2), device="cuda")
    valid = torch.ones((N, H, W), dtype=torch.uint8, device="cuda")
    guide = torch.zeros((N, H, W, 3), dtype=torch.uint8, device="cuda")
    gf = torch.zeros((N, H, W, 3), device="cuda")
    space = torch.ones((25,), dtype=torch.int32, device="cuda")
    color = torch.ones((766,), dtype=torch.int32, device="cuda")
    out, ok = torch.zeros_like(flows), torch.zeros_like(valid)
    ws = torch.empty((L.pwc_flow_filter_workspace_bytes(N, H, W, 2) // 8 + 1,), dtype=torch.float64, device="cuda")
    good = dict(N=N, H=H, W=W, flows=flows, valid=valid, guide=guide, r=r, space=space, color=color, smooth=1, fill=1, min_count=1, iters=2, out=out,
                out_valid=ok, flow_cs=2, out_cs=2, ws=ws)
    call = lambda **kw: _raw(**{**good, **kw})
    assert call() == 0 and call(valid=None) == 0 and call(guide=None, color=None) == 0 and call(iters=1, ws=None) == 0
    for kw in (dict(flows=None), dict(space=None), dict(out=None), dict(out_valid=None), dict(color=None)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(r=0), dict(r=8), dict(C=2), dict(C=0), dict(dtype=2),
               dict(dtype=-1), dict(smooth=0, fill=0), dict(min_count=0), dict(iters=0), dict(flow_cs=1), dict(out_cs=1)):
        assert call(**kw) == EINVAL, kw
    # out over flows (the same tensor, and its second half over the first), out_valid over valid
    assert call(out=flows) == EINVAL and call(out=flows.data_ptr() + 8, N=1) == EINVAL
    assert call(out=flows.data_ptr() + 4 * P_, N=1, iters=1, ws=None) == 0             # (the second image: no byte shared)
    assert call(out_valid=valid) == EINVAL
    assert call(ws=None) == EINVAL and call(ws_bytes=ws.numel() * 8 - 16) == EINVAL
    # the order: a bad radius wins over the range, a small workspace is not looked at beyond the range (it needs none there)
    # (addresses far apart, nothing is launched: out and flows of these sizes must not overlap to get as far as the range)
    far = dict(flows=4096, out=1 << 45, out_valid=1 << 46, valid=None, guide=None, color=None, ws=None)
    assert call(N=65536, H=1, W=1, **far) == ERANGE and call(N=1, H=1 << 16, W=1 << 15, **far) == ERANGE       # N > 65535; H W = 2^31
    assert call(N=65536, H=1, W=1, **{**far, "r": 9}) == EINVAL                                                 # (the radius comes first)
    assert call(flows=flows.data_ptr() + 2) == EALIGN and call(out=out.data_ptr() + 2) == EALIGN
    assert call(space=space.data_ptr() + 1) == EALIGN and call(color=color.data_ptr() + 2) == EALIGN
    assert call(guide=gf.data_ptr() + 2, dtype=1) == EALIGN and call(ws=ws.data_ptr() + 4) == EALIGN
    torch.cuda.synchronize()
    # a byte guide one byte off its allocation's start: legal, and the result is that of the shifted bytes
    raw = torch.zeros((P_ * 3 + 1,), dtype=torch.uint8, device="cuda")
    assert call(guide=raw.data_ptr() + 1) == 0
    torch.cuda.synchronize()


def test_python_argument_checks(P):
    flows = torch.zeros((1, 4, 5, 2), device="cuda")
    with pytest.raises(TypeError):
        P.filter_flow(flows.double())
    with pytest.raises(ValueError):
        P.filter_flow(flows, radius=0)
    with pytest.raises(ValueError):
        P.filter_flow(flows, radius=8)
    with pytest.raises(ValueError):
        P.filter_flow(flows, smooth=False, fill=False)
    with pytest.raises(ValueError):
        P.filter_flow(flows, iters=0)
    with pytest.raises(ValueError):
        P.filter_flow(flows, min_count=0)
    with pytest.raises(ValueError):
        P.filter_flow(flows, guide=torch.zeros((1, 4, 5, 2), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        P.filter_flow(flows, guide=torch.zeros((1, 4, 5, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        P.filter_flow(flows, valid=torch.ones((1, 4, 4), dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        P.filter_flow(flows.cpu())
    out, ok = P.fill_flow(flows)                                                          # iters = ceil(5 / 2) passes by default
    assert torch.equal(out, flows) and bool(ok.all())


def test_infer_continuous_flow_filter_cli(P, tmp_path):
    """The CLI in fresh child processes: three 64 x 128 frames of noise (hence the wide colour sigma), the golden weights.  The .flo files written with --flow_filter 2
    are filter_flow of the .flo files written without it, with the first frame as the guide, bit for bit; every other file is
    the same bytes."""
    from PIL import Image
    from pwcnet_amd import ckpt, flow_io
    from tests import util
    rng = np.random.RandomState(5)
    base = rng.uniform(0, 255, size=(64, 128, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    frames = [np.roll(base, 2 * i, axis=1) for i in range(3)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(seq / f"frame_{i:02d}.png")
    ckpt.save_weights(str(tmp_path / "m.ckpt"), util.model_weights(False))
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "-r", str(tmp_path / "m.ckpt"),
           "--pipeline", "1", "--batch", "2"]
    plain = subprocess.run(cli + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "Figure saved" in plain.stdout, plain.stderr[-2000:]
    flags = ["--flow_filter", "2", "--flow_filter_sigma_space", "1.5", "--flow_filter_sigma_color", "120", "--flow_filter_iters", "2"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o")] + flags, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    a, b = tmp_path / "plain" / "seq", tmp_path / "o" / "seq"
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == sorted(f"frame_{i:02d}{e}" for i in range(2) for e in (".flo", ".png"))
    before = np.stack([flow_io.read_flo(str(a / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(2)])
    want, ok = P.filter_flow(_up(before), guide=_up(np.stack(frames[:2])), radius=2, sigma_space=1.5, sigma_color=120.0, iters=2)
    want = want.cpu().numpy()
    other = P.filter_flow(_up(before), guide=_up(np.stack(frames[1:])), radius=2, sigma_space=1.5, sigma_color=120.0, iters=2)[0]
    assert not torch.equal(other.cpu(), torch.from_numpy(want))                           # (the guide matters on these frames)
    changed = 0
    for i in range(2):
        got = flow_io.read_flo(str(b / f"frame_{i:02d}.flo")).astype(np.float32)
        S.assert_same_bits(got, want[i], f"cli: frame_{i:02d}.flo")
        changed += int((S.bits(got) != S.bits(before[i])).sum())
        assert (a / f"frame_{i:02d}.png").read_bytes() == (b / f"frame_{i:02d}.png").read_bytes()
    print(f"flow filter cli: {changed} of {before.size} flow values changed by the filter")
    assert changed > 0 and bool(ok.all())
    bad = subprocess.run(cli + ["--out", str(tmp_path / "bad"), "--flow_filter", "8"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--flow_filter" in bad.stderr
