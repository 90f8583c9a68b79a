"""Moving regions on the GPU (pwc_regions.hip, pwcnet_amd.regions, infer_continuous.py --regions) against the numpy restatement of
the definition in tests/regions_ref.py (a host union-find, checked on the CPU by tests/test_host_regions.py).

Every output is an integer, or a double made of two divisions of integers: the yardstick is BIT EQUALITY of labels, count, area,
box, sums and mean, no tolerance.  Every case prints its figures before it asserts (profiles/regions_gpu_test_figures.txt)."""
import ctypes
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import regions as RG  # the feature: without it nothing here can be collected
from tests import regions_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3
KEYS = ("labels", "count", "area", "box", "sums", "mean")


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.label_regions is RG.label_regions
    return pwcnet_amd


@functools.lru_cache(maxsize=None)
def tile():
    return RG.tile_shape()


def shapes():
    """The smallest shapes at which the launches can go wrong, from the library's tile; the last is PAST THE SCAN'S PARTS CAP:
    more than 256 parts of 256 pixels (65536 pixels), so a part's chunk is two strips of 256 -- the only cap the launches have
    (every other grid has a workgroup per 256 pixels or per tile and no stride loop)."""
    th, tw = tile()
    return {"1x1": (1, 1), "row": (1, 2 * tw + 3), "column": (2 * th + 3, 1), "tile": (th, tw), "tile+1": (th + 1, tw + 1),
            "tiles": (2 * th + 5, 3 * tw + 7), "past_scan_parts": (8 * th + 3, 8 * tw + 5)}


SHAPE_NAMES = ("1x1", "row", "column", "tile", "tile+1", "tiles", "past_scan_parts")


@functools.lru_cache(maxsize=None)
def masks(shape_name):
    H, W = shapes()[shape_name]
    pats = R.patterns(H, W, *tile())
    return tuple(pats), np.stack(list(pats.values()))


def _up(a):
    return a if a is None or not isinstance(a, np.ndarray) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype.kind == "f" else a


def _gpu(P, mask, **kw):
    kw = {k: _up(v) for k, v in kw.items()}
    labels, count, reg = P.label_regions(_up(mask), **kw)
    assert labels.dtype == torch.int32 and count.dtype == torch.int32 and reg["area"].dtype == torch.int32
    assert reg["box"].dtype == torch.int32 and (reg["mean"] is None or reg["mean"].dtype == torch.float64)
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return dict(labels=cpu(labels), count=cpu(count), area=cpu(reg["area"]), box=cpu(reg["box"]), sums=cpu(reg["sums"]),
                mean=cpu(reg["mean"]))


def _ref(mask, **kw):
    return dict(zip(KEYS, R.label_regions(np.asarray(mask), **kw)))


def _same(tag, got, want):
    diff = {k: (None if want[k] is None else int((_bits(got[k]) != _bits(want[k])).sum())) for k in KEYS}
    print(f"regions {tag}: count {want['count'].tolist()} elements that differ {diff}")
    for k in KEYS:
        if want[k] is None:
            assert got[k] is None, (tag, k)
        else:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (tag, k, got[k].dtype, want[k].dtype)
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (tag, k)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_patterns_equal_the_restatement_bit_for_bit(P, shape_name, connectivity):
    """Every pattern of the shape as one batch (so also: never across images), max_regions = 256, min_area = 1."""
    names, batch = masks(shape_name)
    H, W = batch.shape[1:]
    want = _ref(batch, connectivity=connectivity)
    t0 = time.perf_counter()
    got = _gpu(P, batch, connectivity=connectivity)
    print(f"regions {shape_name} {H}x{W} connectivity {connectivity}: {dict(zip(names, want['count'].tolist()))} "
          f"call and copies {1e3 * (time.perf_counter() - t0):.1f} ms")
    _same(f"{shape_name} c{connectivity}", got, want)
    k = dict(zip(names, want["count"].tolist()))
    assert k["background"] == 0 and k["foreground"] == 1 and k["serpentine"] == 1 and k["u"] == 1 and k["spiral"] == 1
    assert k["checkerboard"] == ((H * W + 1) // 2 if connectivity == 4 or min(H, W) == 1 else 1)
    assert k["corners"] == len({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}) or (min(H, W) <= 2 and max(H, W) <= 2)
    if shape_name in ("tiles", "past_scan_parts"):
        assert k["checkerboard"] > 256 or connectivity == 8                       # the max_regions cut
        assert k["bernoulli0.6"] > 0 and k["diagonal"] > 0 and k["antidiagonal"] > 0


@pytest.mark.parametrize("connectivity", (4, 8))
def test_min_area_and_max_regions(P, connectivity):
    names, batch = masks("tiles")
    pick = np.stack([batch[names.index(n)] for n in ("bernoulli0.4", "bernoulli0.6", "checkerboard", "corners")])
    flows = R.seeded_flows(4, *pick.shape[1:], seed=3)
    for min_area in (1, 2, 5):
        for max_regions in (1, 4, 256):
            kw = dict(connectivity=connectivity, min_area=min_area, max_regions=max_regions)
            _same(f"min_area {min_area} max_regions {max_regions} c{connectivity}", _gpu(P, pick, **kw), _ref(pick, **kw))
            _same(f"min_area {min_area} max_regions {max_regions} c{connectivity} flows", _gpu(P, pick, flows=flows, **kw),
                  _ref(pick, flows=flows, **kw))
    one, five = _ref(pick, connectivity=connectivity), _ref(pick, connectivity=connectivity, min_area=5)
    assert 0 < five["count"][0] < one["count"][0]                                   # 5 drops some components and keeps others


def test_invert_and_mask_dtypes(P):
    names, batch = masks("tiles")
    pick = batch[[names.index("bernoulli0.6"), names.index("spiral")]] * np.uint8(3)   # (non-zero, not just 1)
    for invert in (False, True):
        want = _ref(pick, invert=invert)
        _same(f"uint8 invert {invert}", _gpu(P, pick, invert=invert), want)
        _same(f"bool invert {invert}", _gpu(P, pick != 0, invert=invert), want)
    assert not np.array_equal(_ref(pick, invert=True)["labels"], _ref(pick)["labels"])


def test_unknown_flows_in_the_open_and_under_the_mask_and_the_clamp(P):
    names, batch = masks("tiles")
    pick = batch[[names.index("bernoulli0.6"), names.index("foreground")]]
    flows = R.seeded_flows(2, *pick.shape[1:], seed=5)
    assert np.isnan(flows).any() and np.isinf(flows).any() and (flows == R.SENTINEL).any() and (np.abs(flows[np.isfinite(flows)]) > 65536).any()
    for connectivity in (4, 8):
        want = _ref(pick, flows=flows, connectivity=connectivity)
        _same(f"nan, inf, sentinel in the open c{connectivity}", _gpu(P, pick, flows=flows, connectivity=connectivity), want)
        hidden = flows.copy()
        hidden[pick == 0] = np.nan                                                # under an excluded mask byte: not loaded
        hidden[tuple(np.argwhere(pick == 0)[::2].T)] = R.SENTINEL
        _same(f"nan, sentinel under the mask c{connectivity}", _gpu(P, pick, flows=hidden, connectivity=connectivity), want)
    assert want["area"][1, 0] < pick[1].size and np.abs(want["mean"]).max() > 100.0  # the holes are cut out; the clamp shows
    assert not np.array_equal(want["labels"], _ref(pick, connectivity=8)["labels"])


def test_channel_strides_and_offsets_give_the_same_bits(P):
    names, batch = masks("tile+1")
    pick = batch[[names.index("bernoulli0.6"), names.index("u")]]
    flows = R.seeded_flows(2, *pick.shape[1:], seed=9)
    want = _ref(pick, flows=flows)
    for width, lo in ((3, 0), (3, 1), (4, 0), (4, 1), (4, 2)):
        buf = torch.full(flows.shape[:3] + (width,), float("nan"), dtype=torch.float32, device="cuda")
        buf[..., lo:lo + 2] = _up(flows)
        view = buf[..., lo:lo + 2]
        _same(f"stride {width} offset {lo} (address % 8 = {view.data_ptr() % 8})", _gpu(P, pick, flows=view), want)


@pytest.mark.parametrize("shape_name", ("tiles", "past_scan_parts"))
def test_an_image_alone_gives_the_bits_it_gives_in_a_batch(P, shape_name):
    names, batch = masks(shape_name)
    full = batch[names.index("foreground")]
    for name in ("bernoulli0.4", "serpentine"):
        m = batch[names.index(name)]
        flows = R.seeded_flows(3, *m.shape, seed=11)
        for connectivity in (4, 8):
            alone = _gpu(P, m[None], flows=flows[1:2], connectivity=connectivity)
            three = _gpu(P, np.stack([full, m, full]), flows=flows, connectivity=connectivity)
            _same(f"seam {shape_name} {name} c{connectivity}", {k: v[1:2] for k, v in three.items()}, alone)
            _same(f"two calls {shape_name} {name} c{connectivity}", _gpu(P, m[None], flows=flows[1:2], connectivity=connectivity), alone)
            assert three["labels"][1, 0].any() or name != "serpentine"              # (its first row touches the neighbour's last)


def test_moving_regions_finds_the_rectangle(P):
    """An affine camera flow plus a rectangle moved by (8, -6) px: one kept component at min_area = 16, the rectangle's box, the
    mean residual within 0.2 px of (8, -6) (looser than the < 0.1 px that tests/test_host_motion.py asserts on the fitted
    parameters; confirmed on the CPU restatement by tests/test_host_regions.py)."""
    th, tw = tile()
    flows, rect = R.rectangle_scene(2, 2 * th + 5, 3 * tw + 7, seed=1)
    f = _up(flows)
    matrices, ok, _ = P.fit_motion(f, model="affine")
    labels, count, reg, residual, inlier = P.moving_regions(f, matrices, min_area=16)
    assert bool(ok.all()) and residual.dtype == torch.float32 and inlier.dtype == torch.bool
    want = _ref(inlier.cpu().numpy(), invert=True, flows=residual.cpu().numpy(), min_area=16)
    got = dict(labels=labels.cpu().numpy(), count=count.cpu().numpy(), area=reg["area"].cpu().numpy(), box=reg["box"].cpu().numpy(),
               sums=reg["sums"].cpu().numpy(), mean=reg["mean"].cpu().numpy())
    print(f"regions rectangle scene: count {got['count'].tolist()} box {got['box'][:, 0].tolist()} mean {got['mean'][:, 0].tolist()}")
    _same("moving_regions", got, want)
    for n in range(2):
        assert got["count"][n] == 1 and got["box"][n, 0].tolist() == list(rect)
        assert got["area"][n, 0] == (rect[2] - rect[0] + 1) * (rect[3] - rect[1] + 1)
        assert np.abs(got["mean"][n, 0] - np.array([8.0, -6.0])).max() < 0.2


def test_refusals_by_their_codes(P):
    N, H, W, Rr = 2, 5, 6, 4
    L = _lib.lib()
    nbytes = L.pwc_regions_workspace_bytes(N, H, W)
    mask = torch.ones((N, H, W), dtype=torch.uint8, device="cuda")
    flows = torch.zeros((N, H, W, 4), dtype=torch.float32, device="cuda")
    ws = torch.zeros(nbytes // 8 + 2, dtype=torch.int64, device="cuda")
    labels = torch.full((N * H * W + 1,), -5, dtype=torch.int32, device="cuda")
    count = torch.full((N + 1,), -5, dtype=torch.int32, device="cuda")
    area = torch.full((N * Rr + 1,), -5, dtype=torch.int32, device="cuda")
    box = torch.full((N * Rr * 4 + 1,), -5, dtype=torch.int32, device="cuda")
    sums = torch.full((N * Rr * 2 + 1,), -5, dtype=torch.int64, device="cuda")
    mean = torch.full((N * Rr * 2 + 1,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda v: None if v is None else ctypes.c_void_p(v)                        # noqa: E731

    def call(**change):
        a = dict(mask=mask.data_ptr(), invert=0, flows=flows.data_ptr(), cs=4, N=N, H=H, W=W, conn=8, min_area=1, R=Rr, ws=ws.data_ptr(),
                 nbytes=nbytes, labels=labels.data_ptr(), count=count.data_ptr(), area=area.data_ptr(), box=box.data_ptr(),
                 sums=sums.data_ptr(), mean=mean.data_ptr())
        a.update(change)
        return L.pwc_label_regions(p(a["mask"]), a["invert"], p(a["flows"]), a["cs"], a["N"], a["H"], a["W"], a["conn"], a["min_area"],
                                   a["R"], p(a["ws"]), a["nbytes"], p(a["labels"]), p(a["count"]), p(a["area"]), p(a["box"]),
                                   p(a["sums"]), p(a["mean"]), _lib.current_stream())

    refused = [(EINVAL, dict(mask=None)), (EINVAL, dict(ws=None)), (EINVAL, dict(labels=None)), (EINVAL, dict(count=None)),
               (EINVAL, dict(area=None)), (EINVAL, dict(box=None)), (EINVAL, dict(flows=None)), (EINVAL, dict(sums=None)),
               (EINVAL, dict(mean=None)), (EINVAL, dict(flows=None, sums=None)), (EINVAL, dict(N=0)), (EINVAL, dict(H=0)),
               (EINVAL, dict(W=-1)), (EINVAL, dict(conn=6)), (EINVAL, dict(conn=0)), (EINVAL, dict(min_area=0)), (EINVAL, dict(R=0)),
               (EINVAL, dict(R=65536)), (EINVAL, dict(cs=1)), (EINVAL, dict(nbytes=nbytes - 1)),
               (ERANGE, dict(H=1 << 13, W=(1 << 13) + 1)), (ERANGE, dict(N=65536)),
               (EINVAL, dict(H=1 << 13, W=(1 << 13) + 1, conn=5)),                # EINVAL comes before ERANGE
               (ERANGE, dict(N=65536, flows=flows.data_ptr() + 2)),                # ERANGE before EALIGN
               (EALIGN, dict(nbytes=0, labels=labels.data_ptr() + 2)),             # EALIGN before the workspace's size
               (EALIGN, dict(flows=flows.data_ptr() + 2)), (EALIGN, dict(ws=ws.data_ptr() + 4)), (EALIGN, dict(labels=labels.data_ptr() + 1)),
               (EALIGN, dict(count=count.data_ptr() + 2)), (EALIGN, dict(area=area.data_ptr() + 2)), (EALIGN, dict(box=box.data_ptr() + 2)),
               (EALIGN, dict(sums=sums.data_ptr() + 4)), (EALIGN, dict(mean=mean.data_ptr() + 4))]
    for code, change in refused:
        assert call(**change) == code, change
    assert L.pwc_regions_workspace_bytes(0, H, W) == 0 and L.pwc_regions_workspace_bytes(65536, H, W) == 0
    assert L.pwc_regions_workspace_bytes(1, 1 << 13, (1 << 13) + 1) == 0 and L.pwc_regions_workspace_bytes(1, 1 << 13, 1 << 13) > 0
    torch.cuda.synchronize()
    for t in (labels, count, area, box, sums):
        assert bool((t == -5).all())
    assert bool((mean == 7.0).all())
    print(f"regions refusals: {len(refused)} calls refused, outputs untouched")
    assert call() == 0 and call(flows=None, sums=None, mean=None) == 0
    torch.cuda.synchronize()
    assert count[:N].tolist() == [1, 1] and area[:N * Rr].tolist() == [H * W, 0, 0, 0] * N and bool((labels[:-1] == 1).all())
    with pytest.raises(ValueError):
        P.label_regions(mask, connectivity=6)
    with pytest.raises(ValueError):
        P.label_regions(mask, min_area=0)
    with pytest.raises(ValueError):
        P.label_regions(mask, max_regions=65536)
    with pytest.raises(TypeError):
        P.label_regions(mask.float())
    with pytest.raises(ValueError):
        P.label_regions(mask, flows=flows[:, :, :5, :2])
    with pytest.raises(ValueError):
        P.label_regions(mask.cpu())


def test_infer_continuous_regions_cli(P, tmp_path):
    """The CLI in fresh child processes: four 64 x 128 frames, un-learned weights.  With --motion affine --regions the files equal
    the API's on the .flo files read back; a child without --regions writes the same .flo and .png files byte for byte; --regions
    without --motion is an argparse error."""
    from PIL import Image
    from pwcnet_amd import flow_io
    rng = np.random.RandomState(5)
    base = rng.uniform(0, 255, size=(64, 128, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(4):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2"]
    flags = ["--regions", "--regions_min_area", "2", "--regions_connectivity", "4", "--regions_threshold", "0.001"]
    run = subprocess.run(cli + ["--out", str(tmp_path / "o"), "--motion", "affine"] + flags, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Figure saved" in run.stdout, run.stderr[-2000:]
    out = tmp_path / "o" / "seq"
    flows = _up(np.stack([flow_io.read_flo(str(out / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)]))
    matrices = _up(np.load(tmp_path / "o" / "motion.npy"))
    labels, count, reg = P.moving_regions(flows, matrices, threshold=0.001, connectivity=4, min_area=2, max_regions=256)[:3]
    labels, count = labels.cpu().numpy(), count.cpu().numpy()
    print(f"regions cli: counts {count.tolist()}")
    for i in range(3):
        png = np.asarray(Image.open(out / f"frame_{i:02d}_regions.png"))
        table = np.load(out / f"frame_{i:02d}_regions.npy")
        rows = min(int(count[i]), 256)
        assert png.shape == (64, 128) and png.dtype == np.uint16 and np.array_equal(png, np.minimum(labels[i], 65535))
        assert table.shape == (rows, 7) and table.dtype == np.float64
        assert np.array_equal(table[:, 0], reg["area"][i, :rows].cpu().numpy()) and np.array_equal(table[:, 1:5], reg["box"][i, :rows].cpu().numpy())
        assert np.array_equal(_bits(table[:, 5:]), _bits(reg["mean"][i, :rows].cpu().numpy()))
    plain = subprocess.run(cli + ["--out", str(tmp_path / "plain"), "--motion", "affine"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert not (tmp_path / "plain" / "seq" / "frame_00_regions.png").exists()
    for i in range(3):                                                             # the flag changes nothing else
        for ext in (".flo", ".png"):
            assert (tmp_path / "plain" / "seq" / f"frame_{i:02d}{ext}").read_bytes() == (out / f"frame_{i:02d}{ext}").read_bytes()
    assert (tmp_path / "plain" / "motion.npy").read_bytes() == (tmp_path / "o" / "motion.npy").read_bytes()
    bad = subprocess.run(cli + ["--out", str(tmp_path / "bad"), "--regions"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--regions needs --motion" in bad.stderr
