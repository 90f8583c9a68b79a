"""CPU tests of the moving-regions feature: the numpy restatement of the definition (tests/regions_ref.py) against
scipy.ndimage.label as partitions and against direct computations, the conditions the GPU tests rely on, two mutations the shared
inputs tell apart, the argument checks and the C ABI surface.  No GPU."""
import numpy as np
import pytest
import torch

from tests import motion_ref as MR
from tests import regions_ref as R

TH, TW = 32, 32                                       # pwc_regions_tile_h / _w (test_c_abi_surface holds them to the library)
SHAPES = ((1, 1), (1, 2 * TW + 3), (2 * TH + 3, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 5, 3 * TW + 7))


def _by_first_occurrence(labels):
    """A labelling as a partition: every non-zero label replaced by its rank in raster order of first occurrence."""
    flat = labels.reshape(-1)
    values, first = np.unique(flat[flat != 0], return_index=True) if (flat != 0).any() else (np.array([], flat.dtype), np.array([], int))
    position = np.flatnonzero(flat != 0)[first]
    lut = {int(v): r + 1 for r, v in enumerate(values[np.argsort(position)])}
    return np.array([lut.get(int(v), 0) for v in flat], np.int64).reshape(labels.shape)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_scipy_label_as_partitions(shape, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    for name, m in R.patterns(*shape, TH, TW).items():
        labels, count = R.label_regions(m[None], connectivity, min_area=1, max_regions=4)[:2]
        want, k = ndimage.label(m, structure=structure)
        assert count[0] == k, name
        assert np.array_equal(_by_first_occurrence(labels[0]), _by_first_occurrence(want)), name
        assert np.array_equal(labels[0], _by_first_occurrence(want)), name          # ids ARE the raster order of first pixels


def test_boxes_areas_and_sums_against_direct_computations():
    H, W = 2 * TH + 5, 3 * TW + 7
    m = R.patterns(H, W, TH, TW)["bernoulli0.4"]
    flows = R.seeded_flows(1, H, W, seed=3)
    labels, count, area, box, sums, mean = R.label_regions(m[None], 8, 1, 64, flows=flows)
    fg = R.foreground(m[None], False, flows)[0]
    assert np.array_equal(labels[0] > 0, fg) and count[0] > 64
    for i in range(1, 65):
        ys, xs = np.nonzero(labels[0] == i)
        assert area[0, i - 1] == len(ys) and box[0, i - 1].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
        su = sv = 0                                                               # Python integers: no overflow, any order
        for y, x in zip(ys, xs):
            u, v = float(flows[0, y, x, 0]), float(flows[0, y, x, 1])
            su += int(round(min(max(u, -65536.0), 65536.0) * 65536.0))            # (round half to even, as rint)
            sv += int(round(min(max(v, -65536.0), 65536.0) * 65536.0))
        assert int(sums[0, i - 1, 0]) == su and int(sums[0, i - 1, 1]) == sv
        assert mean[0, i - 1, 0] == (su / 65536.0) / len(ys) and mean[0, i - 1, 1] == (sv / 65536.0) / len(ys)
    assert np.abs(sums).max() > 65536 * 65536                                     # a clamped value took part
    first = [np.flatnonzero(labels[0].reshape(-1) == i)[0] for i in range(1, count[0] + 1)]
    assert first == sorted(first)


def test_what_the_gpu_inputs_rely_on():
    H, W = 2 * TH + 5, 3 * TW + 7
    pats = R.patterns(H, W, TH, TW)
    counts = {c: {n: int(R.label_regions(pats[n][None], c)[1][0]) for n in ("bernoulli0.4", "bernoulli0.6", "checkerboard")} for c in (4, 8)}
    flat = [k for c in counts.values() for k in c.values()]
    assert any(k > 256 for k in flat) and any(0 < k < 256 for k in flat), counts
    assert counts[4]["checkerboard"] == (H * W + 1) // 2 and counts[8]["checkerboard"] == 1
    for c in (4, 8):                                                              # a min_area that drops some and keeps others
        one, five = R.label_regions(pats["bernoulli0.4"][None], c)[1][0], R.label_regions(pats["bernoulli0.4"][None], c, min_area=5)[1][0]
        assert 0 < five < one
        dropped = R.label_regions(pats["bernoulli0.4"][None], c, min_area=5)[0][0]
        assert ((dropped == 0) & (pats["bernoulli0.4"] != 0)).any()
    for name in ("serpentine", "u"):                                              # ONE component, rooted in the first tile, mostly elsewhere
        for c in (4, 8):
            labels, count, area, box = R.label_regions(pats[name][None], c)[:4]
            assert count[0] == 1 and labels[0, 0, 0] == 1 and area[0, 0] == int(pats[name].sum())
            assert box[0, 0].tolist() == [0, 0, W - 1, H - 1]
            assert pats[name][:TH, :TW].sum() < area[0, 0] / 2
    for name in ("diagonal", "antidiagonal"):                                     # they hang together by corners alone
        assert R.label_regions(pats[name][None], 4)[1][0] == int(pats[name].sum()) > R.label_regions(pats[name][None], 8)[1][0]
    assert pats["antidiagonal"][TH, TW - 1] and pats["antidiagonal"][TH - 1, TW] and pats["diagonal"][TH - 1, TW - 1] and pats["diagonal"][TH, TW]
    flows = R.seeded_flows(2, 9, 11, seed=5, cs=4, offset=1)
    assert flows.shape == (2, 9, 11, 4) and (flows[..., 0] == np.float32(-7.5e8)).all() and np.isnan(flows[..., 1:3]).any()


def test_mutations_are_told_apart_by_the_shared_inputs():
    H, W = 2 * TH + 5, 3 * TW + 7
    pats = R.patterns(H, W, TH, TW)
    changed = {"no_antidiagonal": [], "by_area": []}
    for name, m in pats.items():
        want = R.label_regions(m[None], 8)
        for mutation in changed:
            got = R.label_regions(m[None], 8, mutate=mutation)
            if not all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])):
                changed[mutation].append(name)
    assert "antidiagonal" in changed["no_antidiagonal"] and "checkerboard" in changed["no_antidiagonal"], changed
    assert "bernoulli0.4" in changed["by_area"] and "bernoulli0.6" in changed["by_area"], changed


def test_the_rectangle_scene_on_the_restatements():
    """The GPU test's moving_regions scene on the CPU: motion_ref's fit and residual, then the regions: one kept component, the
    rectangle's box, the mean residual within 0.2 px of (8, -6)."""
    flows, rect = R.rectangle_scene(2, 2 * TH + 5, 3 * TW + 7, seed=1)
    fit = MR.fit(flows, None, "affine", 4, 1.0)
    residual, inlier = MR.residual(flows, fit["matrices"], None, 3.0)
    labels, count, area, box, sums, mean = R.label_regions(inlier, 8, 16, 256, flows=residual, invert=True)
    print(f"rectangle scene: count {count.tolist()} box {box[:, 0].tolist()} mean {mean[:, 0].tolist()}")
    assert fit["ok"].all()
    for n in range(2):
        assert count[n] == 1 and box[n, 0].tolist() == list(rect)
        assert np.abs(mean[n, 0] - np.array([8.0, -6.0])).max() < 0.2


def test_argument_checks_come_before_the_device():
    import pwcnet_amd
    from pwcnet_amd import regions
    for name in ("label_regions", "moving_regions"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(regions, name)
    mask = torch.ones((2, 4, 5), dtype=torch.bool)
    flows = torch.zeros((2, 4, 5, 2))
    with pytest.raises(TypeError, match="mask"):
        regions.label_regions(mask.float())
    with pytest.raises(TypeError, match="mask"):
        regions.label_regions(None)
    with pytest.raises(ValueError, match="mask"):
        regions.label_regions(mask[0])
    with pytest.raises(ValueError, match="mask"):
        regions.label_regions(mask[:, :, ::2])
    with pytest.raises(TypeError, match="flows"):
        regions.label_regions(mask, flows=flows.double())
    with pytest.raises(ValueError, match="flows"):
        regions.label_regions(mask, flows=flows[:, :3])
    for bad in (6, 0, True, "8"):
        with pytest.raises(ValueError, match="connectivity"):
            regions.label_regions(mask, connectivity=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_area"):
            regions.label_regions(mask, min_area=bad)
    for bad in (0, 65536, 2.0):
        with pytest.raises(ValueError, match="max_regions"):
            regions.label_regions(mask, max_regions=bad)
    with pytest.raises(ValueError, match="GPU only"):
        regions.label_regions(mask, flows=flows)
    with pytest.raises(TypeError, match="invert"):
        regions.moving_regions(flows, torch.eye(3, dtype=torch.float64).repeat(2, 1, 1), invert=False)
    with pytest.raises(ValueError, match="GPU only"):
        regions.moving_regions(flows, torch.eye(3, dtype=torch.float64).repeat(2, 1, 1), min_area=4)


def test_c_abi_surface():
    from pwcnet_amd import _lib
    assert "pwc_regions.hip" in _lib.SOURCES
    for name in ("pwc_regions_tile_h", "pwc_regions_tile_w", "pwc_regions_workspace_bytes", "pwc_label_regions"):
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert (L.pwc_regions_tile_h(), L.pwc_regions_tile_w()) == (TH, TW)
    for N, H, W in ((1, 1, 1), (3, 13, 19), (2, 260, 256), (8, 448, 1024)):
        parts = min((H * W + 255) // 256, 256)
        assert L.pwc_regions_workspace_bytes(N, H, W) == 4 * (3 * N * H * W + 2 * N * parts)
    assert L.pwc_regions_workspace_bytes(0, 4, 4) == 0 and L.pwc_regions_workspace_bytes(65536, 4, 4) == 0
    assert L.pwc_regions_workspace_bytes(1, 1 << 13, (1 << 13) + 1) == 0 and L.pwc_regions_workspace_bytes(1, 1 << 13, 1 << 13) > 0
    # refusals that need no device: the checks come before any launch
    assert L.pwc_label_regions(None, 0, None, 2, 1, 4, 4, 8, 1, 4, None, 0, None, None, None, None, None, None, None) == -1
    buf = torch.zeros(64, dtype=torch.int64)                                      # (host memory: refused before anything reads it)
    p = buf.data_ptr()
    assert L.pwc_label_regions(p, 0, None, 2, 1, 4, 4, 8, 1, 4, None, 0, p, p, p, p, None, None, None) == -1
    assert L.pwc_label_regions(p, 0, None, 2, 1, 4, 4, 8, 1, 4, p, 1 << 20, p, p, p, p, p, None, None) == -1   # sums without flows
    from infer_continuous import build_parser
    ap = build_parser()
    args = ap.parse_args(["-i", "a", "b"])
    assert not args.regions and args.regions_min_area == 16 and args.regions_connectivity == 8 and args.regions_threshold == 3.0
    args = ap.parse_args(["-i", "a", "b", "--motion", "affine", "--regions", "--regions_min_area", "4", "--regions_connectivity", "4",
                          "--regions_threshold", "1.5"])
    assert (args.regions, args.regions_min_area, args.regions_connectivity, args.regions_threshold) == (True, 4, 4, 1.5)
    with pytest.raises(SystemExit):
        ap.parse_args(["-i", "a", "b", "--regions_connectivity", "6"])
