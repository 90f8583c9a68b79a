"""The numpy restatement of the flow filter (tests/flow_filter_ref.py, the yardstick of tests/test_gpu_flow_filter.py) held to a
second, independent route (whole-image arrays, the counting form and the bit-by-bit selection on the keys), to np.median and
scipy.ndimage.median_filter, and to cases worked by hand; pwcnet_amd.filter_tables held to its formulas; and three mutations of
the restatement shown to change named cases.  No GPU."""
import numpy as np
import pytest

from pwcnet_amd import flow_filter as FF  # the feature: without it nothing here can be collected
from tests import flow_filter_ref as R

X = np.float32(1e10)                                        # an unknown pixel


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the second route
def alt_pass(flows, valid, guide, r, space, color, smooth, fill, min_count, route):
    """One pass over ONE image on whole-image arrays: the window as (2r+1)^2 shifted planes of keys and 64-bit weights (a cell
    beyond the frame has weight 0), then the median by `route`: "counting" (every candidate's cumulative weight, the smallest key
    that reaches T / 2) or "bits" (the key built from bit 31 down)."""
    H, W = flows.shape[:2]
    kn = R.known(flows, valid)
    D = 2 * r + 1
    pad = lambda a, fill_value=0: np.pad(a, ((r, r), (r, r)) + ((0, 0),) * (a.ndim - 2), constant_values=fill_value)
    ku, kv, knp = pad(R.keys(flows[..., 0])), pad(R.keys(flows[..., 1])), pad(kn, False)
    gp = None if guide is None else pad(guide)
    KU, KV, WT = [], [], []
    for dy in range(D):
        for dx in range(D):
            w = np.where(knp[dy:dy + H, dx:dx + W], np.uint64(space[dy * D + dx]), np.uint64(0))
            if guide is not None:
                d = np.abs(gp[dy:dy + H, dx:dx + W] - guide).sum(axis=2)
                w = w * np.asarray(color, np.uint64)[d]
            KU.append(ku[dy:dy + H, dx:dx + W]); KV.append(kv[dy:dy + H, dx:dx + W]); WT.append(w)
    KU, KV, WT = np.stack(KU), np.stack(KV), np.stack(WT)
    n, T = (WT > 0).sum(axis=0), WT.sum(axis=0)

    def median(K):
        if route == "counting":
            best = np.full((H, W), 0xFFFFFFFF, np.uint32)
            for i in range(D * D):
                cum = np.where(K <= K[i], WT, np.uint64(0)).sum(axis=0)
                hit = (WT[i] > 0) & (2 * cum >= T)
                best = np.where(hit & (K[i] < best), K[i], best)
            return best
        prefix = np.zeros((H, W), np.uint32)
        for b in range(31, -1, -1):
            trial = prefix | np.uint32(1 << b)
            below = np.where(K < trial, WT, np.uint64(0)).sum(axis=0)
            prefix = np.where(2 * below < T, trial, prefix)
        return prefix
    med = np.stack([R.unkeys(median(KU)), R.unkeys(median(KV))], axis=2)
    take = np.where(kn, bool(smooth) & (n >= 1), bool(fill) & (n >= min_count))
    ok = kn | take
    out = np.where(take[..., None], med, np.where(kn[..., None], flows[..., :2], X)).astype(np.float32)
    # (np.where on float32 keeps the bits)
    return out, ok.astype(np.uint8)


def alt(flows, guide, valid, r, space, color, smooth, fill, min_count, iters, route):
    g = None if guide is None else R.guide_bytes(guide)
    outs, oks = [], []
    for n in range(flows.shape[0]):
        f, v = flows[n], None if valid is None else valid[n]
        for _ in range(iters):
            f, v = alt_pass(f, v, None if g is None else g[n], r, space, color, smooth, fill, min_count, route)
        outs.append(f); oks.append(v)
    return np.stack(outs), np.stack(oks)


def random_case(seed, N, H, W, kind):
    rs = np.random.RandomState(seed)
    f = (rs.randint(-3, 4, size=(N, H, W, 2)) * 0.5).astype(np.float32)
    pick = rs.uniform(size=f.shape)
    f[pick < 0.1] = -0.0
    f[(pick > 0.9)] = rs.normal(0, 1e6, size=int((pick > 0.9).sum())).astype(np.float32)
    hole = rs.uniform(size=(N, H, W)) < 0.2
    f[hole, 0] = np.array([np.nan, np.inf, 1e10, -np.inf], np.float32)[rs.randint(0, 4, size=int(hole.sum()))]
    valid = rs.uniform(size=(N, H, W)) < 0.8
    guide = None
    if kind == "u8":
        guide = (np.kron(rs.randint(0, 256, size=(N, -(-H // 2), -(-W // 3), 3)), np.ones((1, 2, 3, 1), np.int64))[:, :H, :W]).astype(np.uint8)
    elif kind == "f32":
        guide = rs.uniform(-0.2, 1.2, size=(N, H, W, 1)).astype(np.float32)
        guide[rs.uniform(size=guide.shape) < 0.05] = np.nan
    return f, guide, valid


@pytest.mark.parametrize("route", ("counting", "bits"))
@pytest.mark.parametrize("kind,r", ((None, 1), ("u8", 2), ("f32", 3), ("u8", 7)))
def test_restatement_equals_the_second_route(route, kind, r):
    f, guide, valid = random_case(10 * r + (kind is not None), 2, 7, 12, kind)
    C = 3 if kind == "u8" else 1
    space, color = FF.filter_tables(r, 1.2 + r / 3, 9.0, C)
    space[3] = 0                                             # a zero in the window
    for smooth, fill, min_count, iters in ((True, False, 1, 1), (False, True, 3, 2), (True, True, 1, 3)):
        want = R.filter_flow_ref(f, guide, valid, r, space, color, smooth, fill, min_count, iters)
        got = alt(f, guide, valid, r, space, color, smooth, fill, min_count, iters, route)
        assert np.array_equal(got[1], want[1]), (route, smooth, fill)
        assert np.array_equal(bits(got[0]), bits(want[0])), (route, smooth, fill, int((bits(got[0]) != bits(want[0])).sum()))


@pytest.mark.parametrize("r", (1, 2, 3))
def test_box_window_is_the_plain_median_on_interior_pixels(r):
    """Box table, no guide, every pixel known: an interior window holds (2r+1)^2 values, an odd number, and the lower weighted
    median is THE median.  (Distinct values: np.median returns an element then.)"""
    from scipy.ndimage import median_filter
    rs = np.random.RandomState(3 + r)
    H, W = 11, 16
    f = rs.permutation(2 * H * W).reshape(1, H, W, 2).astype(np.float32) - 100.0
    out, ok = R.filter_flow_ref(f, None, None, r, np.full((2 * r + 1) ** 2, 65535), None)
    assert ok.all()
    for c in range(2):
        assert np.array_equal(out[0, r:-r, r:-r, c], median_filter(f[0, :, :, c], size=2 * r + 1)[r:-r, r:-r])
        for y, x in ((r, r), (H - r - 1, W - r - 1), (H // 2, W // 2)):
            assert out[0, y, x, c] == np.median(f[0, y - r:y + r + 1, x - r:x + r + 1, c])


def row(u, v=None):
    """A 1 x W image from lists."""
    u = np.asarray(u, np.float32)
    return np.stack([u, u if v is None else np.asarray(v, np.float32)], axis=1)[None, None]


def run(u, v=None, r=1, space=None, guide=None, color=None, **kw):
    D = 2 * r + 1
    sp = np.ones(D * D, np.int64) if space is None else np.asarray(space)
    if sp.size == D:                                         # a row table: only the window's middle row is inside a 1 x W frame
        full = np.zeros((D, D), np.int64)
        full[r] = sp
        sp = full.reshape(-1)
    g = None if guide is None else np.asarray(guide, np.uint8).reshape(1, 1, -1, 1)
    out, ok = R.filter_flow_ref(row(u, v), g, None, r, sp, color, **kw)
    return out[0, 0], ok[0, 0]


def test_hand_worked_ties_and_cut_windows():
    out, ok = run([1, 2, 2, 5])
    # windows {1,2} {1,2,2} {2,2,5} {2,5}: the even ones give the LOWER of the two middle values
    assert out[:, 0].tolist() == [1, 2, 2, 2] and ok.all()
    out, _ = run([5, 1, 1])                                  # {5,1} at the border: nothing is replicated (that would give 5)
    assert out[:, 0].tolist() == [1, 1, 1]
    out, _ = run([1, 2, 3], space=[1, 1, 5])                 # centre: weights 1 1 5, T = 7, cumulative 1 2 7 -> 3
    assert out[1, 0] == 3
    out, _ = run([1, 2, 3], space=[3, 1, 3])                 # T = 7: cumulative 3, 4 -> twice 4 reaches 7 -> 2
    assert out[1, 0] == 2
    out, _ = run([1, 2, 3], space=[4, 1, 3])                 # T = 8: twice 4 reaches 8 at the first value -> 1
    assert out[1, 0] == 1


def test_hand_worked_components_are_independent():
    out, _ = run([1, 2, 3], [30, 10, 20])
    assert out[1].tolist() == [2, 20]                        # u from the centre, v from the right neighbour


def test_hand_worked_signed_zeros_and_order():
    out, _ = run([-0.0, 0.0])
    assert bits(out[:, 0]).tolist() == [0x80000000, 0x80000000]          # -0 < +0: the lower of {-0, +0} is -0, with its bits
    out, _ = run([0.0, -0.0, 0.0])
    assert bits(out[:, 0]).tolist() == [0x80000000, 0, 0x80000000]
    out, _ = run([-1e9, -2.5, 1e9])                          # negatives order by value, not by their bits
    assert out[:, 0].tolist() == [-1e9, -2.5, -2.5]
    k = R.keys(np.array([-np.float32(1e9), -1.0, -0.0, 0.0, 1e-45, 1.0, 1e9], np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all() and np.array_equal(bits(R.unkeys(k)), bits([-1e9, -1.0, -0.0, 0.0, 1e-45, 1.0, 1e9]))


def test_hand_worked_zero_weights():
    out, ok = run([1, 9, 3], space=[1, 0, 1])                # the centre has weight 0: it is no candidate
    assert out[:, 0].tolist() == [9, 1, 9] and ok.all()
    out, ok = run([1, X, 3], space=[0, 0, 0], fill=True)     # T = 0: known pixels keep their bits, the hole stays
    assert out[:, 0].tolist() == [1, X, 3] and ok.tolist() == [1, 0, 1] and out[1, 1] == X
    # a colour table that is zero from d = 100 on: the bright pixel is no candidate of the dark ones, and alone in its own window
    color = np.where(np.arange(256) < 100, 7, 0)
    out, _ = run([1, 2, 50], guide=[0, 0, 200], color=color)
    assert out[:, 0].tolist() == [1, 1, 50]


def test_hand_worked_unknowns_min_count_and_passes():
    out, ok = run([1, X, 3], smooth=False, fill=True, min_count=2)
    assert out[:, 0].tolist() == [1, 1, 3] and ok.all()
    out, ok = run([1, X, 3], smooth=False, fill=True, min_count=3)
    assert out[:, 0].tolist() == [1, X, 3] and ok.tolist() == [1, 0, 1]
    out, ok = run([1, X, 3])                                 # smooth alone: the hole stays, its neighbours do not see it
    assert out[:, 0].tolist() == [1, X, 3] and ok.tolist() == [1, 0, 1]
    out, ok = run([1, np.nan, 3], [1, 2, 3], smooth=False, fill=True)   # one bad component makes the pixel unknown: both are filled
    assert out[1].tolist() == [1, 1]
    # a hole of width 2r + 1 = 3: the rim closes in the first pass, the middle in the second
    hole = [1, X, X, X, 2]
    out, ok = run(hole, smooth=False, fill=True, iters=1)
    assert out[:, 0].tolist() == [1, 1, X, 2, 2] and ok.tolist() == [1, 1, 0, 1, 1]
    out, ok = run(hole, smooth=False, fill=True, iters=2)
    assert out[:, 0].tolist() == [1, 1, 1, 2, 2] and ok.all()
    out, ok = run([1, 5, X, X, X, X, X, 7, 9], r=2, smooth=False, fill=True, iters=2)      # r = 2, width 5
    # pass 1: {1,5} -> 1, {5} -> 5, nothing, {7} -> 7, {7,9} -> 7; pass 2: the middle sees {1,5,7,7}, T = 4, twice 1 + 1 reaches it -> 5
    assert ok.all() and out[:, 0].tolist() == [1, 5, 1, 5, 5, 7, 7, 7, 9]


def test_filter_tables_against_the_formulas():
    import math
    for r, ss, sc, C in ((1, 0.8, 5.0, 1), (2, 1.5, 12.0, 3), (7, 3.0, 30.0, 3)):
        space, color = FF.filter_tables(r, ss, sc, C)
        assert space.dtype == color.dtype == np.uint32 and space.shape == ((2 * r + 1) ** 2,) and color.shape == (255 * C + 1,)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                want = 65535.0 * math.exp(-(dx * dx + dy * dy) / (2.0 * ss * ss))
                assert abs(int(space[(dy + r) * (2 * r + 1) + dx + r]) - want) <= 0.5 + 1e-6
        for d in (0, 1, C, 17, 255 * C):
            assert abs(int(color[d]) - 65535.0 * math.exp(-(d / C) / sc)) <= 0.5 + 1e-6
        assert space[len(space) // 2] == 65535 and color[0] == 65535 and space.max() == 65535 and color.max() == 65535
    space, color = FF.filter_tables(3, None, None, 3)
    assert (space == 65535).all() and (color == 65535).all() and color.shape == (766,)
    for bad in (dict(radius=0), dict(radius=8), dict(radius=2, sigma_space=0.0), dict(radius=2, sigma_color=-1.0), dict(radius=2, channels=2)):
        with pytest.raises(ValueError):
            FF.filter_tables(**bad)


def test_mutations_change_their_named_cases():
    """What each rule decides: the restatement with one rule broken differs from the definition on the case that rule is for,
    and only the rules that bear on a case change it."""
    # name -> (row, the pixel looked at, its value under the definition)
    cases = {"odd": ([1, 2, 3], 1, 2), "even at the border": ([1, 2, 9, 9, 9], 0, 1), "border": ([5, 1, 1], 0, 1)}
    changed = {}
    for name, (u, at, want) in cases.items():
        assert run(u=u)[0][at, 0] == want, name
        changed[name] = {m for m in ("strict", "upper", "replicate") if run(u=u, mutate=m)[0][at, 0] != want}
    # `<` for `<=`: the middle of three moves up; the upper median: an even window moves up, an odd one does not;
    # replication: only windows cut by the border change
    assert "strict" in changed["odd"] and "upper" not in changed["odd"] and "replicate" not in changed["odd"]
    assert "upper" in changed["even at the border"]
    assert "replicate" in changed["border"]
    assert run(u=[1, 2, 3], mutate="strict")[0][1, 0] == 3 and run(u=[1, 2, 9, 9, 9], mutate="upper")[0][0, 0] == 2
    assert run(u=[5, 1, 1], mutate="replicate")[0][0, 0] == 5
