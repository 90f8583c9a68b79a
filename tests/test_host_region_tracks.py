"""CPU tests of region tracking: the numpy restatement of the definition (tests/region_links_ref.py) against independent routes --
the vote table against an explicit pixel loop, identities against a dictionary walk --, what the named cases are for, asserted on
the restatement alone, three mutations the cases tell apart, the argument checks and the C ABI surface.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import region_links_ref as L

H, W, R = L.CASE_H, L.CASE_W, L.CASE_R
_AL, _MIS = 4096, 4100      # an aligned and a 4-byte-aligned-only non-null address: argument checks only, nothing is launched
EINVAL, EALIGN, ERANGE = -1, -2, -3


def _link(case, **kw):
    c = L.cases()[case] if isinstance(case, str) else case
    area_a, area_b = L.areas(c["labels_a"][None], R)[0][0], L.areas(c["labels_b"][None], R)[0][0]
    return dict(zip(L.KEYS, L.link_image(c["labels_a"], c["labels_b"], c["flow"], area_a, area_b, c["valid"], **kw)))


def _pixel_loop(labels_a, labels_b, flow, valid, rows):
    """The vote table one pixel at a time, in Python numbers; round() is ties-to-even on its own."""
    h, w = labels_a.shape
    overlap, left = np.zeros((rows, rows + 1), np.int64), np.zeros(rows, np.int64)
    for y in range(h):
        for x in range(w):
            la = int(labels_a[y, x])
            if not 1 <= la <= rows or (valid is not None and valid[y, x] == 0):
                continue
            u, v = float(flow[y, x, 0]), float(flow[y, x, 1])
            if not (abs(u) <= 1e9 and abs(v) <= 1e9):
                continue
            qx, qy = round(x + u), round(y + v)
            if not (0 <= qx <= w - 1 and 0 <= qy <= h - 1):
                left[la - 1] += 1
                continue
            lb = int(labels_b[qy, qx])
            overlap[la - 1, lb if 1 <= lb <= rows else 0] += 1
    return overlap, left


def test_vote_table_by_unique_equals_an_explicit_pixel_loop():
    for name, c in L.cases().items():
        got = L.vote_table(c["labels_a"], c["labels_b"], c["flow"], c["valid"], R)
        want = _pixel_loop(c["labels_a"], c["labels_b"], c["flow"], c["valid"], R)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    rng = np.random.default_rng(3)
    for rows in (1, 4, 40):
        la = rng.integers(-1, rows + 3, size=(2, 33, 65)).astype(np.int32)
        lb = rng.integers(-1, rows + 3, size=(2, 33, 65)).astype(np.int32)
        flows = L.subpixel_flows(2, 33, 65, seed=rows, poison=True)
        valid = (rng.random((2, 33, 65)) < 0.8).astype(np.uint8)
        for n in range(2):
            got, want = L.vote_table(la[n], lb[n], flows[n], valid[n], rows), _pixel_loop(la[n], lb[n], flows[n], valid[n], rows)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0].sum() > 100 and want[1].sum() > 0
    f = L.subpixel_flows(1, 33, 65, seed=5)                                         # the flows the GPU tests use hold exact halves
    assert ((f * 2 == np.rint(f * 2)) & (f != np.rint(f))).mean() > 0.1 and np.abs(f).max() <= 3.0


def _walk(pred, count, rows, first=1):
    """Identities by a dictionary over (image, region)."""
    ident, age, nxt = {}, {}, first
    for s in range(len(count)):
        for b in range(1, min(int(count[s]), rows) + 1):
            p = int(pred[s - 1][b - 1]) if s > 0 else 0
            if p and (s - 1, p) in ident:
                ident[s, b], age[s, b] = ident[s - 1, p], age[s - 1, p] + 1
            else:
                ident[s, b], age[s, b], nxt = nxt, 1, nxt + 1
    return ident, age, nxt


def test_identities_equal_a_dictionary_walk():
    rng = np.random.default_rng(11)
    for rows, S in ((1, 4), (4, 6), (70, 5)):
        count = rng.integers(0, rows + 3, size=S).astype(np.int32)
        pred = rng.integers(0, rows + 1, size=(S - 1, rows)).astype(np.int32)
        ids, age, state = L.identities(pred, count, rows)
        ident, ages, nxt = _walk(pred, count, rows)
        assert state["next_id"] == nxt
        for s in range(S):
            for b in range(1, rows + 1):
                assert ids[s, b - 1] == ident.get((s, b), 0) and age[s, b - 1] == ages.get((s, b), 0)
        for cut in (1, 2):                                                          # fed in pieces: the bits of one call
            st, got = None, []
            for s0 in range(0, S, cut):
                piece = pred[s0:s0 + cut - 1] if st is None else pred[s0 - 1:s0 + cut - 1]
                i, a, st = L.identities(piece, count[s0:s0 + cut], rows, st)
                got.append((i, a))
            assert np.array_equal(np.concatenate([g[0] for g in got]), ids) and np.array_equal(np.concatenate([g[1] for g in got]), age)
            assert st["next_id"] == nxt


def _clip(rects_per_image, moves, h=24, w=40, rows=8, **kw):
    labels = np.stack([L.paint(h, w, r) for r in rects_per_image])
    area, count = L.areas(labels, rows)
    flows = L.constant_flows(labels, moves)
    return labels, count, area, flows, L.track_regions(labels, count, area, flows, **kw)


def test_two_translating_rectangles_keep_their_identities_over_five_images():
    rects = [[(2 + 3 * s, 2 + s, 7 + 3 * s, 6 + s), (30 - 2 * s, 12, 36 - 2 * s, 18)] for s in range(5)]
    moves = [[(3.0, 1.0), (-2.0, 0.0)]] * 5
    labels, count, area, flows, (ids, age, links, state) = _clip(rects, moves)
    assert ids[:, :2].tolist() == [[1, 2]] * 5 and not ids[:, 2:].any() and age[:, :2].tolist() == [[s, s] for s in range(1, 6)]
    assert links["succ"][:, :2].tolist() == [[1, 2]] * 4 and links["votes"][:, 0].tolist() == [[30, 0, 0, 30]] * 4
    assert state["next_id"] == 3
    painted = L.relabel(labels, ids)
    assert np.array_equal(painted, labels)                                          # (ids are 1, 2 here)
    for cut in (1, 2, 5):                                                           # streaming in batches of 1, 2 and S
        st, got = None, []
        for s0 in range(0, 5, cut):
            sl = slice(s0, s0 + cut)
            i, a, ln, st = L.track_regions(labels[sl], count[sl], area[sl], flows[sl], state=st)
            got.append((i, a))
        assert np.array_equal(np.concatenate([g[0] for g in got]), ids) and np.array_equal(np.concatenate([g[1] for g in got]), age)


def test_a_rectangle_vanishes_and_one_appears():
    one, two, new = (2, 2, 7, 6), (20, 3, 26, 9), (10, 14, 15, 20)
    rects = [[one, two], [one, two], [two], [two, new], [(1, 1, 3, 3), two, new]]    # image 4: another one, FIRST in raster order
    moves = [[(0.0, 0.0)] * len(r) for r in rects]
    labels, count, area, flows, (ids, age, links, state) = _clip(rects, moves)
    assert ids[:, :3].tolist() == [[1, 2, 0], [1, 2, 0], [2, 0, 0], [2, 3, 0], [4, 2, 3]]
    assert age[:, :3].tolist() == [[1, 1, 0], [2, 2, 0], [3, 0, 0], [4, 1, 0], [1, 5, 2]]
    assert links["succ"][1, :2].tolist() == [0, 1] and links["best_succ"][1, 0] == 0 and links["votes"][1, 0].tolist() == [0, 30, 0, 30]
    assert links["pred"][2, :2].tolist() == [1, 0] and state["next_id"] == 5
    two_new = [[one], [(1, 1, 3, 3), one, (20, 14, 25, 20)]]                        # two appear at once: numbered in ascending row
    ids2 = _clip(two_new, [[(0.0, 0.0)]] + [[(0.0, 0.0)] * 3])[4][0]
    assert ids2[:, :3].tolist() == [[1, 0, 0], [2, 1, 3]]


def test_split_and_merge():
    s = _link("split")
    assert s["best_succ"][0] == 1 and s["best_pred"][:2].tolist() == [1, 1] and s["succ"][0] == 1 and s["pred"][:2].tolist() == [1, 0]
    assert s["votes"][0].tolist() == [24, 4, 0, 40]
    c = L.cases()["split"]
    labels = np.stack([c["labels_a"], c["labels_b"]])
    area, count = L.areas(labels, R)
    ids, age = L.track_regions(labels, count, area, np.zeros((2, H, W, 2), np.float32))[:2]
    assert ids[:, :2].tolist() == [[1, 0], [1, 2]] and age[:, :2].tolist() == [[1, 0], [2, 1]]      # the larger part keeps it
    m = _link("merge")
    assert m["best_succ"][:2].tolist() == [1, 1] and m["best_pred"][0] == 1 and m["succ"][:2].tolist() == [1, 0] and m["pred"][0] == 1
    ids, age = L.track_regions(labels[::-1], count[::-1], area[::-1], np.zeros((2, H, W, 2), np.float32))[:2]
    assert ids[:, :2].tolist() == [[1, 2], [1, 0]] and age[1, 0] == 2                # the smaller one's identity ends


def test_exact_ties_go_to_the_smallest_index():
    r, c = _link("row_tie"), _link("column_tie")
    table = L.vote_table(**{k: L.cases()["row_tie"][k] for k in ("labels_a", "labels_b", "flow", "valid")}, R=R)[0]
    assert table[0, 1] == table[0, 2] == 4
    assert r["best_succ"][0] == 1 and r["succ"][0] == 1 and r["best_pred"][:2].tolist() == [1, 1] and r["pred"][:2].tolist() == [1, 0]
    assert c["best_pred"][0] == 1 and c["pred"][0] == 1 and c["best_succ"][:2].tolist() == [1, 1] and c["succ"][:2].tolist() == [1, 0]


def test_half_integer_targets_round_to_even():
    c = L.cases()["halves"]
    qx, _ = L.targets(c["flow"])
    x = np.arange(W, dtype=np.float64)
    assert np.array_equal(qx[0], np.where(x % 2 == 0, x, x + 1))                    # x + 0.5: even x rounds DOWN, odd x UP
    assert np.array_equal(qx[1], np.where(x % 2 == 0, x, x - 1))                    # x - 0.5: even x rounds UP to x, odd x DOWN
    assert np.array_equal(qx[2], np.where(x % 2 == 0, x + 2, x + 1)) and np.array_equal(qx[3], np.where(x % 2 == 0, x - 2, x - 1))
    table = L.vote_table(c["labels_a"], c["labels_b"], c["flow"], None, R)[0]
    assert table[0, 1:].sum() == 40 and not table[0, 2::2][:7].any()                # targets are EVEN columns: labels_b = x + 1 is odd
    assert _link("halves")["best_succ"][0] == 5 and _link("halves")["votes"][0].tolist() == [8, 0, 0, 40]                 # (x = 4: two from each row; 6 and 8 tie with it)
    _, qy = L.targets(L.cases()["halves_y"]["flow"])
    assert qy[1, 0] == 2.0 and qy[2, 0] == 2.0 and qy[1, 1] == 0.0 and qy[2, 1] == 0.0 and qy[4, 1] == 2.0


def test_leaving_voters_and_unknown_flows():
    v = _link("leave")["votes"][0].tolist()
    # the first row leaves upwards (16); rows 1 .. 7: columns 0 .. 2 leave left (x - 3 < 0), columns 13 .. 15 right (x + 3.25 -> 16 ..)
    assert v == [128 - 16 - 7 * 6, 0, 16 + 7 * 6, 128]
    c = L.cases()["leave"]
    assert L.targets(c["flow"])[0][1, 12] == 15.0 and L.targets(c["flow"])[1][0, 5] == -1.0
    o, h = _link("poison_open"), _link("poison_hidden")
    assert o["votes"][0].tolist() == [64 - 20, 0, 4, 64 - 16]                       # 16 unknown pixels vote nowhere; 1e9 is known and leaves
    assert o["votes"][1].tolist() == [48, 0, 0, 48]
    assert h["votes"][0].tolist() == [48, 0, 0, 48] and h["votes"][1].tolist() == [36, 0, 0, 36]
    assert np.isnan(L.cases()["poison_hidden"]["flow"]).any() and (L.cases()["poison_hidden"]["flow"] == L.SENTINEL).any()


def test_labels_beyond_the_table():
    b = _link("beyond")
    # a's region 1 lands on b's id R (the last row); a's R + 1 does not vote; a's region 3 lands on an id beyond R: column 0
    assert b["best_succ"][0] == R and b["succ"][0] == R and b["pred"][R - 1] == 1 and b["votes"][0].tolist() == [16, 0, 0, 16]
    assert b["best_succ"][2] == 0 and b["votes"][2].tolist() == [0, 16, 0, 16] and b["votes"][:, 3].sum() == 32
    assert not b["pred"][:R - 1].any()


def test_thresholds_at_equality_and_one_below():
    assert _link("threshold")["votes"][0].tolist() == [12, 0, 0, 12] and _link("threshold_below")["votes"][0].tolist() == [11, 0, 0, 11]
    for kw in (dict(min_overlap=12), dict(min_fraction=0.5), dict(min_overlap=12, min_fraction=0.5)):
        at, below = _link("threshold", **kw), _link("threshold_below", **kw)
        assert at["succ"][0] == 1 and at["pred"][0] == 1 and at["best_succ"][0] == 1
        assert below["succ"][0] == 0 and below["pred"][0] == 0 and below["best_succ"][0] == 1 and below["best_pred"][0] == 1
    assert _link("threshold", min_overlap=13)["succ"][0] == 0 and _link("threshold_below", min_overlap=11)["succ"][0] == 1
    assert _link("threshold", min_fraction=1.0)["succ"][0] == 0 and _link("split", min_fraction=1.0)["succ"][0] == 1   # 24 of min(40, 24)


def test_mutations_are_told_apart_by_their_cases():
    changed = {m: [n for n in L.cases() if any(not np.array_equal(_link(n, mutate=m)[k], _link(n)[k]) for k in L.KEYS)]
               for m in ("ties_largest", "floor_half", "one_sided")}
    assert "row_tie" in changed["ties_largest"] and "column_tie" in changed["ties_largest"], changed
    assert "halves" in changed["floor_half"] and "halves_y" in changed["floor_half"], changed
    assert "merge" in changed["one_sided"] and "split" in changed["one_sided"], changed
    assert "split" not in changed["ties_largest"] and "merge" not in changed["floor_half"] and "row_tie" not in changed["floor_half"]


def test_the_moving_scene_on_the_restatements():
    """The GPU test's scene on the CPU: motion_ref's fit and residual, regions_ref's labels, then the links: each rectangle keeps
    one identity over the five pairs although the per-image ids swap."""
    from tests import motion_ref as MR
    from tests import regions_ref as RR
    flows, rects = L.moving_scene(5, 70, 130, seed=2)
    fit = MR.fit(flows, None, "affine", 4, 1.0)
    residual, inlier = MR.residual(flows, fit["matrices"], None, 3.0)
    labels, count, area, box = RR.label_regions(inlier, 8, 16, 256, flows=residual, invert=True)[:4]
    assert count.tolist() == [2] * 5
    ids, age = L.track_regions(labels, count, area, flows)[:2]
    who = [[[tuple(b) for b in box[s, :2].tolist()].index(r) for r in rects[s]] for s in range(5)]   # row of rectangle k in image s
    assert who[0] != who[4]                                                         # the raster order of the two swaps
    for k in range(2):
        assert len({int(ids[s, who[s][k]]) for s in range(5)}) == 1 and [int(age[s, who[s][k]]) for s in range(5)] == [1, 2, 3, 4, 5]
    assert sorted(ids[0, :2].tolist()) == [1, 2]


def test_argument_checks_come_before_the_device():
    import pwcnet_amd
    from pwcnet_amd import region_tracks as T
    for name in ("link_regions", "region_identities", "relabel_regions", "track_regions"):
        assert name in pwcnet_amd.__all__ and getattr(pwcnet_amd, name) is getattr(T, name)
    la = torch.zeros((2, 4, 5), dtype=torch.int32)
    flows = torch.zeros((2, 4, 5, 2))
    area = torch.zeros((2, 3), dtype=torch.int32)
    count = torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(TypeError, match="labels_a"):
        T.link_regions(la.long(), la, flows, area, area)
    with pytest.raises(ValueError, match="labels_b"):
        T.link_regions(la, la[:, :3], flows, area, area)
    with pytest.raises(TypeError, match="flows_ab"):
        T.link_regions(la, la, flows.double(), area, area)
    with pytest.raises(ValueError, match="flows_ab"):
        T.link_regions(la, la, flows[:, :3], area, area)
    with pytest.raises(ValueError, match="area_a"):
        T.link_regions(la, la, flows, torch.zeros((2, 1025), dtype=torch.int32), area)
    with pytest.raises(ValueError, match="area_b"):
        T.link_regions(la, la, flows, area, area[:, :2])
    with pytest.raises(TypeError, match="valid"):
        T.link_regions(la, la, flows, area, area, valid=la)
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError, match="min_overlap"):
            T.link_regions(la, la, flows, area, area, min_overlap=bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="min_fraction"):
            T.link_regions(la, la, flows, area, area, min_fraction=bad)
    with pytest.raises(ValueError, match="GPU only"):
        T.link_regions(la, la, flows, area, area)
    with pytest.raises(TypeError, match="pred"):
        T.region_identities(None, count)
    with pytest.raises(ValueError, match="pred"):
        T.region_identities(area, count)                                            # two rows of links for two images
    with pytest.raises(TypeError, match="state"):
        T.region_identities(area, count, state={"ids": area[0]})
    with pytest.raises(ValueError, match="GPU only"):
        T.region_identities(area[:1], count)
    with pytest.raises(ValueError, match="ids"):
        T.relabel_regions(la, area[:1])
    with pytest.raises(ValueError, match="GPU only"):
        T.relabel_regions(la, area)
    with pytest.raises(TypeError, match="regions"):
        T.track_regions(la, count, area, flows)
    with pytest.raises(ValueError, match="count"):
        T.track_regions(la, count[:1], {"area": area}, flows)
    with pytest.raises(ValueError, match="flows"):
        T.track_regions(la, count, {"area": area}, flows[:1])
    with pytest.raises(ValueError, match="GPU only"):
        T.track_regions(la, count, {"area": area}, flows)


def test_c_abi_surface_and_refusals_that_need_no_launch():
    from pwcnet_amd import _lib
    names = ("pwc_region_links_workspace_bytes", "pwc_link_regions", "pwc_region_identities", "pwc_relabel_regions")
    assert "pwc_region_links.hip" in _lib.SOURCES and all(n in _lib.SIGNATURES for n in names)
    with open(_lib.os.path.join(_lib.CSRC, "..", "..", "include", "pwc_hip.h")) as f:
        header = f.read()
    assert all(n + "(" in header for n in names) and "region tracking" in header
    lib = _lib.lib()
    for N, rows in ((1, 1), (3, 5), (8, 256), (2, 1024), (65535, 4)):
        assert lib.pwc_region_links_workspace_bytes(N, rows) == (4 * N * rows * (rows + 2) + 7) // 8 * 8
    for N, rows in ((0, 4), (65536, 4), (1, 0), (1, 1025), (-1, -1)):
        assert lib.pwc_region_links_workspace_bytes(N, rows) == 0
    p = lambda v: None if v is None else ctypes.c_void_p(v)                          # noqa: E731

    def link(**change):
        a = dict(la=_AL, lb=_AL, aa=_AL, ab=_AL, flows=_AL, cs=2, valid=None, N=1, H=4, W=4, R=4, mo=1, mf=0.0, ws=_AL, nbytes=1 << 20,
                 succ=_AL, pred=_AL, bs=_AL, bp=_AL, votes=_AL)
        a.update(change)
        return lib.pwc_link_regions(p(a["la"]), p(a["lb"]), p(a["aa"]), p(a["ab"]), p(a["flows"]), a["cs"], p(a["valid"]), a["N"], a["H"],
                                    a["W"], a["R"], a["mo"], a["mf"], p(a["ws"]), a["nbytes"], p(a["succ"]), p(a["pred"]), p(a["bs"]),
                                    p(a["bp"]), p(a["votes"]), None)

    refused = [(EINVAL, dict(la=None)), (EINVAL, dict(lb=None)), (EINVAL, dict(aa=None)), (EINVAL, dict(ab=None)), (EINVAL, dict(flows=None)),
               (EINVAL, dict(ws=None)), (EINVAL, dict(succ=None)), (EINVAL, dict(pred=None)), (EINVAL, dict(bs=None)), (EINVAL, dict(bp=None)),
               (EINVAL, dict(votes=None)), (EINVAL, dict(N=0)), (EINVAL, dict(H=0)), (EINVAL, dict(W=-1)), (EINVAL, dict(R=0)),
               (EINVAL, dict(mo=0)), (EINVAL, dict(mf=-0.25)), (EINVAL, dict(mf=1.5)), (EINVAL, dict(mf=float("nan"))),
               (EINVAL, dict(mf=float("inf"))), (EINVAL, dict(cs=1)),
               (ERANGE, dict(R=1025)), (ERANGE, dict(H=1 << 13, W=(1 << 13) + 1)), (ERANGE, dict(N=65536)),
               (EINVAL, dict(R=1025, mo=0)), (EINVAL, dict(N=65536, cs=1)),                       # EINVAL comes before ERANGE
               (ERANGE, dict(R=1025, flows=_MIS + 2)),                                            # ERANGE before EALIGN
               (EALIGN, dict(nbytes=0, la=_AL + 2)),                                              # EALIGN before the workspace's size
               (EALIGN, dict(la=_AL + 1)), (EALIGN, dict(lb=_AL + 2)), (EALIGN, dict(aa=_AL + 2)), (EALIGN, dict(ab=_AL + 3)),
               (EALIGN, dict(flows=_AL + 2)), (EALIGN, dict(ws=_MIS)), (EALIGN, dict(succ=_AL + 2)), (EALIGN, dict(pred=_AL + 2)),
               (EALIGN, dict(bs=_AL + 2)), (EALIGN, dict(bp=_AL + 2)), (EALIGN, dict(votes=_AL + 2)),
               (EINVAL, dict(nbytes=4 * 4 * 6 - 1)), (EINVAL, dict(nbytes=0))]
    for code, change in refused:
        assert link(**change) == code, change

    def ident(**change):
        a = dict(pred=_AL, count=_AL, ip=None, ap=None, pp=None, nid=1, nin=None, S=2, R=4, ids=_AL, age=_AL, out=_AL)
        a.update(change)
        return lib.pwc_region_identities(p(a["pred"]), p(a["count"]), p(a["ip"]), p(a["ap"]), p(a["pp"]), a["nid"], p(a["nin"]), a["S"],
                                         a["R"], p(a["ids"]), p(a["age"]), p(a["out"]), None)

    refused = [(EINVAL, dict(count=None)), (EINVAL, dict(ids=None)), (EINVAL, dict(age=None)), (EINVAL, dict(out=None)), (EINVAL, dict(pred=None)),
               (EINVAL, dict(ip=_AL)), (EINVAL, dict(ip=_AL, ap=_AL)), (EINVAL, dict(pp=_AL)), (EINVAL, dict(S=0)), (EINVAL, dict(R=0)),
               (EINVAL, dict(nid=0)), (ERANGE, dict(R=1025)), (ERANGE, dict(nid=(1 << 31) - 8)), (ERANGE, dict(nid=(1 << 31) - 8, ids=_AL + 2)),
               (EALIGN, dict(nid=(1 << 31) - 9, ids=_AL + 2)),
               (EINVAL, dict(R=1025, nid=0)), (EALIGN, dict(pred=_AL + 2)), (EALIGN, dict(count=_AL + 1)), (EALIGN, dict(ids=_AL + 2)),
               (EALIGN, dict(age=_AL + 2)), (EALIGN, dict(out=_AL + 2)), (EALIGN, dict(nin=_AL + 2)),
               (EALIGN, dict(ip=_AL + 2, ap=_AL, pp=_AL)), (EALIGN, dict(ip=_AL, ap=_AL + 2, pp=_AL)), (EALIGN, dict(ip=_AL, ap=_AL, pp=_AL + 2))]
    for code, change in refused:
        assert ident(**change) == code, change

    def relabel(**change):
        a = dict(labels=_AL, ids=_AL, S=1, H=4, W=4, R=4, out=_AL)
        a.update(change)
        return lib.pwc_relabel_regions(p(a["labels"]), p(a["ids"]), a["S"], a["H"], a["W"], a["R"], p(a["out"]), None)

    refused = [(EINVAL, dict(labels=None)), (EINVAL, dict(ids=None)), (EINVAL, dict(out=None)), (EINVAL, dict(S=0)), (EINVAL, dict(H=0)),
               (EINVAL, dict(W=0)), (EINVAL, dict(R=0)), (ERANGE, dict(R=1025)), (ERANGE, dict(S=65536)), (ERANGE, dict(H=1 << 13, W=(1 << 13) + 1)),
               (ERANGE, dict(R=1025, out=_AL + 2)), (EALIGN, dict(labels=_AL + 2)), (EALIGN, dict(ids=_AL + 1)), (EALIGN, dict(out=_AL + 2))]
    for code, change in refused:
        assert relabel(**change) == code, change

    from infer_continuous import build_parser
    ap = build_parser()
    args = ap.parse_args(["-i", "a", "b"])
    assert not args.regions_track and args.regions_track_overlap == 1 and args.regions_track_fraction == 0.0
    args = ap.parse_args(["-i", "a", "b", "--motion", "affine", "--regions", "--regions_track", "--regions_track_overlap", "5",
                          "--regions_track_fraction", "0.25"])
    assert (args.regions_track, args.regions_track_overlap, args.regions_track_fraction) == (True, 5, 0.25)
    with pytest.raises(SystemExit):
        ap.parse_args(["-i", "a", "b", "--regions_track_overlap", "0"])
