"""Region tracking on the GPU (pwc_region_links.hip, pwcnet_amd.region_tracks, infer_continuous.py --regions_track) against the
numpy restatement of the definition in tests/region_links_ref.py (checked on the CPU by tests/test_host_region_tracks.py).

Every output is an integer: the yardstick is BIT EQUALITY of succ, pred, best_succ, best_pred, votes, ids, age and the painted
images, no tolerance.  Every case prints its figures before it asserts (profiles/region_tracks_gpu_test_figures.txt)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib
from pwcnet_amd import region_tracks as T  # the feature: without it nothing here can be collected
from tests import region_links_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3
SHAPES = ((1, 1), (1, 67), (67, 1), (64, 64), (33, 65), (70, 130))
ROWS = (1, 4, 256, 1024)


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    assert pwcnet_amd.link_regions is T.link_regions and pwcnet_amd.track_regions is T.track_regions
    return pwcnet_amd


def _up(a):
    return a if a is None or not isinstance(a, np.ndarray) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    return None if t is None else t.cpu().numpy()


def _same(tag, got, want):
    """got, want: dictionaries of arrays with the same keys."""
    diff = {k: int((np.asarray(got[k]) != np.asarray(want[k])).sum()) if np.shape(got[k]) == np.shape(want[k]) else "shape" for k in want}
    print(f"region_tracks {tag}: elements that differ {diff}")
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (tag, k, got[k].shape, got[k].dtype, want[k].shape)
        assert np.array_equal(got[k], want[k]), (tag, k)


def _link(P, la, lb, flows, aa, ab, valid=None, **kw):
    out = P.link_regions(_up(la), _up(lb), _up(flows), _up(aa), _up(ab), valid=_up(valid), **kw)
    assert all(out[k].dtype == torch.int32 for k in L.KEYS)
    return {k: _cpu(out[k]) for k in L.KEYS}


def _bernoulli_labels(P, S, H, W, p, connectivity, rows, seed):
    """label_regions' labels, counts and areas of S Bernoulli(p) masks, on the device and on the host."""
    rng = np.random.default_rng(seed)
    mask = _up((rng.random((S, H, W)) < p).astype(np.uint8))
    labels, count, reg = P.label_regions(mask, connectivity=connectivity, max_regions=rows)
    return labels, count, reg


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_links_of_bernoulli_labels_equal_the_restatement_bit_for_bit(P, shape):
    """Three images per mask kind, linked 0 -> 1 and 1 -> 2 as one batch of two: p = 0.3 and 0.6, both connectivities, R = 1, 4, 256
    and 1024, sub-pixel flows in +-3 px with exact halves; the second link under a mask and with NaN, Inf and the sentinel."""
    H, W = shape
    linked = 0
    for p in (0.3, 0.6):
        for connectivity in (4, 8):
            flows = L.subpixel_flows(2, H, W, seed=int(10 * p) + connectivity)
            poisoned = L.subpixel_flows(2, H, W, seed=int(10 * p) + connectivity, poison=True)
            valid = (np.random.default_rng(H + W).random((2, H, W)) < 0.85).astype(np.uint8) * 3
            for rows in ROWS:
                labels, count, reg = _bernoulli_labels(P, 3, H, W, p, connectivity, rows, seed=100 * H + W)
                la, lb, aa, ab = labels[:-1].contiguous(), labels[1:].contiguous(), reg["area"][:-1].contiguous(), reg["area"][1:].contiguous()
                h = [_cpu(t) for t in (la, lb, aa, ab)]
                tag = f"{H}x{W} p {p} c{connectivity} R {rows} counts {_cpu(count).tolist()}"
                want = L.link_regions(h[0], h[1], flows, h[2], h[3])
                _same(tag, _link(P, la, lb, flows, aa, ab), want)
                _same(tag + " masked, poisoned", _link(P, la, lb, poisoned, aa, ab, valid=valid),
                      L.link_regions(h[0], h[1], poisoned, h[2], h[3], valid))
                _same(tag + " min_overlap 2 min_fraction 0.5", _link(P, la, lb, flows, aa, ab, min_overlap=2, min_fraction=0.5),
                      L.link_regions(h[0], h[1], flows, h[2], h[3], None, 2, 0.5))
                linked += int((want["succ"] != 0).sum())
    assert linked > 0 or min(H, W) == 1


def test_named_cases_as_one_batch(P):
    """tests/test_host_region_tracks.py says what each case is for: split, merge, ties, half-integer targets, leaving voters, unknown
    flows in the open and under the mask, labels beyond R, thresholds at equality and one below."""
    names, la, lb, flows, aa, ab, valid = L.case_batch()
    for kw in (dict(), dict(min_overlap=12), dict(min_fraction=0.5), dict(min_overlap=13, min_fraction=1.0)):
        got = _link(P, la, lb, flows, aa, ab, valid=valid, **kw)
        want = L.link_regions(la, lb, flows, aa, ab, valid, **kw)
        _same(f"named cases {kw}", got, want)
    i = names.index
    assert got["succ"][i("threshold"), 0] == 0 and want["best_succ"][i("halves"), 0] == 5 and want["succ"][i("merge"), :2].tolist() == [1, 0]
    got = _link(P, la, lb, flows, aa, ab, valid=valid, min_overlap=12, min_fraction=0.5)
    assert got["succ"][i("threshold"), 0] == 1 and got["succ"][i("threshold_below"), 0] == 0


def test_one_region_onto_one_region_and_64_distinct_keys_in_a_wave(P):
    """96 x 128, every pixel region 1 on both sides: every vote of the image goes to ONE address.  And 2 x 64 with 64 different
    regions along a row and along the targets: every lane of a wave holds a key of its own (64 turns)."""
    H, W = 96, 128
    one = np.ones((1, H, W), np.int32)
    flows = L.subpixel_flows(1, H, W, seed=4)
    area = np.zeros((1, 256), np.int32)
    area[0, 0] = H * W
    want = L.link_regions(one, one, flows, area, area)
    _same("one region onto one region 96x128", _link(P, one, one, flows, area, area), want)
    assert want["votes"][0, 0, 0] + want["votes"][0, 0, 2] == H * W and want["votes"][0, 0, 2] > 0 and want["succ"][0, 0] == 1
    la = np.broadcast_to(np.arange(1, 65, dtype=np.int32), (1, 2, 64)).copy()
    lb = la[:, :, ::-1].copy()
    zero = np.zeros((1, 2, 64, 2), np.float32)
    aa, ab = L.areas(la, 64)[0], L.areas(lb, 64)[0]
    want = L.link_regions(la, lb, zero, aa, ab)
    _same("64 distinct keys in a wave", _link(P, la, lb, zero, aa, ab), want)
    assert want["succ"][0].tolist() == list(range(64, 0, -1)) and (want["votes"][0, :, 0] == 2).all()


def test_channel_strides_and_offsets_give_the_same_bits(P):
    H, W = 33, 65
    labels, count, reg = _bernoulli_labels(P, 2, H, W, 0.6, 8, 256, seed=21)
    la, lb, aa, ab = labels[:1].contiguous(), labels[1:].contiguous(), reg["area"][:1].contiguous(), reg["area"][1:].contiguous()
    flows = L.subpixel_flows(1, H, W, seed=6, poison=True)
    want = L.link_regions(_cpu(la), _cpu(lb), flows, _cpu(aa), _cpu(ab))
    for width in (2, 3, 4):
        for lo in range(width - 1):
            buf = torch.full((1, H, W, width), float("nan"), dtype=torch.float32, device="cuda")
            buf[..., lo:lo + 2] = _up(flows)
            view = buf[..., lo:lo + 2]
            out = P.link_regions(la, lb, view, aa, ab)
            _same(f"stride {width} offset {lo} (address % 8 = {view.data_ptr() % 8})", {k: _cpu(out[k]) for k in L.KEYS}, want)


def test_an_image_alone_gives_the_bits_it_gives_in_a_batch_and_twice(P):
    """A batch of three with busy neighbours (one region onto one region on both sides of it) against the one-image call."""
    H, W = 70, 130
    for rows in (4, 256):
        labels, count, reg = _bernoulli_labels(P, 2, H, W, 0.6, 4, rows, seed=33)
        full = torch.ones((1, H, W), dtype=torch.int32, device="cuda")
        full_area = torch.full((1, rows), H * W, dtype=torch.int32, device="cuda")
        flows = _up(L.subpixel_flows(3, H, W, seed=8))
        la, lb = torch.cat([full, labels[:1], full]), torch.cat([full, labels[1:], full])
        aa, ab = torch.cat([full_area, reg["area"][:1], full_area]), torch.cat([full_area, reg["area"][1:], full_area])
        three = P.link_regions(la, lb, flows, aa, ab)
        alone = P.link_regions(la[1:2].contiguous(), lb[1:2].contiguous(), flows[1:2], aa[1:2].contiguous(), ab[1:2].contiguous())
        again = P.link_regions(la[1:2].contiguous(), lb[1:2].contiguous(), flows[1:2], aa[1:2].contiguous(), ab[1:2].contiguous())
        _same(f"seam R {rows}", {k: _cpu(three[k][1:2]) for k in L.KEYS}, {k: _cpu(alone[k]) for k in L.KEYS})
        _same(f"two calls R {rows}", {k: _cpu(again[k]) for k in L.KEYS}, {k: _cpu(alone[k]) for k in L.KEYS})
        assert int(three["votes"][0, 0, 3]) == H * W and bool((alone["succ"] != 0).any())


@pytest.mark.parametrize("rows", ROWS)
def test_identities_and_relabel_equal_the_restatement(P, rows):
    """Links drawn at random (any int32 row index is legal input), S = 1, 2 and 5, alone and continued from a state."""
    rng = np.random.default_rng(rows)
    for S in (1, 2, 5):
        count = rng.integers(0, rows + 3, size=S).astype(np.int32)
        pred = rng.integers(0, rows + 1, size=(S - 1, rows)).astype(np.int32)
        pred[pred > 0] = np.where(rng.random(int((pred > 0).sum())) < 0.5, pred[pred > 0], 0)
        if S > 1:
            pred[0, 0] = rows + 5 if rows < 1024 else -2                            # an index beyond the table: fresh
        ids, age, state = P.region_identities(_up(pred), _up(count))
        want = L.identities(pred, count, rows)
        _same(f"identities R {rows} S {S}", dict(ids=_cpu(ids), age=_cpu(age), next_id=_cpu(state["next_id"])[0:1]),
              dict(ids=want[0], age=want[1], next_id=np.asarray([want[2]["next_id"]], np.int32)))
        more = rng.integers(0, rows + 1, size=(S, rows)).astype(np.int32)
        ids2, age2, state2 = P.region_identities(_up(more), _up(count[::-1].copy()), state=state)
        want2 = L.identities(more, count[::-1], rows, want[2])
        _same(f"identities R {rows} S {S} continued", dict(ids=_cpu(ids2), age=_cpu(age2), next_id=_cpu(state2["next_id"])[0:1]),
              dict(ids=want2[0], age=want2[1], next_id=np.asarray([want2[2]["next_id"]], np.int32)))
        assert state2["next_id_bound"] == 1 + 2 * S * rows >= want2[2]["next_id"]
        labels = rng.integers(-2, rows + 4, size=(S, 33, 65)).astype(np.int32)
        _same(f"relabel R {rows} S {S}", dict(out=_cpu(P.relabel_regions(_up(labels), ids))), dict(out=L.relabel(labels, want[0])))


def _track(P, labels, count, reg, flows, valid=None, state=None, **kw):
    ids, age, links, state = P.track_regions(labels, count, reg, flows, valid=valid, state=state, **kw)
    return dict(ids=_cpu(ids), age=_cpu(age), **{k: _cpu(links[k]) for k in L.KEYS}), state


def _track_ref(labels, count, reg, flows, valid=None, **kw):
    ids, age, links, _ = L.track_regions(_cpu(labels), _cpu(count), _cpu(reg["area"]), flows, valid, **kw)
    return dict(ids=ids, age=age, **links)


@pytest.mark.parametrize("rows", ROWS)
def test_track_regions_in_one_call_and_in_batches(P, rows):
    """S = 1 (no link, ids only), 2 and 5 on Bernoulli labels; batches of 1, 2 and S give the bits of one call; under a mask."""
    H, W = 33, 65
    for S in (1, 2, 5):
        labels, count, reg = _bernoulli_labels(P, S, H, W, 0.6 if rows > 4 else 0.3, 8, rows, seed=7 * S + rows)
        flows = L.subpixel_flows(S, H, W, seed=S, poison=True)
        valid = (np.random.default_rng(S).random((S, H, W)) < 0.9).astype(np.uint8)
        for mask in (None, valid):
            want = _track_ref(labels, count, reg, flows, mask, min_overlap=2)
            got, _ = _track(P, labels, count, reg, _up(flows), _up(mask), min_overlap=2)
            _same(f"track R {rows} S {S} mask {mask is not None}", got, want)
            for cut in sorted({1, 2, S}):
                st, parts = None, []
                for s0 in range(0, S, cut):
                    sl = slice(s0, s0 + cut)
                    piece = {"area": reg["area"][sl].contiguous()}
                    part, st = _track(P, labels[sl].contiguous(), count[sl].contiguous(), piece, _up(flows[sl]),
                                      None if mask is None else _up(mask[sl]), st, min_overlap=2)
                    parts.append(part)
                joined = {k: np.concatenate([p[k] for p in parts]) for k in ("ids", "age")}
                # (the first piece holds cut - 1 links, every later one the link from the state as well: S - 1 in all)
                links = {k: np.concatenate([p[k] for p in parts]) for k in L.KEYS}
                _same(f"track R {rows} S {S} mask {mask is not None} in batches of {cut}", dict(joined, **links), want)


def test_track_regions_behind_moving_regions(P):
    """Two rectangles on a translating background (tests/test_host_region_tracks.py runs the same scene on the restatements): the
    per-image ids of the two swap on the way, their identities do not."""
    flows, rects = L.moving_scene(5, 70, 130, seed=2)
    f = _up(flows)
    matrices, ok, _ = P.fit_motion(f, model="affine")
    labels, count, reg = P.moving_regions(f, matrices, min_area=16)[:3]
    got, state = _track(P, labels, count, reg, f)
    _same("moving scene", got, _track_ref(labels, count, reg, flows))
    ids, age, box = got["ids"], got["age"], _cpu(reg["box"])
    assert bool(ok.all()) and _cpu(count).tolist() == [2] * 5
    who = [[[tuple(b) for b in box[s, :2].tolist()].index(r) for r in rects[s]] for s in range(5)]
    assert who[0] != who[4]
    for k in range(2):
        assert len({int(ids[s, who[s][k]]) for s in range(5)}) == 1 and [int(age[s, who[s][k]]) for s in range(5)] == [1, 2, 3, 4, 5]
    painted = _cpu(P.relabel_regions(labels, _up(ids)))
    for s in range(5):
        for k, (x0, y0, x1, y1) in enumerate(rects[s]):
            assert (painted[s, y0:y1 + 1, x0:x1 + 1] == ids[0, who[0][k]]).all()
    assert int(state["next_id"][0]) == 3 and state["next_id_bound"] == 1 + 5 * 256
    print(f"region_tracks moving scene: rows of the rectangles per pair {who} identities {ids[:, :2].tolist()}")


def test_refusals_by_their_codes(P):
    N, H, W, R = 2, 5, 6, 4
    lib = _lib.lib()
    nbytes = lib.pwc_region_links_workspace_bytes(N, R)
    assert nbytes == 4 * N * R * (R + 2)
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device="cuda")         # noqa: E731
    la, lb, aa, ab = i32(N * H * W, 1), i32(N * H * W, 1), i32(N * R, H * W), i32(N * R, H * W)
    flows = torch.zeros((N, H, W, 4), dtype=torch.float32, device="cuda")
    valid = torch.ones((N, H, W), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(nbytes // 8 + 2, dtype=torch.int64, device="cuda")
    outs = {k: i32(N * R * (4 if k == "votes" else 1) + 1, -5) for k in L.KEYS}
    p = lambda v: None if v is None else ctypes.c_void_p(v)                          # noqa: E731

    def link(**change):
        a = dict(la=la.data_ptr(), lb=lb.data_ptr(), aa=aa.data_ptr(), ab=ab.data_ptr(), flows=flows.data_ptr(), cs=4, valid=valid.data_ptr(),
                 N=N, H=H, W=W, R=R, mo=1, mf=0.0, ws=ws.data_ptr(), nbytes=nbytes, **{k: outs[k].data_ptr() for k in L.KEYS})
        a.update(change)
        return lib.pwc_link_regions(p(a["la"]), p(a["lb"]), p(a["aa"]), p(a["ab"]), p(a["flows"]), a["cs"], p(a["valid"]), a["N"], a["H"],
                                    a["W"], a["R"], a["mo"], a["mf"], p(a["ws"]), a["nbytes"], p(a["succ"]), p(a["pred"]),
                                    p(a["best_succ"]), p(a["best_pred"]), p(a["votes"]), _lib.current_stream())

    refused = [(EINVAL, dict(la=None)), (EINVAL, dict(lb=None)), (EINVAL, dict(aa=None)), (EINVAL, dict(ab=None)), (EINVAL, dict(flows=None)),
               (EINVAL, dict(ws=None)), (EINVAL, dict(succ=None)), (EINVAL, dict(pred=None)), (EINVAL, dict(best_succ=None)),
               (EINVAL, dict(best_pred=None)), (EINVAL, dict(votes=None)), (EINVAL, dict(N=0)), (EINVAL, dict(H=0)), (EINVAL, dict(W=-1)),
               (EINVAL, dict(R=0)), (EINVAL, dict(mo=0)), (EINVAL, dict(mf=-0.5)), (EINVAL, dict(mf=1.0000001)), (EINVAL, dict(mf=float("nan"))),
               (EINVAL, dict(cs=1)), (EINVAL, dict(nbytes=nbytes - 1)),
               (ERANGE, dict(R=1025)), (ERANGE, dict(H=1 << 13, W=(1 << 13) + 1)), (ERANGE, dict(N=65536)),
               (EINVAL, dict(R=1025, cs=1)), (ERANGE, dict(N=65536, flows=flows.data_ptr() + 2)),
               (EALIGN, dict(nbytes=0, la=la.data_ptr() + 2)), (EALIGN, dict(flows=flows.data_ptr() + 2)), (EALIGN, dict(ws=ws.data_ptr() + 4)),
               (EALIGN, dict(lb=lb.data_ptr() + 1)), (EALIGN, dict(aa=aa.data_ptr() + 2)), (EALIGN, dict(ab=ab.data_ptr() + 2))] + \
              [(EALIGN, {k: outs[k].data_ptr() + 2}) for k in L.KEYS]
    for code, change in refused:
        assert link(**change) == code, change
    ids, age, nxt = i32(2 * R + 1, -5), i32(2 * R + 1, -5), i32(2, -5)
    count = i32(2, 3)

    def ident(**change):
        a = dict(pred=outs["pred"].data_ptr(), count=count.data_ptr(), ip=None, ap=None, pp=None, nid=1, nin=None, S=2, R=R, ids=ids.data_ptr(),
                 age=age.data_ptr(), out=nxt.data_ptr())
        a.update(change)
        return lib.pwc_region_identities(p(a["pred"]), p(a["count"]), p(a["ip"]), p(a["ap"]), p(a["pp"]), a["nid"], p(a["nin"]), a["S"],
                                         a["R"], p(a["ids"]), p(a["age"]), p(a["out"]), _lib.current_stream())

    refused_ident = [(EINVAL, dict(count=None)), (EINVAL, dict(ids=None)), (EINVAL, dict(pred=None)), (EINVAL, dict(ip=aa.data_ptr())),
                     (EINVAL, dict(S=0)), (EINVAL, dict(nid=0)), (ERANGE, dict(R=1025)), (ERANGE, dict(nid=(1 << 31) - 2 * R)),
                     (EALIGN, dict(ids=ids.data_ptr() + 2)), (EALIGN, dict(out=nxt.data_ptr() + 2))]
    for code, change in refused_ident:
        assert ident(**change) == code, change
    painted = i32(N * H * W + 1, -5)

    def relabel(**change):
        a = dict(labels=la.data_ptr(), ids=ids.data_ptr(), S=N, H=H, W=W, R=R, out=painted.data_ptr())
        a.update(change)
        return lib.pwc_relabel_regions(p(a["labels"]), p(a["ids"]), a["S"], a["H"], a["W"], a["R"], p(a["out"]), _lib.current_stream())

    refused_relabel = [(EINVAL, dict(labels=None)), (EINVAL, dict(out=None)), (EINVAL, dict(H=0)), (ERANGE, dict(R=1025)), (ERANGE, dict(S=65536)),
                       (EALIGN, dict(ids=ids.data_ptr() + 2)), (EALIGN, dict(out=painted.data_ptr() + 1))]
    for code, change in refused_relabel:
        assert relabel(**change) == code, change
    torch.cuda.synchronize()
    for t in list(outs.values()) + [ids, age, nxt, painted]:
        assert bool((t == -5).all())
    print(f"region_tracks refusals: {len(refused) + len(refused_ident) + len(refused_relabel)} calls refused, outputs untouched")
    assert link() == 0 and link(valid=None) == 0
    torch.cuda.synchronize()
    assert outs["succ"][:N * R].tolist() == [1, 0, 0, 0] * N and outs["votes"][:4].tolist() == [H * W, 0, 0, H * W] and int(outs["succ"][-1]) == -5
    assert ident() == 0 and relabel() == 0
    torch.cuda.synchronize()
    assert ids[:2 * R].tolist() == [1, 2, 3, 0, 1, 4, 5, 0] and age[:2 * R].tolist() == [1, 1, 1, 0, 2, 1, 1, 0] and nxt.tolist() == [6, -5]
    assert bool((painted[:-1] == 1).all()) and int(painted[-1]) == -5
    with pytest.raises(ValueError):
        P.link_regions(la.view(N, H, W), lb.view(N, H, W), flows[..., :2], aa.view(N, R), ab.view(N, R), min_overlap=0)
    with pytest.raises(ValueError):
        P.link_regions(la.view(N, H, W), lb.view(N, H, W), flows[..., :2], aa.view(N, R), ab.view(N, R), min_fraction=2.0)
    with pytest.raises(ValueError):
        P.link_regions(la.view(N, H, W).cpu(), lb.view(N, H, W), flows[..., :2], aa.view(N, R), ab.view(N, R))
    with pytest.raises(TypeError):
        P.relabel_regions(la.view(N, H, W).float(), ids[:N * R].view(N, R))


def test_infer_continuous_regions_track_cli(P, tmp_path):
    """The CLI in fresh child processes: four 64 x 128 frames in batches of two pairs, un-learned weights.  Two children without the
    flag write the same bytes; a child with it writes the same files besides its own, and its tables equal the API's on the .flo
    files read back (one call over the three pairs: the CLI's two batches stream); the flag without --regions is an argparse
    error."""
    from PIL import Image
    from pwcnet_amd import flow_io
    rng = np.random.RandomState(5)
    base = rng.uniform(0, 255, size=(64, 128, 3)).astype(np.uint8)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(4):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(seq / f"frame_{i:02d}.png")
    cli = [sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i", str(seq / "frame_*.png"), "--pipeline", "1", "--batch", "2",
           "--motion", "affine"]
    flags = ["--regions", "--regions_min_area", "2", "--regions_connectivity", "4", "--regions_threshold", "0.001"]
    runs = {name: subprocess.run(cli + ["--out", str(tmp_path / name)] + flags + extra, capture_output=True, text=True, timeout=300)
            for name, extra in (("a", []), ("b", []), ("t", ["--regions_track", "--regions_track_overlap", "2"]))}
    for name, run in runs.items():
        assert run.returncode == 0 and "Figure saved" in run.stdout, (name, run.stderr[-2000:])
    files = {name: sorted(str(f.relative_to(tmp_path / name)) for f in (tmp_path / name).rglob("*") if f.is_file()) for name in runs}
    assert files["a"] == files["b"] and not any("_ids" in f or "tracks" in f for f in files["a"])
    for f in files["a"]:                                                               # without the flag: byte for byte, twice
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes() == (tmp_path / "t" / f).read_bytes(), f
    extra = sorted(set(files["t"]) - set(files["a"]))
    assert extra == sorted([os.path.join("seq", f"frame_{i:02d}_regions_ids.{e}") for i in range(3) for e in ("npy", "png")] + ["regions_tracks.npy"])
    out = tmp_path / "t" / "seq"
    flows = _up(np.stack([flow_io.read_flo(str(out / f"frame_{i:02d}.flo")).astype(np.float32) for i in range(3)]))
    matrices = _up(np.load(tmp_path / "t" / "motion.npy"))
    labels, count, reg = P.moving_regions(flows, matrices, threshold=0.001, connectivity=4, min_area=2, max_regions=256)[:3]
    ids, age = P.track_regions(labels, count, reg, flows, min_overlap=2)[:2]
    painted = P.relabel_regions(labels, ids).clamp(max=65535).cpu().numpy()
    ids, age, count = ids.cpu().numpy(), age.cpu().numpy(), count.cpu().numpy()
    spans = {}
    for i in range(3):
        rows = min(int(count[i]), 256)
        table = np.load(out / f"frame_{i:02d}_regions_ids.npy")
        png = np.asarray(Image.open(out / f"frame_{i:02d}_regions_ids.png"))
        assert table.shape == (rows, 2) and table.dtype == np.int32
        assert np.array_equal(table[:, 0], ids[i, :rows]) and np.array_equal(table[:, 1], age[i, :rows])
        assert png.shape == (64, 128) and png.dtype == np.uint16 and np.array_equal(png, painted[i])
        for identity in ids[i, :rows].tolist():
            spans.setdefault(identity, [i, i])[1] = i
    tracks = np.load(tmp_path / "t" / "regions_tracks.npy")
    assert tracks.dtype == np.int32 and tracks.tolist() == [[k, v[0], v[1]] for k, v in sorted(spans.items())]
    print(f"region_tracks cli: counts {count.tolist()} identities {len(spans)} carried over a pair {int((age > 1).sum())}")
    bad = subprocess.run(cli + ["--out", str(tmp_path / "bad"), "--regions_track"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--regions_track needs --regions" in bad.stderr
