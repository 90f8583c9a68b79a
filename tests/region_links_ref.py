"""numpy restatement of the DEFINITION of include/pwc_hip.h, "region tracking" -- not of the kernels' route: voters, targets and
votes of whole images at once (np.unique over pair keys), the two bests by argmax, the mutual rule, then identities image by
image.  tests/test_host_region_tracks.py checks it on the CPU against an explicit pixel loop and a dictionary walk;
tests/test_gpu_region_tracks.py holds the kernels to it bit for bit.  Also the scenes and seeded inputs both share.

`mutate` switches on one deliberate fault at a time, for the host tests that show the shared cases tell it apart:
    "ties_largest"  a tie of overlaps goes to the largest index instead of the smallest
    "floor_half"    floor(x + 0.5) instead of rint (ties away from even targets)
    "one_sided"     succ = best_succ and pred = best_pred wherever the thresholds pass, without the mutual agreement
"""
import numpy as np

SENTINEL = np.float32(1e10)
KEYS = ("succ", "pred", "best_succ", "best_pred", "votes")


def voters(labels_a, flow, valid, R):
    """(H,W) bool: la in 1 .. R, the valid byte, flow_io.flow_valid's rule."""
    v = (labels_a >= 1) & (labels_a <= R)
    if valid is not None:
        v &= np.asarray(valid) != 0
    with np.errstate(invalid="ignore"):
        v &= (np.abs(flow[..., 0]) <= np.float32(1e9)) & (np.abs(flow[..., 1]) <= np.float32(1e9))
    return v


def targets(flow, mutate=None):
    """(qx, qy) doubles of every pixel: rint of ONE double addition each (NaN where the flow is)."""
    H, W = flow.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        sx = x.astype(np.float64) + flow[..., 0].astype(np.float64)
        sy = y.astype(np.float64) + flow[..., 1].astype(np.float64)
        if mutate == "floor_half":
            return np.floor(sx + 0.5), np.floor(sy + 0.5)
        return np.rint(sx), np.rint(sy)


def vote_table(labels_a, labels_b, flow, valid, R, mutate=None):
    """overlap (R, R+1) int64 (row a-1, column c) and left (R,) int64 of one image pair."""
    H, W = labels_a.shape
    v = voters(labels_a, flow, valid, R)
    qx, qy = targets(flow, mutate)
    with np.errstate(invalid="ignore"):
        inside = v & (qx >= 0.0) & (qx <= float(W - 1)) & (qy >= 0.0) & (qy <= float(H - 1))       # compared as doubles
    gone = v & ~inside
    left = np.bincount(labels_a[gone].astype(np.int64) - 1, minlength=R).astype(np.int64)
    la = labels_a[inside].astype(np.int64)
    lb = labels_b[qy[inside].astype(np.int64), qx[inside].astype(np.int64)].astype(np.int64)
    c = np.where((lb >= 1) & (lb <= R), lb, 0)
    overlap = np.zeros((R, R + 1), np.int64)
    keys, n = np.unique((la - 1) * (R + 1) + c, return_counts=True)
    overlap.reshape(-1)[keys] = n
    return overlap, left


def _best(table, axis, mutate):
    """1-based arg-max along `axis` of an (R,R) table, ties to the smallest index, 0 where the maximum is 0."""
    if mutate == "ties_largest":
        flipped = np.flip(table, axis=axis)
        at = table.shape[axis] - 1 - np.argmax(flipped, axis=axis)
    else:
        at = np.argmax(table, axis=axis)             # (the first of equal maxima)
    return np.where(table.max(axis=axis) > 0, at + 1, 0).astype(np.int32)


def link_image(labels_a, labels_b, flow, area_a, area_b, valid=None, min_overlap=1, min_fraction=0.0, mutate=None):
    R = area_a.shape[0]
    overlap, left = vote_table(labels_a, labels_b, flow, valid, R, mutate)
    regions = overlap[:, 1:]
    best_succ, best_pred = _best(regions, 1, mutate), _best(regions, 0, mutate)
    votes = np.zeros((R, 4), np.int32)
    rows = np.arange(R)
    votes[:, 0] = np.where(best_succ > 0, regions[rows, np.maximum(best_succ, 1) - 1], 0)
    votes[:, 1], votes[:, 2], votes[:, 3] = overlap[:, 0], left, overlap.sum(axis=1) + left
    succ, pred = np.zeros(R, np.int32), np.zeros(R, np.int32)

    def accept(a, b):
        ov = int(regions[a - 1, b - 1])
        return ov >= min_overlap and float(ov) >= np.float64(min_fraction) * np.float64(min(int(area_a[a - 1]), int(area_b[b - 1])))

    for a in range(1, R + 1):
        b = int(best_succ[a - 1])
        if b and (mutate == "one_sided" or best_pred[b - 1] == a) and accept(a, b):
            succ[a - 1] = b
    for b in range(1, R + 1):
        a = int(best_pred[b - 1])
        if a and (mutate == "one_sided" or best_succ[a - 1] == b) and accept(a, b):
            pred[b - 1] = a
    return succ, pred, best_succ, best_pred, votes


def link_regions(labels_a, labels_b, flows, area_a, area_b, valid=None, min_overlap=1, min_fraction=0.0, mutate=None):
    """The batch: {"succ", "pred", "best_succ", "best_pred": (N,R) int32, "votes": (N,R,4) int32}."""
    N, R = labels_a.shape[0], area_a.shape[1]
    out = [link_image(labels_a[n], labels_b[n], flows[n], area_a[n], area_b[n], None if valid is None else valid[n], min_overlap,
                      min_fraction, mutate) for n in range(N)]
    if not out:
        return {k: np.zeros((0, R, 4) if k == "votes" else (0, R), np.int32) for k in KEYS}
    return {k: np.stack([o[i] for o in out]) for i, k in enumerate(KEYS)}


def identities(pred, count, R, state=None):
    """ids (S,R) int32, age (S,R) int32, state {"ids", "age", "next_id"}.  pred: (S-1,R), or (S,R) with a state (row 0: the
    link from the state's image)."""
    S = len(count)
    ids, age = np.zeros((S, R), np.int32), np.zeros((S, R), np.int32)
    next_id = 1 if state is None else int(state["next_id"])
    before = None if state is None else (state["ids"], state["age"])
    for s in range(S):
        link = None if before is None else pred[s - 1 if state is None else s]
        for b in range(1, min(int(count[s]), R) + 1):
            p = 0 if link is None else int(link[b - 1])
            if 1 <= p <= R and before[0][p - 1] != 0:
                ids[s, b - 1], age[s, b - 1] = before[0][p - 1], before[1][p - 1] + 1
            else:
                ids[s, b - 1], age[s, b - 1] = next_id, 1
                next_id += 1
        before = (ids[s], age[s])
    return ids, age, {"ids": ids[-1].copy(), "age": age[-1].copy(), "next_id": next_id}


def relabel(labels, ids):
    R = ids.shape[1]
    out = np.zeros_like(labels)
    for s in range(labels.shape[0]):
        lut = np.concatenate([[0], ids[s]]).astype(np.int32)
        ok = (labels[s] >= 1) & (labels[s] <= R)
        out[s] = np.where(ok, lut[np.where(ok, labels[s], 0)], 0)
    return out


def track_regions(labels, count, area, flows, valid=None, state=None, min_overlap=1, min_fraction=0.0, mutate=None):
    """ids, age, links, state: the Python function's contract on numpy arrays (flows: all S, linked with flows[:-1])."""
    R = area.shape[1]
    if state is None:
        la, lb, fa, aa, ab, va = labels[:-1], labels[1:], flows[:-1], area[:-1], area[1:], None if valid is None else valid[:-1]
    else:
        la, lb = np.concatenate([state["labels"][None], labels[:-1]]), labels
        fa = np.concatenate([state["flow"][None], flows[:-1]])
        aa, ab = np.concatenate([state["area"][None], area[:-1]]), area
        va = None
        if valid is not None or state["valid"] is not None:
            head = state["valid"] if state["valid"] is not None else np.ones(labels.shape[1:], np.uint8)
            tail = valid[:-1] if valid is not None else np.ones((labels.shape[0] - 1,) + labels.shape[1:], np.uint8)
            va = np.concatenate([head[None], tail])
    links = link_regions(la, lb, fa, aa, ab, va, min_overlap, min_fraction, mutate)
    ids, age, ident = identities(links["pred"], count, R, state)
    ident.update(labels=labels[-1].copy(), area=area[-1].copy(), flow=flows[-1].copy(), valid=None if valid is None else valid[-1].copy())
    return ids, age, links, ident


# ---------------------------------------------------------------- scenes
def paint(H, W, rects):
    """(labels (H,W) int32, area (R,) int64-free list): rectangles (x0, y0, x1, y1) inclusive painted with the ids 1, 2, ... in the
    order given (the caller lists them in raster order of their first pixels, as label_regions numbers them)."""
    labels = np.zeros((H, W), np.int32)
    for k, (x0, y0, x1, y1) in enumerate(rects, 1):
        labels[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = k
    return labels


def areas(labels, R):
    """(S,R) int32 pixel counts of the ids 1 .. R, (S,) int32 counts of the distinct ids."""
    area = np.stack([np.bincount(l[(l >= 1) & (l <= R)].astype(np.int64) - 1, minlength=R) for l in labels]).astype(np.int32)
    count = np.asarray([len(np.unique(l[l >= 1])) for l in labels], np.int32)
    return area, count


def constant_flows(labels, moves):
    """(S,H,W,2) float32: every pixel of id k of image s moves by moves[s][k - 1]; the background by (0, 0)."""
    S, H, W = labels.shape
    flows = np.zeros((S, H, W, 2), np.float32)
    for s in range(S):
        for k, (u, v) in enumerate(moves[s], 1):
            flows[s][labels[s] == k] = (u, v)
    return flows


def subpixel_flows(N, H, W, seed, poison=False):
    """(N,H,W,2) float32 in +-3 px: a third exact halves, a third quarters, a third anything; poison: a few NaN, Inf, sentinel."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, size=(N, H, W, 1))
    halves = rng.integers(-6, 7, size=(N, H, W, 2)) * 0.5
    quarters = rng.integers(-12, 13, size=(N, H, W, 2)) * 0.25
    free = rng.uniform(-3.0, 3.0, size=(N, H, W, 2))
    f = np.where(kind == 0, halves, np.where(kind == 1, quarters, free)).astype(np.float32)
    if poison:
        flat = f.reshape(-1, 2)
        pick = rng.permutation(flat.shape[0])
        k = max(1, flat.shape[0] // 17)
        flat[pick[0:k], 0] = np.nan
        flat[pick[k:2 * k], 1] = np.inf
        flat[pick[2 * k:3 * k]] = SENTINEL
        flat[pick[3 * k:4 * k], 0] = -np.inf
    return f


def moving_scene(S, H, W, seed=0):
    """flows (S,H,W,2) float32 of S pairs of a clip: a background that translates by (1.5, -0.75) px with a little noise, and two
    rectangles that move on their own by (8, -6) and (-7, 5) px RELATIVE to it, drifting by their whole motion from pair to pair.
    Returns the flows and the rectangles of every pair [(x0, y0, x1, y1), (..)]."""
    rng = np.random.default_rng(seed)
    flows = np.empty((S, H, W, 2), np.float32)
    rects = []
    bg = np.array([1.5, -0.75])
    own = (np.array([8.0, -6.0]), np.array([-7.0, 5.0]))
    w, h = max(W // 6, 6), max(H // 5, 6)
    start = (np.array([W // 8, H // 2]), np.array([W - W // 8 - w, H // 8]))
    for s in range(S):
        f = np.broadcast_to(bg, (H, W, 2)) + rng.standard_normal((H, W, 2)) * 0.05
        here = []
        for k in range(2):
            x0, y0 = np.rint(start[k] + s * (bg + own[k])).astype(int)
            f[y0:y0 + h, x0:x0 + w] += own[k]
            here.append((int(x0), int(y0), int(x0 + w - 1), int(y0 + h - 1)))
        flows[s] = f.astype(np.float32)
        rects.append(here)
    return flows, rects


# ---------------------------------------------------------------- the named single-pair cases (8 x 16 pixels, R = 20)
CASE_H, CASE_W, CASE_R = 8, 16, 20


def cases():
    """{name: dict(labels_a, labels_b, flow, valid)} of one pair each, all CASE_H x CASE_W with CASE_R table rows; what each is for
    is asserted on the restatement by tests/test_host_region_tracks.py."""
    H, W, R = CASE_H, CASE_W, CASE_R
    zero = np.zeros((H, W, 2), np.float32)
    columns = np.broadcast_to(np.arange(1, W + 1, dtype=np.int32), (H, W)).copy()       # labels_b = x + 1: the vote names the target
    out = {}
    out["split"] = dict(labels_a=paint(H, W, [(2, 2, 11, 5)]), labels_b=paint(H, W, [(2, 2, 7, 5), (9, 2, 11, 5)]), flow=zero, valid=None)
    out["merge"] = dict(labels_a=paint(H, W, [(2, 2, 7, 5), (9, 2, 11, 5)]), labels_b=paint(H, W, [(2, 2, 11, 5)]), flow=zero, valid=None)
    out["row_tie"] = dict(labels_a=paint(H, W, [(2, 2, 5, 3)]), labels_b=paint(H, W, [(2, 2, 3, 3), (4, 2, 5, 3)]), flow=zero, valid=None)
    out["column_tie"] = dict(labels_a=paint(H, W, [(2, 2, 3, 3), (4, 2, 5, 3)]), labels_b=paint(H, W, [(2, 2, 5, 3)]), flow=zero, valid=None)
    halves = np.zeros((H, W, 2), np.float32)
    for y, u in enumerate((0.5, -0.5, 1.5, -1.5)):                                     # row y of region 1 moves by u
        halves[y, :, 0] = u
    la = np.zeros((H, W), np.int32)
    la[0:4, 2:12] = 1
    out["halves"] = dict(labels_a=la, labels_b=columns, flow=halves, valid=None)
    vertical = np.zeros((H, W, 2), np.float32)
    vertical[..., 1] = np.where(np.arange(W) % 2 == 0, 0.5, -1.5)[None, :]
    out["halves_y"] = dict(labels_a=paint(H, W, [(1, 1, 10, 6)]), labels_b=np.broadcast_to(np.arange(1, H + 1, dtype=np.int32)[:, None], (H, W)).copy(),
                           flow=vertical, valid=None)
    leave = np.zeros((H, W, 2), np.float32)
    leave[:, :8, 0] = -3.0                                                              # the left half moves left, the right half right
    leave[:, 8:, 0] = 3.25
    leave[0, :, 1] = -0.75                                                              # the first row up and out
    out["leave"] = dict(labels_a=paint(H, W, [(0, 0, 15, 7)]), labels_b=paint(H, W, [(0, 0, 15, 7)]), flow=leave, valid=None)
    poison = np.zeros((H, W, 2), np.float32)
    poison[1, 1:5, 0] = np.nan
    poison[2, 1:5, 1] = np.inf
    poison[3, 1:5] = SENTINEL
    poison[4, 1:5, 0] = -np.inf
    poison[5, 1:5, 1] = np.float32(1.0e9)                                               # the largest known value: a voter that leaves
    out["poison_open"] = dict(labels_a=paint(H, W, [(0, 0, 7, 7), (9, 0, 14, 7)]), labels_b=paint(H, W, [(0, 0, 7, 7), (9, 0, 14, 7)]),
                              flow=poison, valid=None)
    hidden = np.zeros((H, W, 2), np.float32)
    valid = np.ones((H, W), np.uint8)
    valid[1:5, 1:5] = 0
    hidden[1:5, 1:5] = poison[1:5, 1:5]
    hidden[6, 9:12] = np.nan                                                            # under a label that is no voter's
    lab = paint(H, W, [(0, 0, 7, 7), (9, 0, 14, 5)])
    lab[6, 9:12] = 0
    valid[0, 0] = 7                                                                     # (non-zero, not just 1)
    out["poison_hidden"] = dict(labels_a=lab, labels_b=paint(H, W, [(0, 0, 7, 7), (9, 0, 14, 7)]), flow=hidden, valid=valid)
    beyond_a = paint(H, W, [(0, 0, 3, 3), (5, 0, 8, 3), (10, 0, 13, 3)])
    beyond_a[beyond_a == 2] = R + 1
    beyond_a[4:, :4] = -3
    beyond_a[4:, 4:8] = np.iinfo(np.int32).max
    beyond_b = paint(H, W, [(0, 0, 3, 3), (5, 0, 8, 3), (10, 0, 13, 3)])
    beyond_b[beyond_b == 3] = R + 7
    beyond_b[beyond_b == 1] = R                                                         # the last row of the table
    beyond_b[4:, 8:] = np.iinfo(np.int32).min
    out["beyond"] = dict(labels_a=beyond_a, labels_b=beyond_b, flow=zero, valid=None)
    half = np.ones((H, W), np.uint8)
    half[2:6, 6:9] = 0                                                                  # rectangle 1 (4 x 6) keeps 12 voters, all on b's 1
    out["threshold"] = dict(labels_a=paint(H, W, [(3, 2, 8, 5)]), labels_b=paint(H, W, [(3, 2, 8, 5)]), flow=zero, valid=half)
    below = half.copy()
    below[2, 3] = 0                                                                     # one voter fewer: 11
    out["threshold_below"] = dict(labels_a=paint(H, W, [(3, 2, 8, 5)]), labels_b=paint(H, W, [(3, 2, 8, 5)]), flow=zero, valid=below)
    return out


def case_batch(names=None):
    """The cases as ONE batch: labels_a, labels_b (N,H,W) int32, flows (N,H,W,2), area_a, area_b (N,R) int32, valid (N,H,W) uint8."""
    c = cases()
    names = list(c) if names is None else list(names)
    la, lb = np.stack([c[n]["labels_a"] for n in names]), np.stack([c[n]["labels_b"] for n in names])
    flows = np.stack([c[n]["flow"] for n in names])
    valid = np.stack([c[n]["valid"] if c[n]["valid"] is not None else np.ones((CASE_H, CASE_W), np.uint8) for n in names])
    return names, la, lb, flows, areas(la, CASE_R)[0], areas(lb, CASE_R)[0], valid
