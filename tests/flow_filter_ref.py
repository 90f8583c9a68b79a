"""The flow filter of include/pwc_hip.h ("flow filter") restated in plain numpy: a loop over the pixels, the
candidates of each gathered from the part of its window inside the frame, the weighted median read off the cumulative sum of the
weights taken in sorted key order.  The GPU tests hold pwc_flow_filter_f32 to these bits; tests/test_host_flow_filter.py holds
this file to a second route, to np.median and to hand-worked cases.

`mutate` deliberately breaks one rule (None: the definition) so that the host tests can show which cases each rule decides:
    "strict"     sums the weights of the keys BELOW K instead of up to K in the cumulative rule
    "upper"      the upper weighted median (the smallest K whose cumulative weight EXCEEDS T / 2)
    "replicate"  the window is clamped to the border (edge pixels repeated) instead of cut by it
"""
import numpy as np

SENTINEL = np.float32(1e10)


def keys(x):
    """The total order of the definition: float32 (any shape) -> uint32 keys, -0 < +0."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.asarray(k, np.uint32)
    b = np.where(k >> np.uint32(31), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return b.view(np.float32)


def known(flows, valid=None):
    """Known(q): the valid byte is non-zero and both components are finite and at most 1e9 in magnitude."""
    f = np.asarray(flows, np.float32)
    with np.errstate(invalid="ignore"):
        k = (np.abs(f[..., 0]) <= np.float32(1e9)) & (np.abs(f[..., 1]) <= np.float32(1e9))
    if valid is not None:
        k &= np.asarray(valid).astype(np.uint8) != 0
    return k


def guide_bytes(guide):
    """(N,H,W,C) uint8 or float32 -> int64 bytes: rint(clamp((double)v * 255, 0, 255)), ties to even, a NaN is 0."""
    g = np.asarray(guide)
    if g.dtype == np.uint8:
        return g.astype(np.int64)
    assert g.dtype == np.float32, g.dtype
    t = g.astype(np.float64) * 255.0
    t = np.where(np.isnan(t), 0.0, t)
    return np.rint(np.clip(t, 0.0, 255.0)).astype(np.int64)


def weighted_median(vals, w, mutate=None):
    """The lower weighted median of float32 `vals` under integer weights `w` (all > 0, at least one): the value with the
    smallest key K such that 2 * (sum of the weights of the keys <= K) >= T."""
    k = keys(vals)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    T = int(sum(int(x) for x in w))
    cum = 0
    sums = []
    for i in order:                      # the sum in sorted order, Python integers: exact
        cum += int(w[i])
        sums.append(cum)
    for j in range(len(ks)):
        last = j + 1 == len(ks) or ks[j + 1] != ks[j]          # the sum over ALL the keys <= K: the last of a run of equal keys
        if not last:
            continue
        if mutate == "strict":
            first = j
            while first > 0 and ks[first - 1] == ks[j]:
                first -= 1
            s = sums[first - 1] if first > 0 else 0
            hit = 2 * s >= T
        elif mutate == "upper":
            hit = 2 * sums[j] > T
        else:
            hit = 2 * sums[j] >= T
        if hit:
            return vals[order[j]]
    return vals[order[-1]]               # (only a mutation gets here)


def filter_pass(flows, valid, guide, radius, space_table, color_table, smooth, fill, min_count, mutate=None):
    """One pass over a batch: flows (N,H,W,>=2) float32, valid (N,H,W) or None, guide bytes (N,H,W,C) int64 or None ->
    (out (N,H,W,2) float32, out_valid (N,H,W) uint8)."""
    f = np.asarray(flows, np.float32)
    N, H, W = f.shape[:3]
    r = int(radius)
    D = 2 * r + 1
    space = [int(x) for x in np.asarray(space_table).reshape(-1)]
    assert len(space) == D * D
    color = None if guide is None else [int(x) for x in np.asarray(color_table).reshape(-1)]
    kn = known(f, valid)
    out = np.empty((N, H, W, 2), np.float32)
    out_valid = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        kl = kn[n].tolist()                                    # (Python lists and integers: the pixel loop reads nothing else)
        gl = None if guide is None else guide[n].tolist()
        flat = f[n].reshape(H * W, -1)
        for y in range(H):
            for x in range(W):
                idx, ws = [], []
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        qy, qx = y + dy, x + dx
                        if mutate == "replicate":
                            qy, qx = min(max(qy, 0), H - 1), min(max(qx, 0), W - 1)
                        if not (0 <= qy < H and 0 <= qx < W) or not kl[qy][qx]:
                            continue
                        wq = space[(dy + r) * D + (dx + r)]
                        if gl is not None:
                            wq *= color[sum(abs(a - b) for a, b in zip(gl[qy][qx], gl[y][x]))]
                        if wq > 0:
                            idx.append(qy * W + qx)
                            ws.append(wq)
                vals_u, vals_v = flat[idx, 0], flat[idx, 1]
                cnt = len(ws)
                if kn[n, y, x]:
                    take = bool(smooth) and cnt >= 1
                    ok = True
                else:
                    take = bool(fill) and cnt >= min_count
                    ok = take
                if take:
                    out[n, y, x, 0] = weighted_median(vals_u, ws, mutate)
                    out[n, y, x, 1] = weighted_median(vals_v, ws, mutate)
                elif ok:
                    out[n, y, x] = f[n, y, x, :2]
                else:
                    out[n, y, x] = SENTINEL
                out_valid[n, y, x] = 1 if ok else 0
    return out, out_valid


def filter_flow_ref(flows, guide=None, valid=None, radius=2, space_table=None, color_table=None, smooth=True, fill=False,
                    min_count=1, iters=1, mutate=None):
    """The whole call: `iters` passes, each on the flow and the mask of the one before; guide and tables stay."""
    assert smooth or fill
    assert min_count >= 1 and iters >= 1 and 1 <= radius <= 7
    g = None if guide is None else guide_bytes(guide)
    f, v = np.asarray(flows, np.float32), valid
    for _ in range(iters):
        f, v = filter_pass(f, v, g, radius, space_table, color_table, smooth, fill, min_count, mutate)
    return f, v
