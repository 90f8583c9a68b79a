"""numpy restatement of the DEFINITION of include/pwc_hip.h, "moving regions" -- not of the kernels' route: a host union-find over
the pixels in raster order, then roots, areas, ids, boxes, int64 sums and means exactly as the header states them.
tests/test_host_regions.py checks it on the CPU against scipy.ndimage.label and direct computations; tests/test_gpu_regions.py
holds the kernels to it bit for bit.  Also the patterns and seeded inputs both share.

`mutate` switches on one deliberate fault at a time, for the host tests that show the shared inputs tell it apart:
    "no_antidiagonal"  connectivity 8 without the pair (x, y) -- (x + 1, y - 1)
    "by_area"          ids numbered by descending area instead of by root
"""
import numpy as np

SENTINEL = np.float32(1e10)


def foreground(mask, invert=False, flows=None):
    """(N,H,W) bool: the mask byte (inverted: its absence) and, where flows is given, flow_io.flow_valid's rule."""
    fg = (np.asarray(mask) == 0) if invert else (np.asarray(mask) != 0)
    if flows is not None:
        with np.errstate(invalid="ignore"):
            fg = fg & (np.abs(flows[..., 0]) <= np.float32(1e9)) & (np.abs(flows[..., 1]) <= np.float32(1e9))
    return fg


def roots_of(fg, connectivity, mutate=None):
    """(H,W) int64: the smallest linear index of every foreground pixel's component, -1 for background.  A union-find over
    the pixels in raster order; the larger root is always hung under the smaller, so a root is its component's minimum."""
    H, W = fg.shape
    flat = fg.reshape(-1).tolist()
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def union(i, j):
        i, j = find(i), find(j)
        if i < j:
            parent[j] = i
        elif j < i:
            parent[i] = j

    for y in range(H):
        row = y * W
        for x in range(W):
            i = row + x
            if not flat[i]:
                continue
            if x > 0 and flat[i - 1]:
                union(i, i - 1)
            if y > 0:
                if flat[i - W]:
                    union(i, i - W)
                if connectivity == 8:
                    if x > 0 and flat[i - W - 1]:
                        union(i, i - W - 1)
                    if x < W - 1 and flat[i - W + 1] and mutate != "no_antidiagonal":
                        union(i, i - W + 1)
    out = np.full(H * W, -1, np.int64)
    for i in range(H * W):
        if flat[i]:
            out[i] = find(i)
    return out.reshape(H, W)


def fixed(u):
    """q = (int64) rint(clamp(u, -65536, 65536) * 65536.0) of float32 values; a NaN (never a foreground pixel's) gives 0."""
    u = np.asarray(u, np.float32).astype(np.float64)
    return np.rint(np.clip(np.where(np.isnan(u), 0.0, u), -65536.0, 65536.0) * 65536.0).astype(np.int64)


def label_image(fg, connectivity, min_area, max_regions, flow=None, mutate=None):
    """One image: labels (H,W) int32, K, area (R,) int32, box (R,4) int32, sums (R,2) int64 or None, mean (R,2) float64 or None."""
    H, W = fg.shape
    R = max_regions
    root = roots_of(fg, connectivity, mutate).reshape(-1)
    ids, areas = np.unique(root[root >= 0], return_counts=True)          # ascending root
    kept = areas >= min_area
    ids, areas = ids[kept], areas[kept]
    if mutate == "by_area":
        order = np.argsort(-areas, kind="stable")
        ids, areas = ids[order], areas[order]
    K = len(ids)
    lut = np.zeros(H * W + 1, np.int32)                                  # (index -1, background, reads the last entry: 0)
    lut[ids] = np.arange(1, K + 1, dtype=np.int32)
    labels = lut[root]
    area, box = np.zeros(R, np.int32), np.zeros((R, 4), np.int32)
    sums = mean = None
    if flow is not None:
        sums, mean = np.zeros((R, 2), np.int64), np.zeros((R, 2), np.float64)
        q = fixed(flow[..., :2]).reshape(-1, 2)
    ys, xs = np.divmod(np.arange(H * W), W)
    rows = min(K, R)
    sel = (labels >= 1) & (labels <= rows)
    lab = labels[sel].astype(np.int64) - 1
    if rows:
        area[:rows] = np.bincount(lab, minlength=rows)
        x0, y0 = np.full(rows, W, np.int64), np.full(rows, H, np.int64)
        x1, y1 = np.full(rows, -1, np.int64), np.full(rows, -1, np.int64)
        np.minimum.at(x0, lab, xs[sel]); np.minimum.at(y0, lab, ys[sel])
        np.maximum.at(x1, lab, xs[sel]); np.maximum.at(y1, lab, ys[sel])
        box[:rows] = np.stack([x0, y0, x1, y1], axis=1)
        if flow is not None:
            np.add.at(sums[:, 0], lab, q[sel, 0])
            np.add.at(sums[:, 1], lab, q[sel, 1])
            mean[:rows] = (sums[:rows].astype(np.float64) / np.float64(65536.0)) / area[:rows].astype(np.float64)[:, None]
    return labels.reshape(H, W), K, area, box, sums, mean


def label_regions(mask, connectivity=8, min_area=1, max_regions=256, flows=None, invert=False, mutate=None):
    """The batch: labels (N,H,W) int32, count (N,) int32, area (N,R), box (N,R,4), sums (N,R,2) or None, mean (N,R,2) or None."""
    fg = foreground(mask, invert, flows)
    out = [label_image(fg[n], connectivity, min_area, max_regions, None if flows is None else flows[n], mutate)
           for n in range(fg.shape[0])]
    stack = lambda k: None if out[0][k] is None else np.stack([o[k] for o in out])
    return stack(0), np.asarray([o[1] for o in out], np.int32), stack(2), stack(3), stack(4), stack(5)


# ---------------------------------------------------------------- patterns
def serpentine(H, W):
    """Full rows at every other row, joined alternately at the right and the left end: ONE component (either connectivity)
    that crosses every vertical seam in every other row and starts at pixel 0."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def u_shape(H, W):
    """Two arms in the first and the last column that meet only in the last row: ONE component whose root is pixel 0."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0] = 1
    m[:, W - 1] = 1
    m[H - 1] = 1
    return m


def spiral(H, W):
    """A one-pixel path that winds inwards from pixel 0 and keeps a gap of one pixel to its earlier turns: ONE component."""
    m = np.zeros((H, W), np.uint8)
    inside = lambda x, y: 0 <= x < W and 0 <= y < H
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        nx, ny = x + dx, y + dy
        if inside(nx, ny) and not m[ny, nx] and not (inside(nx + dx, ny + dy) and m[ny + dy, nx + dx]):
            x, y, turns = nx, ny, 0
            m[y, x] = 1
        else:
            dx, dy, turns = -dy, dx, turns + 1
    return m


def patterns(H, W, th, tw):
    """{name: (H,W) uint8 mask}: the cases of the issue, at any shape.  The diagonals repeat every th + tw pixels; with a
    square tile the main ones pass through the tile corners (k th, k tw) by the pair (k tw - 1, k th - 1) -- (k tw, k th) and
    the anti-diagonals through the corner (th, tw) by the pair (tw - 1, th) -- (tw, th - 1), and so on along them."""
    y, x = np.mgrid[0:H, 0:W]
    out = {}
    out["background"] = np.zeros((H, W), np.uint8)
    out["foreground"] = np.ones((H, W), np.uint8)
    c = np.zeros((H, W), np.uint8)
    c[0, 0] = c[0, W - 1] = c[H - 1, 0] = c[H - 1, W - 1] = 1
    out["corners"] = c
    out["checkerboard"] = ((x + y) % 2 == 0).astype(np.uint8)
    out["diagonal"] = ((x - y) % (th + tw) == 0).astype(np.uint8)
    out["antidiagonal"] = ((x + y) % (th + tw) == th + tw - 1).astype(np.uint8)
    out["serpentine"] = serpentine(H, W)
    out["spiral"] = spiral(H, W)
    out["u"] = u_shape(H, W)
    for p in (0.4, 0.6):
        rng = np.random.default_rng(1000 + int(p * 10) + 7 * H + W)
        out[f"bernoulli{p}"] = (rng.random((H, W)) < p).astype(np.uint8)
    return out


def seeded_flows(N, H, W, seed, cs=2, offset=0):
    """(N,H,W,cs) float32 whose channels offset, offset + 1 are a flow with a few NaN, Inf, sentinel values and magnitudes
    beyond 65536 (the clamp); the other channels hold a value that would show if it were read."""
    rng = np.random.default_rng(seed)
    buf = np.full((N, H, W, cs), np.float32(-7.5e8), np.float32)
    f = (rng.standard_normal((N, H, W, 2)) * 4.0).astype(np.float32)
    flat = f.reshape(-1, 2)
    n = flat.shape[0]
    pick = rng.permutation(n)
    k = max(1, n // 23)
    flat[pick[0 * k:1 * k], 0] = np.nan
    flat[pick[1 * k:2 * k], 1] = np.inf
    flat[pick[2 * k:3 * k]] = SENTINEL
    flat[pick[3 * k:4 * k], 0] = np.float32(70000.25)
    flat[pick[4 * k:5 * k], 1] = np.float32(-1.0e6)
    flat[pick[5 * k:6 * k], 0] = np.float32(65536.0)
    buf[..., offset:offset + 2] = f
    return buf


def rectangle_scene(N, H, W, seed=0):
    """tests/test_gpu_motion.py's kind of scene: an affine camera flow with a little noise, a rectangle moved by (8, -6) px
    on top of it.  Returns flows (N,H,W,2) float32 and the rectangle (x0, y0, x1, y1) inclusive."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    flows = np.empty((N, H, W, 2), np.float32)
    x0, y0, x1, y1 = W // 4, H // 3, W // 4 + max(W // 5, 5), H // 3 + max(H // 5, 5)
    for n in range(N):
        u = 1.5 + 0.01 * (x - W / 2) - 0.004 * (y - H / 2)
        v = -0.75 + 0.003 * (x - W / 2) + 0.008 * (y - H / 2)
        u[y0:y1 + 1, x0:x1 + 1] += 8.0
        v[y0:y1 + 1, x0:x1 + 1] += -6.0
        noise = rng.standard_normal((H, W, 2)) * 0.05
        flows[n, ..., 0] = (u + noise[..., 0]).astype(np.float32)
        flows[n, ..., 1] = (v + noise[..., 1]).astype(np.float32)
    return flows, (x0, y0, x1, y1)
