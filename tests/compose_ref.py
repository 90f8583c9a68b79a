"""Float64 restatement of flow composition (pwcnet_amd.compose, csrc/pwc_compose.hip) in numpy: the forward, the validity mask,
both gradients, and K_t, the number of contributions a flow_bc cell receives.  Checked on the CPU by tests/test_host_compose.py
(against torch.autograd on a float64 torch statement of the same formula); the GPU tests compare the kernels against it.

    f = flow_ab[p], q = (x + f0, y + f1); x0 = floor(qx), x1 = min(x0 + 1, W - 1), wx = qx - x0, likewise in y
    out[p,k] = f_k + sum over the four corners c of b_c flow_bc[c,k],  b_c = (wx | 1 - wx)(wy | 1 - wy)
    p valid iff valid_ab[p], f known (finite, |.| <= 1e9), q in [0, W - 1] x [0, H - 1], all four corners valid_bc and known

Every array that leaves here is float64 / bool / int64; the inputs are the float32 / uint8 arrays the kernels read."""
import numpy as np

SENTINEL = 1e10
# why a pixel is invalid, the first rule that fails in the order of the definition; 0: valid
VALID, OWN_MASK, SENTINEL_F, OUT_OF_FRAME, MASKED_CORNER, SENTINEL_CORNER = range(6)


def known(a):
    """flow_io.flow_valid's rule per pixel: both components finite with |.| <= 1e9."""
    with np.errstate(invalid="ignore"):
        return (np.isfinite(a) & (np.abs(a) <= 1e9)).all(axis=-1)


class Geometry:
    """Where every pixel samples and whether it is valid: the constants of a composition (no gradient passes through them)."""

    def __init__(self, ab, bc, vab=None, vbc=None):
        ab, bc = np.asarray(ab), np.asarray(bc)
        assert ab.dtype == np.float32 and bc.dtype == np.float32 and ab.shape == bc.shape and ab.shape[3] == 2
        N, H, W, _ = ab.shape
        self.shape = (N, H, W)
        own = np.ones((N, H, W), bool) if vab is None else np.asarray(vab) != 0
        f_ok = own & known(ab)
        self.f = np.where(f_ok[..., None], ab.astype(np.float64), 0.0)         # a pixel ruled out reads no flow
        qx = np.arange(W, dtype=np.float64)[None, None, :] + self.f[..., 0]
        qy = np.arange(H, dtype=np.float64)[None, :, None] + self.f[..., 1]
        inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
        qx, qy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)
        fx0, fy0 = np.floor(qx), np.floor(qy)
        self.x0, self.y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        self.x1, self.y1 = np.minimum(self.x0 + 1, W - 1), np.minimum(self.y0 + 1, H - 1)
        self.wx, self.wy = qx - fx0, qy - fy0
        self.n = np.broadcast_to(np.arange(N)[:, None, None], (N, H, W))
        bmask = np.ones((N, H, W), bool) if vbc is None else np.asarray(vbc) != 0
        bknown = known(bc)
        cm = np.ones((N, H, W), bool)
        ck = np.ones((N, H, W), bool)
        for cy, cx, _ in self.corners():
            cm &= bmask[self.n, cy, cx]
            ck &= bknown[self.n, cy, cx]
        self.reason = np.where(~own, OWN_MASK, np.where(~f_ok, SENTINEL_F, np.where(~inside, OUT_OF_FRAME, np.where(
            ~cm, MASKED_CORNER, np.where(~ck, SENTINEL_CORNER, VALID)))))
        self.valid = self.reason == VALID
        self.B = np.where(bknown[..., None], bc.astype(np.float64), 0.0)       # only known corners are ever used

    def corners(self):
        """(row, column, weight) of the four corners, each (N,H,W)."""
        wx, wy = self.wx, self.wy
        return ((self.y0, self.x0, (1 - wy) * (1 - wx)), (self.y0, self.x1, (1 - wy) * wx),
                (self.y1, self.x0, wy * (1 - wx)), (self.y1, self.x1, wy * wx))

    def at(self, cy, cx):
        return self.B[self.n, cy, cx]                                          # (N,H,W,2)


def compose(ab, bc, vab=None, vbc=None):
    """(out (N,H,W,2) float64 with the sentinel at invalid pixels, valid (N,H,W) bool, A (N,H,W,2), geometry); A = |f_k| + the sum
    of b_c |flow_bc[c,k]|, the magnitude the forward bound is stated in."""
    geo = Geometry(ab, bc, vab, vbc)
    S = np.zeros(geo.shape + (2,))
    A = np.abs(geo.f)
    for cy, cx, b in geo.corners():
        S += b[..., None] * geo.at(cy, cx)
        A = A + b[..., None] * np.abs(geo.at(cy, cx))
    v = geo.valid[..., None]
    return np.where(v, geo.f + S, SENTINEL), geo.valid, np.where(v, A, 0.0), geo


def compose_grad(ab, bc, g, vab=None, vbc=None):
    """The gradient of the sum over the valid p and k of g[p,k] out[p,k]:
    dict(dab, dab_mag (A': the sum of the magnitudes of dab's exact terms), dbc, K (N,H,W) the number of contributions per
    flow_bc cell, m (N,) the largest |g| over the valid pixels of each image, valid)."""
    geo = Geometry(ab, bc, vab, vbc)
    N, H, W = geo.shape
    v = geo.valid[..., None]
    gz = np.where(v, np.asarray(g).astype(np.float64), 0.0)                    # g at an invalid pixel is not read
    B00, B01, B10, B11 = (geo.at(cy, cx) for cy, cx, _ in geo.corners())
    wx, wy = geo.wx[..., None], geo.wy[..., None]
    sx = (1 - wy) * (B01 - B00) + wy * (B11 - B10)                             # dS_k/dqx; 0 where the clamp made x1 = x0
    sy = (1 - wx) * (B10 - B00) + wx * (B11 - B01)
    sx_mag = (1 - wy) * (np.abs(B01) + np.abs(B00)) + wy * (np.abs(B11) + np.abs(B10))
    sy_mag = (1 - wx) * (np.abs(B10) + np.abs(B00)) + wx * (np.abs(B11) + np.abs(B01))
    dab = gz + np.stack([(gz * sx).sum(-1), (gz * sy).sum(-1)], axis=-1)
    mag = np.abs(gz) + np.stack([(np.abs(gz) * sx_mag).sum(-1), (np.abs(gz) * sy_mag).sum(-1)], axis=-1)
    dbc = np.zeros((N, H, W, 2))
    K = np.zeros((N, H, W), np.int64)
    for cy, cx, b in geo.corners():
        for k in range(2):
            np.add.at(dbc[..., k], (geo.n, cy, cx), np.where(geo.valid, b * gz[..., k], 0.0))
        np.add.at(K, (geo.n, cy, cx), geo.valid.astype(np.int64))
    with np.errstate(invalid="ignore"):
        m = np.abs(gz).reshape(N, -1).max(axis=1)
    return dict(dab=np.where(v, dab, 0.0), dab_mag=np.where(v, mag, 0.0), dbc=dbc, K=K, m=m, valid=geo.valid)


def chain(flows, valids=None):
    """The left fold of compose over float32 arrays, each step rounded to float32 as the kernel stores it; (flow, valid)."""
    valids = [None] * len(flows) if valids is None else valids
    acc, mask = np.asarray(flows[0]), valids[0]
    for f, v in zip(flows[1:], valids[1:]):
        out, mask, _, _ = compose(acc, np.asarray(f), mask, v)
        acc = out.astype(np.float32)
    return acc, mask


# ------------------------------------------------------------------ cases
MODES = ("none", "ab", "bc", "both")


def masks_of(mode, vab, vbc):
    return (vab if mode in ("ab", "both") else None, vbc if mode in ("bc", "both") else None)


def random_case(N, H, W, seed, integer=False):
    """(flow_ab, flow_bc, valid_ab, valid_bc, g): float32 / uint8 numpy arrays, seeded.  Displacements within +-1.5 pixels (0 along
    an axis of one pixel, where anything else leaves the frame), one pixel in twenty thrown far out of the frame; sentinels,
    NaN and Inf in both flows; masks of about 85 % and 95 % ones.  integer: flow_ab rounded to whole pixels (every weight 0 or
    1), and the LAST image all unknown (the sentinel in every flow_ab pixel).  A single pixel (H W = 1) is all or nothing: it is
    left valid, it checks the clamped geometry and not the masks.
    Asserted here, on the restatement alone, for images of 35 pixels or more: in every masked case 10 % to 90 % of each
    image's pixels are valid (but for the image made unknown on purpose), and every branch of the validity rule is taken."""
    rs = np.random.RandomState(seed)
    ab = rs.uniform(-1.5, 1.5, size=(N, H, W, 2))
    if integer:
        ab = np.round(ab)
    if W == 1:
        ab[..., 0] = 0.0
    if H == 1:
        ab[..., 1] = 0.0
    bc = rs.uniform(-3.0, 3.0, size=(N, H, W, 2))
    vab = (rs.uniform(size=(N, H, W)) < 0.85).astype(np.uint8)
    vbc = (rs.uniform(size=(N, H, W)) < 0.95).astype(np.uint8)
    g = rs.uniform(-1.0, 1.0, size=(N, H, W, 2))
    if H * W > 1:
        far = rs.uniform(size=(N, H, W)) < 0.05
        ab[..., 0] = np.where(far, ab[..., 0] + 2.0 * W, ab[..., 0])
        pick = rs.uniform(size=(N, H, W))
        ab[pick < 0.02] = SENTINEL
        ab[(pick >= 0.02) & (pick < 0.04), 1] = np.nan
        ab[(pick >= 0.04) & (pick < 0.06), 0] = -np.inf
        pick = rs.uniform(size=(N, H, W))
        bc[pick < 0.01] = SENTINEL
        bc[(pick >= 0.01) & (pick < 0.02), 0] = np.nan
        bc[(pick >= 0.02) & (pick < 0.03), 1] = np.inf
        if integer:
            ab[N - 1] = SENTINEL
    else:
        vab[:], vbc[:] = 1, 1
    ab, bc, g = ab.astype(np.float32), bc.astype(np.float32), g.astype(np.float32)
    if H * W >= 35:
        seen = set()
        for mode in MODES:
            geo = Geometry(ab, bc, *masks_of(mode, vab, vbc))
            seen |= set(np.unique(geo.reason).tolist())
            if mode == "none":
                continue
            share = geo.valid.reshape(N, -1).mean(axis=1)[:N - 1 if integer else N]
            assert ((share >= 0.1) & (share <= 0.9)).all(), (N, H, W, seed, mode, share)
        assert seen == {VALID, OWN_MASK, SENTINEL_F, OUT_OF_FRAME, MASKED_CORNER, SENTINEL_CORNER}, (N, H, W, seed, seen)
    return ab, bc, vab, vbc, g
