"""Helpers of the batch-seam tests (tests/test_gpu_batch_seams.py on the GPU, tests/test_host_batch_seams.py for the float64
references and for the helpers themselves).  Not a test file.

The property: an image's outputs depend on that image's inputs alone, bit for bit.  A SUBJECT image `s` is put in the middle of
a batch of N = 3 -- a seam on both sides -- with three kinds of neighbours (NEIGHBOURS):

  random   independent random data,
  copies   copies of the subject,
  poison   every float input NaN, every mask all-true, every upstream gradient 0; flows are the exception, because a flow steers
           a gather or a scatter: the neighbours get large FINITE flows that point at the subject's rows (+-H, +-2H px in y), so a
           kernel that clamps against the strip of N * H rows instead of the image reads or writes the subject.

An op is a function `f(inputs) -> outputs` on dicts of numpy arrays whose first axis is the image; the GPU module wraps the HIP
entry points that way, the host module the float64 restatements.  Every input has a ROLE that says how its neighbours are made.

  check_isolation(f, subject, roles)            point 1: f(batch)[1] is the same bits for the three kinds of neighbours
  check_batch_equals_single(f, subject, out)    point 2: ... and the bits of f(subject alone)[0]
  check_neighbours_zero / check_untouched       the gradient rules: nothing is written into a neighbour that has no upstream

The comparisons are on the raw bits (a NaN equals the same NaN, -0.0 differs from 0.0)."""
import numpy as np

N_BATCH, SUBJECT = 3, 1
NEIGHBOURS = ("random", "copies", "poison")

# roles of an input
FLOAT = "float"            # values: random / copy / NaN
FINITE = "finite"          # values of an op whose documented contract turns ONE non-finite contribution into a NaN of the whole
#                            call (the fixed-point accumulators' poison word): random / copy / large finite numbers
FLOW = "flow"              # (.., H, W, 2) px: random / copy / +-H, +-2H px in y
FLOW10 = "flow10"          # a flow that is only looked at (visualisation): random neighbours ten times larger / copy / the
#                            same +-H, +-2H px as FLOW (for H = 1 those are SMALLER than the subject's radius: there only the
#                            random kind makes the point about the per-image maximum)
MASK = "mask"              # bool: random / copy / all true
UPSTREAM = "upstream"      # the gradient that reaches a per-image or per-pixel output: random / copy / 0
SHARED = "shared"          # not per image (weights, parameters): passed through


def bits(a):
    """The raw bits of an array as unsigned integers of the same width (bool: the bytes)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a.view(np.uint8)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def assert_same_bits(a, b, what):
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype}{a.shape} against {b.dtype}{b.shape}"
    diff = bits(a) != bits(b)
    if diff.any():
        at = tuple(int(i) for i in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits, first at {at}: "
                             f"{a[at]!r} against {b[at]!r}")


def neighbour(role, s, kind, rng, side):
    """A neighbour of subject input `s` (leading axis 1) for `role`; side: -1 the image before, +1 the one after."""
    if kind == "copies":
        return s.copy()
    if role in (FLOW, FLOW10):
        if kind == "random":
            return rng.normal(0.0, 2.0 if role == FLOW else 10.0 * float(np.abs(s).max()), size=s.shape).astype(s.dtype)
        H = s.shape[-3]
        out = rng.uniform(-0.4, 0.4, size=s.shape).astype(s.dtype)            # poison: towards the subject, by H and by 2 H
        rows = np.arange(H).reshape(H, 1) + np.zeros(s.shape[-3:-1], dtype=np.int64)
        out[..., 1] += np.where(rows % 2 == 0, -side * H, -side * 2 * H).astype(s.dtype)
        return out
    if role == MASK:
        return (rng.uniform(size=s.shape) < 0.6).astype(s.dtype) if kind == "random" else np.ones_like(s)
    if role == UPSTREAM:
        return rng.uniform(-1.0, 1.0, size=s.shape).astype(s.dtype) if kind == "random" else np.zeros_like(s)
    if role in (FLOAT, FINITE):
        if kind == "random":
            if s.dtype == np.uint8:
                return rng.randint(0, 256, size=s.shape).astype(np.uint8)
            return rng.uniform(-1.0, 1.0, size=s.shape).astype(s.dtype)
        if s.dtype == np.uint8:
            return np.full_like(s, 255)
        return np.full_like(s, np.nan if role == FLOAT else 1.0e3)
    raise ValueError(role)


def batch_of(subject, roles, kind, seed=0):
    """The batch of three: the subject's inputs in the middle, `kind` neighbours on both sides."""
    rng = np.random.RandomState(1000 + seed)
    out = {}
    for name, s in subject.items():
        if s is None or roles[name] == SHARED:
            out[name] = s
            continue
        assert s.shape[0] == 1, (name, s.shape)
        out[name] = np.concatenate([neighbour(roles[name], s, kind, rng, -1), s, neighbour(roles[name], s, kind, rng, +1)], axis=0)
    return out


def check_isolation(f, subject, roles, seed=0, what=""):
    """Point 1.  Returns the outputs of the three batches (kind -> dict)."""
    outs = {kind: f(batch_of(subject, roles, kind, seed)) for kind in NEIGHBOURS}
    base = outs[NEIGHBOURS[0]]
    for kind in NEIGHBOURS[1:]:
        assert outs[kind].keys() == base.keys()
        for key, v in base.items():
            assert v.shape[0] == N_BATCH, (what, key, v.shape)
            assert_same_bits(outs[kind][key][SUBJECT], v[SUBJECT], f"{what} isolation: {key} of the subject, {kind} against "
                                                                  f"{NEIGHBOURS[0]} neighbours")
    return outs


def check_batch_equals_single(f, subject, batch_out, what="", second_class=()):
    """Point 2: the subject's outputs in a batch are the bits of the subject run alone.  Keys in `second_class` (a per-image sum
    whose partition depends on the launch size) are left to the caller's float64 rule.  Returns the single's outputs."""
    single = f(dict(subject))
    assert single.keys() == batch_out.keys()
    for key, v in single.items():
        assert v.shape[0] == 1, (what, key, v.shape)
        if key not in second_class:
            assert_same_bits(batch_out[key][SUBJECT], v[0], f"{what} batch against single: {key}")
    return single


def check_neighbours_zero(grad, what=""):
    """A gradient whose upstream is non-zero for the subject only: the neighbours' part is exact zeros (of either sign: adding
    -0.0 changes no bit of what it is accumulated onto; a NaN is not a zero)."""
    for n in range(N_BATCH):
        if n != SUBJECT:
            nz = ~(np.asarray(grad[n]) == 0)
            assert not nz.any(), f"{what}: image {n} has no upstream but {int(nz.sum())} non-zero elements of its gradient"


def quiet_batch(subject, roles, seed=0):
    """Random finite neighbours whose upstream gradients are 0: what check_neighbours_zero and check_untouched are run on."""
    batch = batch_of(subject, roles, "random", seed)
    for name, role in roles.items():
        if role == UPSTREAM and batch[name] is not None:
            batch[name][[n for n in range(N_BATCH) if n != SUBJECT]] = 0
    return batch


def check_untouched(after, before, what=""):
    """accumulate=True with an upstream for the subject only: the neighbours' part is bitwise what was there before."""
    for n in range(N_BATCH):
        if n != SUBJECT:
            assert_same_bits(after[n], before[n], f"{what}: accumulate onto image {n}, which has no upstream")


def check_close(got, ref, rel, what=""):
    """max |got - ref| <= rel * max |ref| (tests/test_gpu_grad.py `close`, on numpy); returns the relative error."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-30)
    err = float(np.abs(got - ref).max()) / scale if ref.size else 0.0
    assert np.isfinite(got).all() and err <= rel, f"{what}: relative error {err:.3e} above {rel:.1e}"
    return err


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30) if ref.size else 0.0


# ------------------------------------------------------------------ subjects
# Shapes that put a seam inside blocks, waves and windows: 5 x 7 (one 256-lane block covers all three images), 9 x 13 (an image
# ends mid-wave: 117 = 64 + 53), H in {1, 2, 3} (below the windows of census, SSIM and the second differences), H = 4 and 8 (one row
# above SSIM's 3 x 3 and census' 7 x 7 window: the smallest images in which those terms keep pixels); no H * W is a multiple of
# 64, no W a multiple of 4.
SHAPES = ((5, 7), (9, 13), (1, 9), (2, 9), (3, 9), (4, 9), (8, 9))


def subject_flow(H, W, seed, max_off=2):
    """(1,H,W,2) float32 px: an integer field, constant on 3 x 3 tiles, of up to max_off px plus a fraction in [0.15, 0.85] -- every
    sample coordinate keeps 0.15 px from the integers (the kinks of floor and the frame's border), near the border some leave.
    H in 2 .. 8: see below (y keeps 0.0375 px from the integers).  H = 1: as the taller ones -- every sample with a y flow
    leaves the one row, the terms that mask such samples are empty and only their zeros and counts are pinned."""
    rs = np.random.RandomState(seed)
    th, tw = -(-H // 3), -(-W // 3)
    off = rs.randint(-max_off, max_off + 1, size=(1, th, tw, 2)).astype(np.float64)
    integer = np.kron(off, np.ones((1, 3, 3, 1)))[:, :H, :W]
    flow = integer + rs.uniform(0.15, 0.85, size=(1, H, W, 2))
    if 2 <= H <= 8:
        # a short image: no integer part and a y fraction scaled to min(1, (H - 1) / 4), so that samples stay inside the H rows and
        # the windowed terms keep pixels (a window clamped against N * H instead of H then changes a number, not a zero)
        flow = flow - integer
        flow[..., 1] *= min(1.0, (H - 1) / 4.0)
    return flow.astype(np.float32)


def subject_image(H, W, C, seed):
    return np.random.RandomState(seed).uniform(0.0, 1.0, size=(1, H, W, C)).astype(np.float32)


def subject_mask(H, W, seed, keep=0.7):
    return np.random.RandomState(seed).uniform(size=(1, H, W)) < keep


def pair_subject(H, W, C=3, seed=0, masked=True):
    """images_0, images_1, flows, valid, dsums of the data terms."""
    sub = {"im0": subject_image(H, W, C, 10 + seed), "im1": subject_image(H, W, C, 20 + seed), "flow": subject_flow(H, W, 30 + seed),
           "valid": subject_mask(H, W, 40 + seed) if masked else None, "dsums": np.array([0.75], np.float32)}
    roles = {"im0": FLOAT, "im1": FLOAT, "flow": FLOW, "valid": MASK, "dsums": UPSTREAM}
    return sub, roles


def fb_subject(H, W, seed=0, masked=True):
    """flows_fw, flows_bw (roughly each other's inverse, so the check keeps a share of the pixels), masks, upstreams."""
    fw = subject_flow(H, W, 50 + seed, max_off=1)
    rs = np.random.RandomState(60 + seed)
    bw = (-fw + rs.uniform(-0.3, 0.3, size=fw.shape)).astype(np.float32)
    sub = {"fw": fw, "bw": bw, "valid_fw": subject_mask(H, W, 70 + seed) if masked else None,
           "valid_bw": subject_mask(H, W, 80 + seed) if masked else None,
           "dsums_fw": np.array([0.75], np.float32), "dsums_bw": np.array([-1.5], np.float32)}
    roles = {"fw": FLOW, "bw": FLOW, "valid_fw": MASK, "valid_bw": MASK, "dsums_fw": UPSTREAM, "dsums_bw": UPSTREAM}
    return sub, roles


# ------------------------------------------------------------------ the float64 references as ops
def _t(a, dt=None):
    import torch
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dt) if dt is not None and t.is_floating_point() else t


def _n(t):
    return t.detach().cpu().numpy()


def _with_grad(run, flow_keys, ups_keys, inp, dt):
    """run(tensors) -> dict of outputs whose `ups_keys` pair with sums; adds d<flow> = the gradient of sum(ups * sums)."""
    import torch
    t = {k: _t(v, dt) for k, v in inp.items()}
    for k in flow_keys:
        t[k] = t[k].clone().requires_grad_(True)
    out = run(t)
    total = sum((t[u] * out[s]).sum() for s, u in ups_keys.items())
    grads = torch.autograd.grad(total, [t[k] for k in flow_keys], allow_unused=True)
    res = {k: _n(v) for k, v in out.items()}
    for k, g in zip(flow_keys, grads):
        res["d" + k] = _n(g if g is not None else torch.zeros_like(t[k]))
    return res


def ref_photometric(inp, dt=None, eps=1e-3, q=0.5):
    import torch
    from tests import unsup_ref as ur
    dt = dt or torch.float64

    def run(t):
        s, c, _ = ur.photometric_ref(t["im0"], t["im1"], t["flow"], 1.0, t["valid"], eps, q)
        return {"sums": s, "counts": c.to(torch.int32)}
    return _with_grad(run, ["flow"], {"sums": "dsums"}, inp, dt)


def ref_smoothness(inp, dt=None, order=1, with_image=True, eps=1e-3, q=0.5, alpha=10.0):
    import torch
    from tests import unflow_ref as uf
    from tests import unsup_ref as ur
    dt = dt or torch.float64
    fn = ur.smoothness_ref if order == 1 else uf.smoothness2_ref

    def run(t):
        return {"sums": fn(t["flow"], t["im0"] if with_image else None, alpha, eps, q)}
    return _with_grad(run, ["flow"], {"sums": "dsums"}, inp, dt)


def ref_census(inp, dt=None, radius=3):
    import torch
    from tests import census_ref as cr
    dt = dt or torch.float64

    def run(t):
        s, c, _ = cr.census_ref(t["im0"], t["im1"], t["flow"], 1.0, t["valid"], radius)
        return {"sums": s, "counts": c.to(torch.int32)}
    return _with_grad(run, ["flow"], {"sums": "dsums"}, inp, dt)


def ref_ssim(inp, dt=None, radius=1):
    import torch
    from tests import ssim_ref as sr
    dt = dt or torch.float64

    def run(t):
        s, c, _ = sr.ssim_ref(t["im0"], t["im1"], t["flow"], 1.0, t["valid"], radius)
        return {"sums": s, "counts": c.to(torch.int32)}
    return _with_grad(run, ["flow"], {"sums": "dsums"}, inp, dt)


def ref_fb_valid(inp, dt=None):
    import torch
    from tests import fb_ref as fr
    a, b = fr.fb_ref(_t(inp["fw"]), _t(inp["bw"]), 1.0, 0.01, 0.5, _t(inp["valid_fw"]), _t(inp["valid_bw"]))
    return {"mask_fw": _n(a.mask), "mask_bw": _n(b.mask), "counts_fw": _n(a.counts.to(torch.int32)),
            "counts_bw": _n(b.counts.to(torch.int32))}


def ref_fb_near_ties(inp):
    from tests import fb_ref as fr
    a, b = fr.fb_ref(_t(inp["fw"]), _t(inp["bw"]), 1.0, 0.01, 0.5, _t(inp["valid_fw"]), _t(inp["valid_bw"]))
    return bool(fr.near_ties(a).any() or fr.near_ties(b).any())


def ref_fb_consistency(inp, dt=None, eps=1e-3, q=0.5):
    import torch
    from tests import unflow_ref as uf
    dt = dt or torch.float64

    def run(t):
        sa, ca, _, sb, cb, _ = uf.fb_consistency_ref(t["fw"], t["bw"], 1.0, t["valid_fw"], t["valid_bw"], eps, q)
        return {"sums_fw": sa, "counts_fw": ca.to(torch.int32), "sums_bw": sb, "counts_bw": cb.to(torch.int32)}
    return _with_grad(run, ["fw", "bw"], {"sums_fw": "dsums_fw", "sums_bw": "dsums_bw"}, inp, dt)


def distill_subject(h, w, seed=0):
    """A student h x w read against a teacher (h + 2) x (w + 3) through the window at (1, 2)."""
    rs = np.random.RandomState(90 + seed)
    H, W = h + 2, w + 3
    sub = {"student": rs.normal(0, 2, (1, h, w, 2)).astype(np.float32), "teacher": rs.normal(0, 2, (1, H, W, 2)).astype(np.float32),
           "teacher_valid": rs.uniform(size=(1, H, W)) < 0.7, "exclude": rs.uniform(size=(1, h, w)) < 0.2,
           "dsums": np.array([0.75], np.float32)}
    # the student and the teacher are compared, neither steers an address: both are poisoned with NaN
    roles = {"student": FLOAT, "teacher": FLOAT, "teacher_valid": MASK, "exclude": MASK, "dsums": UPSTREAM}
    return sub, roles


DISTILL_OFFSET = (1, 2)


def ref_distill(inp, dt=None, eps=1e-3, q=0.5):
    import torch
    from tests import distill_ref as dr
    t = {k: _t(v, torch.float64) for k, v in inp.items()}
    sums, counts = dr.distill_sums(t["student"], t["teacher"], DISTILL_OFFSET, t["teacher_valid"], t["exclude"], eps, q)
    grad = dr.distill_grad(t["student"], t["teacher"], t["dsums"], DISTILL_OFFSET, t["teacher_valid"], t["exclude"], eps, q)
    return {"sums": _n(sums), "counts": _n(counts.to(torch.int32)), "dstudent": _n(grad)}


def compose_subject(H, W, seed=0, masked=True):
    sub = {"ab": subject_flow(H, W, 100 + seed, max_off=1), "bc": subject_flow(H, W, 110 + seed, max_off=1),
           "vab": subject_mask(H, W, 120 + seed, 0.8) if masked else None, "vbc": subject_mask(H, W, 130 + seed, 0.9) if masked else None,
           "g": np.random.RandomState(140 + seed).uniform(-1, 1, (1, H, W, 2)).astype(np.float32)}
    roles = {"ab": FLOW, "bc": FLOW, "vab": MASK, "vbc": MASK, "g": UPSTREAM}
    return sub, roles


def ref_compose(inp, dt=None):
    from tests import compose_ref as cr
    out, valid, A, _ = cr.compose(inp["ab"], inp["bc"], inp["vab"], inp["vbc"])
    gr = cr.compose_grad(inp["ab"], inp["bc"], inp["g"], inp["vab"], inp["vbc"])
    N = out.shape[0]
    # the magnitudes the bounds of tests/test_gpu_compose.py are stated in ride along: A, A', K (contributions per cell), m
    return {"ac": out, "valid": valid, "dab": gr["dab"], "dbc": gr["dbc"], "ac_mag": A, "dab_mag": gr["dab_mag"],
            "K": gr["K"], "m": np.asarray(gr["m"]).reshape(N)}


def splat_subject(H, W, C=3, seed=0):
    rs = np.random.RandomState(150 + seed)
    sub = {"x": rs.uniform(-1, 1, (1, H, W, C)).astype(np.float32), "flow": subject_flow(H, W, 160 + seed),
           "w": rs.uniform(0.5, 1.5, (1, H, W)).astype(np.float32), "valid": subject_mask(H, W, 170 + seed, 0.8),
           "g_out": rs.uniform(-1, 1, (1, H, W, C)).astype(np.float32), "g_cov": rs.uniform(-1, 1, (1, H, W)).astype(np.float32)}
    # FINITE: one non-finite contribution raises the poison word of the whole call (include/pwc_hip.h, forward_splat's docstring)
    roles = {"x": FINITE, "flow": FLOW, "w": FINITE, "valid": MASK, "g_out": UPSTREAM, "g_cov": UPSTREAM}
    return sub, roles


def ref_splat(inp, mode="sum"):
    from tests import splat_ref as sr
    t = {k: _t(v) for k, v in inp.items()}
    out, cov, cnt = sr.splat_ref(t["x"], t["flow"], t["w"], t["valid"], 1.0, mode)
    (dx, dw, df), (adx, adw, adf), _ = sr.splat_grads_ref(t["x"], t["flow"], t["w"], t["valid"], 1.0, mode, t["g_out"], t["g_cov"])
    return {"out": _n(out), "cov": _n(cov), "dx": _n(dx), "dw": _n(dw), "dflow": _n(df), "cnt": _n(cnt), "dx_mag": _n(adx),
            "dw_mag": _n(adw), "dflow_mag": _n(adf)}


# ------------------------------------------------------------------ restatements written for the seam tests, per image
def _per_image(fn, n_out=None):
    """A batched op out of a one-image restatement: every image on its own, the results stacked."""
    def f(inp):
        N = next(v.shape[0] for v in inp.values() if v is not None)
        outs = [fn({k: (None if v is None else v[n:n + 1]) for k, v in inp.items()}) for n in range(N)]
        return {k: np.concatenate([o[k] for o in outs], axis=0) for k in outs[0]}
    return f


def warp_one(x, flow, bilinear):
    """float64: nearest moves by the flow truncated toward zero and clips, bilinear blends the four corners, each clipped on its
    own, with the weights of the unclipped floors (csrc/pwc_common.h, pwc_bilinear_corners)."""
    _, H, W, C = x.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    px, py = xs + flow[0, ..., 0].astype(np.float64), ys + flow[0, ..., 1].astype(np.float64)
    X = x[0].astype(np.float64)
    if not bilinear:
        fx, fy = np.trunc(flow[0, ..., 0]).astype(int), np.trunc(flow[0, ..., 1]).astype(int)
        return X[np.clip(ys.astype(int) + fy, 0, H - 1), np.clip(xs.astype(int) + fx, 0, W - 1)][None]
    x0, y0 = np.floor(px), np.floor(py)
    wx, wy = (px - x0)[..., None], (py - y0)[..., None]

    def at(yy, xx):
        return X[np.clip(yy, 0, H - 1).astype(int), np.clip(xx, 0, W - 1).astype(int)]
    return ((1 - wy) * ((1 - wx) * at(y0, x0) + wx * at(y0, x0 + 1)) + wy * ((1 - wx) * at(y0 + 1, x0) + wx * at(y0 + 1, x0 + 1)))[None]


def ref_warp(bilinear):
    return _per_image(lambda i: {"y": warp_one(i["x"], i["flow"], bilinear)})


def cost_volume_one(f0, f1, R=4, slope=0.1):
    """float64: the mean over channels of f0 times f1 shifted through the (2R+1)^2 window, zero outside, leaky ReLU."""
    _, H, W, _ = f0.shape
    a, b = f0[0].astype(np.float64), np.pad(f1[0].astype(np.float64), ((R, R), (R, R), (0, 0)))
    ref = np.stack([(a * b[dy:dy + H, dx:dx + W]).mean(-1) for dy in range(2 * R + 1) for dx in range(2 * R + 1)], axis=-1)
    return np.where(ref > 0, ref, slope * ref)[None]


ref_cost_volume = _per_image(lambda i: {"cv": cost_volume_one(i["f0"], i["f1"])})


def flow_norm_one(pred, gt, valid, ord, gt_div=20.0, scale=0.5):
    """float64 sum of ||pred - gt[::2, ::2] / gt_div||_ord over the kept pixels (gt / gt_div is the kernel's one float32
    division), its number, and scale times its gradient by pred (0 where the norm is 0 or the pixel is masked)."""
    h, w = pred.shape[1:3]
    d = pred[0].astype(np.float64) - (gt[0, ::2, ::2] / np.float32(gt_div)).astype(np.float64)
    keep = valid[0, ::2, ::2] if valid is not None else np.ones((h, w), bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        if ord == 1:
            term, g = np.abs(d).sum(-1), np.sign(d)
        else:
            term = np.sqrt((d * d).sum(-1))
            g = np.where(term[..., None] > 0, d / term[..., None], 0.0)
    g = np.where(keep[..., None], scale * g, 0.0)
    return {"sums": np.array([term[keep].sum()]), "counts": np.array([keep.sum()], np.int32), "dpred": g[None]}


def ref_flow_norm(ord):
    return _per_image(lambda i: flow_norm_one(i["pred"], i["gt"], i["valid"], ord))


def feature_norm_one(f0, f1):
    """float64: the pair's mean and 1 / sqrt(variance + 1e-16) over both maps, and the two normalised maps."""
    both = np.concatenate([f0.ravel(), f1.ravel()]).astype(np.float64)
    mean = both.mean()
    rstd = 1.0 / np.sqrt(((both - mean) ** 2).mean() + 1e-16)
    return {"y0": (f0.astype(np.float64) - mean) * rstd, "y1": (f1.astype(np.float64) - mean) * rstd, "stats": np.array([[mean, rstd]])}


ref_feature_norm = _per_image(lambda i: feature_norm_one(i["f0"], i["f1"]))


def ref_resize(size):
    """tests/fit_ref.py has the half-pixel resize; the network's is TF's legacy one: oracle/torch_ref.py resize_legacy in float64."""
    def f(inp):
        import torch
        from oracle import torch_ref as tr
        return {"y": tr.resize_legacy(torch.from_numpy(inp["x"]).double(), size).numpy()}
    return f


def ref_pyramids(factors=(4, 2), min_fraction=0.5):
    def f(inp):
        import torch
        from tests import pyramid_ref as pr
        out = {f"frame{k}": v.numpy() for k, v in zip(factors, pr.frame_pyramid_ref(torch.from_numpy(inp["frames"]), factors))}
        masks, counts = pr.mask_pyramid_ref(torch.from_numpy(inp["valid"]), factors, min_fraction)
        out.update({f"mask{k}": v.numpy() for k, v in zip(factors, masks)})
        out.update({f"count{k}": v.numpy() for k, v in zip(factors, counts)})
        return out
    return f


def ref_vis(inp):
    from tests import vis_ref as vr
    return {"radius": vr.max_radius(inp["flow"], inp["valid"]), "color": vr.color(inp["flow"], None, inp["valid"])[0],
            "error": vr.error_color(inp["flow"], inp["gt"], inp["valid"])}


def vis_subject(H, W, masked=True):
    rs = np.random.RandomState(420)
    sub = {"flow": rs.normal(0, 3, (1, H, W, 2)).astype(np.float32), "gt": rs.normal(0, 3, (1, H, W, 2)).astype(np.float32),
           "valid": subject_mask(H, W, 430) if masked else None}
    return sub, {"flow": FLOW10, "gt": FLOW10, "valid": MASK}


def ref_featnorm_module(inp):
    """tests/featnorm_ref.py, the float64 torch restatement that tests/test_gpu_featnorm.py uses."""
    import torch
    from tests import featnorm_ref as fr
    y0, y1 = fr.feature_norm(torch.from_numpy(inp["f0"]).double(), torch.from_numpy(inp["f1"]).double())[:2]
    return {"y0": y0.numpy(), "y1": y1.numpy()}


def chain_subject(H, W):
    sub = {f"f{i}": subject_flow(H, W, 200 + i, max_off=1) for i in range(3)}
    sub.update({f"v{i}": subject_mask(H, W, 210 + i, 0.9) for i in range(3)})
    return sub, {k: (FLOW if k[0] == "f" else MASK) for k in sub}


def ref_chain(inp):
    from tests import compose_ref as cr
    ac, valid = cr.chain([inp[f"f{i}"] for i in range(3)], [inp[f"v{i}"] for i in range(3)])
    return {"ac": np.asarray(ac), "valid": np.asarray(valid)}


FIT_FACTOR = 4


def fit_subject(H, W, dtype="float32"):
    """Frames H x W fitted to the next multiples of FIT_FACTOR, and a flow at that size refitted to H x W.  The flow is
    resampled, it steers nothing: NaN neighbours."""
    rs = np.random.RandomState(700)
    FH, FW = -(-H // FIT_FACTOR) * FIT_FACTOR, -(-W // FIT_FACTOR) * FIT_FACTOR
    frames = rs.randint(0, 256, (1, H, W, 3)).astype(np.uint8) if dtype == "uint8" else rs.uniform(0, 1, (1, H, W, 3)).astype(np.float32)
    return {"frames": frames, "flow": rs.normal(0, 3, (1, FH, FW, 2)).astype(np.float32)}, {"frames": FLOAT, "flow": FLOAT}


def ref_fit(mode, H, W):
    def f(inp):
        from tests import fit_ref as fr
        with np.errstate(invalid="ignore"):
            a, sa = fr.fit_frames(inp["frames"], mode, FIT_FACTOR)
            b, sb = fr.refit_flow(inp["flow"], H, W, mode)
        return {"fitted": a, "refit": b, "fitted_mag": sa, "refit_mag": sb}
    return f


TRACK_POINTS = 24


def track_subject(H, W, with_bw=True):
    """One flow slice of a sequence (and its backward flow and masks) and the query points that step across it.  In the batch
    of three the slices are consecutive frames of ONE sequence, group n of the points starts at frame n, and "image n's
    output" is where group n stands, and in what state, after its first step: a step across slice n reads slice n alone."""
    rs = np.random.RandomState(800)
    fw = subject_flow(H, W, 810, max_off=1)
    sub = {"fw": fw, "bw": (-fw + rs.uniform(-0.3, 0.3, fw.shape)).astype(np.float32) if with_bw else None,
           "vfw": subject_mask(H, W, 820, 0.9), "vbw": subject_mask(H, W, 830, 0.9) if with_bw else None,
           "points": np.stack([rs.uniform(0, W - 1, TRACK_POINTS), rs.uniform(0, H - 1, TRACK_POINTS)], axis=1).astype(np.float32)}
    return sub, {"fw": FLOW, "bw": FLOW, "vfw": MASK, "vbw": MASK, "points": SHARED}


def track_op(track):
    """`track` = track_points or track_ref.track on numpy arrays -> the per-slice op described in track_subject."""
    def f(inp):
        T, P = inp["fw"].shape[0], inp["points"].shape[0]
        pts = np.tile(inp["points"], (T, 1))
        start = np.repeat(np.arange(T, dtype=np.int32), P)
        tracks, status = track(inp["fw"], pts, inp["bw"], start, inp["vfw"], inp["vbw"])
        sel = [slice(n * P, (n + 1) * P) for n in range(T)]
        return {"to": np.stack([tracks[n + 1, sel[n]] for n in range(T)]), "status": np.stack([status[n + 1, sel[n]] for n in range(T)])}
    return f


def ref_track(inp):
    from tests import track_ref as tk
    return track_op(lambda fw, pts, bw, start, vf, vb: tk.track(fw, pts, bw, start, None, vf, vb))(inp)


def augment_subject(H, W, dtype="float32"):
    """Frames, flow, labels and ONE (1, 32) record, the same for every image of a batch (role SHARED): a crop of (H - 2) x
    (W - 2) placed with zoom 1.1, 5 degrees and a fractional shift, colour records with a pow.  10 % of the flow unlabelled."""
    from tests import augment_ref as ar
    rs = np.random.RandomState(900)
    crop = (H - 2, W - 2)
    c, pc = ((W - 1) / 2.0, (H - 1) / 2.0), ((crop[1] - 1) / 2.0, (crop[0] - 1) / 2.0)
    rec = ar.record(ar.similarity(c, pc, zoom=1.1, deg=5.0, shift=(0.3, -0.2)), ar.similarity(c, pc, zoom=1.1, deg=5.0, shift=(0.6, -0.4)),
                    (1.1, 0.93, 1.04, 1.3, 1.15, 0.03), (1.12, 0.95, 1.02, 1.3, 1.15, 0.04))[None]
    u8 = [rs.randint(0, 256, (1, H, W, 3)).astype(np.uint8) for _ in range(2)]
    im0, im1 = u8 if dtype == "uint8" else [ar.to_float32(a) for a in u8]
    sub = {"im0": im0, "im1": im1, "flow": rs.uniform(-2, 2, (1, H, W, 2)).astype(np.float32), "valid": rs.uniform(size=(1, H, W)) >= 0.1,
           "record": rec}
    return sub, {"im0": FLOAT, "im1": FLOAT, "flow": FLOAT, "valid": MASK, "record": SHARED}, crop


def ref_augment(crop, nearest):
    def f(inp, raw=False):
        from tests import augment_ref as ar
        N = inp["im0"].shape[0]
        with np.errstate(invalid="ignore"):
            r = ar.augment(inp["im0"], inp["im1"], np.repeat(inp["record"], N, axis=0), crop, inp["flow"], inp["valid"], nearest)
        return r if raw else {k: r[k] for k in ("out0", "out1", "flow", "valid")}
    return f
