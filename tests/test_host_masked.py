"""Host-side tests of the sparse-ground-truth path (validity masks in the losses, the trainer and the flow metrics): argument
checks of the new C entry points (nothing is launched), the .flo sentinel, the float64 host form of the flow metrics and the
sharded evaluation with masks on CPU tensors.  No GPU needed.  The numpy references of this file (metrics_ref, metric_inputs)
are shared with tests/test_gpu_masked_loss.py."""
import ctypes

import numpy as np
import pytest
import torch

from pwcnet_amd import _lib, flow_io, losses, sharding

_AL = ctypes.c_void_p(4096)     # an aligned non-null address: argument checks only, nothing is launched
_EINVAL, _ERANGE, _EUNSUP = -1, -3, -4

E_THRESHOLDS, G_THRESHOLDS = (1.0, 3.0, 5.0), (10.0, 40.0)


# ------------------------------------------------------------------ shared references
def metric_inputs(N, H, W, seed, frac_valid=None):
    """(gt, pred, valid) float32 / bool: ||gt|| drawn from {5, 20, 60} and the error length from {0.5, 2, 4, 7}, each times a
    random direction, so that no pixel sits near a threshold of the metrics; valid: None, or about frac_valid True."""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(0, 2 * np.pi, (N, H, W)), rs.uniform(0, 2 * np.pi, (N, H, W))
    g = rs.choice([5.0, 20.0, 60.0], size=(N, H, W))
    e = rs.choice([0.5, 2.0, 4.0, 7.0], size=(N, H, W))
    gt = np.stack([g * np.cos(a), g * np.sin(a)], axis=3).astype(np.float32)
    pred = (gt.astype(np.float64) + np.stack([e * np.cos(b), e * np.sin(b)], axis=3)).astype(np.float32)
    valid = None if frac_valid is None else rs.uniform(size=(N, H, W)) < frac_valid
    return gt, pred, valid


def assert_clear_of_thresholds(gt, pred, valid, margin=1e-3):
    """Every valid pixel's e and g (float64 of the fp32 inputs) keep `margin` relative distance from 1, 3, 5, 0.05 g, 10, 40."""
    m = np.ones(gt.shape[:3], bool) if valid is None else valid
    e = np.linalg.norm(pred.astype(np.float64) - gt.astype(np.float64), axis=3)[m]
    g = np.linalg.norm(gt.astype(np.float64), axis=3)[m]
    for t in E_THRESHOLDS:
        assert np.all(np.abs(e - t) >= margin * t), t
    for t in G_THRESHOLDS:
        assert np.all(np.abs(g - t) >= margin * t), t
    assert np.all(np.abs(e - 0.05 * g) >= margin * np.maximum(e, 0.05 * g))


def metrics_ref(gt, pred, valid):
    """The twelve per-image values of pwc_flow_metrics_f32 in numpy float64: select the valid pixels, then count and sum."""
    N = gt.shape[0]
    out = np.zeros((N, 12), np.float64)
    for n in range(N):
        m = np.ones(gt.shape[1:3], bool) if valid is None else np.asarray(valid[n], bool)
        d = pred[n][m].astype(np.float64) - gt[n][m].astype(np.float64)
        e = np.sqrt((d * d).sum(1))
        g = np.sqrt((gt[n][m].astype(np.float64) ** 2).sum(1))
        b0, b1, b2 = g < 10, (g >= 10) & (g < 40), g >= 40
        out[n] = [e.size, e.sum(), ((e > 3) & (e > 0.05 * g)).sum(), (e > 1).sum(), (e > 3).sum(), (e > 5).sum(),
                  b0.sum(), e[b0].sum(), b1.sum(), e[b1].sum(), b2.sum(), e[b2].sum()]
    return out


COUNT_COLS, SUM_COLS = [0, 2, 3, 4, 5, 6, 8, 10], [1, 7, 9, 11]


def summary_ref(m):
    """summarize_metrics restated on a (12,) numpy vector."""
    r = lambda a, b: a / b if b > 0 else None
    n = m[0]
    return {"epe": m[1] / n if n else 0.0, "fl_all": m[2] / n if n else 0.0, "px1": m[3] / n if n else 0.0,
            "px3": m[4] / n if n else 0.0, "px5": m[5] / n if n else 0.0, "epe_s0_10": r(m[7], m[6]),
            "epe_s10_40": r(m[9], m[8]), "epe_s40": r(m[11], m[10]), "valid_px": int(n)}


def assert_summary(got, exp, rel=1e-5):
    assert set(exp) <= set(got), set(exp) - set(got)
    for k, v in exp.items():
        if v is None or k == "valid_px":
            assert got[k] == v, (k, got[k], v)
        else:
            assert got[k] is not None and abs(got[k] - v) <= rel * max(abs(v), 1e-6), (k, got[k], v)


# ------------------------------------------------------------------ C ABI: checks before any launch
def test_masked_entry_points_refuse_bad_arguments_before_launching():
    L = _lib.lib()
    sums = lambda **kw: L.pwc_flow_norm_masked_sums_f32(*[dict(dict(
        pred=_AL, pred_cs=2, gt=_AL, gt_cs=2, valid=_AL, N=2, H=4, W=8, GH=16, GW=32, gt_div=20.0, ord=2, ws=_AL, wsf=1 << 16,
        out=_AL, counts=_AL, stream=None), **kw)[k] for k in
        "pred pred_cs gt gt_cs valid N H W GH GW gt_div ord ws wsf out counts stream".split()])
    grad = lambda **kw: L.pwc_flow_norm_masked_grad_f32(*[dict(dict(
        pred=_AL, pred_cs=2, gt=_AL, gt_cs=2, valid=_AL, N=2, H=4, W=8, GH=16, GW=32, gt_div=20.0, ord=2, scale=1.0, dpred=_AL,
        dpred_cs=2, acc=0, stream=None), **kw)[k] for k in
        "pred pred_cs gt gt_cs valid N H W GH GW gt_div ord scale dpred dpred_cs acc stream".split()])
    met = lambda **kw: L.pwc_flow_metrics_f32(*[dict(dict(
        pred=_AL, pred_cs=2, gt=_AL, gt_cs=2, valid=None, N=2, H=4, W=8, ws=_AL, wsf=1 << 16, out=_AL, stream=None), **kw)[k]
        for k in "pred pred_cs gt gt_cs valid N H W ws wsf out stream".split()])
    for name in ("pred", "gt", "valid", "ws", "out", "counts"):
        assert sums(**{name: None}) == _EINVAL, name
    for name in ("pred", "gt", "valid", "dpred"):
        assert grad(**{name: None}) == _EINVAL, name
    for name in ("pred", "gt", "ws", "out"):
        assert met(**{name: None}) == _EINVAL, name
    for f in (sums, grad):
        assert f(ord=3) == _EUNSUP and f(ord=0) == _EUNSUP
        assert f(gt_div=0.0) == _EINVAL
        assert f(N=0) == _EINVAL and f(H=-1) == _EINVAL and f(GW=0) == _EINVAL
        assert f(pred_cs=1) == _EINVAL and f(gt_cs=1) == _EINVAL
    assert grad(dpred_cs=1) == _EINVAL
    assert met(N=0) == _EINVAL and met(W=0) == _EINVAL and met(pred_cs=1) == _EINVAL and met(gt_cs=0) == _EINVAL
    assert sums(wsf=0) == _EINVAL and met(wsf=0) == _EINVAL
    assert sums(wsf=L.pwc_flow_norm_masked_workspace_floats(2, 4, 8) - 1) == _EINVAL
    assert met(wsf=L.pwc_flow_metrics_workspace_floats(2, 4, 8) - 1) == _EINVAL
    assert sums(H=65536, W=65536) == _ERANGE and sums(N=65536) == _ERANGE
    assert met(H=65536, W=65536) == _ERANGE and met(N=65536) == _ERANGE
    # an image whose last pixels the int pixel index of the sums loops cannot step over (it advances by up to 65536 past them):
    # refused; the largest it can is let through to the workspace check
    def plain(N=2, H=4, W=8, wsf=1 << 16):
        return L.pwc_flow_norm_sums_f32(_AL, 2, _AL, 2, N, H, W, 16, 32, 20.0, 2, _AL, wsf, _AL, None)

    for f in (sums, met, plain):
        assert f(H=1, W=(1 << 31) - 1) == _ERANGE and f(H=1, W=(1 << 31) - 65536) == _ERANGE
        assert f(H=1, W=(1 << 31) - 1, wsf=0) == _ERANGE
        assert f(H=1, W=(1 << 31) - 1 - 65536, wsf=0) == _EINVAL


def test_masked_workspace_sizes():
    L = _lib.lib()
    for f in (L.pwc_flow_norm_masked_workspace_floats, L.pwc_flow_metrics_workspace_floats):
        assert f(0, 4, 4) == 0 and f(2, 0, 4) == 0 and f(2, 4, -1) == 0
    # one part per 256 pixels, at most 256 parts of an image: a sum and a count per part / twelve words per part
    assert L.pwc_flow_norm_masked_workspace_floats(2, 16, 32) == 2 * 2 * 2
    assert L.pwc_flow_norm_masked_workspace_floats(3, 384, 448) == 2 * 3 * 256
    assert L.pwc_flow_norm_masked_workspace_floats(2, 16, 32) == 2 * L.pwc_flow_norm_workspace_floats(2, 16, 32)
    assert L.pwc_flow_metrics_workspace_floats(2, 15, 17) == 12 * 2 * 1
    assert L.pwc_flow_metrics_workspace_floats(2, 256, 257) == 12 * 2 * 256


# ------------------------------------------------------------------ the .flo sentinel
def test_flow_valid_follows_the_flo_convention():
    f = np.zeros((3, 4, 2), np.float32)
    f[0, 0] = (1.5, -2.0)
    f[0, 1] = (np.nan, 0.0)
    f[0, 2] = (0.0, np.inf)
    f[0, 3] = (-np.inf, 1.0)
    f[1, 0] = (1e10, 0.0)
    f[1, 1] = (0.0, -1e10)
    f[1, 2] = (1e9, -1e9)                 # the threshold itself is still a measurement
    f[1, 3] = (1.0000001e9 * 1.001, 0.0)
    v = flow_io.flow_valid(f)
    exp = np.ones((3, 4), bool)
    exp[0, 1:] = False
    exp[1, 0] = exp[1, 1] = exp[1, 3] = False
    assert v.dtype == bool and v.shape == (3, 4) and np.array_equal(v, exp)
    assert flow_io.flow_valid(f[None]).shape == (1, 3, 4)
    with pytest.raises(ValueError):
        flow_io.flow_valid(np.zeros((3, 4, 3), np.float32))
    # flow_to_color blanks exactly those pixels
    assert np.array_equal(flow_io.flow_to_color(f)[~exp], flow_io.flow_to_color(np.zeros((1, 1, 2)))[0].repeat((~exp).sum(), 0))


# ------------------------------------------------------------------ flow metrics, host form
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 15, 17), (1, 257, 1), (2, 64, 65)])
@pytest.mark.parametrize("masked", [False, True])
def test_flow_metrics_on_cpu_tensors_vs_numpy(N, H, W, masked):
    gt, pred, valid = metric_inputs(N, H, W, seed=H + 3 * W, frac_valid=0.6 if masked else None)
    assert_clear_of_thresholds(gt, pred, valid)
    ref = metrics_ref(gt, pred, valid)
    if masked:                                     # whatever sits at an invalid pixel must not matter
        gt, pred = gt.copy(), pred.copy()
        gt[~valid] = np.array([np.nan, 1e10], np.float32)
        pred[~valid] = np.nan
    tv = None if valid is None else torch.from_numpy(valid)
    got = losses.flow_metrics(torch.from_numpy(gt), torch.from_numpy(pred), tv)
    assert got.dtype == torch.float64 and tuple(got.shape) == (N, 12) and not got.is_cuda
    got = got.numpy()
    assert np.array_equal(got[:, COUNT_COLS], ref[:, COUNT_COLS])
    assert np.allclose(got[:, SUM_COLS], ref[:, SUM_COLS], rtol=1e-12, atol=0)
    if masked:
        u8 = losses.flow_metrics(torch.from_numpy(gt), torch.from_numpy(pred), tv.to(torch.uint8) * 255).numpy()
        assert np.array_equal(u8, got)
    assert_summary(losses.summarize_metrics(torch.from_numpy(got)), summary_ref(ref.sum(0)), rel=1e-12)
    assert_summary(losses.summarize_metrics(torch.from_numpy(got).sum(0)), summary_ref(ref.sum(0)), rel=1e-12)


def test_summarize_metrics_empty_buckets_and_nothing_valid():
    gt = np.zeros((1, 4, 4, 2), np.float32)
    gt[..., 0] = 20.0                               # every pixel in the 10..40 bucket
    pred = gt.copy()
    pred[..., 1] = 4.0                              # e = 4 everywhere: > 3 and > 0.05 * 20
    s = losses.summarize_metrics(losses.flow_metrics(torch.from_numpy(gt), torch.from_numpy(pred)))
    assert s == {"epe": 4.0, "fl_all": 1.0, "px1": 1.0, "px3": 1.0, "px5": 0.0, "epe_s0_10": None, "epe_s10_40": 4.0,
                 "epe_s40": None, "valid_px": 16}
    none = torch.zeros((1, 4, 4), dtype=torch.bool)
    m = losses.flow_metrics(torch.from_numpy(gt), torch.from_numpy(pred), none)
    assert not m.any()
    s = losses.summarize_metrics(m)
    assert s["epe"] == 0.0 and s["fl_all"] == 0.0 and s["px1"] == 0.0 and s["valid_px"] == 0
    assert s["epe_s0_10"] is None and s["epe_s10_40"] is None and s["epe_s40"] is None


# ------------------------------------------------------------------ mask argument checks (before the library is called)
def test_mask_dtype_and_shape_are_checked_before_the_library_is_called(monkeypatch):
    from pwcnet_amd import grad_ops as G
    from pwcnet_amd.modules import View

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    N, GH, GW = 2, 8, 16
    gt, pred = torch.zeros((N, GH, GW, 2)), torch.zeros((N, 2, 4, 2))
    v = View(4096, 2, N, 2, 4, 2)
    g = View(4096, 2, N, GH, GW, 2)
    for call in (lambda m: G.flow_norm_grad(v, g, v, gt_div=20.0, valid=m),
                 lambda m: losses._norm_sums(pred, gt, 2, gt_div=20.0, valid=m),
                 lambda m: losses.L1loss(gt, gt, valid=m), lambda m: losses.L2loss(gt, gt, valid=m),
                 lambda m: losses.EPE(gt, gt, valid=m),
                 lambda m: losses.multiscale_loss(gt, [pred], [1.0], valid=m),
                 lambda m: losses.multirobust_loss(gt, [pred], [1.0], valid=m),
                 lambda m: losses.flow_metrics(gt, gt, valid=m)):
        with pytest.raises(TypeError):
            call(torch.ones((N, GH, GW), dtype=torch.float32))
        with pytest.raises(TypeError):
            call(np.ones((N, GH, GW), bool))
        with pytest.raises(ValueError):
            call(torch.ones((N, GH, GW, 1), dtype=torch.bool))
        with pytest.raises(ValueError):
            call(torch.ones((N, GH, GW + 1), dtype=torch.uint8))
    # a well-formed mask on the CPU beside GPU views is refused as well (the kernels read device memory)
    with pytest.raises(ValueError):
        G.flow_norm_grad(v, g, v, valid=torch.ones((N, GH, GW), dtype=torch.bool))


# ------------------------------------------------------------------ sharded evaluation with masks (CPU tensors)
def _pairs(sizes, fracs, seed, tuples=4):
    """Pairs of the given (h, w) sizes: image_0 carries the pair's index, the stub forward returns the stored prediction.
    fracs: valid fraction per pair (None: no mask item, 0.0: nothing valid); invalid ground truth is the sentinel / NaN."""
    items, clean = [], []
    for i, ((h, w), fr) in enumerate(zip(sizes, fracs)):
        gt, pred, _ = metric_inputs(1, h, w, seed + i)
        rs = np.random.RandomState(seed + 100 + i)
        valid = None if fr is None else rs.uniform(size=(h, w)) < fr
        clean.append((gt[0], pred[0], valid))
        g = gt[0].copy()
        if valid is not None:
            g[~valid] = np.where(rs.uniform(size=(int((~valid).sum()), 1)) < 0.5, np.float32(1e10), np.float32(np.nan))
        im = np.full((h, w, 3), float(i), np.float32)
        it = (torch.from_numpy(im), torch.from_numpy(im.copy()), torch.from_numpy(g))
        if tuples == 4 and valid is not None:
            it = it + (torch.from_numpy(valid),)
        items.append((it, torch.from_numpy(pred[0])))
    return items, clean


def evaluation_case(device, seed=5):
    """(forward, load_pair, n, expected result dict) of a masked evaluation: 5 pairs of two sizes, valid fractions from 0 to
    1, one pair without a mask item; the expectation is computed in numpy float64 over all pixels of all pairs at once."""
    sizes = [(16, 24), (16, 24), (8, 40), (8, 40), (16, 24)]
    fracs = [0.9, 0.05, 0.0, 0.5, None]
    items, clean = _pairs(sizes, fracs, seed)
    stored = [p for _, p in items]

    def forward(im0, im1):
        return torch.stack([stored[int(round(float(im0[j, 0, 0, 0])))] for j in range(im0.shape[0])]).to(device)

    total = np.zeros(12)
    per_pair = []
    for gt, pred, valid in clean:
        assert_clear_of_thresholds(gt[None], pred[None], None if valid is None else valid[None])
        m = metrics_ref(gt[None], pred[None], None if valid is None else valid[None])[0]
        total += m
        per_pair.append(m[1] / m[0] if m[0] else 0.0)
    exp = summary_ref(total)
    exp["pairs"] = len(items)
    return forward, (lambda i: items[i][0]), len(items), exp, per_pair


def test_evaluate_pairs_with_masks_and_metrics_on_cpu():
    forward, load_pair, n, exp, per_pair = evaluation_case("cpu")
    res = sharding.evaluate_pairs(forward, load_pair, n, batch=2, device="cpu", metrics=True)
    assert res["pairs"] == exp.pop("pairs")
    assert_summary(res, exp, rel=1e-6)                # (the host form computes e from fp32 differences)
    assert np.allclose(res["per_pair_epe"], per_pair, rtol=1e-6, atol=0) and res["per_pair_epe"][2] == 0.0
    # a mean of per-pair means is a different number: the check above is pixel-weighted
    assert abs(np.mean(per_pair) - exp["epe"]) > 1e-3 * exp["epe"]
    # masks without metrics: the same masked epe, no metric keys
    plain = sharding.evaluate_pairs(forward, load_pair, n, batch=2, device="cpu")
    assert sorted(plain) == ["epe", "pairs", "per_pair_epe"]
    assert abs(plain["epe"] - exp["epe"]) <= 1e-6 * exp["epe"]
    assert np.allclose(plain["per_pair_epe"], per_pair, rtol=1e-6, atol=0) and plain["per_pair_epe"][2] == 0.0


def test_evaluate_pairs_without_masks_is_unchanged():
    """3-tuples and metrics=False: the keys and the values of the evaluation before masks existed, computed here the way it
    computed them (fp32 norms, per-pair mean in fp32, float64 sum over all pixels)."""
    sizes = [(16, 24), (16, 24), (8, 40), (16, 24)]
    items, clean = _pairs(sizes, [None] * 4, seed=9, tuples=3)
    stored = [p for _, p in items]
    forward = lambda im0, im1: torch.stack([stored[int(round(float(im0[j, 0, 0, 0])))] for j in range(im0.shape[0])])
    res = sharding.evaluate_pairs(forward, lambda i: items[i][0], len(items), batch=3, device="cpu")
    assert sorted(res) == ["epe", "pairs", "per_pair_epe"] and res["pairs"] == 4
    norms = [torch.linalg.vector_norm(torch.from_numpy(g) - torch.from_numpy(p), ord=2, dim=2) for g, p, _ in clean]
    # batch 3 splits where the size changes: pairs 0-1 share a batch, 2 and 3 stand alone
    batches = [torch.stack(norms[0:2]), norms[2][None], norms[3][None]]
    assert res["per_pair_epe"] == [v for b in batches for v in b.mean(dim=(1, 2)).double().tolist()]
    assert res["epe"] == sum(float(b.double().sum()) for b in batches) / sum(float(b.numel()) for b in batches)
