"""Loss functions of the reference (losses.py) on the HIP path -- forward values only.

Same names, argument order and meaning as reference losses.py:4-48.  Every function returns a
0-dim float32 tensor on the inputs' device.  Sparse ground truth (KITTI, Sintel's invalid/ masks, the .flo sentinel):
every loss takes `valid`, an (N,H,W) torch.bool / torch.uint8 mask at the ground truth's resolution, and then sums over
the valid pixels only (pwc_flow_norm_masked_sums_f32); flow_metrics / summarize_metrics give the numbers quoted for
such sets (masked EPE, Fl-all, 1/3/5-px rates, EPE by motion magnitude).  The per-image sums of norms come from
pwc_flow_norm_sums_f32 (deterministic two-stage reduction); the handful of per-image scalars is
combined with torch (mean over the batch, level weights).

Note on multirobust_loss: the reference body (losses.py:45-46) computes `_l = L1loss(...)` and
then uses an undefined name `loss_level`, i.e. it raises NameError when called; what the code
evidently means -- weight * (L1 + epsilon)**q per level, Sec. 4 of the PWC-Net paper -- is what
is implemented here.
"""
import torch

from . import _lib
from .grad_ops import mask_ptr
from .modules import _p, as_view


def _norm_sums(pred, gt, ord, gt_div=1.0, valid=None):
    """Per-image sums over the pixels of ||pred - nearest_downsample(gt) / gt_div||_ord: (sums, view of pred).  With a mask
    (grad_ops.mask_ptr's format, at gt's resolution) the sums run over the valid pixels and the per-image numbers of valid
    pixels at pred's resolution come back as well: (sums, view of pred, counts int32)."""
    if valid is not None:                      # the mask's own faults first: before any tensor reaches the library
        vp = mask_ptr(valid, gt.shape[0], gt.shape[1], gt.shape[2], gt.device)
    pv, pred = as_view(pred, "flows")
    gv, gt = as_view(gt, "flows_gt")
    assert pv.C == 2 and gv.C == 2 and pv.N == gv.N, "flows must be (N,h,w,2)"
    L = _lib.lib()
    out = torch.empty((pv.N,), dtype=torch.float32, device=pred.device)
    if valid is None:
        ws = torch.empty((max(L.pwc_flow_norm_workspace_floats(pv.N, pv.H, pv.W), 1),), dtype=torch.float32, device=pred.device)
        _lib.check(L.pwc_flow_norm_sums_f32(_p(pv.ptr), pv.cs, _p(gv.ptr), gv.cs, pv.N, pv.H, pv.W, gv.H, gv.W,
                                            float(gt_div), int(ord), _p(ws.data_ptr()), ws.numel(),
                                            _p(out.data_ptr()), _lib.current_stream()), "flow norm sums")
        return out, pv
    ws = torch.empty((max(L.pwc_flow_norm_masked_workspace_floats(pv.N, pv.H, pv.W), 1),), dtype=torch.float32, device=pred.device)
    counts = torch.empty((pv.N,), dtype=torch.int32, device=pred.device)
    _lib.check(L.pwc_flow_norm_masked_sums_f32(_p(pv.ptr), pv.cs, _p(gv.ptr), gv.cs, vp, pv.N, pv.H, pv.W, gv.H, gv.W,
                                               float(gt_div), int(ord), _p(ws.data_ptr()), ws.numel(), _p(out.data_ptr()),
                                               _p(counts.data_ptr()), _lib.current_stream()), "masked flow norm sums")
    return out, pv, counts


def L1loss(x, y, valid=None):   # shape(# batch, h, w, 2)
    """reference losses.py:4-5: mean over the batch of the per-image sum of L1 norms (valid: over the valid pixels)."""
    return _norm_sums(y, x, 1, valid=valid)[0].mean()


def L2loss(x, y, valid=None):   # shape(# batch, h, w, 2)
    """reference losses.py:7-8."""
    return _norm_sums(y, x, 2, valid=valid)[0].mean()


def EPE(flows_gt, flows, valid=None):
    """End point error (reference losses.py:11-13); both flows unscaled.  valid: sum of the errors over the number of
    valid pixels of the whole batch; 0 when nothing is valid."""
    if valid is None:
        sums, v = _norm_sums(flows, flows_gt, 2)
        return sums.sum() / float(v.N * v.H * v.W)
    sums, _, counts = _norm_sums(flows, flows_gt, 2, valid=valid)
    return sums.sum() / counts.sum().clamp(min=1).to(torch.float32)


def multiscale_loss(flows_gt, flows_pyramid, weights, name="multiscale_loss", valid=None):
    """reference losses.py:15-32: flows_gt unscaled; it is divided by 20 and
    nearest-neighbour-downsampled to every pyramid level inside -- and so is the mask, when one is given: the reference's
    reduction is kept (per-image sum over the valid pixels, mean over the batch, level weights)."""
    loss = None
    for weight, fs in zip(weights, flows_pyramid):
        sums = _norm_sums(fs, flows_gt, 2, gt_div=20.0, valid=valid)[0]
        term = float(weight) * sums.mean()
        loss = term if loss is None else loss + term
    return loss


def multirobust_loss(flows_gt, flows_pyramid, weights, epsilon=0.01, q=0.4, name="multirobust_loss", valid=None):
    """reference losses.py:34-48 (see the module docstring about its undefined name)."""
    loss = None
    for weight, fs in zip(weights, flows_pyramid):
        sums = _norm_sums(fs, flows_gt, 1, gt_div=20.0, valid=valid)[0]
        term = float(weight) * (sums.mean() + float(epsilon)) ** float(q)
        loss = term if loss is None else loss + term
    return loss


# ------------------------------------------------------------------ flow metrics
METRIC_FIELDS = ("n_valid", "sum_e", "n_fl", "n_e1", "n_e3", "n_e5", "n_s0_10", "sum_e_s0_10", "n_s10_40", "sum_e_s10_40",
                 "n_s40", "sum_e_s40")


def _flow_metrics_host(flows_gt, flows, valid):
    """pwc_flow_metrics_f32 in float64 torch, for CPU tensors (evaluate_pairs under gloo)."""
    gt, pred = flows_gt.double(), flows.double()
    N = gt.shape[0]
    m = torch.ones(gt.shape[:3], dtype=torch.bool) if valid is None else valid.bool()
    zero = torch.zeros((), dtype=torch.float64)
    d = torch.where(m.unsqueeze(3), pred - gt, zero)              # selected out: NaN at an invalid pixel stays there
    e = torch.linalg.vector_norm(d, ord=2, dim=3)
    g = torch.linalg.vector_norm(torch.where(m.unsqueeze(3), gt, zero), ord=2, dim=3)
    b0, b1, b2 = m & (g < 10), m & (g >= 10) & (g < 40), m & (g >= 40)

    def n(c):
        return c.reshape(N, -1).sum(1).double()

    def se(c):
        return torch.where(c, e, zero).reshape(N, -1).sum(1)

    return torch.stack([n(m), se(m), n(m & (e > 3) & (e > 0.05 * g)), n(m & (e > 1)), n(m & (e > 3)), n(m & (e > 5)),
                        n(b0), se(b0), n(b1), se(b1), n(b2), se(b2)], dim=1)


def flow_metrics(flows_gt, flows, valid=None):
    """(N, 12) float64 per-image sums behind the numbers quoted for optical flow, METRIC_FIELDS in order: with e the
    end-point error and g the ground truth's magnitude at a valid pixel (both flows unscaled, one resolution),
    n_valid, sum e, KITTI's outliers n(e > 3 and e > 0.05 g), n(e > 1), n(e > 3), n(e > 5), and pixel count / sum e for
    g < 10, 10 <= g < 40, g >= 40.  valid: (N, h, w) torch.bool / torch.uint8, None = every pixel.  CUDA tensors go through
    pwc_flow_metrics_f32 (one pass); CPU tensors are computed with torch in float64.  Sums of these rows over images,
    batches and ranks stay meaningful: summarize_metrics turns them into rates."""
    if tuple(flows_gt.shape) != tuple(flows.shape) or flows.dim() != 4 or flows.shape[3] != 2:
        raise ValueError(f"flow_metrics: flows {tuple(flows.shape)} and flows_gt {tuple(flows_gt.shape)} must both be (N,h,w,2)")
    N, H, W = flows.shape[:3]
    if not flows.is_cuda:
        if valid is not None:
            if valid.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"valid: expected a torch.bool or torch.uint8 tensor, got {valid.dtype}")
            if tuple(valid.shape) != (N, H, W):
                raise ValueError(f"valid: expected shape {(N, H, W)}, got {tuple(valid.shape)}")
        return _flow_metrics_host(flows_gt, flows, valid)
    vp = None if valid is None else mask_ptr(valid, N, H, W, flows.device)
    pv, flows = as_view(flows, "flows")
    gv, flows_gt = as_view(flows_gt, "flows_gt")
    L = _lib.lib()
    ws = torch.empty((max(L.pwc_flow_metrics_workspace_floats(N, H, W), 1),), dtype=torch.float32, device=flows.device)
    out = torch.empty((N, 12), dtype=torch.float64, device=flows.device)
    _lib.check(L.pwc_flow_metrics_f32(_p(pv.ptr), pv.cs, _p(gv.ptr), gv.cs, vp, N, H, W, _p(ws.data_ptr()), ws.numel(),
                                      _p(out.data_ptr()), _lib.current_stream()), "flow metrics")
    return out


def summarize_metrics(m):
    """An (N, 12) flow_metrics tensor -- or a sum of several, (12,) -- as a dict: epe, fl_all (KITTI's outlier rate), px1 / px3 /
    px5 (fractions of the valid pixels with an error above 1 / 3 / 5 px), epe_s0_10 / epe_s10_40 / epe_s40 (EPE by
    ground-truth motion magnitude) and valid_px.  Rates are fractions in [0, 1]; an empty bucket gives None; with nothing
    valid epe and the rates are 0."""
    m = torch.as_tensor(m, dtype=torch.float64).reshape(-1, 12).sum(0).cpu().tolist()
    n = m[0]

    def ratio(a, b):
        return a / b if b > 0 else None

    return {"epe": m[1] / n if n > 0 else 0.0, "fl_all": m[2] / n if n > 0 else 0.0,
            "px1": m[3] / n if n > 0 else 0.0, "px3": m[4] / n if n > 0 else 0.0, "px5": m[5] / n if n > 0 else 0.0,
            "epe_s0_10": ratio(m[7], m[6]), "epe_s10_40": ratio(m[9], m[8]), "epe_s40": ratio(m[11], m[10]),
            "valid_px": int(n)}
