"""Training augmentation on the GPU: an affine crop of both frames, colour jitter, and the ground-truth flow transformed exactly.

`draw_params` draws, on the host, one 32-double record per pair -- a random scale, rotation, translation and mirror applied to both
frames, a small extra transform of the second frame relative to the first, and gain / gamma / contrast / brightness jitter --
and `augment_pairs` applies the records in ONE launch of csrc/pwc_augment.hip to whole uint8 (or float32) frames, the flow and its
validity mask: a quarter of the bytes to upload, and no resampling on the host.  `crop_params` is the record of the plain
integer crop, which the launch reproduces bit for bit.

The record (include/pwc_hip.h), pixel centres at integer indices:
     0 ..  5  M0 = (a b c; d e f): output pixel (x, y) -> frame-0 position q0 = (a x + b y + c, d x + e y + f)
     6 .. 11  M1, the same map into frame 1
    12 .. 17  I1, the inverse of M1 (computed here in float64, so kernel and reference use the same numbers)
    18 .. 23  frame 0 photometric: gain r, g, b; gamma; contrast; brightness
    24 .. 29  frame 1 photometric
    30 .. 31  zero
Flow: out_flow(p) = I1 (q0 + flow(q0)) - p -- zoom, rotation, mirror and the relative transform are all this one formula.
out_valid(p) = 1 iff q0 lies inside the frame and every tap the flow sample used is labelled; elsewhere out_flow is 0.
Everything is formed in double and rounded to float32 once.  No autograd: these are inputs of a training step.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .fit import _check

RECORD = 32
PHOTO_IDENTITY = (1.0, 1.0, 1.0, 1.0, 1.0, 0.0)
FLOW_INTERP = {"bilinear": 0, "nearest": 1}
MAX_REJECTIONS = 20


def invert_affine(m):
    """(a, b, c, d, e, f) of the inverse of the map (a b c; d e f), in float64."""
    a, b, c, d, e, f = (float(v) for v in m)
    det = a * e - b * d
    if det == 0.0:
        raise ValueError(f"augment: the affine map {tuple(m)} is singular")
    ia, ib, id_, ie = e / det, -b / det, -d / det, a / det
    return np.array([ia, ib, -(ia * c + ib * f), id_, ie, -(id_ * c + ie * f)], np.float64)


def _corners_inside(m, frame_hw, crop_hw):
    H, W = frame_hw
    ch, cw = crop_hw
    for x in (0.0, cw - 1.0):
        for y in (0.0, ch - 1.0):
            qx, qy = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
            if not (0.0 <= qx <= W - 1.0 and 0.0 <= qy <= H - 1.0):
                return False
    return True


def _span(v, what):
    """A (lo, hi) range from a pair, or from one number r >= 1 meaning (1 / r, r)."""
    if np.ndim(v) == 0:
        r = float(v)
        if r <= 0:
            raise ValueError(f"draw_params: {what} must be positive, got {v}")
        lo, hi = min(r, 1.0 / r), max(r, 1.0 / r)
    else:
        lo, hi = (float(t) for t in v)
    if not 0 < lo <= hi:
        raise ValueError(f"draw_params: {what} must be a range 0 < lo <= hi, got {v}")
    return lo, hi


def _log_uniform(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _affine(cx, cy, pcx, pcy, lin, tx, ty):
    """q = (cx + tx, cy + ty) + lin (p - (pcx, pcy)) as (a, b, c, d, e, f)."""
    (a, b), (d, e) = lin
    return np.array([a, b, cx + tx - (a * pcx + b * pcy), d, e, cy + ty - (d * pcx + e * pcy)], np.float64)


def _rotation(deg):
    t = np.deg2rad(deg)
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]], np.float64)


def draw_params(N, frame_hw, crop_hw, rng, scale=(1.0, 1.0), rotate_deg=0.0, translate_frac=0.0, flip=0.5, rel_scale=1.0,
                rel_rotate_deg=0.0, rel_translate_px=0.0, color=True):
    """(N, 32) float64 records for N pairs of `frame_hw` = (H, W) frames cut to `crop_hw` = (ch, cw).  Host only; deterministic
    in `rng`, a numpy.random.RandomState.

    Both frames: zoom s log-uniform in `scale` = (lo, hi) (s > 1 magnifies), rotation uniform in +-`rotate_deg`, the crop's
    centre moved off the frame's by uniform +-`translate_frac` of the frame's width and height, mirrored left-right with
    probability `flip`.  Frame 1 relative to frame 0: zoom log-uniform in `rel_scale` (a pair, or one number r for
    (1 / r, r)), rotation +-`rel_rotate_deg`, shift +-`rel_translate_px` pixels.  `color`: gain per channel, gamma, contrast and
    brightness of frame 0, and a small gain and brightness change of frame 1 against it.  Zeros (1s for the scales) switch a
    part off; everything off is the centred crop.

    A draw is kept only if the crop's four corners map inside both frames (then every sample of the crop does); after 20
    rejected draws the sample falls back to the centred identity crop with the colour record it drew last.  ValueError if the
    crop is larger than the frame."""
    H, W = (int(v) for v in frame_hw)
    ch, cw = (int(v) for v in crop_hw)
    if N < 1 or min(H, W, ch, cw) < 1:
        raise ValueError(f"draw_params: N {N}, frame {H} x {W} and crop {ch} x {cw} must be positive")
    if ch > H or cw > W:
        raise ValueError(f"draw_params: the crop {ch} x {cw} is larger than the frame {H} x {W}")
    if not isinstance(rng, np.random.RandomState):
        raise ValueError(f"draw_params: rng must be a numpy.random.RandomState, got {type(rng).__name__}")
    s_lo, s_hi = _span(scale, "scale")
    r_lo, r_hi = _span(rel_scale, "rel_scale")
    if not 0.0 <= float(flip) <= 1.0:
        raise ValueError(f"draw_params: flip is a probability, got {flip}")
    if min(float(rotate_deg), float(translate_frac), float(rel_rotate_deg), float(rel_translate_px)) < 0:
        raise ValueError("draw_params: rotate_deg, translate_frac, rel_rotate_deg and rel_translate_px must be non-negative")
    cx, cy, pcx, pcy = (W - 1) / 2.0, (H - 1) / 2.0, (cw - 1) / 2.0, (ch - 1) / 2.0
    out = np.zeros((N, RECORD), np.float64)
    for n in range(N):
        kept = False
        for _ in range(MAX_REJECTIONS + 1):
            # every draw takes the same numbers from rng, whatever is switched off
            s = _log_uniform(rng, s_lo, s_hi)
            rot = rng.uniform(-1.0, 1.0) * float(rotate_deg)
            tx, ty = rng.uniform(-1.0, 1.0, size=2) * float(translate_frac) * (W, H)
            mirror = rng.uniform() < float(flip)
            rs = _log_uniform(rng, r_lo, r_hi)
            rrot = rng.uniform(-1.0, 1.0) * float(rel_rotate_deg)
            rtx, rty = rng.uniform(-1.0, 1.0, size=2) * float(rel_translate_px)
            jit = rng.uniform(-1.0, 1.0, size=10)
            lin0 = _rotation(rot) @ np.diag([-1.0 if mirror else 1.0, 1.0]) / s
            lin1 = _rotation(rrot) @ lin0 / rs
            m0 = _affine(cx, cy, pcx, pcy, lin0, tx, ty)
            m1 = _affine(cx, cy, pcx, pcy, lin1, tx + rtx, ty + rty)
            if _corners_inside(m0, (H, W), (ch, cw)) and _corners_inside(m1, (H, W), (ch, cw)):
                kept = True
                break
        if not kept:
            m0 = m1 = _affine(cx, cy, pcx, pcy, np.eye(2), 0.0, 0.0)
        out[n, 0:6], out[n, 6:12], out[n, 12:18] = m0, m1, invert_affine(m1)
        if color:
            gains = np.exp(jit[0:3] * np.log(1.25))
            gamma, contrast, brightness = np.exp(jit[3] * np.log(1.5)), 1.0 + 0.3 * jit[4], 0.1 * jit[5]
            out[n, 18:24] = (*gains, gamma, contrast, brightness)
            out[n, 24:30] = (*(gains * (1.0 + 0.03 * jit[6:9])), gamma, contrast, brightness + 0.02 * jit[9])
        else:
            out[n, 18:24] = out[n, 24:30] = PHOTO_IDENTITY
    return out


def crop_params(N, y0, x0):
    """(N, 32) records of the plain crop whose top-left pixel is (y0, x0) (integers, or N of each): identity geometry with an
    integer offset and the identity photometric record -- augment_pairs then returns frame[y0:y0 + ch, x0:x0 + cw], the flow
    and the mask cut the same way, bit for bit."""
    y0, x0 = np.broadcast_to(np.asarray(y0), (N,)), np.broadcast_to(np.asarray(x0), (N,))
    if not (np.issubdtype(y0.dtype, np.integer) and np.issubdtype(x0.dtype, np.integer)):
        raise ValueError("crop_params: y0 and x0 must be integers")
    out = np.zeros((N, RECORD), np.float64)
    for base, sign in ((0, 1.0), (6, 1.0), (12, -1.0)):
        out[:, base + 0] = out[:, base + 4] = 1.0
        out[:, base + 2], out[:, base + 5] = sign * x0, sign * y0
    out[:, 18:24] = out[:, 24:30] = PHOTO_IDENTITY
    return out


def augment_pairs(images_0, images_1, params, crop_shape, flows=None, valid=None, flow_interp="bilinear"):
    """(N, H, W, 3) uint8 or float32 frames on the GPU, (N, 32) records (a numpy array, uploaded here, or a float64 GPU tensor),
    crop_shape (OH, OW) -> (x0, x1, flow, valid): the augmented frames (N, OH, OW, 3) float32, and with `flows` (N, H, W, 2)
    float32 the transformed flow (N, OH, OW, 2) float32 and its mask (N, OH, OW) torch.bool; None, None without.  `valid`:
    (N, H, W) torch.bool mask of the labelled pixels of `flows` (None: all).  flow_interp "bilinear" or "nearest" (sparse
    ground truth such as KITTI's: no blending of neighbours).  One launch on the current stream."""
    _check(images_0, "augment_pairs: images_0", 3, (torch.uint8, torch.float32))
    _check(images_1, "augment_pairs: images_1", 3, (torch.uint8, torch.float32))
    if images_0.shape != images_1.shape or images_0.dtype != images_1.dtype or images_0.device != images_1.device:
        raise ValueError(f"augment_pairs: the frames differ, {tuple(images_0.shape)} {images_0.dtype} on {images_0.device} and "
                         f"{tuple(images_1.shape)} {images_1.dtype} on {images_1.device}")
    if flow_interp not in FLOW_INTERP:
        raise ValueError(f"augment_pairs: unknown flow_interp {flow_interp!r} (one of {sorted(FLOW_INTERP)})")
    N, H, W, _ = images_0.shape
    dev = images_0.device
    try:
        OH, OW = (int(v) for v in crop_shape)
    except (TypeError, ValueError):
        raise ValueError(f"augment_pairs: crop_shape must be (OH, OW), got {crop_shape!r}") from None
    if OH < 1 or OW < 1:
        raise ValueError(f"augment_pairs: crop_shape {OH} x {OW} must be positive")
    if isinstance(params, np.ndarray):
        if params.shape != (N, RECORD) or params.dtype != np.float64:
            raise ValueError(f"augment_pairs: params must be ({N}, {RECORD}) float64, got {params.shape} {params.dtype}")
        params = torch.from_numpy(np.ascontiguousarray(params)).to(dev)
    elif isinstance(params, torch.Tensor):
        if tuple(params.shape) != (N, RECORD) or params.dtype != torch.float64 or params.device != dev or not params.is_contiguous():
            raise ValueError(f"augment_pairs: params must be a dense ({N}, {RECORD}) float64 tensor on {dev}, got "
                             f"{tuple(params.shape)} {params.dtype} on {params.device}")
    else:
        raise ValueError(f"augment_pairs: params must be a numpy array or a torch tensor, got {type(params).__name__}")
    if flows is None:
        if valid is not None:
            raise ValueError("augment_pairs: a valid mask belongs to flows, and flows is None")
    else:
        _check(flows, "augment_pairs: flows", 2, (torch.float32,))
        if tuple(flows.shape) != (N, H, W, 2) or flows.device != dev:
            raise ValueError(f"augment_pairs: flows must be ({N}, {H}, {W}, 2) on {dev}, got {tuple(flows.shape)} on {flows.device}")
        if valid is not None:
            if not isinstance(valid, torch.Tensor) or valid.dtype != torch.bool:
                raise ValueError(f"augment_pairs: valid must be a torch.bool tensor, got {getattr(valid, 'dtype', type(valid).__name__)}")
            if tuple(valid.shape) != (N, H, W) or valid.device != dev or not valid.is_contiguous():
                raise ValueError(f"augment_pairs: valid must be a dense ({N}, {H}, {W}) mask on {dev}, got {tuple(valid.shape)} "
                                 f"on {valid.device}")
    out0 = torch.empty((N, OH, OW, 3), dtype=torch.float32, device=dev)
    out1 = torch.empty((N, OH, OW, 3), dtype=torch.float32, device=dev)
    out_flow = out_valid = None
    if flows is not None:
        out_flow = torch.empty((N, OH, OW, 2), dtype=torch.float32, device=dev)
        out_valid = torch.empty((N, OH, OW), dtype=torch.bool, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pwc_augment_pairs_f32(ptr(images_0), ptr(images_1), int(images_0.dtype == torch.uint8), ptr(flows),
                                                    ptr(valid), ptr(params), ptr(out0), ptr(out1), ptr(out_flow), ptr(out_valid),
                                                    N, H, W, OH, OW, FLOW_INTERP[flow_interp], _lib.current_stream()),
                   "pwc_augment_pairs_f32")
    return out0, out1, out_flow, out_valid
