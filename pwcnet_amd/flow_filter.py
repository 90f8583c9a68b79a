"""Edge-aware weighted-median filtering and hole filling of flow fields on the HIP path (csrc/pwc_flow_filter.hip).

    filter_tables(radius, sigma_space=None, sigma_color=None, channels=3)   -> (space (2r+1)^2, color 255 C + 1) uint32 numpy
    filter_flow(flows, guide=None, valid=None, radius=2, ...)               -> (flows_out (N,H,W,2) float32, valid_out (N,H,W) bool)
    fill_flow(flows, valid=None, guide=None, radius=2, ..., iters=None)     -> the same, known pixels untouched, holes filled

Every output pixel is the weighted median, per component, of the known flow values in its (2r+1)^2 window; the weights are
integers from two tables -- spatial distance, and colour difference of the guide image to the centre pixel -- so that the result
is a selection defined by the input alone: the kernel equals its numpy restatement bit for bit (tests/flow_filter_ref.py).  The
exact definition is in include/pwc_hip.h, "flow filter", and DESIGN.md 23.  Unknown pixels are those of compose_flows,
motion_residual and sparse ground truth: the .flo sentinel 1e10 (flow_io.flow_valid's rule) or a zero of `valid`.  No autograd.

radius = 2 and the sigmas in the command-line tools are choices: nobody has tuned them, and nobody has measured what the filter
does to EPE or Fl-all.
"""
import math

import numpy as np
import torch

from . import _lib
from .interp import _check_mask
from .modules import _p, as_view
from .motion import _check_device, _ptr
from .unsup import _check_nhwc

MAX_RADIUS = _lib.FLOW_FILTER_MAX_RADIUS
TABLE_MAX = 65535


def add_cli_arguments(ap):
    """The --flow_filter flags of infer.py, infer_continuous.py and evaluate.py (all default off)."""
    ap.add_argument("--flow_filter", type=int, default=0, metavar="R",
                    help="filter the final flow with a weighted median of radius R = 1 .. 7 guided by the first frame, before it "
                         "is written, scored or used [0: off]")
    ap.add_argument("--flow_filter_sigma_space", type=float, default=None, metavar="S", help="--flow_filter: spatial sigma in pixels [a box]")
    ap.add_argument("--flow_filter_sigma_color", type=float, default=None, metavar="C",
                    help="--flow_filter: colour sigma in grey levels per channel [no colour term]")
    ap.add_argument("--flow_filter_iters", type=int, default=1, metavar="K", help="--flow_filter: passes [1]")


def check_cli_arguments(ap, args):
    """The flags' rules as argparse errors; returns filter_flow's keyword arguments, None without --flow_filter."""
    if not 0 <= args.flow_filter <= MAX_RADIUS:
        ap.error(f"--flow_filter must be in 1 .. {MAX_RADIUS} (0: off), got {args.flow_filter}")
    for name in ("flow_filter_sigma_space", "flow_filter_sigma_color"):
        v = getattr(args, name)
        if v is not None and not (v > 0.0 and math.isfinite(v)):
            ap.error(f"--{name} must be positive and finite, got {v}")
    if args.flow_filter_iters < 1:
        ap.error(f"--flow_filter_iters must be at least 1, got {args.flow_filter_iters}")
    if args.flow_filter == 0:
        return None
    return dict(radius=args.flow_filter, sigma_space=args.flow_filter_sigma_space, sigma_color=args.flow_filter_sigma_color,
                iters=args.flow_filter_iters)


def _check_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius: expected an integer in 1 .. {MAX_RADIUS}, got {radius!r}")
    return int(radius)


def _check_sigma(sigma, what):
    if sigma is None:
        return None
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (
            float(sigma) > 0.0 and math.isfinite(float(sigma))):
        raise ValueError(f"{what}: expected None or a positive finite number, got {sigma!r}")
    return float(sigma)


def filter_tables(radius, sigma_space=None, sigma_color=None, channels=3):
    """(space_table, color_table): the two uint32 weight tables of filter_flow, on the host.

    space_table[(dy+r)(2r+1) + (dx+r)] = rint(65535 exp(-(dx^2 + dy^2) / (2 sigma_space^2))), pixels;
    color_table[d] = rint(65535 exp(-(d / channels) / sigma_color)) for d = 0 .. 255 channels, the sum over the channels of the
    absolute byte differences, so that sigma_color is in grey levels per channel.  None gives 65535 everywhere: a box window, or
    no colour term.  float64 numpy arithmetic, rint to even."""
    r = _check_radius(radius)
    sigma_space = _check_sigma(sigma_space, "sigma_space")
    sigma_color = _check_sigma(sigma_color, "sigma_color")
    if channels not in (1, 3):
        raise ValueError(f"channels: expected 1 or 3, got {channels!r}")
    d = np.arange(-r, r + 1, dtype=np.float64)
    d2 = (d[:, None] ** 2 + d[None, :] ** 2).reshape(-1)
    if sigma_space is None:
        space = np.full(d2.shape, TABLE_MAX, np.uint32)
    else:
        space = np.rint(65535.0 * np.exp(-d2 / (2.0 * sigma_space * sigma_space))).astype(np.uint32)
    k = np.arange(255 * channels + 1, dtype=np.float64)
    if sigma_color is None:
        color = np.full(k.shape, TABLE_MAX, np.uint32)
    else:
        color = np.rint(65535.0 * np.exp(-(k / float(channels)) / sigma_color)).astype(np.uint32)
    return space, color


def _check_table(t, what, length):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    t = np.asarray(t)
    if t.dtype.kind not in "iu":
        raise TypeError(f"{what}: expected an integer table, got dtype {t.dtype}")
    if t.shape != (length,):
        raise ValueError(f"{what}: expected {length} entries, got shape {t.shape}")
    if t.size and (int(t.min()) < 0 or int(t.max()) > TABLE_MAX):
        raise ValueError(f"{what}: entries must be in 0 .. {TABLE_MAX} (a weight is the 32-bit product of two), got "
                         f"{int(t.min())} .. {int(t.max())}")
    return np.ascontiguousarray(t.astype(np.uint32))


def _check_guide(guide, N, H, W):
    if guide is None:
        return 0
    if not isinstance(guide, torch.Tensor) or guide.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"guide: expected a torch.uint8 or torch.float32 tensor, got "
                        f"{guide.dtype if isinstance(guide, torch.Tensor) else type(guide)}")
    if guide.dim() != 4 or tuple(guide.shape[:3]) != (N, H, W) or guide.shape[3] not in (1, 3):
        raise ValueError(f"guide: expected shape {(N, H, W)} + (1 or 3,), the flows' (N, H, W), got {tuple(guide.shape)}")
    return int(guide.shape[3])


def filter_flow(flows, guide=None, valid=None, radius=2, sigma_space=None, sigma_color=None, tables=None, smooth=True, fill=False,
                min_count=1, iters=1):
    """(flows_out (N,H,W,2) float32, valid_out (N,H,W) torch.bool): the weighted median of every pixel's window
    (pwc_flow_filter_f32: one launch per pass on the current stream, no host synchronisation).

    flows: (N,H,W,2) float32 in pixels, on the GPU; a channel slice of a wider buffer is read in place; read detached.  valid:
    (N,H,W) torch.bool / torch.uint8, contiguous, None = every pixel; a pixel whose flow fails flow_io.flow_valid's rule (a NaN,
    an Inf, the sentinel 1e10) is unknown as well.  guide: (N,H,W,1 or 3) torch.uint8, or float32 in [0, 1] (taken to bytes:
    rint(255 v), clamped, a NaN is 0), usually the first frame; None = no colour term.  radius: 1 .. 7.
    sigma_space (pixels), sigma_color (grey levels per channel): filter_tables' arguments, None = a box / no colour term;
    tables = (space_table, color_table) gives the integer weights directly (entries 0 .. 65535, checked here) and the sigmas
    must then be None.  The candidates of a pixel are the KNOWN pixels of its window inside the frame whose weight
    space_table[offset] * color_table[sum_c |guide difference|] is not zero; nothing is replicated beyond the border.
    smooth: a known pixel becomes the median of its candidates (itself among them).  fill: an unknown pixel with at least
    min_count candidates becomes their median and known.  Every other known pixel keeps its bits, every other unknown pixel is
    (1e10, 1e10) and False in valid_out.  iters passes, each on the result of the one before: a hole wider than radius closes from
    its rim inwards.  The median is the lower weighted median per component under a total order of the floats (-0 < +0); the
    output holds the bits of an input value.  An image's result does not depend on its neighbours in the batch; two calls give
    the same bits.  radius = 2 is an untuned choice.  No autograd."""
    _check_nhwc(flows, "flows", (2,))
    N, H, W, _ = flows.shape
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"flows: empty tensor, shape {tuple(flows.shape)}")
    _check_mask(valid, "valid", N, H, W)
    C = _check_guide(guide, N, H, W)
    r = _check_radius(radius)
    if not smooth and not fill:
        raise ValueError("smooth, fill: at least one of them must be set")
    for what, v in (("min_count", min_count), ("iters", iters)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{what}: expected an integer >= 1, got {v!r}")
    if tables is not None:
        if sigma_space is not None or sigma_color is not None:
            raise ValueError("tables: give either the tables or the sigmas, not both")
        if not isinstance(tables, (tuple, list)) or len(tables) != 2:
            raise ValueError("tables: expected (space_table, color_table)")
        space = _check_table(tables[0], "tables[0]", (2 * r + 1) ** 2)
        color = None if tables[1] is None and C == 0 else _check_table(tables[1], "tables[1]", 255 * max(C, 1) + 1)
    else:
        space, color = filter_tables(r, sigma_space, sigma_color, max(C, 1))
    _check_device(flows, flows=flows, valid=valid, guide=guide)
    fv, flows = as_view(flows.detach(), "flows")
    dev = flows.device
    if guide is not None:
        guide = guide.detach().contiguous()
    space_d = torch.from_numpy(space.view(np.int32)).to(dev)
    color_d = None if color is None or C == 0 else torch.from_numpy(color.view(np.int32)).to(dev)
    L = _lib.lib()
    nbytes = L.pwc_flow_filter_workspace_bytes(N, H, W, int(iters))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev) if nbytes else None
    out = torch.empty((N, H, W, 2), dtype=torch.float32, device=dev)
    out_valid = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    dtype = _lib.FLOW_FILTER_F32 if guide is not None and guide.dtype == torch.float32 else _lib.FLOW_FILTER_U8
    _lib.check(L.pwc_flow_filter_f32(_p(fv.ptr), fv.cs, _ptr(valid), _ptr(guide), dtype, max(C, 1), N, H, W, r,
                                     _p(space_d.data_ptr()), _ptr(color_d), 1 if smooth else 0, 1 if fill else 0, int(min_count),
                                     int(iters), _ptr(ws), nbytes, _p(out.data_ptr()), 2, _p(out_valid.data_ptr()),
                                     _lib.current_stream()), "filter flow")
    return out, out_valid.view(torch.bool)


def fill_flow(flows, valid=None, guide=None, radius=2, sigma_space=None, sigma_color=None, tables=None, min_count=1, iters=None):
    """filter_flow(smooth=False, fill=True): the known pixels keep their bits, the unknown ones are filled from their known
    neighbours, the rim of a hole first.

    iters: the number of passes, the caller's to give -- nothing is read back from the device to decide it.  A pass closes at
    least `radius` pixels of a hole's rim wherever the weights are not zero, so None means ceil(max(H, W) / radius), the count
    that closes any hole of a frame with at least one known pixel (box tables, min_count = 1); a caller who knows the holes are
    narrow should give a small count -- every pass is a launch over the whole frame."""
    if iters is None:
        _check_nhwc(flows, "flows", (2,))
        iters = max(1, -(-max(flows.shape[1], flows.shape[2]) // _check_radius(radius)))
    return filter_flow(flows, guide=guide, valid=valid, radius=radius, sigma_space=sigma_space, sigma_color=sigma_color,
                       tables=tables, smooth=False, fill=True, min_count=min_count, iters=iters)
