"""Moving regions on the HIP path: the connected components of a mask, numbered, with their areas, boxes and mean flows
(csrc/pwc_regions.hip).

    label_regions(mask, connectivity=8, min_area=1, max_regions=256, flows=None, invert=False)
        -> (labels (N,H,W) int32, count (N,) int32, {"area": (N,R) int32, "box": (N,R,4) int32, "mean": (N,R,2) float64 or None})
    moving_regions(flows, matrices, valid=None, threshold=3.0, **label_kw)
        -> (labels, count, regions, residual, inlier)

A component's id is its rank among the kept components of its image in raster order of their first pixel, so the result is a
function of the input alone: two calls give the same bits and an image's result does not depend on its neighbours in the batch.
The definition is in include/pwc_hip.h, "moving regions"; the kernels equal its numpy restatement bit for bit
(tests/regions_ref.py).  Ten launches on the current stream, no host synchronisation.  No autograd.
"""
import numpy as np
import torch

from . import _lib
from .interp import _check_mask
from .modules import _p, as_view
from .motion import _check_device, _ptr, motion_residual
from .unsup import _check_nhwc

MAX_REGIONS = _lib.REGIONS_MAX_REGIONS


def tile_shape():
    """(th, tw): the tile the first launch labels in the LDS; components that cross its seams are joined by the second."""
    L = _lib.lib()
    return L.pwc_regions_tile_h(), L.pwc_regions_tile_w()


def _check_int(value, what, lo, hi=None):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
        bound = f"in {lo} .. {hi}" if hi is not None else f"of at least {lo}"
        raise ValueError(f"{what}: expected an integer {bound}, got {value!r}")
    return int(value)


def label_regions(mask, connectivity=8, min_area=1, max_regions=256, flows=None, invert=False):
    """(labels (N,H,W) torch.int32, count (N,) torch.int32, regions): the connected components of every mask of a batch
    (pwc_label_regions).

    mask: (N,H,W) torch.bool / torch.uint8, contiguous, on the GPU; foreground where it is non-zero (invert=True: where it is
    zero).  flows: None or (N,H,W,2) float32 in pixels (a channel slice of a wider buffer is read in place; read detached): a
    pixel whose flow fails flow_io.flow_valid's rule is background as well, and the regions get their mean flow.  connectivity:
    4 (shared edges) or 8 (edges or corners); never across images.  min_area: components with fewer pixels are dropped (their
    pixels get label 0).  max_regions: R, the rows of the tables, 1 .. 65535.
    labels holds the id of every pixel's component, 1 .. K in raster order of the components' first pixels, 0 for background;
    count[n] = K, the true number even where K > R.  regions: {"area": (N,R) int32, "box": (N,R,4) int32 x0 y0 x1 y1 inclusive,
    "mean": (N,R,2) float64 mean flow, or None without flows}, row id - 1 for the ids 1 .. min(K, R), zero elsewhere.  The mean
    is an exact integer sum of the flow in 1/65536 px (components clamped to +-65536 px) divided by the area; the dictionary also
    holds that sum, "sums": (N,R,2) int64 or None.  No autograd."""
    if mask is None:
        raise TypeError("mask: expected a torch.bool or torch.uint8 tensor, got None")
    if isinstance(mask, torch.Tensor) and mask.dim() != 3:
        raise ValueError(f"mask: expected an (N, H, W) tensor, got shape {tuple(mask.shape)}")
    if isinstance(mask, torch.Tensor) and min(mask.shape) < 1:
        raise ValueError(f"mask: empty tensor, shape {tuple(mask.shape)}")
    N, H, W = mask.shape if isinstance(mask, torch.Tensor) else (0, 0, 0)
    _check_mask(mask, "mask", N, H, W)
    if flows is not None:
        _check_nhwc(flows, "flows", (2,))
        if tuple(flows.shape[:3]) != (N, H, W):
            raise ValueError(f"flows: expected (N,H,W) {(N, H, W)}, the mask's, got {tuple(flows.shape[:3])}")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity: expected 4 or 8, got {connectivity!r}")
    min_area = _check_int(min_area, "min_area", 1)
    max_regions = _check_int(max_regions, "max_regions", 1, MAX_REGIONS)
    _check_device(mask, mask=mask, flows=flows)
    dev = mask.device
    fv = None
    if flows is not None:
        fv, flows = as_view(flows.detach(), "flows")
    L = _lib.lib()
    nbytes = L.pwc_regions_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise _lib.PwcHipError(f"label regions failed: a batch of {N} masks of {H} x {W} is beyond {_lib.REGIONS_MAX_IMAGES} "
                               f"images of {_lib.REGIONS_MAX_PIXELS} pixels")
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
    labels = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    area = torch.empty((N, max_regions), dtype=torch.int32, device=dev)
    box = torch.empty((N, max_regions, 4), dtype=torch.int32, device=dev)
    sums = mean = None
    if flows is not None:
        sums = torch.empty((N, max_regions, 2), dtype=torch.int64, device=dev)
        mean = torch.empty((N, max_regions, 2), dtype=torch.float64, device=dev)
    _lib.check(L.pwc_label_regions(_p(mask.data_ptr()), 1 if invert else 0, _p(fv.ptr) if fv is not None else None,
                                   fv.cs if fv is not None else 2, N, H, W, int(connectivity), min_area, max_regions,
                                   _p(ws.data_ptr()), nbytes, _p(labels.data_ptr()), _p(count.data_ptr()), _p(area.data_ptr()),
                                   _p(box.data_ptr()), _ptr(sums), _ptr(mean), _lib.current_stream()), "label regions")
    return labels, count, {"area": area, "box": box, "mean": mean, "sums": sums}


def moving_regions(flows, matrices, valid=None, threshold=3.0, projective=False, **label_kw):
    """(labels, count, regions, residual, inlier): what moves on its own, as objects -- motion_residual followed by
    label_regions(inlier, invert=True, flows=residual, ...), nothing in between.

    flows, matrices, valid, threshold, projective: motion_residual's (matrices are fit_motion's, or fit_homography's with
    projective=True).  label_kw: connectivity, min_area,
    max_regions of label_regions.  A region is a connected set of pixels whose flow is known and differs from the dominant motion
    by more than `threshold` px; unknown pixels hold 1e10 in the residual and fall out through the flow rule.  regions["mean"] is
    a region's mean motion RELATIVE to the camera, in pixels.  Nothing here judges segmentation quality on real video."""
    unknown = set(label_kw) - {"connectivity", "min_area", "max_regions"}
    if unknown:
        raise TypeError(f"moving_regions: unexpected keyword arguments {sorted(unknown)}")
    residual, inlier = motion_residual(flows, matrices, valid=valid, threshold=threshold, projective=projective)
    labels, count, regions = label_regions(inlier, flows=residual, invert=True, **label_kw)
    return labels, count, regions, residual, inlier
