"""Region tracking on the HIP path: the join between the label images of consecutive pairs (csrc/pwc_region_links.hip).

    link_regions(labels_a, labels_b, flows_ab, area_a, area_b, valid=None, min_overlap=1, min_fraction=0.0)
        -> {"succ", "pred", "best_succ", "best_pred": (N,R) int32, "votes": (N,R,4) int32}
    region_identities(pred, count, state=None) -> (ids (S,R) int32, age (S,R) int32, state)
    relabel_regions(labels, ids) -> (S,H,W) int32
    track_regions(labels, count, regions, flows, valid=None, state=None, min_overlap=1, min_fraction=0.0)
        -> (ids (S,R), age (S,R), links, state)

label_regions' ids are per image.  A region a of one image is LINKED to the region b of the next where most of a's pixels land on
b under the flow between them, most of what lands on b comes from a, and the overlap passes the two thresholds; an identity is
carried along links and is fresh where there is none.  The result is a function of the input alone, and a sequence fed in
batches through `state` gives the bits of one call.  The definition is in include/pwc_hip.h, "region tracking"; the kernels equal
its numpy restatement bit for bit (tests/region_links_ref.py).  No host synchronisation.  No autograd.
"""
import math

import numpy as np
import torch

from . import _lib
from .interp import _check_mask
from .modules import _p, as_view
from .motion import _check_device, _ptr
from .regions import _check_int
from .unsup import _check_nhwc

MAX_REGIONS = _lib.LINKS_MAX_REGIONS
_ID_LIMIT = 1 << 31


def _check_i32(t, what, shape=None, dims=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{what}: expected a torch.int32 tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t)}")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{what}: expected a {dims}-D tensor, got shape {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if min(t.shape, default=1) < 1:
        raise ValueError(f"{what}: empty tensor, shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: the tensor must be contiguous")


def _check_rows(R, what):
    if R > MAX_REGIONS:
        raise ValueError(f"{what}: expected at most {MAX_REGIONS} table rows (max_regions), got {R}")


def _check_thresholds(min_overlap, min_fraction):
    min_overlap = _check_int(min_overlap, "min_overlap", 1)
    if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float)) or not math.isfinite(min_fraction) \
            or not 0.0 <= min_fraction <= 1.0:
        raise ValueError(f"min_fraction: expected a number in [0, 1], got {min_fraction!r}")
    return min_overlap, float(min_fraction)


def link_regions(labels_a, labels_b, flows_ab, area_a, area_b, valid=None, min_overlap=1, min_fraction=0.0):
    """{"succ", "pred", "best_succ", "best_pred": (N,R) torch.int32, "votes": (N,R,4) torch.int32}: for N independent pairs of
    label images, which region of b every region of a becomes (pwc_link_regions, five launches).

    labels_a, labels_b: (N,H,W) int32, label_regions' ids (any value is legal: ids outside 1 .. R do not vote, and count as
    background where a vote lands on them).  area_a, area_b: (N,R) int32, label_regions' "area" tables; R <= 1024.  flows_ab:
    (N,H,W,2) float32, frame a -> frame b in pixels (a channel slice of a wider buffer is read in place; read detached).  valid:
    (N,H,W) torch.bool / torch.uint8, contiguous, None = every pixel.
    Every pixel of a region a whose flow is known votes for the region of b at its rounded target (ties to even), or for "left
    the frame".  best_succ[a-1] is the b with the most votes of a's, best_pred[b-1] the a with the most votes for b, ties to
    the smaller id, 0 for none.  succ[a-1] = b and pred[b-1] = a where the two agree, the overlap is at least min_overlap
    pixels and at least min_fraction of the smaller of the two areas; 0 elsewhere.  votes[a-1] = (the overlap with
    best_succ, landed on no region, left the frame, all voters of a).  A split shows as several b with one best_pred, a merge as
    several a with one best_succ; only the mutual pair is a link.  min_overlap = 1 and min_fraction = 0 are untuned defaults.
    No autograd."""
    _check_i32(labels_a, "labels_a", dims=3)
    N, H, W = labels_a.shape
    _check_i32(labels_b, "labels_b", shape=(N, H, W))
    _check_nhwc(flows_ab, "flows_ab", (2,))
    if tuple(flows_ab.shape[:3]) != (N, H, W):
        raise ValueError(f"flows_ab: expected (N,H,W) {(N, H, W)}, the labels', got {tuple(flows_ab.shape[:3])}")
    _check_i32(area_a, "area_a", dims=2)
    if area_a.shape[0] != N:
        raise ValueError(f"area_a: expected {N} rows of areas, one per image, got shape {tuple(area_a.shape)}")
    R = area_a.shape[1]
    _check_rows(R, "area_a")
    _check_i32(area_b, "area_b", shape=(N, R))
    _check_mask(valid, "valid", N, H, W)
    min_overlap, min_fraction = _check_thresholds(min_overlap, min_fraction)
    _check_device(labels_a, labels_a=labels_a, labels_b=labels_b, flows_ab=flows_ab, area_a=area_a, area_b=area_b, valid=valid)
    dev = labels_a.device
    fv, flows_ab = as_view(flows_ab.detach(), "flows_ab")
    L = _lib.lib()
    nbytes = L.pwc_region_links_workspace_bytes(N, R)
    if nbytes == 0:
        raise _lib.PwcHipError(f"link regions failed: a batch of {N} images with {R} table rows is beyond "
                               f"{_lib.REGIONS_MAX_IMAGES} images of {MAX_REGIONS} rows")
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    out = {k: torch.empty((N, R), dtype=torch.int32, device=dev) for k in ("succ", "pred", "best_succ", "best_pred")}
    out["votes"] = torch.empty((N, R, 4), dtype=torch.int32, device=dev)
    _lib.check(L.pwc_link_regions(_ptr(labels_a), _ptr(labels_b), _ptr(area_a), _ptr(area_b), _p(fv.ptr), fv.cs, _ptr(valid), N, H, W,
                                  R, min_overlap, min_fraction, _p(ws.data_ptr()), nbytes, _ptr(out["succ"]), _ptr(out["pred"]),
                                  _ptr(out["best_succ"]), _ptr(out["best_pred"]), _ptr(out["votes"]), _lib.current_stream()),
               "link regions")
    return out


def _check_state(state, R, keys):
    if not isinstance(state, dict) or any(k not in state for k in keys):
        raise TypeError(f"state: expected the state an earlier call returned (a dict with {', '.join(keys)}), got "
                        f"{sorted(state) if isinstance(state, dict) else type(state)}")
    _check_i32(state["ids"], "state['ids']", shape=(R,))
    _check_i32(state["age"], "state['age']", shape=(R,))
    _check_i32(state["next_id"], "state['next_id']", shape=(1,))
    bound = state["next_id_bound"]
    if isinstance(bound, bool) or not isinstance(bound, (int, np.integer)) or bound < 1:
        raise ValueError(f"state['next_id_bound']: expected an integer of at least 1, got {bound!r}")


def region_identities(pred, count, state=None):
    """(ids (S,R) torch.int32, age (S,R) torch.int32, state): identities for the regions of S consecutive label images, carried
    along links (pwc_region_identities, one launch).

    count: (S,) int32, label_regions' counts.  pred: (S-1,R) int32, link_regions' "pred" of the links s-1 -> s ((0,R) for one image
    without a state); with `state`, (S,R): its first row is the link from the earlier call's last image to
    image 0.  Row b-1 of image s, for b up to min(count[s], R), takes the identity of region pred[b-1] of the image before and
    its age + 1, or, where that is 0, the next fresh identity (in ascending b) and age 1; the other rows hold 0.  Identities
    start at 1 and are never used twice.  state: None, or what an earlier call returned -- {"ids": (R,), "age": (R,), "next_id":
    (1,) int32 on the device, "next_id_bound": int}; the pieces of a sequence then equal one call, bit for bit, and nothing
    is copied to the host (next_id_bound counts every row as fresh: it is what the 31-bit range is checked with).
    No autograd."""
    _check_i32(count, "count", dims=1)
    S = count.shape[0]
    links = S - 1 if state is None else S
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.int32:
        raise TypeError(f"pred: expected a torch.int32 tensor ((0, R) for one image without a state), got "
                        f"{pred.dtype if isinstance(pred, torch.Tensor) else type(pred)}")
    if pred.dim() != 2 or pred.shape[0] != links or pred.shape[1] < 1 or not pred.is_contiguous():
        raise ValueError(f"pred: expected a contiguous ({links}, R) tensor of links for {S} images"
                         f"{' and a state' if state is not None else ''}, got shape {tuple(pred.shape)}")
    R = pred.shape[1]
    _check_rows(R, "pred")
    if state is not None:
        _check_state(state, R, ("ids", "age", "next_id", "next_id_bound"))
    bound = 1 if state is None else int(state["next_id_bound"])
    if bound + S * R >= _ID_LIMIT:
        raise ValueError(f"state['next_id_bound']: {bound} + {S} x {R} identities do not fit 31 bits")
    others = dict(pred=pred) if state is None else dict(pred=pred, **{f"state['{k}']": state[k] for k in ("ids", "age", "next_id")})
    _check_device(count, count=count, **others)
    dev = count.device
    ids = torch.empty((S, R), dtype=torch.int32, device=dev)
    age = torch.empty((S, R), dtype=torch.int32, device=dev)
    next_id = torch.empty((1,), dtype=torch.int32, device=dev)
    if state is None:
        link, prev = (pred if S > 1 else None), (None, None, None, None)
    else:
        link, prev = (pred[1:] if S > 1 else None), (state["ids"], state["age"], pred[0], state["next_id"])
    _lib.check(_lib.lib().pwc_region_identities(_ptr(link), _ptr(count), _ptr(prev[0]), _ptr(prev[1]), _ptr(prev[2]), bound,
                                                _ptr(prev[3]), S, R, _ptr(ids), _ptr(age), _ptr(next_id), _lib.current_stream()),
               "region identities")
    return ids, age, {"ids": ids[-1].clone(), "age": age[-1].clone(), "next_id": next_id, "next_id_bound": bound + S * R}


def relabel_regions(labels, ids):
    """(S,H,W) torch.int32: every label image painted with its regions' identities -- out = ids[s, la-1] where la = labels[s]
    is in 1 .. R, 0 elsewhere (pwc_relabel_regions, one launch).  labels: (S,H,W) int32; ids: (S,R) int32, R <= 1024."""
    _check_i32(labels, "labels", dims=3)
    S, H, W = labels.shape
    _check_i32(ids, "ids", dims=2)
    if ids.shape[0] != S:
        raise ValueError(f"ids: expected {S} rows, one per label image, got shape {tuple(ids.shape)}")
    R = ids.shape[1]
    _check_rows(R, "ids")
    _check_device(labels, labels=labels, ids=ids)
    out = torch.empty_like(labels)
    _lib.check(_lib.lib().pwc_relabel_regions(_ptr(labels), _ptr(ids), S, H, W, R, _ptr(out), _lib.current_stream()),
               "relabel regions")
    return out


_TRACK_STATE = ("labels", "area", "count", "ids", "age", "flow", "valid", "next_id", "next_id_bound")


def track_regions(labels, count, regions, flows, valid=None, state=None, min_overlap=1, min_fraction=0.0):
    """(ids (S,R) torch.int32, age (S,R) torch.int32, links, state): identities for the regions of S consecutive pairs --
    link_regions on (labels[:-1], labels[1:], flows[:-1]) followed by region_identities, nothing in between.

    labels (S,H,W), count (S,), regions: what label_regions / moving_regions returned for the S pairs i -> i + 1 of a sequence
    (regions["area"]: (S,R) int32, R <= 1024); flows: (S,H,W,2) float32, ALL S flows, the ones the labels were made from (a
    channel slice is read in place); valid: (S,H,W) mask or None.  Image s lives in the pixels of frame s, and flows[s] says
    where they go in frame s + 1, where image s + 1 lives: flows[-1] links to the next call's image 0.
    state: None, or what an earlier call returned: clones of the last labels, area row, count, ids, ages, flows[-1] and
    valid[-1], and next_id.  The next call's image 0 is linked from them, so a sequence fed in batches gives the bits of one call
    (track_points' streaming contract).  links: link_regions' dictionary, S - 1 links without a state, S with one (the first
    from the earlier call's last image).  min_overlap, min_fraction: link_regions'.  ids[s, b-1] is the identity of region b
    of pair s, age how many consecutive pairs it has been seen in.  Nothing here re-identifies a region after a gap or judges
    tracking quality on real video.  No autograd."""
    _check_i32(labels, "labels", dims=3)
    S, H, W = labels.shape
    _check_i32(count, "count", shape=(S,))
    if not isinstance(regions, dict) or "area" not in regions:
        raise TypeError(f"regions: expected label_regions' dictionary with \"area\", got {type(regions)}")
    area = regions["area"]
    _check_i32(area, "regions['area']", dims=2)
    if area.shape[0] != S:
        raise ValueError(f"regions['area']: expected {S} rows of areas, one per image, got shape {tuple(area.shape)}")
    R = area.shape[1]
    _check_rows(R, "regions['area']")
    _check_nhwc(flows, "flows", (2,))
    if tuple(flows.shape[:3]) != (S, H, W):
        raise ValueError(f"flows: expected (N,H,W) {(S, H, W)}, the labels', got {tuple(flows.shape[:3])}")
    _check_mask(valid, "valid", S, H, W)
    _check_thresholds(min_overlap, min_fraction)
    if state is not None:
        _check_state(state, R, _TRACK_STATE)
        if tuple(state["labels"].shape) != (H, W):
            raise ValueError(f"state['labels']: expected shape {(H, W)}, the labels', got {tuple(state['labels'].shape)}")
    _check_device(labels, labels=labels, count=count, flows=flows, valid=valid, **{"regions['area']": area})
    flows = flows.detach()
    if state is None:
        la, lb, fa, aa, ab, va = labels[:-1], labels[1:], flows[:-1], area[:-1], area[1:], None if valid is None else valid[:-1]
    else:
        _check_device(labels, **{f"state['{k}']": state[k] for k in _TRACK_STATE[:7]})
        la, lb = torch.cat([state["labels"][None], labels[:-1]]), labels
        fa = torch.cat([state["flow"][None], flows[:-1]])
        aa, ab = torch.cat([state["area"][None], area[:-1]]), area
        va = None
        if valid is not None or state["valid"] is not None:
            ones = lambda *shape: torch.ones(shape, dtype=torch.uint8, device=labels.device)       # noqa: E731
            head = state["valid"] if state["valid"] is not None else ones(H, W)
            tail = valid[:-1] if valid is not None else ones(S - 1, H, W)
            va = torch.cat([head[None].to(torch.uint8), tail.to(torch.uint8)])
    if la.shape[0] > 0:
        links = link_regions(la.contiguous(), lb.contiguous(), fa, aa.contiguous(), ab.contiguous(),
                             valid=None if va is None else va.contiguous(), min_overlap=min_overlap, min_fraction=min_fraction)
    else:
        links = {k: torch.empty((0, R), dtype=torch.int32, device=labels.device) for k in ("succ", "pred", "best_succ", "best_pred")}
        links["votes"] = torch.empty((0, R, 4), dtype=torch.int32, device=labels.device)
    ids, age, ident = region_identities(links["pred"], count, None if state is None else {k: state[k] for k in
                                                                                           ("ids", "age", "next_id", "next_id_bound")})
    ident.update(labels=labels[-1].clone(), area=area[-1].clone(), count=count[-1:].clone(), flow=flows[-1].clone(),
                 valid=None if valid is None else valid[-1].clone())
    return ids, age, links, ident
