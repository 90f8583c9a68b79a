"""Pins the bits of the loss, loss-gradient and metric kernels: the norm sums and gradient (plain and masked), the photometric
and smoothness sums and gradients, the flow metrics.

Their numerics are contracts -- the partition of an image into at most 256 parts, the fixed tree a workgroup adds in, the parts
added in index order, the nearest-neighbour index from a rounded product, the ground truth divided, the plain / accumulate
store -- so the comparison is exact equality with a recording, no tolerance.  The recording (tests/golden/loss_bits.json.gz) is
written by tests/golden/make_loss_bits_golden.py from a library known to be right and only re-recorded on purpose (a deliberate
change of arithmetic).  Inputs are rebuilt here from numpy.random.RandomState with fixed seeds.  Sums are compared as uint32 /
int32 bit patterns (the metrics' doubles as uint64), gradients as the SHA-256 of the whole destination buffer -- the padding
channels of the strided records included -- with the first values kept beside it for diagnosis.

Shapes (N, H, W): one pixel; 255 pixels (one ragged part); three parts, the last ragged; 257 x 256 (the 256-part cap is reached
and the second grid-stride trip is ragged); for the gradients also 513 x 1025, just over 4096 workgroups of 256 pixels, so
that their grid-stride loop takes a second trip.  The norm kernels see every shape with a ground truth of its own size and
with one of (4H+1, 4W+3): the floor of the index and its clip at GH - 1 both act.  Every record is strided."""
import gzip
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_grad_ops import _wide

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_bits.json.gz")

SUM_SHAPES = [(1, 1, 1), (2, 15, 17), (3, 17, 31), (2, 257, 256)]
BIG = (2, 513, 1025)
GRAD_SHAPES = SUM_SHAPES + [BIG]
EPS, Q, ALPHA, FLOW_SCALE = 0.01, 0.45, 10.0, 1.25


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(t):
    """The values of a float32 / int32 / float64 tensor as integers holding their bit patterns."""
    a = t.detach().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).reshape(-1).tolist() if a.dtype.kind == "f" \
        else a.reshape(-1).tolist()


def _digest(buf):
    """A gradient's whole destination buffer: SHA-256 of its bytes and the bits of its first 16 floats."""
    torch.cuda.synchronize()
    a = np.ascontiguousarray(buf.cpu().numpy())
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "head": a.reshape(-1)[:16].view(np.uint32).tolist()}


def _dest(N, H, W, rs):
    """A strided gradient destination: channels 4, 5 of 8-float records, every float of the buffer non-zero."""
    buf, view = _wide(_gpu(rs.uniform(-0.1, 0.1, (N, H, W, 2))), 8, 4)
    buf[..., :4] = 5.0
    buf[..., 6:] = -5.0
    return buf, view


def _masks(N, H, W, valid):
    """About half valid; at (2, 15, 17) also with an image that has no valid pixel."""
    out = {"half": torch.from_numpy(valid).cuda()}
    if (N, H, W) == (2, 15, 17):
        empty = valid.copy()
        empty[1] = False
        out["empty1"] = torch.from_numpy(empty).cuda()
    return out


# ------------------------------------------------------------------ norm sums and gradient
def _norm_inputs(N, H, W, big):
    GH, GW = (4 * H + 1, 4 * W + 3) if big else (H, W)
    rs = _rs("norm", N, H, W, big)
    gt = rs.uniform(-60, 60, (N, GH, GW, 2)).astype(np.float32)
    pred = rs.uniform(-3, 3, (N, H, W, 2)).astype(np.float32)
    pred[0, 0, 0] = gt[0, 0, 0] / np.float32(20.0)                # a zero difference
    valid = rs.uniform(size=(N, GH, GW)) < 0.5
    wgt, vgt = _wide(_gpu(gt), 4, 1)
    wp, vp = _wide(_gpu(pred), 6, 2)
    return (wgt, vgt), (wp, vp), _masks(N, H, W, valid)


def _norm_sums(N, H, W, big):
    from pwcnet_amd import losses
    (wgt, _), (wp, _), masks = _norm_inputs(N, H, W, big)
    out = {}
    for order in (1, 2):
        out[f"plain/ord{order}"] = _bits(losses._norm_sums(wp[..., 2:4], wgt[..., 1:3], order, gt_div=20.0)[0])
        for name, m in masks.items():
            sums, _, counts = losses._norm_sums(wp[..., 2:4], wgt[..., 1:3], order, gt_div=20.0, valid=m)
            out[f"masked/{name}/ord{order}"] = [_bits(sums), _bits(counts)]
    return out


def _norm_grad(N, H, W, big):
    from pwcnet_amd import grad_ops
    (wgt, vgt), (wp, vp), masks = _norm_inputs(N, H, W, big)      # (a view is an address: wgt, wp keep the memory)
    out = {}
    for order in (1, 2):
        for name, m in [("plain", None)] + [(f"masked/{k}", v) for k, v in masks.items()]:
            for acc in (False, True):
                buf, vd = _dest(N, H, W, _rs("norm dest", N, H, W))
                grad_ops.flow_norm_grad(vp, vgt, vd, gt_div=20.0, ord=order, scale=0.16, accumulate=acc, valid=m)
                out[f"{name}/ord{order}/{'acc' if acc else 'set'}"] = _digest(buf)
    return out


# ------------------------------------------------------------------ photometric and smoothness terms
def _unsup_inputs(N, H, W, C):
    rs = _rs("unsup", N, H, W, C)
    flows = rs.uniform(-3, 3, (N, H, W, 2)).astype(np.float32)
    flows[0, 0, 0] = 0.0                                             # a sample point on a pixel, inside the frame
    wf, _ = _wide(_gpu(flows), 5, 2)
    ims = [_wide(_gpu(rs.uniform(0, 1, (N, H, W, C))), C + 2, 1)[0][..., 1:1 + C] for _ in range(2)]
    valid = torch.from_numpy(rs.uniform(size=(N, H, W)) < 0.5).cuda()
    dsums = _gpu(rs.uniform(-2, 2, (N,)))
    return wf[..., 2:4], ims, valid, dsums


def _photo_sums(N, H, W):
    from pwcnet_amd import unsup
    out = {}
    for C in (1, 3, 4):
        flows, (im0, im1), valid, _ = _unsup_inputs(N, H, W, C)
        for name, m in (("all", None), ("valid", valid)):
            sums, counts = unsup.photometric_sums(im0, im1, flows, FLOW_SCALE, m, EPS, Q)
            out[f"c{C}/{name}"] = [_bits(sums), _bits(counts)]
    return out


def _photo_grad(N, H, W):
    from pwcnet_amd import unsup
    out = {}
    for C in (1, 3, 4):
        flows, (im0, im1), valid, dsums = _unsup_inputs(N, H, W, C)
        for name, m in (("all", None), ("valid", valid)):
            for acc in (False, True):
                buf, _ = _dest(N, H, W, _rs("photo dest", N, H, W))
                unsup.photometric_grad(im0, im1, flows, dsums, buf[..., 4:6], FLOW_SCALE, m, EPS, Q, accumulate=acc)
                out[f"c{C}/{name}/{'acc' if acc else 'set'}"] = _digest(buf)
    return out


def _smooth_sums(N, H, W):
    from pwcnet_amd import unsup
    flows, (im0, _), _, _ = _unsup_inputs(N, H, W, 3)
    return {name: _bits(unsup.smoothness_sums(flows, im, ALPHA, EPS, Q)) for name, im in (("no image", None), ("c3", im0))}


def _smooth_grad(N, H, W):
    from pwcnet_amd import unsup
    flows, (im0, _), _, dsums = _unsup_inputs(N, H, W, 3)
    out = {}
    for name, im in (("no image", None), ("c3", im0)):
        for acc in (False, True):
            buf, _ = _dest(N, H, W, _rs("smooth dest", N, H, W))
            unsup.smoothness_grad(flows, dsums, buf[..., 4:6], im, ALPHA, EPS, Q, accumulate=acc)
            out[f"{name}/{'acc' if acc else 'set'}"] = _digest(buf)
    return out


# ------------------------------------------------------------------ metrics
def _metrics(N, H, W):
    from pwcnet_amd import losses
    rs = _rs("metrics", N, H, W)
    gt = rs.uniform(-60, 60, (N, H, W, 2)).astype(np.float32)
    pred = gt + rs.uniform(-6, 6, (N, H, W, 2)).astype(np.float32)
    valid = rs.uniform(size=(N, H, W)) < 0.5
    wg, _ = _wide(_gpu(gt), 5, 3)
    wp, _ = _wide(_gpu(pred), 4, 1)
    out = {"all": _bits(losses.flow_metrics(wg[..., 3:5], wp[..., 1:3], None))}
    for name, m in _masks(N, H, W, valid).items():
        out[f"valid/{name}"] = _bits(losses.flow_metrics(wg[..., 3:5], wp[..., 1:3], m))
    return out


def _name(kind, shape, *more):
    return "/".join([kind, "x".join(str(v) for v in shape), *more])


CASES = {}
for _s in SUM_SHAPES:
    for _big in (False, True):
        CASES[_name("norm_sums", _s, "gt4x" if _big else "gt1x")] = (_norm_sums, (*_s, _big))
    CASES[_name("photometric_sums", _s)] = (_photo_sums, _s)
    CASES[_name("smoothness_sums", _s)] = (_smooth_sums, _s)
    CASES[_name("metrics", _s)] = (_metrics, _s)
for _s in GRAD_SHAPES:
    for _big in (False, True):
        if not (_big and _s == BIG):                 # (a 4x ground truth of the largest shape would be 270 MB)
            CASES[_name("norm_grad", _s, "gt4x" if _big else "gt1x")] = (_norm_grad, (*_s, _big))
    CASES[_name("photometric_grad", _s)] = (_photo_grad, _s)
    CASES[_name("smoothness_grad", _s)] = (_smooth_grad, _s)


def record(case):
    """What the library computes for a case, JSON-ready."""
    fn, args = CASES[case]
    return json.loads(json.dumps(fn(*args)))


@pytest.fixture(scope="module")
def golden():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    with gzip.open(FIXTURE, "rb") as f:
        return json.loads(f.read().decode())


def test_the_recording_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_loss_kernel_bits(golden, case):
    got, exp = record(case), golden[case]
    assert sorted(got) == sorted(exp), (sorted(got), sorted(exp))
    bad = {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]}
    for k, (g, e) in bad.items():
        print(f"{case} {k}: got {g} recorded {e}")
    assert not bad, f"{case}: {sorted(bad)} differ from the recording"
