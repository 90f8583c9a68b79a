"""GPU tests that take every capped, grid-strided launch PAST its cap: the second trip of the stride loop is what runs at the
training and full-size configurations, and the per-kernel tests stay below the caps.

The caps, read from pwcnet_amd/csrc (unit = what one lane takes per trip; "largest before" = the largest count a test outside
this module hands the launch, as far as its shapes were traced; "here" = the case of this module that crosses the cap):

  launch (source)                                    cap                    largest before        here
  -------------------------------------------------  ---------------------  --------------------  ---------------------------------
  loss-gradient gathers, pwc_loss_grad_blocks (loss_common.h): 4096 workgroups x 256 lanes = 1 048 576 pixels of N*H*W
    photometric_grad              (pwc_unsup.hip)    1 048 576 px           2x384x448 = 344 064   5x448x480 = 1 075 200 [gathers]
    flow_smoothness_grad          (pwc_unsup.hip)    1 048 576 px           344 064               1 075 200 [gathers]
    flow_smoothness2_grad         (pwc_unsup.hip)    1 048 576 px           344 064               1 075 200 [gathers]
    census_grad (gather)          (pwc_census.hip)   1 048 576 px           344 064               1 075 200 [gathers]
    ssim_grad (gather)            (pwc_ssim.hip)     1 048 576 px           344 064               1 075 200 [gathers]
    fb_consistency_grad, grid.y 2 (pwc_fbcheck.hip)  1 048 576 px           344 064               1 075 200 [gathers]
    flow_norm_grad, masked or not (pwc_flow_loss.hip) 1 048 576 px          4x96x112 = 43 008     1 075 200 [flow_norm]
    flow_distill_grad             (pwc_distill.hip)  1 048 576 px           3x1x257               1 075 200 [distill]
    flow_compose, flow_compose_grad (scatter, finish) (pwc_compose.hip)  1 048 576 px  344 064  1 075 200 [compose]
    splat scatter / finish, splat_grad (pwc_splat.hip) 1 048 576 px           344 064               1 075 200 [splat]
  per-image partitions of the sums kernels and of fb_valid (pwc_loss_parts: 256 parts x 256 lanes = 65 536 pixels PER IMAGE, grid
    (parts, N)): crossed by the 272 x 256 cases of test_gpu_unsup.py, test_gpu_census.py, test_gpu_ssim.py, test_gpu_unflow.py and
    test_gpu_fbcheck.py::test_masks_and_counts_vs_float64; the census / ssim tile loops (tile += gridDim.x) by the same cases (272
    tiles for 256 parts).  fb_valid is not a pwc_loss_grad_blocks launch; it still gets a batch case here [fb_valid].
  lrelu_grad_kernel               (pwc_backward.hip) 8192 x 256 float4      2x5x7x4 = 280         4x96x112x49 = 2 107 392
  add_kernel                      (pwc_backward.hip) 8192 x 256 floats      (helper only)         4x48x56x196 = 2 107 392
  resize_bilinear_grad            (pwc_backward.hip) 8192 x 256             test_gpu_grad_ops.py::test_resize_grad_grid_stride
  adam_step                       (pwc_backward.hip) 8192 x 256             test_gpu_grad_ops.py::test_adam_step_sweep (5 000 003)
  channel_sums parts              (pwc_backward.hip) 2048 parts             test_gpu_grad_ops.py::test_channel_sums_sweep (524 289 px)
  warp_kernel, both kinds, +copy  (pwc_ops.hip)      65535 rows of N*H      8x112 = 896 (forward) 1x65601, 3x21900 = 65 700
  resize_kernel<4,2,1>, +status   (pwc_ops.hip)      65535 rows of N*OH     1x448 = 448           1x65604, 3x21868 = 65 604
  resize_pair_kernel              (pwc_ops.hip)      65535 rows of N*OH     8x112 = 896 (forward) 1x65604, 3x21868
  resize_x4_c2_kernel             (pwc_ops.hip)      none (one lane per source cell, no stride loop)
  resize_pair2x_kernel            (pwc_ops.hip)      16384 x 256 units      below the cap         520x480x17 = 4 243 200 [pair x2]
  copy_channels_kernel            (pwc_ops.hip)      4096 x 256 items       2x5x7x33 = 2310       180x180x33, 182x182x32 float4
  absmax_kernel                   (pwc_ops.hip)      2048 x 256 floats      (status test, small)  130x130x33 = 557 700
  flow_vis_tiles_kernel, runs of four pixels (pwc_flowvis.hip) 16384 x 256 runs  test_gpu_vis.py::test_more_runs_than_the_grid_has_lanes (8.4 M runs)
  fit_frames / refit_flow, fit_grid (pwc_fit.hip)    2048 x 256 quads/pairs 2x128x192/4 = 12 288  1x1088x2048: 557 056 quads, 1 050 600 pairs
  weight packing: conv_fp32_pack (conv_fp32_common.h: mfma 9, wino 16, wino4 36 positions), conv3x3_sk_pack, conv3x3_h2_pack and its
    stride-2 form: 4096 x 256 lanes; largest before 36x160x128 = 737 280; here 1 179 648 in each family [weight_packing].  There is
    no capped workspace-fill launch in these files: the stream-K workspaces are refilled from the host.
  warp_grad_fix_finish_kernel     (pwc_backward.hip) 8192 x 256 of N*H*W*C  4x96x112x32           3x96x112x68 = 2 193 408 [warp_grad_finish]
  conv3x3_head2_c32_kernel        (conv3x3_direct.hip) 2048 x 32 px         2x16x24               20x56x64 = 71 680 [flow_head_c32]
  conv3x3_smallcin_kernel<3,16>   (conv3x3_direct.hip) 8192 x 256 float4: only behind the matrix-pipe first layer, which takes every input
    below 2^31 bytes with at most 131 072 output columns; not reachable at a testable size.  NOT crossed.
  conv_fp32_split_reduce          (conv_fp32_common.h) 2048 x 256 float4 behind the tap split (conv3x3_mfma.hip), 4096 x 256 behind the
    channel split (conv3x3_wino.hip), of M * Cout / 4; largest before 1792 x 16 = 28 672 and 3584 x 32 = 114 688; here 688 128
    [tap_split_reduce] and 1 179 648 [channel_split_reduce]
  feature norm (pwc_featnorm.hip): parts kernels 256 x 256 groups of four values per frame, apply kernels 512 x 256; largest before
    64 x 96 x 32 / 4 = 49 152; here 147 456 (16-byte path) and 145 137 (scalar path) [feature_norm]
  cost_volume_roll_kernel         (cost_volume_roll.hip) 256 persistent workgroups over N * strips * segments work items:
    test_gpu_ops.py::test_cost_volume_rolling_kernel_full_size (16 x 112 x 256: 512 items)

What each group asserts is in the tests' docstrings.  The loss-gradient cases share ONE batch geometry, 5 x 448 x 480 (H != W: a
swapped / W and / H shows; one image, 215 040 pixels, stays under the cap; the last image's flat indices are all >= 860 160 and
its last 26 624 pixels are second-trip work): a complete overwrite of a NaN-filled output, bitwise equality with the call on each
image alone (the path the per-kernel tests pin to float64), the last image against the float64 restatement under the kernel's own
bound (`_grad_bound` of tests/test_gpu_unsup.py, `close` of tests/test_gpu_grad.py, distill's 2^-23 rule), strided views, accumulate.

pwc_add_f32 with accumulate is `*d + alpha * src`: observed on an MI355X as the two fp32 operations (no fma), so the tests ask for
equality with the same two operations in torch and need no 1-ulp allowance; they print how many elements differ.

Index width of the per-image sums loops (int pixel index stepped by up to 65536): refused on the host, tests/test_host_*.py; no GPU
test of a 2^31-pixel image is possible at sensible cost.

Still open: conv3x3_smallcin_kernel<3,16> only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import census_ref as cr
from tests import distill_ref as dr
from tests import fit_ref as fr
from tests import ssim_ref as sr
from tests import unflow_ref as uf
from tests import unsup_ref as ur
from tests.test_gpu_distill import _check_grad as _check_distill_grad
from tests.test_gpu_fit import judge as _fit_judge
from tests.test_gpu_grad import V, View, _rel_err, close, gpu, rnd
from tests.test_gpu_grad_ops import _outside, _wide
from tests.test_gpu_ops import close as close_oracle
from tests.test_gpu_unsup import _grad_bound

pytestmark = pytest.mark.gpu

N, H, W, C = 5, 448, 480, 3                 # 1 075 200 pixels against the gathers' 1 048 576; one image 215 040
LAST = N - 1
GRAD_CAP = 4096 * 256
FLOW_SCALE, EPS, Q = 5.0, 1e-3, 0.5
UPSTREAM = (0.75, -1.5, 1.25, -0.5, 2.0)    # the gradient that reaches sums[n]: per image, of both signs
UPSTREAM_BW = (-0.5, 1.25, -1.0, 0.625, -1.75)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")


@pytest.fixture(scope="module")
def us():
    _need_gpu()
    from pwcnet_amd import unsup
    return unsup


@pytest.fixture(scope="module")
def go():
    _need_gpu()
    from pwcnet_amd import grad_ops
    return grad_ops


@pytest.fixture(scope="module")
def pa():
    _need_gpu()
    import pwcnet_amd
    from pwcnet_amd import _lib
    _lib.lib()
    return pwcnet_amd


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ 2. loss-gradient gathers past 1 048 576 pixels
@functools.lru_cache(maxsize=None)
def _photo_case():
    """tests/unsup_ref.py's builder at the batch geometry: flows of up to 3 px on 16 x 16 tiles of which 13 % are thrown out of
    frame (so that whole SSIM windows stay in frame), a ~70 % mask."""
    assert N * H * W > GRAD_CAP > H * W and LAST * H * W < GRAD_CAP
    return ur.build_case(N=N, H=H, W=W, C=C, flow_scale=FLOW_SCALE, seed=11, block=16, far=0.13)


@functools.lru_cache(maxsize=None)
def _fb_case():
    return uf.build_case(N=N, H=H, W=W, flow_scale=FLOW_SCALE, seed=12, noise=0.5)


def _one(case, n, keys):
    """Image n of a case, as the restatements take it."""
    return {k: (None if case[k] is None else case[k][n:n + 1]) for k in keys}


def _t(a, dt):
    return torch.from_numpy(a).to(dt)


def _ref_photometric(dt):
    c = _one(_photo_case(), LAST, ("im0", "im1", "flow", "valid"))
    fl = _t(c["flow"], dt).requires_grad_(True)
    sums, _, contributing = ur.photometric_ref(_t(c["im0"], dt), _t(c["im1"], dt), fl, FLOW_SCALE, torch.from_numpy(c["valid"]), EPS, Q)
    (sums * UPSTREAM[LAST]).sum().backward()
    return [fl.grad], contributing


def _ref_smooth(dt, order, with_image):
    c = _one(_photo_case(), LAST, ("im0", "flow"))
    fl = _t(c["flow"], dt).requires_grad_(True)
    fn = ur.smoothness_ref if order == 1 else uf.smoothness2_ref
    sums = fn(fl, _t(c["im0"], dt) if with_image else None, ur.ALPHA, EPS, Q)
    (sums * UPSTREAM[LAST]).sum().backward()
    return [fl.grad], torch.ones((1, H, W), dtype=torch.bool)


def _ref_census(dt, radius, scale):
    c = _one(_photo_case(), LAST, ("im0", "im1", "flow", "valid"))
    fl = _t(c["flow"], dt).requires_grad_(True)
    sums, _, contributing = cr.census_ref(_t(c["im0"], dt), _t(c["im1"], dt), fl, FLOW_SCALE, torch.from_numpy(c["valid"]),
                                          radius=radius, scale=scale, **cr.CONSTS)
    (sums * UPSTREAM[LAST]).sum().backward()
    return [fl.grad], contributing


def _ref_ssim(dt, radius):
    c = _one(_photo_case(), LAST, ("im0", "im1", "flow", "valid"))
    fl = _t(c["flow"], dt).requires_grad_(True)
    sums, _, contributing = sr.ssim_ref(_t(c["im0"], dt), _t(c["im1"], dt), fl, FLOW_SCALE, torch.from_numpy(c["valid"]), radius)
    (sums * UPSTREAM[LAST]).sum().backward()
    return [fl.grad], contributing


def _ref_consistency(dt):
    c = _one(_fb_case(), LAST, ("fw", "bw", "valid_fw", "valid_bw"))
    out = uf.consistency_run(dict(c, flow_scale=FLOW_SCALE), EPS, Q, dt, upstream=((UPSTREAM[LAST],), (UPSTREAM_BW[LAST],)))
    lesser = out[2] if float(out[2].double().mean()) < float(out[5].double().mean()) else out[5]
    return [out[6], out[7]], lesser          # (the direction of which fewer pixels contribute)


# name -> the restatement of the last image in a dtype: (gradients, contributing pixels).  Settings: one or two of those the
# kernel's own test uses.
_REFS = {
    "photometric": lambda dt: _ref_photometric(dt),
    "smoothness": lambda dt: _ref_smooth(dt, 1, True),
    "smoothness_noimg": lambda dt: _ref_smooth(dt, 1, False),
    "smoothness2": lambda dt: _ref_smooth(dt, 2, True),
    "census_r3_k255": lambda dt: _ref_census(dt, 3, 255.0),
    "census_r1_k8": lambda dt: _ref_census(dt, 1, 8.0),
    "ssim_r1": lambda dt: _ref_ssim(dt, 1),
    "fb_consistency": lambda dt: _ref_consistency(dt),
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 gradients, float32 gradients, contributing share) of the LAST image alone -- computed once and shared."""
    g64, contributing = _REFS[name](torch.float64)
    g32, _ = _REFS[name](torch.float32)
    return g64, g32, float(contributing.double().mean())


class _Batch:
    """The batch on the GPU, once: every input a channel slice of a wider buffer (`_wide`, the outside channels zero)."""

    def __init__(self):
        c, f = _photo_case(), _fb_case()
        self.im0 = _wide(gpu(c["im0"]), C + 3, 2)[0][..., 2:2 + C]
        self.im1 = _wide(gpu(c["im1"]), C + 1, 1)[0][..., 1:1 + C]
        self.flow = _wide(gpu(c["flow"]), 6, 3)[0][..., 3:5]
        self.valid = torch.from_numpy(c["valid"]).cuda()
        self.fw = _wide(gpu(f["fw"]), 6, 3)[0][..., 3:5]
        self.bw = _wide(gpu(f["bw"]), 3, 1)[0][..., 1:3]
        self.valid_fw, self.valid_bw = torch.from_numpy(f["valid_fw"]).cuda(), torch.from_numpy(f["valid_bw"]).cuda()
        self.up = torch.tensor(UPSTREAM, dtype=torch.float32, device="cuda")
        self.up_bw = torch.tensor(UPSTREAM_BW, dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def batch(us):
    return _Batch()


def _call(us, b, name, s, outs, acc):
    """The gradient kernel of `name` on the images s (a slice) of the batch into outs (channel slices), accumulate or not."""
    if name == "photometric":
        us.photometric_grad(b.im0[s], b.im1[s], b.flow[s], b.up[s], outs[0], FLOW_SCALE, b.valid[s], EPS, Q, accumulate=acc)
    elif name.startswith("smoothness"):
        us.smoothness_grad(b.flow[s], b.up[s], outs[0], None if name.endswith("noimg") else b.im0[s], ur.ALPHA, EPS, Q,
                           accumulate=acc, order=2 if name == "smoothness2" else 1)
    elif name.startswith("census"):
        radius, scale = (3, 255.0) if name == "census_r3_k255" else (1, 8.0)
        us.census_grad(b.im0[s], b.im1[s], b.flow[s], b.up[s], outs[0], FLOW_SCALE, b.valid[s], radius=radius, scale=scale,
                       accumulate=acc, **cr.CONSTS)
    elif name.startswith("ssim"):
        us.ssim_grad(b.im0[s], b.im1[s], b.flow[s], b.up[s], outs[0], FLOW_SCALE, b.valid[s], radius=int(name[-1]), accumulate=acc)
    elif name == "fb_consistency":
        us.fb_consistency_grad(b.fw[s], b.bw[s], b.up[s], b.up_bw[s], outs[0], outs[1], FLOW_SCALE, b.valid_fw[s], b.valid_bw[s],
                               EPS, Q, accumulate=acc)
    else:
        raise ValueError(name)


def _nan_outputs(n_images, count):
    """`count` NaN-filled (n, H, W, 5) buffers and their channel slices 1:3, the gradients' destinations."""
    bufs = [torch.full((n_images, H, W, 5), float("nan"), device="cuda") for _ in range(count)]
    return bufs, [w[..., 1:3] for w in bufs]


@pytest.mark.parametrize("name", sorted(_REFS))
def test_loss_gradient_gather_past_the_grid_cap(us, batch, name):
    """5 x 448 x 480 pixels against the 1 048 576 of one pass.  (1) nothing of a NaN-filled destination survives a plain call and
    the channels beside it stay NaN; (2) image n of the batch is, bit for bit, the call on image n alone (under the cap); (3) the
    last image, whose flat indices are all in the fifth image and whose tail is second-trip work, meets the float64 restatement
    under the bound of the kernel's own test; (4) accumulate adds what the plain call writes.  The reference has to have
    something to say: at least half of that image's pixels contribute and its gradient is not zero."""
    g64, g32, share = _reference(name)
    print(f"{name}: {share:.3f} of the last image's pixels contribute; max |ref| {[float(g.abs().max()) for g in g64]}")
    assert share >= 0.5, share
    assert all(float(g.abs().max()) > 0 for g in g64)
    bufs, outs = _nan_outputs(N, len(g64))
    _call(us, batch, name, slice(None), outs, False)
    torch.cuda.synchronize()
    for w, o in zip(bufs, outs):
        assert not bool(torch.isnan(o).any()), "a pixel kept its sentinel"
        assert bool(torch.isnan(w[..., :1]).all()) and bool(torch.isnan(w[..., 3:]).all())
    for n in range(N):
        _, single = _nan_outputs(1, len(g64))
        _call(us, batch, name, slice(n, n + 1), single, False)
        for o, s1 in zip(outs, single):
            assert torch.equal(o[n:n + 1], s1), f"image {n} of the batch differs from the call on it alone"
    for what, o, r64, r32 in zip(("d/dflows", "d/dflows_bw"), outs, g64, g32):
        err, err32 = _rel_err(o[LAST:], r64), _rel_err(r32, r64)
        print(f"{name} {what}: last image rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {_grad_bound(err32):.3e}")
        assert err <= _grad_bound(err32)
    base = [gpu(rnd((N, H, W, 5), 90 + k)) for k in range(len(g64))]
    acc = [w.clone() for w in base]
    _call(us, batch, name, slice(None), [w[..., 1:3] for w in acc], True)
    torch.cuda.synchronize()
    for w, w0, o in zip(acc, base, outs):
        assert torch.equal(w[LAST, ..., 1:3], (w0[..., 1:3] + o)[LAST])
        assert torch.equal(w[..., :1], w0[..., :1]) and torch.equal(w[..., 3:], w0[..., 3:])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("masked", [False, True])
def test_flow_norm_grad_past_the_grid_cap(go, order, masked):
    """pwc_flow_norm_grad_f32 / pwc_flow_norm_masked_grad_f32 at 5 x 448 x 480 predictions under an 896 x 960 ground truth (the
    nearest-neighbour index at factor 2), ~30 % invalid: overwrite, per-image bits, the last image against float64 autograd
    under `close` (2e-5 of the largest reference element, the bound of test_flow_norm_grad_sweep), accumulate under `close`
    (it is one fma, as there)."""
    from oracle import torch_ref as tr
    rs = np.random.RandomState(40 + order)
    GH, GW = 2 * H, 2 * W
    gt = (rs.randint(-60, 61, (N, GH, GW, 2)) * 2.5).astype(np.float32)
    valid = rs.uniform(size=(N, GH, GW)) < 0.7
    gtd = gt[:, ::2, ::2].astype(np.float64) / 20.0
    vd = valid[:, ::2, ::2] if masked else np.ones((N, H, W), bool)
    assert np.array_equal(gtd, tr.resize_nearest(torch.from_numpy(gt.astype(np.float64)) / 20.0, (H, W)).numpy())
    pred = (gtd + rs.uniform(-0.5, 0.5, (N, H, W, 2))).astype(np.float32)
    scale = 0.32 / N
    pt = torch.tensor(pred[LAST:].astype(np.float64), requires_grad=True)
    (scale * torch.linalg.vector_norm(pt - torch.from_numpy(gtd[LAST:]), ord=order, dim=3)[torch.from_numpy(vd[LAST:])].sum()).backward()
    r = pt.grad.numpy()
    assert float(vd[LAST].mean()) >= 0.5 and float(np.abs(r).max()) > 0
    bad = gt.copy()
    if masked:
        bad[~valid] = np.nan
    ggt, gpred = _wide(gpu(bad), 4, 1)[0], _wide(gpu(pred), 6, 2)[0]
    gmask = torch.from_numpy(valid).cuda() if masked else None

    def run(s, out, acc=False):
        go.flow_norm_grad(V(gpred[s][..., 2:4]), V(ggt[s][..., 1:3]), V(out), gt_div=20.0, ord=order, scale=scale, accumulate=acc,
                          valid=None if gmask is None else gmask[s])

    wide = torch.full((N, H, W, 8), float("nan"), device="cuda")
    run(slice(None), wide[..., 4:6])
    torch.cuda.synchronize()
    got = wide[..., 4:6]
    assert not bool(torch.isnan(got).any()) and bool(torch.isnan(_outside(wide, 4, 2)).all())
    for n in range(N):
        one = torch.full((1, H, W, 8), float("nan"), device="cuda")
        run(slice(n, n + 1), one[..., 4:6])
        assert torch.equal(one[..., 4:6], got[n:n + 1]), n
    close(got[LAST:], r)
    assert not bool(got[LAST][torch.from_numpy(~vd[LAST]).cuda()].any())
    b = rnd((N, H, W, 2), 44) * scale
    acc = _wide(gpu(b), 7, 3)[0]
    run(slice(None), acc[..., 3:5], acc=True)
    torch.cuda.synchronize()
    close(acc[LAST:, ..., 3:5], b[LAST:] + r)
    assert not bool(_outside(acc, 3, 2).any())


def test_flow_distill_grad_past_the_grid_cap(us):
    """pwc_flow_distill_grad_f32, student 5 x 448 x 480 read against a 452 x 486 teacher at offset (2, 3), both masks: overwrite,
    per-image bits, the last image against the float64 closed form under the 2^-23 |ref| rule of tests/test_gpu_distill.py,
    accumulate (it adds exactly what the plain call writes)."""
    rs = np.random.RandomState(51)
    student, teacher, _, _ = dr.random_case(N, H, W, H + 4, W + 6, seed=50)
    tv = torch.from_numpy((rs.uniform(size=(N, H + 4, W + 6)) < 0.9).astype(np.uint8))
    ex = torch.from_numpy((rs.uniform(size=(N, H, W)) < 0.1).astype(np.uint8))
    dsums = torch.tensor(UPSTREAM, dtype=torch.float32)
    off = (2, 3)
    s1 = slice(LAST, N)
    ref = dr.distill_grad(student[s1], teacher[s1], dsums[s1], off, tv[s1], ex[s1], EPS, Q)
    share = float(dr.contributes(student[s1], teacher[s1], off, tv[s1], ex[s1]).double().mean())
    print(f"distill: {share:.3f} of the last image's pixels contribute")
    assert share >= 0.5 and float(ref.abs().max()) > 0
    gs = _wide(student.cuda(), 6, 3)[0][..., 3:5]
    gt_ = _wide(teacher.cuda(), 3, 1)[0][..., 1:3]
    gtv, gex, gd = tv.cuda(), ex.cuda(), dsums.cuda()

    def run(s, out, acc=False):
        us.flow_distill_grad(gs[s], gt_[s], gd[s], out, off, gtv[s], gex[s], EPS, Q, accumulate=acc)

    wide = torch.full((N, H, W, 5), float("nan"), device="cuda")
    run(slice(None), wide[..., 1:3])
    torch.cuda.synchronize()
    got = wide[..., 1:3]
    assert not bool(torch.isnan(got).any()) and bool(torch.isnan(_outside(wide, 1, 2)).all())
    for n in range(N):
        one = torch.full((1, H, W, 5), float("nan"), device="cuda")
        run(slice(n, n + 1), one[..., 1:3])
        assert torch.equal(one[..., 1:3], got[n:n + 1]), n
    _check_distill_grad("5x448x480, last image", got[LAST:], ref)
    base = gpu(rnd((N, H, W, 5), 52))
    acc = base.clone()
    run(slice(None), acc[..., 1:3], acc=True)
    torch.cuda.synchronize()
    assert torch.equal(acc[LAST, ..., 1:3], (base[..., 1:3] + got)[LAST])
    assert torch.equal(_outside(acc, 1, 2), _outside(base, 1, 2))


# ------------------------------------------------------------------ 3. lrelu_grad_ and add_ on their own
def _lrelu_inputs(shape, seed):
    y, dy = rnd(shape, seed), rnd(shape, seed + 1)
    flat = y.reshape(-1)
    flat[::7] = 0.0                          # the y == 0 boundary: `y > 0` is false, the gradient there is slope
    flat[3::11] = -0.0
    return y, dy


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (1, 1, 1, 196), (2, 3, 5, 4), (1, 5, 7, 196)])
@pytest.mark.parametrize("slope", [0.1, 0.25])
def test_lrelu_grad_edges(go, shape, slope):
    """One pixel and a few, C of 4 and 196 (float4 lanes), y and dy as 16-byte-aligned slices of wider records: a select and one
    multiply, so the result equals the same fp32 expression in torch bit for bit; y == 0 (and -0) takes the slope; the channels
    outside the slices stay as they were."""
    n, h, w, c = shape
    y, dy = _lrelu_inputs(shape, 60 + c)
    wy, vy = _wide(gpu(y), c + 8, 4)
    wd, vd = _wide(gpu(dy), c + 12, 8)
    want = torch.where(wy[..., 4:4 + c] > 0, wd[..., 8:8 + c], wd[..., 8:8 + c] * slope).clone()
    go.lrelu_grad_(vy, vd, slope)
    torch.cuda.synchronize()
    assert torch.equal(wd[..., 8:8 + c], want)
    zero = torch.from_numpy(y == 0).cuda()
    assert bool(zero.any()) and torch.equal(wd[..., 8:8 + c][zero], (gpu(dy) * slope)[zero])
    assert not bool(_outside(wd, 8, c).any()) and torch.equal(wy[..., 4:4 + c], gpu(y))
    close(wd[..., 8:8 + c], dy.astype(np.float64) * np.where(y > 0, 1.0, float(np.float32(slope))), rel=2.0 ** -24)    # one rounding


def test_lrelu_grad_past_the_grid_cap(go):
    """4 x 96 x 112 x 196: 2 107 392 float4 groups against the 2 097 152 of one pass; every element checked."""
    shape = (4, 96, 112, 196)
    assert shape[0] * shape[1] * shape[2] * (shape[3] // 4) > 8192 * 256
    y, dy = _lrelu_inputs(shape, 70)
    gy, gd = gpu(y), gpu(dy)
    want = torch.where(gy > 0, gd, gd * 0.1)
    go.lrelu_grad_(V(gy), V(gd))
    torch.cuda.synchronize()
    assert torch.equal(gd, want)


def _check_add(got, src, dst0, alpha, accumulate, tag):
    """got against the two fp32 operations alpha * src (+ dst0) in torch, bit for bit: the multiply and the add are not
    contracted into one fma (observed on an MI355X: no element differs, at alpha -0.75 either)."""
    v = src * alpha
    want = dst0 + v if accumulate else v
    differ = int((got != want).sum())
    print(f"add {tag}: alpha {alpha} accumulate {accumulate}: {differ} of {got.numel()} elements differ from mul-then-add")
    assert torch.equal(got, want), tag


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 81), (2, 3, 5, 2), (2, 3, 5, 33), (1, 4, 3, 81)])
@pytest.mark.parametrize("alpha", [1.0, -0.75, 0.0])
@pytest.mark.parametrize("accumulate", [False, True])
def test_add_edges(go, shape, alpha, accumulate):
    """pwc_add_f32, the scalar kernel that moves gradients between channel slices: one pixel and a few, C of 1, 2, 33 and 81,
    source and destination as slices of wider records at unaligned offsets, alpha of 1, -0.75 and 0, overwrite and accumulate
    into non-zero memory; the channels outside the destination slice stay as they were."""
    n, h, w, c = shape
    src = gpu(rnd(shape, 80 + c))
    ws, vs = _wide(src, c + 3, 1)
    wd = gpu(rnd((n, h, w, c + 5), 81 + c))
    before = wd.clone()
    go.add_(vs, View(wd.data_ptr() + 4 * 3, c + 5, n, h, w, c), alpha=alpha, accumulate=accumulate)
    torch.cuda.synchronize()
    _check_add(wd[..., 3:3 + c], src, before[..., 3:3 + c], alpha, accumulate, f"{shape}")
    assert torch.equal(_outside(wd, 3, c), _outside(before, 3, c)) and torch.equal(ws[..., 1:1 + c], src)


def test_add_past_the_grid_cap(go):
    """4 x 48 x 56 x 196 = 2 107 392 elements against the 2 097 152 of one pass: a plain call over a NaN-filled destination, then
    an accumulating one; every element checked."""
    shape = (4, 48, 56, 196)
    assert int(np.prod(shape)) > 8192 * 256
    src = gpu(rnd(shape, 85))
    dst = torch.full(shape, float("nan"), device="cuda")
    go.add_(V(src), V(dst), alpha=-0.75, accumulate=False)
    torch.cuda.synchronize()
    _check_add(dst, src, None, -0.75, False, "past the cap")
    base = gpu(rnd(shape, 86))
    dst = base.clone()
    go.add_(V(src), V(dst), alpha=-0.75, accumulate=True)
    torch.cuda.synchronize()
    _check_add(dst, src, base, -0.75, True, "past the cap")


# ------------------------------------------------------------------ 4. the 65535-row cap of the forward warp and the resizes
def _tall_flow(n, h, w, seed):
    """Sub-pixel and multi-pixel displacements; in y they straddle the top and bottom borders of every image, and a few rows
    jump by tens of pixels."""
    rs = np.random.RandomState(seed)
    flow = rs.uniform(-3.7, 3.7, size=(n, h, w, 2)).astype(np.float32)
    far = rs.uniform(size=(n, h, w)) < 0.02
    flow[far, 1] = rs.choice(np.array([-40.25, 17.5, 33.75], np.float32), size=int(far.sum()))
    return flow


@pytest.mark.parametrize("kind", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", [(1, 65601, 3, 4), (3, 21900, 2, 8)])
def test_warp_past_the_row_cap(pa, kind, shape):
    """N * H rows against grid.y's 65535: one tall image, and three where the cap falls inside the last one, so the second trip
    has to get n and gy from its row.  The plain warp and the warp with the fused channel copy against the oracle's warp under
    test_warp_vs_oracle's tolerances (nearest: exact); the copied slice is exact."""
    from pwcnet_amd.modules import sub_view
    n, h, w, c = shape
    assert n * h > 65535 > (n - 1) * h
    x, f0 = rnd(shape, 91), rnd(shape, 92)
    flow = _tall_flow(n, h, w, 93)
    gx, g0, gf = gpu(x), gpu(f0), gpu(flow)
    exp = orc.warp(x, flow, kind)
    out = pa.WarpingLayer(kind)(gx, gf)
    if kind == "nearest":
        np.testing.assert_array_equal(out.cpu().numpy(), exp)
    else:
        close_oracle(out, exp, rel=2e-6, floor=2e-6)
    out2 = torch.full(shape, float("nan"), device="cuda")
    E = torch.full((n, h, w, c + 12), -4.0, device="cuda")
    gf2 = gpu(flow / 2.5)
    pa.WarpingLayer(kind)._run(V(gx), V(gf2), V(out2), flow_scale=2.5, copy=(V(g0), sub_view(V(E), 8, c)))
    torch.cuda.synchronize()
    close_oracle(out2, orc.warp(x, flow / np.float32(2.5), kind, flow_scale=2.5), rel=2e-6, floor=1e-6)
    assert torch.equal(E[..., 8:8 + c], g0)
    assert float(E[..., :8].max()) == -4.0 and float(E[..., 8 + c:].max()) == -4.0 and float(E[..., :8].min()) == -4.0


@pytest.mark.parametrize("shape", [(1, 16401, 2, 2), (3, 5467, 3, 2), (1, 16401, 2, 4), (3, 5467, 3, 3)])
def test_resize_past_the_row_cap(pa, shape):
    """N * OH output rows against grid.y's 65535 at factor 4: resize_kernel in its float2, float4 and scalar forms (a two-channel
    source goes to a destination of channel stride 4, which keeps it off the one-lane-per-cell x4 kernel), with and without the
    status word, against the oracle under test_resize_vs_oracle's tolerance; an Inf in a source row that only second-trip
    output rows read sets PWC_STATUS_NONFINITE."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    n, h, w, c = shape
    oh, ow = 4 * h, 4 * w
    assert n * oh > 65535 > (n - 1) * oh
    x = rnd(shape, 95) * 3.0
    xg = gpu(x)
    exp = orc.resize_bilinear(x, (oh, ow), 20.0)
    cs = 4 if c == 2 else c
    wide = torch.full((n, oh, ow, cs), -5.0, device="cuda")
    _lib.check(L.pwc_resize_bilinear_f32(_p(xg), c, _p(wide), cs, n, h, w, c, oh, ow, 20.0, None))
    torch.cuda.synchronize()
    close_oracle(wide[..., :c], exp, rel=1e-6, floor=1e-6)
    assert cs == c or float(wide[..., c:].max()) == float(wide[..., c:].min()) == -5.0
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.full((n, oh, ow, cs), -5.0, device="cuda")
    _lib.check(L.pwc_resize_bilinear_status_f32(_p(xg), c, _p(ws), cs, n, h, w, c, oh, ow, 20.0, _p(st), None))
    torch.cuda.synchronize()
    assert torch.equal(ws, wide) and int(st[0]) == 0
    if c == 2:                                  # the dense destination: the x4 kernel, no row loop -- the same values
        assert torch.equal(pa.resize_bilinear(xg, (oh, ow), 20.0), wide[..., :2].contiguous())
    first_second_trip_row = 65535 - (n - 1) * oh            # of the last image's output rows
    ys = first_second_trip_row // 4 + 3                      # a source row that only rows past it read (rows 4 ys - 3 .. 4 ys + 3)
    assert 4 * ys - 4 >= first_second_trip_row and ys < h
    xg[n - 1, ys, w - 1, c - 1] = float("inf")
    _lib.check(L.pwc_resize_bilinear_status_f32(_p(xg), c, _p(ws), cs, n, h, w, c, oh, ow, 20.0, _p(st), None))
    torch.cuda.synchronize()
    assert int(st[0]) & _lib.STATUS_NONFINITE


@pytest.mark.parametrize("shape", [(1, 16401, 2, 4), (3, 5467, 3, 8)])
def test_resize_pair_past_the_row_cap(pa, shape):
    """pwc_resize_bilinear_pair_f32 at factor 4 (resize_pair_kernel: the x2 per-cell kernel does not take it): flows and features
    into channel slices of one buffer, against the oracle under test_resize_pair_vs_oracle's tolerance."""
    from pwcnet_amd import _lib
    n, h, w, c = shape
    oh, ow = 4 * h, 4 * w
    assert n * oh > 65535 > (n - 1) * oh
    fl, ft = rnd((n, h, w, 2), 96), rnd(shape, 97)
    gfl, gft = gpu(fl), gpu(ft)
    E = torch.full((n, oh, ow, 8 + c + 4), -2.0, device="cuda")       # [pad 4 | flow 2 pad 2 | feat C | pad 4]
    _lib.check(_lib.lib().pwc_resize_bilinear_pair_f32(_p(gfl), 2, ctypes.c_void_p(E.data_ptr() + 16), 8 + c + 4, _p(gft), c,
                                                       ctypes.c_void_p(E.data_ptr() + 32), 8 + c + 4, n, h, w, c, oh, ow, None))
    torch.cuda.synchronize()
    close_oracle(E[..., 4:6], orc.resize_bilinear(fl, (oh, ow)), rel=1e-6, floor=1e-6)
    close_oracle(E[..., 8:8 + c], orc.resize_bilinear(ft, (oh, ow)), rel=1e-6, floor=1e-6)
    assert float(E[..., :4].max()) == -2.0 and float(E[..., 6:8].max()) == -2.0 and float(E[..., 8 + c:].max()) == -2.0
    assert float(E[..., :4].min()) == -2.0 and float(E[..., 6:8].min()) == -2.0 and float(E[..., 8 + c:].min()) == -2.0


@pytest.mark.parametrize("shape,cs,off", [((1, 180, 180, 33), 40, 3), ((1, 182, 182, 128), 136, 4)])
def test_copy_channels_past_the_grid_cap(pa, shape, cs, off):
    """More than 4096 x 256 items: 1 069 200 floats on the scalar kernel, 1 059 968 float4 groups on the vector one.  Exact,
    and the channels outside the slice stay as they were."""
    from pwcnet_amd.modules import _copy_channels, sub_view
    n, h, w, c = shape
    vec4 = c % 4 == 0 and cs % 4 == 0 and off % 4 == 0
    assert n * h * w * (c // 4 if vec4 else c) > 4096 * 256
    src = gpu(rnd(shape, 98))
    dst = torch.full((n, h, w, cs), float("nan"), device="cuda")
    _copy_channels(V(src), sub_view(V(dst), off, c), c)
    torch.cuda.synchronize()
    assert torch.equal(dst[..., off:off + c], src) and bool(torch.isnan(_outside(dst, off, c)).all())


def test_absmax_past_the_grid_cap(pa):
    """130 x 130 x 33 = 557 700 floats against 2048 x 256, as a slice of a wider record, the maximum in the last element (a lane's
    second trip): status[1] holds its bits."""
    from pwcnet_amd import _lib
    n, h, w, c = 1, 130, 130, 33
    assert n * h * w * c > 2048 * 256
    x = rnd((n, h, w, c), 99)
    x[0, h - 1, w - 1, c - 1] = -7.5
    buf, _ = _wide(gpu(x), c + 3, 2)
    buf[..., :2], buf[..., 2 + c:] = 100.0, 100.0             # outside the slice: not read
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().pwc_absmax_f32(ctypes.c_void_p(buf.data_ptr() + 8), c + 3, n * h * w, c, _p(st), None))
    torch.cuda.synchronize()
    assert int(st[1]) == int(np.float32(7.5).view(np.int32)) and int(st[0]) == 0


# ------------------------------------------------------------------ 5. fit_frames / refit_flow past fit_grid's cap
@pytest.mark.parametrize("mode", fr.MODES)
def test_fit_and_refit_past_the_grid_cap(pa, mode):
    """1 x 1030 x 2040 frames fitted to 1088 x 2048 (557 056 float4 groups of pixels against 2048 x 256) and a 1088 x 2048 flow
    refitted to 1030 x 2040 (1 050 600 pairs), against tests/fit_ref.py under test_gpu_fit.py's own judgement (pad: bitwise;
    resize: its bound)."""
    n, h, w = 1, 1030, 2040
    oh, ow = fr.ceil_to(h), fr.ceil_to(w)
    assert (n * oh * ow + 3) // 4 > 2048 * 256 and (n * h * w + 1) // 2 > 2048 * 256
    u8 = np.random.RandomState(101).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    ref, S = fr.fit_frames(u8, mode)
    y, info = pa.fit_frames(torch.from_numpy(u8).cuda(), mode)
    assert info == (mode, h, w, oh, ow)
    _fit_judge(f"fit {mode} {h}x{w} -> {oh}x{ow}", y, ref, S, mode)
    from tests import util
    flow = util.flow_field(n, oh, ow, seed=102)
    rref, rS = fr.refit_flow(flow, h, w, mode)
    ry = pa.refit_flow(torch.from_numpy(flow).cuda(), pa.fit_info(h, w, mode))
    _fit_judge(f"refit {mode} {oh}x{ow} -> {h}x{w}", ry, rref, rS, mode)


# ------------------------------------------------------------------ 2b. the other launches of pwc_loss_grad_blocks' width
def test_fb_valid_over_a_batch_past_the_gathers_cap(us):
    """pwc_fb_valid_u8 at 5 x 448 x 480.  Its grid is (parts, N, 2): an image is cut into at most 256 parts, so the cap is 65 536
    pixels PER IMAGE (tests/test_gpu_fbcheck.py's 272 x 256 cases cross it once; here a lane makes four trips).  The C entry over
    0xAB-filled masks leaves bytes 0 / 1 only; image n equals the call on it alone; the last image equals the float64
    restatement outside the near-tie set (test_gpu_fbcheck.py's rule)."""
    from pwcnet_amd import _lib
    from tests import fb_ref
    from tests.test_gpu_fbcheck import _check_direction
    c = _fb_case()
    fw = _wide(gpu(c["fw"]), 6, 3)[0][..., 3:5]
    bw = _wide(gpu(c["bw"]), 3, 1)[0][..., 1:3]
    vf, vb = torch.from_numpy(c["valid_fw"]).cuda(), torch.from_numpy(c["valid_bw"]).cuda()
    outs = [torch.full((N, H, W), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    _lib.check(_lib.lib().pwc_fb_valid_u8(_p(fw), 6, _p(bw), 3, FLOW_SCALE, _p(vf), _p(vb), N, H, W, 0.01, 0.5, _p(outs[0]), _p(outs[1]),
                                          None, None, None, 0, _lib.current_stream()))
    torch.cuda.synchronize()
    assert all(set(o.unique().tolist()) <= {0, 1} for o in outs)
    m_fw, m_bw, c_fw, c_bw = us.fb_valid(fw, bw, FLOW_SCALE, 0.01, 0.5, vf, vb, return_counts=True)
    assert torch.equal(m_fw.view(torch.uint8), outs[0]) and torch.equal(m_bw.view(torch.uint8), outs[1])
    for n in range(N):
        s = slice(n, n + 1)
        one = us.fb_valid(fw[s], bw[s], FLOW_SCALE, 0.01, 0.5, vf[s], vb[s], return_counts=True)
        for x, y in zip((m_fw[s], m_bw[s], c_fw[s], c_bw[s]), one):
            assert torch.equal(x, y), n
    s = slice(LAST, N)
    a, b = fb_ref.fb_ref(torch.from_numpy(c["fw"][s]), torch.from_numpy(c["bw"][s]), FLOW_SCALE, 0.01, 0.5,
                         torch.from_numpy(c["valid_fw"][s]), torch.from_numpy(c["valid_bw"][s]))
    assert 0.2 <= float(a.mask.double().mean()) <= 0.8 and 0.2 <= float(b.mask.double().mean()) <= 0.8
    _check_direction("last image fw", m_fw[s].contiguous(), c_fw[s], a)
    _check_direction("last image bw", m_bw[s].contiguous(), c_bw[s], b)


@functools.lru_cache(maxsize=None)
def _compose_case():
    from tests import compose_ref as R
    ab, bc, vab, vbc, g = R.random_case(N, H, W, seed=61)
    s = slice(LAST, N)
    return ab, bc, vab, vbc, g, R.compose(ab[s], bc[s], vab[s], vbc[s])[:3], R.compose_grad(ab[s], bc[s], g[s], vab[s], vbc[s])


def _nan_slice(a=None, shape=None):
    """Channels 1:3 of a NaN-filled 5-channel buffer, holding a (or nothing): (buffer, slice)."""
    wide = torch.full(tuple(shape if a is None else a.shape[:3]) + (5,), float("nan"), dtype=torch.float32, device="cuda")
    if a is not None:
        wide[..., 1:3] = torch.from_numpy(a).cuda()
    return wide, wide[..., 1:3]


def test_flow_compose_and_its_gradient_past_the_grid_cap(pa):
    """pwc_flow_compose_f32 and pwc_flow_compose_grad_f32 (scatter and finish kernels) at 5 x 448 x 480, both masks, every flow
    and gradient a channel slice: the forward through the C entry over a NaN-filled flow and 0xAB-filled mask (nothing
    survives), per-image bits for forward and both gradients, the last image under test_gpu_compose.py's own bounds, and
    accumulate adds exactly what the plain call writes.  At least half of the last image's pixels are valid in the
    restatement."""
    from pwcnet_amd import _lib
    from tests.test_gpu_compose import _check_forward, _check_grad
    ab, bc, vab, vbc, g, ref_fwd, ref_grad = _compose_case()
    share = float(ref_fwd[1].mean())
    print(f"compose: {share:.3f} of the last image's pixels are valid")
    assert share >= 0.5 and float(np.abs(ref_grad["dab"]).max()) > 0 and float(np.abs(ref_grad["dbc"]).max()) > 0
    (_, ta), (_, tb), (_, tg) = _nan_slice(ab), _nan_slice(bc), _nan_slice(g)
    ma, mb = torch.from_numpy(vab).cuda(), torch.from_numpy(vbc).cuda()
    wo, out = _nan_slice(shape=(N, H, W))
    vout = torch.full((N, H, W), 0xAB, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().pwc_flow_compose_f32(_p(ta), 5, _p(tb), 5, _p(ma), _p(mb), N, H, W, _p(out), 5, _p(vout), _lib.current_stream()))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and set(vout.unique().tolist()) <= {0, 1}
    assert bool(torch.isnan(wo[..., :1]).all()) and bool(torch.isnan(wo[..., 3:]).all())
    (wa, da), (wb, db) = _nan_slice(shape=(N, H, W)), _nan_slice(shape=(N, H, W))
    pa.compose_grad(ta, tb, tg, ma, mb, dflow_ab=da, dflow_bc=db)
    torch.cuda.synchronize()
    for w_, d in ((wa, da), (wb, db)):
        assert not bool(torch.isnan(d).any()) and bool(torch.isnan(w_[..., :1]).all()) and bool(torch.isnan(w_[..., 3:]).all())
    for n in range(N):
        s = slice(n, n + 1)
        o1, v1 = pa.compose_flows(ta[s], tb[s], ma[s], mb[s])
        a1, b1 = pa.compose_grad(ta[s], tb[s], tg[s], ma[s], mb[s])
        assert torch.equal(o1, out[s]) and torch.equal(v1.view(torch.uint8), vout[s]), n
        assert torch.equal(a1, da[s]) and torch.equal(b1, db[s]), n
    s = slice(LAST, N)
    _check_forward("5x448x480, last image", out[s], vout[s].view(torch.bool).contiguous(), ref_fwd)
    _check_grad("5x448x480, last image", da[s], db[s], ref_grad)
    base = gpu(rnd((2, N, H, W, 5), 62))
    acc = base.clone()
    pa.compose_grad(ta, tb, tg, ma, mb, dflow_ab=acc[0][..., 1:3], dflow_bc=acc[1][..., 1:3], accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(acc[0][LAST, ..., 1:3], (base[0][..., 1:3] + da)[LAST]) and torch.equal(acc[1][LAST, ..., 1:3], (base[1][..., 1:3] + db)[LAST])
    assert torch.equal(_outside(acc[0], 1, 2), _outside(base[0], 1, 2)) and torch.equal(_outside(acc[1], 1, 2), _outside(base[1], 1, 2))


def test_splat_and_its_gradient_past_the_grid_cap(pa):
    """pwc_splat_f32 (scatter and finish) and pwc_splat_grad_f32 at 5 x 448 x 480 x 3, mode "sum", a ~70 % source mask, x and the
    flows channel slices: per-image bits for the forward and the three gradients, the gradients over NaN-filled destinations
    (nothing survives, the channels beside stay NaN), the last image under test_gpu_splat.py's bounds (forward 2^-24 |ref| + n
    STEP, gradients 2^-23 A), accumulate adds exactly what the plain call writes."""
    from pwcnet_amd import splat as sl
    from tests import splat_ref as sp
    from tests.test_gpu_splat import STEP
    rs = np.random.RandomState(71)
    x = torch.from_numpy(rs.uniform(0, 1, (N, H, W, C)).astype(np.float32))
    w = torch.from_numpy(rs.uniform(0.5, 2, (N, H, W)).astype(np.float32))
    flow = torch.from_numpy(sp.smooth_flow(N, H, W, 6.0, 72))
    valid = torch.from_numpy(rs.uniform(size=(N, H, W)) < 0.7)
    g_out = torch.from_numpy(rs.uniform(-1, 1, (N, H, W, C)).astype(np.float32))
    g_cov = torch.from_numpy(rs.uniform(-1, 1, (N, H, W)).astype(np.float32))
    s = slice(LAST, N)
    (rx, rw, rf), (ax, aw, af), ok = sp.splat_grads_ref(x[s], flow[s], w[s], valid[s], 1.0, "sum", g_out[s], g_cov[s])
    with torch.no_grad():
        ref, ref_cov, cnt = sp.splat_ref(x[s], flow[s], w[s], valid[s], 1.0, "sum")
    share = float(ok.double().mean())
    print(f"splat: {share:.3f} of the last image's pixels contribute")
    assert share >= 0.5 and float(rf.abs().max()) > 0
    gx = _wide(x.cuda(), C + 3, 2)[0][..., 2:2 + C]
    gf = _wide(flow.cuda(), 4, 1)[0][..., 1:3]
    gw, gv, gg, gc = w.cuda(), valid.cuda(), g_out.cuda(), g_cov.cuda()
    out, cov = sl.forward_splat(gx, gf, gw, valid=gv)
    wdx = torch.full((N, H, W, C + 2), float("nan"), device="cuda")
    wdf = torch.full((N, H, W, 5), float("nan"), device="cuda")
    dw = torch.full((N, H, W), float("nan"), device="cuda")
    dx, df = wdx[..., 1:1 + C], wdf[..., 1:3]
    sl.splat_grad(gx, gf, gg, gc, gw, gv, mode="sum", dx=dx, dweights=dw, dflows=df)
    torch.cuda.synchronize()
    for t in (dx, dw, df):
        assert not bool(torch.isnan(t).any())
    assert bool(torch.isnan(_outside(wdx, 1, C)).all()) and bool(torch.isnan(_outside(wdf, 1, 2)).all())
    for n in range(N):
        i = slice(n, n + 1)
        o1, c1 = sl.forward_splat(gx[i], gf[i], gw[i], valid=gv[i])
        x1, w1, f1 = sl.splat_grad(gx[i], gf[i], gg[i], gc[i], gw[i], gv[i], mode="sum")
        assert torch.equal(o1, out[i]) and torch.equal(c1, cov[i]), n
        assert torch.equal(x1, dx[i]) and torch.equal(w1, dw[i]) and torch.equal(f1, df[i]), n
    for what, got, want, n_ in (("out", out[s], ref, cnt[..., None]), ("coverage", cov[s], ref_cov, cnt)):
        err = (got.double().cpu() - want).abs()
        assert bool((err <= 2.0 ** -24 * want.abs() + n_ * STEP + 1e-30).all()), what
    for what, got, want, A in (("dx", dx[s], rx, ax), ("dweights", dw[s], rw, aw), ("dflows", df[s], rf, af)):
        err = (got.double().cpu() - want).abs()
        print(f"splat {what}: max err / (2^-23 A) {float((err / (2.0 ** -23 * A).clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= 2.0 ** -23 * A).all()), what
        assert not bool(got.cpu()[~ok].any())
    bx, bw_, bf = gpu(rnd((N, H, W, C), 73)), gpu(rnd((N, H, W), 74)), gpu(rnd((N, H, W, 2), 75))
    ax_, aw_, af_ = sl.splat_grad(gx, gf, gg, gc, gw, gv, mode="sum", dx=bx.clone(), dweights=bw_.clone(), dflows=bf.clone(), accumulate=True)
    assert torch.equal(ax_[LAST], (bx + dx)[LAST]) and torch.equal(aw_[LAST], (bw_ + dw)[LAST]) and torch.equal(af_[LAST], (bf + df)[LAST])


# ------------------------------------------------------------------ 5b. the other capped launches
def test_warp_grad_finish_past_the_grid_cap(go):
    """warp_grad_fix_finish_kernel converts the fixed-point accumulators of the deterministic warp gradient, 8192 x 256 elements
    per pass: 3 x 96 x 112 x 68 = 2 193 408.  dx and dflow against float64 autograd under test_warp_grad's bounds; two runs give
    the same bits."""
    from oracle import torch_ref as tr
    from tests import util
    from tests.test_gpu_grad import t64
    n, h, w, c = 3, 96, 112, 68
    assert n * h * w * c > 8192 * 256
    x, dy = rnd((n, h, w, c), 105), rnd((n, h, w, c), 106)
    flow = util.flow_field(n, h, w, seed=107, sigma=2.0) + 0.137
    xt, ft = t64(x), t64(flow)
    (tr.bilinear_warp(xt, ft * 1.25) * t64(dy, False)).sum().backward()
    gx, gfl, gdy = gpu(x), gpu(flow), gpu(dy)
    runs = []
    for _ in range(2):
        dx = torch.zeros((n, h, w, c), device="cuda")
        dfl = torch.full((n, h, w, 2), float("nan"), device="cuda")
        go.warp_grad(V(gx), V(gfl), 1.25, V(gdy), V(dx), V(dfl))
        torch.cuda.synchronize()
        runs.append((dx, dfl))
    close(runs[0][0], xt.grad, rel=1e-5)
    close(runs[0][1], ft.grad, rel=1e-4)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_flow_head_c32_kernel_past_the_grid_cap(pa):
    """conv3x3_head2_c32_kernel (32 -> 2 channels on images below 4096 pixels, which the matrix-pipe head does not take): 2048
    workgroups x 32 pixels; 20 x 56 x 64 = 71 680 pixels.  Against the oracle under test_conv_direct_vs_oracle's tolerance, with
    and without the residual."""
    from tests.test_gpu_ops import run_conv_direct
    n, h, w = 20, 56, 64
    assert n * h * w > 2048 * 32 and h * w < 4096
    x = rnd((n, h, w, 32), 111)
    k = rnd((3, 3, 32, 2), 112) * float(1.0 / np.sqrt(9 * 32))
    b = rnd((2,), 113) * 0.1
    res = rnd((n, h, w, 2), 114)
    close_oracle(run_conv_direct(x, k, b, 1, 1, None), orc.conv3x3(x, k, b, 1, 1, None))
    close_oracle(run_conv_direct(x, k, b, 1, 1, None, residual=res), orc.conv3x3(x, k, b, 1, 1, None, residual=res))


def test_resize_pair_x2_per_cell_kernel_past_the_grid_cap(pa):
    """resize_pair2x_kernel: 16384 x 256 units of (source pixel, float2 / float4 group); 1 x 520 x 480 pixels x 17 units =
    4 243 200 against 4 194 304, so the last rows are second-trip work.  Nothing of a NaN-filled destination survives inside the
    slices and the padding channels stay NaN; the first and the last 24 source rows against the oracle under
    test_resize_pair_vs_oracle's tolerance (an x2 output row depends on its source row and the next only)."""
    from pwcnet_amd.modules import _resize_pair, sub_view
    n, h, w, c = 1, 520, 480, 64
    assert n * h * w * (1 + c // 4) > 16384 * 256
    fl, ft = rnd((n, h, w, 2), 115), rnd((n, h, w, c), 116)
    gfl, gft = gpu(fl), gpu(ft)
    E = torch.full((n, 2 * h, 2 * w, 8 + c + 4), float("nan"), device="cuda")       # [pad 4 | flow 2 pad 2 | feat C | pad 4]
    Ev = V(E)
    _resize_pair(V(gfl), sub_view(Ev, 4, 2), V(gft), sub_view(Ev, 8, c))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(E[..., 4:6]).any()) and not bool(torch.isnan(E[..., 8:8 + c]).any())
    assert bool(torch.isnan(E[..., :4]).all()) and bool(torch.isnan(E[..., 6:8]).all()) and bool(torch.isnan(E[..., 8 + c:]).all())
    r = 24
    for rows, orows in ((slice(0, r + 1), slice(0, 2 * r)), (slice(h - r, h), slice(2 * (h - r), 2 * h))):
        k = rows.stop - rows.start
        close_oracle(E[:, orows, :, 4:6], orc.resize_bilinear(np.ascontiguousarray(fl[:, rows]), (2 * k, 2 * w))[:, :orows.stop - orows.start],
                     rel=1e-6, floor=1e-6)
        close_oracle(E[:, orows, :, 8:8 + c], orc.resize_bilinear(np.ascontiguousarray(ft[:, rows]), (2 * k, 2 * w))[:, :orows.stop - orows.start],
                     rel=1e-6, floor=1e-6)


@pytest.mark.parametrize("family,cin,cout", [("mfma", 1024, 128), ("wino", 576, 128), ("wino4", 256, 128), ("h2", 256, 512),
                                             ("sk", 256, 256), ("h2_stride2", 256, 128)])
def test_weight_packing_past_the_grid_cap(pa, family, cin, cout):
    """The weight packers launch at most 4096 x 256 lanes and stride over the rest: a layer whose packed image is larger
    (1 179 648 elements in each case here), run on a small image and compared with the oracle's convolution under the family's
    own tolerance -- a weight the second trip misplaced is a wrong output channel."""
    from pwcnet_amd import _lib
    from tests.test_gpu_ops import run_conv_h2, run_conv_mfma, run_conv_wino, run_conv_wino4
    L = _lib.lib()
    n, h, w = 1, 16, 32
    x = rnd((n, h, w, cin), 121)
    k = rnd((3, 3, cin, cout), 122) * float(1.0 / np.sqrt(9 * cin))
    b = rnd((cout,), 123) * 0.1
    lanes = {"mfma": 9 * cin * cout, "wino": 16 * cin * cout, "wino4": 36 * cin * cout, "h2": (cin // 16) * (cout // 32) * 9 * 512,
             "sk": 18 * cin * cout, "h2_stride2": (cin // 4) * (cout // 32) * 9 * 512}[family]
    assert lanes > 4096 * 256
    if family == "mfma":
        close_oracle(run_conv_mfma(x, k, b, 1, 1, 0.1), orc.conv3x3(x, k, b, 1, 1, 0.1))
    elif family == "wino":
        close_oracle(run_conv_wino(x, k, b, 0.1), orc.conv3x3(x, k, b, 1, 1, 0.1), rel=2e-5)
    elif family == "wino4":
        close_oracle(run_conv_wino4(x, k, b, 0.1), orc.conv3x3(x, k, b, 1, 1, 0.1), rel=2e-5)
    elif family == "h2":
        close_oracle(run_conv_h2(x, k, b, 0.1), orc.conv3x3(x, k, b, 1, 1, 0.1))
    else:
        xg, kg, bg = gpu(x), gpu(k), gpu(b)
        if family == "sk":
            packed = torch.empty(L.pwc_conv3x3_sk_packed_floats(cin, cout), device="cuda")
            _lib.check(L.pwc_conv3x3_sk_pack_f32(_p(kg), None, cin, cin, cout, _p(packed), None))
            y = torch.full((n, h, w, cout), -7.0, device="cuda")
            _lib.check(L.pwc_conv3x3_sk_f32(_p(xg), cin, _p(packed), _p(bg), _p(y), cout, n, h, w, cin, cout, 1, 1, 1, 0.1, None))
            exp = orc.conv3x3(x, k, b, 1, 1, 0.1)
        else:
            packed = torch.empty(L.pwc_conv3x3_h2_stride2_packed_floats(cin, cout), device="cuda")
            _lib.check(L.pwc_conv3x3_h2_stride2_pack_f32(_p(kg), None, cin, cin, cout, _p(packed), None))
            y = torch.full((n, h // 2, w // 2, cout), -7.0, device="cuda")
            _lib.check(L.pwc_conv3x3_h2_stride2_f32(_p(xg), cin, _p(packed), _p(bg), _p(y), cout, n, h, w, cin, cout, 1, 0.1, None, 0,
                                                    None, None))
            exp = orc.conv3x3(x, k, b, 2, 1, 0.1)
        torch.cuda.synchronize()
        close_oracle(y, exp)


@pytest.mark.parametrize("h,w,c", [(96, 96, 64), (95, 97, 63)])
def test_feature_norm_past_its_grid_caps(h, w, c):
    """pwc_feature_norm_f32 and pwc_feature_norm_grad_f32 cut a frame into groups of four values: the parts kernels walk them on
    at most 256 parts x 256 lanes (65 536 groups) and the apply kernels on 512 x 256 (131 072).  96 x 96 x 64 is 147 456 groups
    on the 16-byte path, 95 x 97 x 63 is 145 137 on the scalar path with a last group of one value; N = 2.  Forward, statistics
    and gradient against the float64 restatement under tests/test_gpu_featnorm.py's bounds; a pair alone gives the bits it
    gives in the batch; accumulate adds exactly what the plain call writes."""
    _need_gpu()
    from pwcnet_amd import grad_ops as G
    from pwcnet_amd.modules import FeatureNormLayer
    from tests import featnorm_ref as R
    from tests.test_gpu_featnorm import _forward_check, _inputs, _run
    n = 2
    groups = (h * w * c + 3) // 4
    assert groups > 512 * 256 and (c % 4 == 0 or (h * w * c) % 4 == 1)
    f0, f1 = _inputs((n, h, w, c), "lrelu", seed=h * 1000 + c)
    g0, g1 = R.lrelu_maps((n, h, w, c), seed=h * 100 + c + 1, shift=-0.3)
    t0, t1, u0, u1 = gpu(f0), gpu(f1), gpu(g0), gpu(g1)
    y0, y1, stats = _run(FeatureNormLayer, t0, t1)
    mean, rstd = _forward_check(f"{h}x{w}x{c} past the caps", y0, y1, f0, f1)
    st = stats.cpu().numpy()
    assert np.abs(st[:, 0] - mean).max() <= 2.0 ** -40 * np.abs(mean).max() and np.abs(st[:, 1] / rstd - 1).max() <= 2.0 ** -30
    r0, r1, A0, A1 = R.feature_norm_grads(f0, f1, g0, g1)
    d = torch.full((2, n, h, w, c), float("nan"), device="cuda")
    G.feature_norm_grad(V(t0), V(t1), V(u0), V(u1), stats, V(d[0]), V(d[1]))
    torch.cuda.synchronize()
    worst = max(float((np.abs(got.cpu().double().numpy() - ref) / (2.0 ** -23 * A)).max()) for got, ref, A in ((d[0], r0, A0), (d[1], r1, A1)))
    print(f"featnorm backward {h}x{w}x{c}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst
    for i in range(n):
        s = slice(i, i + 1)
        a0, a1, st1 = _run(FeatureNormLayer, t0[s].clone(), t1[s].clone())
        assert torch.equal(a0, y0[s]) and torch.equal(a1, y1[s]) and torch.equal(st1, stats[s]), i
        d1 = torch.empty((2, 1, h, w, c), device="cuda")
        G.feature_norm_grad(V(t0[s]), V(t1[s]), V(u0[s]), V(u1[s]), st1, V(d1[0]), V(d1[1]))
        assert torch.equal(d1, d[:, s]), i
    base = gpu(R.lrelu_maps((2 * n, h, w, c), seed=5)[0]).view(2, n, h, w, c)
    acc = base.clone()
    G.feature_norm_grad(V(t0), V(t1), V(u0), V(u1), stats, V(acc[0]), V(acc[1]), accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, base + d)


def test_tap_split_reduce_past_the_grid_cap(pa):
    """conv_fp32_split_reduce behind the tap split of pwc_conv3x3_f32: 2048 x 256 float4 groups of M * Cout / 4; 1 x 96 x 112 pixels
    x 256 output channels is 688 128.  Against the oracle under test_conv_mfma_tap_split_vs_oracle's tolerance, dense and into a
    wider record; two launches give the same bits."""
    from tests.test_gpu_ops import run_conv_mfma
    n, h, w, cin, cout = 1, 96, 112, 64, 256
    assert n * h * w * (cout // 4) > 2048 * 256
    x = rnd((n, h, w, cin), 131)
    k = rnd((3, 3, cin, cout), 132) * float(1.0 / np.sqrt(9 * cin))
    b = rnd((cout,), 133) * 0.1
    exp = orc.conv3x3(x, k, b, 1, 1, 0.1)
    y = run_conv_mfma(x, k, b, 1, 1, 0.1, split=3)
    close_oracle(y, exp)
    y2 = run_conv_mfma(x, k, b, 1, 1, 0.1, split=3, y_cs=cout + 4)
    close_oracle(y2[..., :cout], exp)
    assert float(y2[..., cout:].min()) == -7.0 and float(y2[..., cout:].max()) == -7.0
    assert torch.equal(y, run_conv_mfma(x, k, b, 1, 1, 0.1, split=3))


def test_channel_split_reduce_past_the_grid_cap(pa):
    """conv_fp32_split_reduce behind the channel split of pwc_conv3x3_wino_split_f32: 4096 x 256 float4 groups; 1 x 128 x 144
    pixels x 256 output channels is 1 179 648.  Against the oracle under test_conv_winograd_channel_split's tolerance, with the
    activation into a dense output and without it into an unaligned record."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    n, h, w, cin, cout, csplit = 1, 128, 144, 64, 256, 2
    assert n * h * w * (cout // 4) > 4096 * 256
    x = rnd((n, h, w, cin), 135)
    k = rnd((3, 3, cin, cout), 136) * float(1.0 / np.sqrt(9 * cin))
    b = rnd((cout,), 137) * 0.1
    xg, kg, bg = gpu(x), gpu(k), gpu(b)
    packed = torch.empty(L.pwc_conv3x3_wino_packed_floats(cin, cout), device="cuda")
    _lib.check(L.pwc_conv3x3_wino_pack_f32(_p(kg), None, cin, cin, cout, _p(packed), None))
    ws = torch.full((L.pwc_conv3x3_wino_split_workspace_floats(n, h, w, cout, csplit) + 8,), float("nan"), device="cuda")
    for y_cs, slope in ((cout, 0.1), (cout + 3, None)):
        y = torch.full((n, h, w, y_cs), -7.0, device="cuda")
        _lib.check(L.pwc_conv3x3_wino_split_f32(_p(xg), cin, _p(packed), _p(bg), _p(y), y_cs, n, h, w, cin, cout, 1,
                                                0 if slope is None else 1, 0.0 if slope is None else slope, csplit, _p(ws), ws.numel(), None))
        torch.cuda.synchronize()
        close_oracle(y[..., :cout], orc.conv3x3(x, k, b, 1, 1, slope), rel=2e-5)
        if y_cs > cout:
            assert float(y[..., cout:].min()) == -7.0 and float(y[..., cout:].max()) == -7.0
