"""Batched ops pinned to their one-image result at image seams (tests/seam_util.py has the construction; the helpers and the
float64 references are checked without a GPU by tests/test_host_batch_seams.py).

Almost every kernel here treats a batch as one strip of N * H rows or one list of N * H * W pixels, so the characteristic bug is
a seam bug: a halo row fetched from the neighbour, a block that straddles two images crediting the wrong one, a window clamped
against N * H, a scatter landing in the neighbour's accumulators.  For a subject image in the middle of a batch of three:

  1. isolation      f(batch)[1] is the same BITS whether the neighbours are random, copies of the subject, or poisoned (NaN
                    images, all-true masks, zero upstream, finite flows of +-H / +-2H px that point at the subject's rows);
  2. batch = single f(batch)[1] is the bits of f(subject alone)[0], per-pixel outputs, counts, masks and per-image sums alike;
  3. the single     is compared with the op's float64 reference at the op's existing bound (cited per test).
  gradients         upstream non-zero for the subject only: the neighbours' gradient is exact zeros, and with accumulate=True
                    it is bitwise what was there before.

Shapes (seam_util.SHAPES): 5 x 7 (one 256-lane block covers all three images), 9 x 13 (an image ends mid-wave), H in {1, 2, 3}
(below the windows).  No H * W is a multiple of 64, no W a multiple of 4.

Second class -- per-image sums whose partition into partial sums depends on the launch size, compared with float64 instead of
bit for bit: of the per-image sums NONE.  Two per-CALL sums are second class because they are not per image at all: the channel
sums (one vector per call, parts by pixel count; tests/test_gpu_grad.py:63, :72) and wgrad (test_wgrad_is_linear_over_images;
tests/test_gpu_grad.py:223).  The loss, metric and label-free sums cut an IMAGE (not the batch) into parts
(csrc/loss_common.h: grid.y is the image, the parts are added in index order), the distillation sums and the feature-norm
moments are doubles added in a fixed per-image order, the scatters are 64-bit fixed point: all are first class and are held to
the bits.

Isolation that cannot hold for NaN by documented contract (role FINITE in seam_util: the neighbours are poisoned with large
finite numbers instead): forward_splat / splat_grad -- one non-finite contribution anywhere in the call raises the call's ONE
poison word and every element of the result is NaN (include/pwc_hip.h, forward_splat's docstring); the deterministic warp
gradient likewise (grad_ops.warp_grad's docstring).  compose_grad's poison is per
image and is tested as such.

Coverage.  test = a test of this module; "existing" = a test that already runs N >= 2 at a seam-cutting shape against singles.
Shapes of the conv and fused cost-volume cases: H at a tile's rows and one row either side (mfma: the tile's pixel count, it
tiles the N * H * W pixels; the others: the rows stated above `_rows_around`).

  family / kernel                                   where
  ------------------------------------------------  ---------------------------------------------------------------------------
  warp bilinear, warp nearest                       test_warp
  warp with fused copy                              test_warp_with_fused_copy
  resize (x2, to odd sizes, x4 flow upsampling)     test_resize
  resize pair                                       test_resize_pair
  cost volume (pwc_cost_volume_f32, C = 16 and 20)  test_cost_volume
  cost volume concat, concat h2, blk                test_cost_volume_concat_kinds (H = 7, 8, 9 around the 4-row blocks)
  cost volume coarse, plain fused warp              test_cost_volume_coarse_and_fused_warp (H = 7, 8, 9)
  cost volume rolling                               test_cost_volume_rolling (65 x 67: the kernel's 4096-pixel threshold)
  conv3x3 mfma: every tile id, tap split 3 and 9    test_conv_mfma_tiles (H * 7 at BM - 7, BM, BM + 7 px, BM from
                                                    pwc_conv3x3_tile_shape), test_conv_mfma_tap_split (stride 1 and 2)
  conv3x3 halo                                      test_conv_halo (131 x 501: the kernel's 65536-pixel threshold)
  conv3x3 wino, wino4, h2 (default variant), direct test_conv_families, test_conv_families_at_tile_height
  conv3x3 h2 stride-2                               test_conv_h2_stride2
  conv3x3 sk (library's choice and every tile id)   test_conv_sk
  conv3x3 t32 (stride 1, 2), w32 (32, 64 channels)  test_conv_t32_w32
  conv3x3 c16pair, c3c16pair                        test_conv_c16pair, test_conv_c3c16pair
  conv dgrad (routed: stride 1 and zero-stuffed)    test_conv_dgrad_routed
  conv dgrad_s2_narrow                              test_dgrad_s2_narrow
  wgrad (linearity over images)                     test_wgrad_is_linear_over_images
  feature norm forward (+ stats), gradient          test_feature_norm, test_feature_norm_grad
  flow-norm sums and grads (masked and not),        test_flow_norm, test_flow_metrics
  flow metrics
  lrelu grad, lrelu grad + channel sums, channel    test_lrelu_grad_and_channel_sums (plain lrelu grad refuses C % 4 != 0: asserted)
  sums
  resize grad, warp grad (both forms),              test_resize_grad, test_warp_grad, test_cost_volume_grad
  cost-volume grad
  photometric sums + grad                           test_photometric
  smoothness order 1 and 2, sums + grad             test_smoothness
  census sums + grad (radius 1 and 3)               test_census
  SSIM sums + grad                                  test_ssim
  forward-backward masks + counts                   test_fb_valid
  forward-backward consistency sums + grad          test_fb_consistency
  distillation sums + grad                          test_distill
  splat (sum, average), range map, splat grad       test_splat, test_range_map
  compose, compose grad, chain_flows                test_compose, test_compose_grad_poison_is_per_image, test_chain_flows
  frame / mask pyramids                             test_pyramids
  fit / refit (resize and pad, float32 and uint8)   test_fit_and_refit
  augment (one record for every image)              test_augment
  track_points                                      test_track_points (one sequence per call: the seams are between its slices)
  visualisation: max radius, colour, error colour   test_vis (the neighbours' flows ten times the subject's)
  montage tiles                                     test_montage; existing: tests/test_gpu_vis.py::test_montage_against_restatement
                                                    (N = 2 at 23 x 37 and 24 x 40, each image alone, torch.equal)

Every case prints its figures before it asserts; a run's figures are in profiles/batch_seams_gpu_test_figures.txt."""
import numpy as np
import pytest
import torch

from tests import seam_util as su

pytestmark = pytest.mark.gpu
EPS, Q = 1e-3, 0.5


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    return pwcnet_amd


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(**tensors):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in tensors.items()}


def points_1_and_2(name, f, sub, roles):
    """Points 1 and 2; (the three batches' outputs, the single's)."""
    outs = su.check_isolation(f, sub, roles, what=name)
    single = su.check_batch_equals_single(f, sub, outs["random"], what=name)
    return outs, single


def gradient_rules(name, f, acc, sub, roles, keys):
    """f on the quiet batch (upstream for the subject only): the neighbours' `keys` are exact zeros; acc(batch, bases) -- the
    accumulating call onto pre-filled tensors -- leaves the neighbours' part bitwise alone (what it adds to the subject's is the
    op's own tests' matter)."""
    quiet = su.quiet_batch(sub, roles)
    plain = f(quiet)
    rs = np.random.RandomState(77)
    bases = {k: rs.uniform(-1, 1, plain[k].shape).astype(np.float32) for k in keys}
    after = acc(quiet, {k: v.copy() for k, v in bases.items()})
    for k in keys:
        su.check_neighbours_zero(plain[k], f"{name} {k}")
        su.check_untouched(after[k], bases[k], f"{name} {k}")


def sums_and_grad_vs_float64(name, single, ref, sub, sums=("sums",), counts=("counts",), grads=("dflow",)):
    """Point 3 of the loss terms.  Counts exact; sums 1e-5 relative (tests/test_gpu_unsup.py:70 `close(sums, s64, rel=1e-5)`, the
    same line in test_gpu_census.py:75, test_gpu_ssim.py:72, test_gpu_unflow.py:82); gradients: max-abs error over the largest
    reference element at most max(4 x the float32 run of the same formulas, 2e-5) (test_gpu_unsup.py:52 `_grad_bound`)."""
    r64, r32 = ref(sub, torch.float64), ref(sub, torch.float32)
    for k in counts:
        assert single[k].dtype == np.int32 and np.array_equal(single[k], r64[k]), (name, k, single[k], r64[k])
    for k in sums:
        err = su.rel_err(single[k], r64[k])
        print(f"{name} {k}: {single[k].tolist()} ref {r64[k].tolist()} counts {[single[c].tolist() for c in counts]} rel err {err:.3e} (bound 1e-05)")
        su.check_close(single[k], r64[k], 1e-5, f"{name} {k}")
    for k in grads:
        err, err32 = su.rel_err(single[k], r64[k]), su.rel_err(r32[k], r64[k])
        bound = max(4.0 * err32, 2e-5)
        print(f"{name} {k}: rel err HIP {err:.3e}, float32 torch {err32:.3e}, bound {bound:.3e}, max |ref| {np.abs(r64[k]).max():.3e}")
        assert np.isfinite(single[k]).all() and err <= bound, (name, k, err, bound)


# ------------------------------------------------------------------ label-free data terms
def _pair_op(sums_fn, grad_fn, **kw):
    def f(inp):
        im0, im1, fl, v, ds = (cu(inp[k]) for k in ("im0", "im1", "flow", "valid", "dsums"))
        sums, counts = sums_fn(im0, im1, fl, 1.0, v, **kw)
        return host(sums=sums, counts=counts, dflow=grad_fn(im0, im1, fl, ds, None, 1.0, v, **kw))

    def acc(inp, bases):
        im0, im1, fl, v, ds = (cu(inp[k]) for k in ("im0", "im1", "flow", "valid", "dsums"))
        return host(dflow=grad_fn(im0, im1, fl, ds, cu(bases["dflow"]), 1.0, v, accumulate=True, **kw))
    return f, acc


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_photometric(P, shape, masked):
    from pwcnet_amd import unsup as us
    name = f"photometric {shape} masked={masked}"
    sub, roles = su.pair_subject(*shape, masked=masked)
    f, acc = _pair_op(us.photometric_sums, us.photometric_grad, eps=EPS, q=Q)
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dflow",))
    sums_and_grad_vs_float64(name, single, lambda s, dt: su.ref_photometric(s, dt, EPS, Q), sub)


@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_census(P, shape, radius):
    """H <= 2 radius (here H in {1, 2, 3, 4, 5} for radius 3, {1, 2} for radius 1): counts and sums 0, no error (census_sums'
    docstring) -- asserted through the reference; those shapes pin zeros only.  A window clamped against N * H would show where
    pixels survive: radius 1 at H = 3 (3 pixels), 4, 5, 8, 9; radius 3 at H = 8 (6 pixels, one row above the 7 x 7 window) and
    9 (14)."""
    from pwcnet_amd import unsup as us
    name = f"census {shape} r{radius}"
    sub, roles = su.pair_subject(*shape)
    f, acc = _pair_op(us.census_sums, us.census_grad, radius=radius)
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dflow",))
    sums_and_grad_vs_float64(name, single, lambda s, dt: su.ref_census(s, dt, radius), sub)
    if shape[0] <= 2 * radius:
        assert single["counts"][0] == 0 and single["sums"][0] == 0 and not single["dflow"].any()


@pytest.mark.parametrize("shape", su.SHAPES)
def test_ssim(P, shape):
    """Pixels survive at H = 4 (2, one row above the 3 x 3 window around a sample), 5, 8 and 9; H <= 3 pins zeros only (a
    window and its bilinear sample do not fit into three rows)."""
    from pwcnet_amd import unsup as us
    name = f"ssim {shape}"
    sub, roles = su.pair_subject(*shape)
    f, acc = _pair_op(us.ssim_sums, us.ssim_grad, radius=1)
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dflow",))
    sums_and_grad_vs_float64(name, single, lambda s, dt: su.ref_ssim(s, dt, 1), sub)
    if shape[0] <= 2:
        assert single["counts"][0] == 0 and single["sums"][0] == 0 and not single["dflow"].any()


@pytest.mark.parametrize("with_image", [True, False])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_smoothness(P, shape, order, with_image):
    """Order 2 at H < 3 has no y terms (smoothness_sums' docstring): the reference says the same."""
    from pwcnet_amd import unsup as us
    name = f"smoothness{order} {shape} image={with_image}"
    sub, roles = su.pair_subject(*shape)

    def f(inp):
        fl, im, ds = cu(inp["flow"]), cu(inp["im0"]) if with_image else None, cu(inp["dsums"])
        return host(sums=us.smoothness_sums(fl, im, 10.0, EPS, Q, order),
                    dflow=us.smoothness_grad(fl, ds, None, im, 10.0, EPS, Q, False, order))

    def acc(inp, bases):
        fl, im, ds = cu(inp["flow"]), cu(inp["im0"]) if with_image else None, cu(inp["dsums"])
        return host(dflow=us.smoothness_grad(fl, ds, cu(bases["dflow"]), im, 10.0, EPS, Q, True, order))
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dflow",))
    sums_and_grad_vs_float64(name, single, lambda s, dt: su.ref_smoothness(s, dt, order, with_image, EPS, Q), sub, counts=())


# ------------------------------------------------------------------ forward-backward check and consistency term
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_fb_valid(P, shape, masked):
    """Point 3: the masks and counts are the reference's exactly (tests/test_gpu_fbcheck.py holds them to that away from
    near-ties; the subject is asserted to have none)."""
    from pwcnet_amd import unsup as us
    name = f"fb_valid {shape} masked={masked}"
    sub, roles = su.fb_subject(*shape, masked=masked)

    def f(inp):
        m = us.fb_valid(cu(inp["fw"]), cu(inp["bw"]), 1.0, 0.01, 0.5, cu(inp["valid_fw"]), cu(inp["valid_bw"]), return_counts=True)
        return host(mask_fw=m[0], mask_bw=m[1], counts_fw=m[2], counts_bw=m[3])
    outs, single = points_1_and_2(name, f, sub, roles)
    assert not su.ref_fb_near_ties(sub)
    ref = su.ref_fb_valid(sub)
    print(f"{name}: counts {single['counts_fw'].tolist()} {single['counts_bw'].tolist()} ref {ref['counts_fw'].tolist()} {ref['counts_bw'].tolist()}")
    for k in ref:
        assert np.array_equal(single[k], ref[k]), (name, k)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_fb_consistency(P, shape, masked):
    from pwcnet_amd import unsup as us
    name = f"fb_consistency {shape} masked={masked}"
    sub, roles = su.fb_subject(*shape, masked=masked)

    def args(inp):
        return [cu(inp[k]) for k in ("fw", "bw", "valid_fw", "valid_bw", "dsums_fw", "dsums_bw")]

    def f(inp):
        fw, bw, vf, vb, df, db = args(inp)
        s = us.fb_consistency_sums(fw, bw, 1.0, vf, vb, EPS, Q)
        g = us.fb_consistency_grad(fw, bw, df, db, None, None, 1.0, vf, vb, EPS, Q)
        return host(sums_fw=s[0], counts_fw=s[1], sums_bw=s[2], counts_bw=s[3], dfw=g[0], dbw=g[1])

    def acc(inp, bases):
        fw, bw, vf, vb, df, db = args(inp)
        g = us.fb_consistency_grad(fw, bw, df, db, cu(bases["dfw"]), cu(bases["dbw"]), 1.0, vf, vb, EPS, Q, accumulate=True)
        return host(dfw=g[0], dbw=g[1])
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dfw", "dbw"))
    sums_and_grad_vs_float64(name, single, lambda s, dt: su.ref_fb_consistency(s, dt, EPS, Q), sub, sums=("sums_fw", "sums_bw"),
                             counts=("counts_fw", "counts_bw"), grads=("dfw", "dbw"))


# ------------------------------------------------------------------ distillation
@pytest.mark.parametrize("shape", su.SHAPES)
def test_distill(P, shape):
    """Point 3 at tests/test_gpu_distill.py's bounds: counts exact, sums (2^-24 + (4 h w + 16) 2^-53) |ref| (`_sums_bound`,
    line 65), gradient 2^-23 |ref| per element (`_check_grad`, line 78)."""
    from pwcnet_amd import unsup as us
    name = f"distill {shape}"
    h, w = shape
    sub, roles = su.distill_subject(h, w)

    def args(inp):
        return [cu(inp[k]) for k in ("student", "teacher", "teacher_valid", "exclude", "dsums")]

    def f(inp):
        s, t, tv, ex, ds = args(inp)
        sums, counts = us.flow_distill_sums(s, t, su.DISTILL_OFFSET, tv, ex, EPS, Q)
        return host(sums=sums, counts=counts, dstudent=us.flow_distill_grad(s, t, ds, None, su.DISTILL_OFFSET, tv, ex, EPS, Q))

    def acc(inp, bases):
        s, t, tv, ex, ds = args(inp)
        return host(dstudent=us.flow_distill_grad(s, t, ds, cu(bases["dstudent"]), su.DISTILL_OFFSET, tv, ex, EPS, Q, accumulate=True))
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dstudent",))
    ref = su.ref_distill(sub, None, EPS, Q)
    assert np.array_equal(single["counts"], ref["counts"])
    err, tol = np.abs(single["sums"] - ref["sums"]), (2.0 ** -24 + (4.0 * h * w + 16.0) * 2.0 ** -53) * np.abs(ref["sums"])
    gerr, gtol = np.abs(single["dstudent"] - ref["dstudent"]), 2.0 ** -23 * np.abs(ref["dstudent"])
    print(f"{name}: counts {ref['counts'].tolist()}, sums worst error / bound {float((err / np.maximum(tol, 1e-300)).max()):.3f}, "
          f"gradient {float((gerr / np.maximum(gtol, 1e-300)).max()):.3f}")
    assert (err <= tol).all() and (gerr <= gtol).all()


# ------------------------------------------------------------------ splatting
def _splat_args(inp):
    return [cu(inp[k]) for k in ("x", "flow", "w", "valid", "g_out", "g_cov")]


@pytest.mark.parametrize("mode", ["sum", "average"])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_splat(P, shape, mode):
    """Point 3 at tests/test_gpu_splat.py's bounds: sum mode (and the coverage of either) 2^-24 |ref| + cnt STEP + 1e-30 (lines
    103, 129), average mode 2^-24 |ref| + e (1 + |ref|) / (D - e) + 1e-30 where the denominator is at least MIN_DEN (line 123),
    gradients 2^-23 A (line 220; average mode where every positive denominator a pixel reaches is at least MIN_DEN_GRAD)."""
    from pwcnet_amd import splat as sl
    from tests import splat_ref as sp
    from tests.test_gpu_splat import STEP
    name = f"splat {mode} {shape}"
    sub, roles = su.splat_subject(*shape)

    def f(inp):
        x, fl, w, v, go, gc = _splat_args(inp)
        out, cov = sl.forward_splat(x, fl, w, v, 1.0, mode)
        dx, dw, df = sl.splat_grad(x, fl, go, gc, w, v, 1.0, mode)
        return host(out=out, cov=cov, dx=dx, dw=dw, dflow=df)

    def acc(inp, bases):
        x, fl, w, v, go, gc = _splat_args(inp)
        dx, dw, df = sl.splat_grad(x, fl, go, gc, w, v, 1.0, mode, cu(bases["dx"]), cu(bases["dw"]), cu(bases["dflow"]), True)
        return host(dx=dx, dw=dw, dflow=df)
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dx", "dw", "dflow"))
    ref = su.ref_splat(sub, mode)
    cnt, den = ref["cnt"].astype(np.float64), ref["cov"]
    assert (np.abs(single["cov"] - den) <= 2.0 ** -24 * np.abs(den) + cnt * STEP + 1e-30).all()
    err = np.abs(single["out"] - ref["out"])
    if mode == "sum":
        bound, sel = 2.0 ** -24 * np.abs(ref["out"]) + cnt[..., None] * STEP + 1e-30, np.ones(err.shape, bool)
        gsel = np.ones(den.shape, bool)
    else:
        e = (cnt * STEP)[..., None]
        use = den >= sp.MIN_DEN
        bound = 2.0 ** -24 * np.abs(ref["out"]) + e * (1 + np.abs(ref["out"])) / (np.where(use, den, 1.0)[..., None] - e) + 1e-30
        sel = np.broadcast_to(use[..., None], err.shape)
        gsel = np.broadcast_to(not bool(((den > 0) & (den < sp.MIN_DEN_GRAD)).any()), den.shape)
        assert not single["out"][~(den > 0)].any()
    worst = float((err / bound)[sel].max()) if sel.any() else 0.0
    figures = [f"out worst error / bound {worst:.3f}"]
    assert (err <= bound)[sel].all(), name
    for k in ("dx", "dw", "dflow"):
        gerr, gtol = np.abs(single[k] - ref[k]), 2.0 ** -23 * ref[k + "_mag"]
        m = gsel if gerr.ndim == 3 else np.broadcast_to(gsel[..., None], gerr.shape)
        figures.append(f"{k} {float((gerr / np.maximum(gtol, 1e-300))[m].max()) if m.any() else 0.0:.3f}")
        assert (gerr <= gtol)[m].all(), (name, k)
    print(f"{name}: most contributions {int(cnt.max())}, " + ", ".join(figures))


@pytest.mark.parametrize("shape", su.SHAPES)
def test_range_map(P, shape):
    """The splat without a frame; point 3: the coverage bound of tests/test_gpu_splat.py:129 against splat_ref with x = None."""
    from pwcnet_amd import splat as sl
    from tests import splat_ref as sp
    from tests.test_gpu_splat import STEP
    name = f"range_map {shape}"
    sub, roles = su.splat_subject(*shape)
    sub = {k: sub[k] for k in ("flow", "valid")}

    def f(inp):
        return host(range=sl.range_map(cu(inp["flow"]), 1.0, cu(inp["valid"])))
    outs, single = points_1_and_2(name, f, sub, roles)
    _, den, cnt = sp.splat_ref(None, torch.from_numpy(sub["flow"]), None, torch.from_numpy(sub["valid"]), 1.0)
    den, cnt = den.numpy(), cnt.numpy()
    err, bound = np.abs(single["range"] - den), 2.0 ** -24 * den + cnt * STEP + 1e-30
    print(f"{name}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------ composition
def _compose_op():
    from pwcnet_amd import compose as C

    def args(inp):
        return [cu(inp[k]) for k in ("ab", "bc", "vab", "vbc", "g")]

    def f(inp):
        ab, bc, va, vb, g = args(inp)
        ac, valid = C.compose_flows(ab, bc, va, vb)
        dab, dbc = C.compose_grad(ab, bc, g, va, vb)
        return host(ac=ac, valid=valid, dab=dab, dbc=dbc)

    def acc(inp, bases):
        ab, bc, va, vb, g = args(inp)
        dab, dbc = C.compose_grad(ab, bc, g, va, vb, cu(bases["dab"]), cu(bases["dbc"]), accumulate=True)
        return host(dab=dab, dbc=dbc)
    return f, acc


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_compose(P, shape, masked):
    """Point 3 by tests/test_gpu_compose.py's own `_check_forward` and `_check_grad` (its docstring states the bounds)."""
    from tests.test_gpu_compose import _check_forward, _check_grad
    name = f"compose {shape} masked={masked}"
    sub, roles = su.compose_subject(*shape, masked=masked)
    f, acc = _compose_op()
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, acc, sub, roles, ("dab", "dbc"))
    ref = su.ref_compose(sub)
    _check_forward(name, torch.from_numpy(single["ac"]), torch.from_numpy(single["valid"]), (ref["ac"], ref["valid"], ref["ac_mag"]))
    _check_grad(name, torch.from_numpy(single["dab"]), torch.from_numpy(single["dbc"]), ref)


@pytest.mark.parametrize("shape", [(5, 7), (9, 13)])
def test_compose_grad_poison_is_per_image(P, shape):
    """compose_grad's docstring: a non-finite g at a valid pixel of an image makes THAT image's dflow_bc all NaN.  With NaN
    upstream for the neighbours: theirs is all NaN, the subject's is bitwise the single's -- and with NaN upstream for the
    subject only, the neighbours' are bitwise what they are in a clean batch."""
    name = f"compose poison {shape}"
    sub, roles = su.compose_subject(*shape, masked=False)
    f, _ = _compose_op()
    single, clean = f(sub), su.batch_of(sub, roles, "random")
    want = f(clean)
    assert single["valid"].any()
    nan_around = {k: v.copy() for k, v in clean.items() if v is not None}
    nan_around.update(vab=None, vbc=None)
    nan_around["g"][[0, 2]] = np.nan
    got = f(nan_around)
    for n in (0, 2):
        assert want["valid"][n].any() and np.isnan(got["dbc"][n]).all(), (name, n)
    for k in single:
        su.assert_same_bits(got[k][1], single[k][0], f"{name}: {k} of the subject between poisoned neighbours")
    nan_inside = {k: (None if v is None else v.copy()) for k, v in clean.items()}
    nan_inside["g"][1] = np.nan
    got = f(nan_inside)
    assert np.isnan(got["dbc"][1]).all()
    for n in (0, 2):
        for k in want:
            su.assert_same_bits(got[k][n], want[k][n], f"{name}: {k} of image {n} next to a poisoned subject")


@pytest.mark.parametrize("shape", [(5, 7), (9, 13)])
def test_chain_flows(P, shape):
    """A chain of three flows per image; point 3: the valid mask is compose_ref.chain's, the flow within 2^-22 (1 + |ref|) px
    of it -- compose_ref.chain rounds each step to float32 as the kernel stores it, so the two differ by the one-rounding bound
    of the last step and what the earlier steps' last-bit differences move the sample, both a few float32 ulps."""
    from pwcnet_amd import compose as C
    from tests import compose_ref as R
    name = f"chain {shape}"
    H, W = shape
    sub, roles = su.chain_subject(H, W)

    def f(inp):
        ac, valid = C.chain_flows([cu(inp[f"f{i}"]) for i in range(3)], [cu(inp[f"v{i}"]) for i in range(3)])
        return host(ac=ac, valid=valid)
    outs, single = points_1_and_2(name, f, sub, roles)
    ref, mask = R.chain([sub[f"f{i}"] for i in range(3)], [sub[f"v{i}"] for i in range(3)])
    assert np.array_equal(single["valid"], mask), name
    err = np.abs(single["ac"].astype(np.float64) - ref)[mask]
    print(f"{name}: valid {int(mask.sum())} of {mask.size}, max err {float(err.max()) if err.size else 0.0:.3e} px")
    assert (err <= 2.0 ** -22 * (1 + np.abs(ref[mask]))).all()


# ------------------------------------------------------------------ forward ops
@pytest.mark.parametrize("C", [4, 16])
@pytest.mark.parametrize("kind", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_warp(P, shape, kind, C):
    """Point 3: nearest is a copy (exact; the subject's flow keeps 0.15 px from the integers, where the truncation steps);
    bilinear within 2^-20 for x in [0, 1]: a weight is two differences and a product (3 roundings, 3 x 2^-24 relative), a term
    one more, and the four terms are added with one rounding each: at most 4 x 4 x 2^-24 of the largest value, 1."""
    from pwcnet_amd import modules as M
    name = f"warp {kind} {shape} C={C}"
    sub = {"x": su.subject_image(*shape, C, 300), "flow": su.subject_flow(*shape, 310)}
    roles = {"x": su.FLOAT, "flow": su.FLOW}
    layer = M.WarpingLayer(kind)

    def f(inp):
        return host(y=layer(cu(inp["x"]), cu(inp["flow"])))
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = su.warp_one(sub["x"], sub["flow"], kind == "bilinear")
    err = float(np.abs(single["y"] - ref).max())
    print(f"{name}: max err {err:.3e}")
    assert err <= (0.0 if kind == "nearest" else 2.0 ** -20)


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("factor", ["x2", "x4", "odd"])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_resize(P, shape, factor, C):
    """Point 3: oracle/torch_ref.py's resize_legacy in float64 times `mul`, at tests/test_gpu_ops.py's bound for the resize
    (`close`, line 43: 1e-5 of the largest reference value, floor 1e-6)."""
    from pwcnet_amd import modules as M
    H, W = shape
    size, mul = {"x2": ((2 * H, 2 * W), 2.0), "x4": ((4 * H, 4 * W), 20.0), "odd": ((2 * H + 1, 3 * W - 2), 1.0)}[factor]
    name = f"resize {shape} -> {size} C={C}"
    sub, roles = {"x": su.subject_image(H, W, C, 320)}, {"x": su.FLOAT}

    def f(inp):
        return host(y=M.resize_bilinear(cu(inp["x"]), size, mul))
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = su.ref_resize(size)(sub)["y"] * mul
    assert np.isfinite(single["y"]).all() and single["y"].shape == ref.shape == (1,) + size + (C,)
    err, tol = float(np.abs(single["y"] - ref).max()), max(1e-6, 1e-5 * float(np.abs(ref).max()))
    print(f"{name}: max err {err:.3e} (bound {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("C", [16, 20])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_cost_volume(P, shape, C):
    """pwc_cost_volume_f32 through CostVolumeLayer (search range 4: the 9 x 9 window is taller than every H here, so each
    image's window hangs over both seams).  Point 3: |got - ref| <= 2^-21 of the largest |ref| (C + 1 <= 21 float32 additions
    of products of values in [-1, 1], against float64)."""
    from pwcnet_amd import modules as M
    name = f"cost_volume {shape} C={C}"
    H, W = shape
    rs = np.random.RandomState(330)
    sub = {"f0": rs.uniform(-1, 1, (1, H, W, C)).astype(np.float32), "f1": rs.uniform(-1, 1, (1, H, W, C)).astype(np.float32)}
    roles = {"f0": su.FLOAT, "f1": su.FLOAT}
    layer = M.CostVolumeLayer(4)

    def f(inp):
        return host(cv=layer(cu(inp["f0"]), cu(inp["f1"])))
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = su.cost_volume_one(sub["f0"], sub["f1"])
    err = float(np.abs(single["cv"] - ref).max())
    print(f"{name}: max err {err:.3e}, max |ref| {np.abs(ref).max():.3e}")
    assert err <= 2.0 ** -21 * np.abs(ref).max()


@pytest.mark.parametrize("C", [16, 19])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_feature_norm(P, shape, C):
    """The pair's moments are taken per image: y0, y1 and the (mean, rstd) doubles.  Point 3 at tests/test_gpu_featnorm.py's
    forward bound (its docstring, line 5): |got - ref| <= 2^-24 |ref| + 2^-40 (1 + |mean| rstd); stats: line 92."""
    from pwcnet_amd import modules as M
    name = f"feature_norm {shape} C={C}"
    H, W = shape
    rs = np.random.RandomState(340)
    sub = {"f0": rs.uniform(-1, 2, (1, H, W, C)).astype(np.float32), "f1": rs.uniform(-1, 2, (1, H, W, C)).astype(np.float32)}
    roles = {"f0": su.FLOAT, "f1": su.FLOAT}
    layer = M.FeatureNormLayer()

    def f(inp):
        y0, y1, stats = layer(cu(inp["f0"]), cu(inp["f1"]), with_stats=True)
        return host(y0=y0, y1=y1, stats=stats)
    outs, single = points_1_and_2(name, f, sub, roles)
    want = su.feature_norm_one(sub["f0"], sub["f1"])
    mean, rstd = want["stats"][0]
    assert abs(single["stats"][0, 0] - mean) <= 2.0 ** -40 * abs(mean) and abs(single["stats"][0, 1] / rstd - 1) <= 2.0 ** -30
    worst = 0.0
    for k in ("y0", "y1"):
        ref = want[k]
        tol = 2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * (1 + abs(mean) * rstd)
        worst = max(worst, float((np.abs(single[k] - ref) / tol).max()))
    print(f"{name}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ pyramids and visualisation
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape", [(4, 12), (8, 4), (12, 20)])
def test_pyramids(P, shape, dtype):
    """frame_pyramid and mask_pyramid with factors (4, 2): H and W must be multiples of the largest factor, so the shapes are
    the smallest such -- 4 x 12 (one row of level cells per image: the next row of cells is the next image), 8 x 4, 12 x 20 (240
    pixels: a 256-lane block ends in the next image).  Point 3: tests/pyramid_ref.py's bits, frames, masks and counts alike
    (what tests/test_gpu_pyramid.py holds them to: the sum in double, rounded once)."""
    from pwcnet_amd import pyramid as py
    from tests import pyramid_ref as pr
    name = f"pyramids {shape} {dtype}"
    H, W = shape
    rs = np.random.RandomState(400)
    frames = rs.randint(0, 256, (1, H, W, 3)).astype(np.uint8) if dtype == "uint8" else rs.uniform(0, 1, (1, H, W, 3)).astype(np.float32)
    sub, roles = {"frames": frames, "valid": su.subject_mask(H, W, 410, 0.8)}, {"frames": su.FLOAT, "valid": su.MASK}
    factors = (4, 2)

    def f(inp):
        levels = py.frame_pyramid(cu(inp["frames"]), factors)
        masks, counts = py.mask_pyramid(cu(inp["valid"]), factors, 0.5, return_counts=True)
        out = {f"frame{k}": v for k, v in zip(factors, levels)}
        out.update({f"mask{k}": v for k, v in zip(factors, masks)})
        out.update({f"count{k}": v for k, v in zip(factors, counts)})
        return host(**out)
    outs, single = points_1_and_2(name, f, sub, roles)
    ref_frames = pr.frame_pyramid_ref(torch.from_numpy(frames), factors)
    ref_masks, ref_counts = pr.mask_pyramid_ref(torch.from_numpy(sub["valid"]), factors, 0.5)
    for k, rf, rm, rc in zip(factors, ref_frames, ref_masks, ref_counts):
        su.assert_same_bits(single[f"frame{k}"], rf.numpy(), f"{name}: level {k} against the restatement")
        assert np.array_equal(single[f"mask{k}"], rm.numpy()) and np.array_equal(single[f"count{k}"], rc.numpy()), (name, k)
    print(f"{name}: frames, masks and counts are the restatement's bits")


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_vis(P, shape, masked):
    """The per-image maximum radius is taken per image: the neighbours' flows are ten times the subject's (a radius shared
    across the seam would wash the subject's colours out).  Point 3: the radius is tests/vis_ref.py's bit for bit
    (flow_max_radius' docstring), the colours obey vis_ref.check_color, the error colours are exact (tests/test_gpu_vis.py)."""
    from pwcnet_amd import vis
    from tests import vis_ref as vr
    name = f"vis {shape} masked={masked}"
    H, W = shape
    sub, roles = su.vis_subject(H, W, masked)

    def f(inp):
        fl, gt, v = cu(inp["flow"]), cu(inp["gt"]), cu(inp["valid"])
        return host(radius=vis.flow_max_radius(fl, v), color=vis.flow_to_color(fl, None, v), error=vis.flow_error_color(fl, gt, v))
    outs, single = points_1_and_2(name, f, sub, roles)
    for n in (0, 2):
        assert outs["random"]["radius"][n] > 3 * single["radius"][0]
    su.assert_same_bits(single["radius"], vr.max_radius(sub["flow"], sub["valid"]), f"{name}: radius against numpy")
    want, t = vr.color(sub["flow"], None, sub["valid"])
    differ, near = vr.check_color(single["color"], want, t)
    assert np.array_equal(single["error"], vr.error_color(sub["flow"], sub["gt"], sub["valid"]))
    print(f"{name}: radius {single['radius'][0]:.6f} (neighbours {outs['random']['radius'][0]:.3f}, {outs['random']['radius'][2]:.3f}), "
          f"{differ} colour values differ from the restatement's ({near} under the allowance)")


# ------------------------------------------------------------------ supervised losses and metrics
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("ord", [1, 2])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_flow_norm(P, shape, ord, masked):
    """pwc_flow_norm[_masked]_sums_f32 and their gradients: a prediction at h x w against a ground truth at 2h x 2w (nearest
    down-sampling: index 2 i), gt_div 20.  The flows are compared, they steer nothing: the neighbours are poisoned with NaN.
    Point 3: counts exact, sums 1e-5 relative (tests/test_gpu_masked_loss.py:95 `close(sums, ref, rel=1e-5)`), the gradient
    2e-5 of the largest reference element (test_gpu_masked_loss.py:161 `close(got, r)`, the default of tests/test_gpu_grad.py's
    `close`).  The kernels take one `scale` per call, no per-image upstream: an image without upstream is one whose mask is all
    false (masked form) -- its dpred is exact zeros and accumulate leaves it bitwise alone; the unmasked form has no such image."""
    from pwcnet_amd import grad_ops as G
    from pwcnet_amd import losses
    name = f"flow_norm ord{ord} {shape} masked={masked}"
    h, w = shape
    rs = np.random.RandomState(500)
    sub = {"pred": rs.normal(0, 0.2, (1, h, w, 2)).astype(np.float32), "gt": rs.normal(0, 4, (1, 2 * h, 2 * w, 2)).astype(np.float32),
           "valid": su.subject_mask(2 * h, 2 * w, 510) if masked else None}
    roles = {"pred": su.FLOAT, "gt": su.FLOAT, "valid": su.MASK}

    def f(inp):
        pred, gt, v = cu(inp["pred"]), cu(inp["gt"]), cu(inp["valid"])
        res = losses._norm_sums(pred, gt, ord, 20.0, v)
        dpred = torch.empty_like(pred)
        G.flow_norm_grad(G.view_of(pred), G.view_of(gt), G.view_of(dpred), 20.0, ord, 0.5, False, v)
        out = {"sums": res[0], "dpred": dpred}
        if masked:
            out["counts"] = res[2]
        return host(**out)
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = su.flow_norm_one(sub["pred"], sub["gt"], sub["valid"], ord)
    keep, want = (sub["valid"][0, ::2, ::2] if masked else np.ones((h, w), bool)), float(ref["sums"][0])
    err = abs(float(single["sums"][0]) - want) / max(want, 1e-30)
    print(f"{name}: sum {float(single['sums'][0]):.6f} ref {want:.6f} rel err {err:.3e} (bound 1e-05)")
    assert err <= 1e-5
    if masked:
        assert int(single["counts"][0]) == int(keep.sum())
        assert not single["dpred"][0][~keep].any()
    gerr = su.rel_err(single["dpred"], ref["dpred"])
    print(f"{name}: dpred rel err {gerr:.3e} (bound 2e-05)")
    su.check_close(single["dpred"], ref["dpred"], 2e-5, f"{name} dpred")
    if masked:
        quiet = su.batch_of(sub, roles, "random")
        quiet["valid"][[0, 2]] = False
        su.check_neighbours_zero(f(quiet)["dpred"], f"{name} dpred")
        base = rs.uniform(-1, 1, quiet["pred"].shape).astype(np.float32)
        acc, qp, qg, qv = cu(base), cu(quiet["pred"]), cu(quiet["gt"]), cu(quiet["valid"])      # (Views do not own memory)
        G.flow_norm_grad(G.view_of(qp), G.view_of(qg), G.view_of(acc), 20.0, ord, 0.5, True, qv)
        su.check_untouched(host(a=acc)["a"], base, f"{name} dpred")


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_flow_metrics(P, shape, masked):
    """The (N, 12) float64 rows of pwc_flow_metrics_f32.  Point 3: the library's own float64 host path (losses.flow_metrics on
    CPU tensors): the six counts exact, the sums of end-point errors 1e-5 relative (float32 errors added per image)."""
    from pwcnet_amd import losses
    name = f"flow_metrics {shape} masked={masked}"
    H, W = shape
    rs = np.random.RandomState(520)
    gt = (rs.normal(0, 1, (1, H, W, 2)) * rs.choice([1.0, 15.0, 60.0], size=(1, H, W, 1))).astype(np.float32)
    sub = {"gt": gt, "flow": (gt + rs.normal(0, 2, gt.shape)).astype(np.float32), "valid": su.subject_mask(H, W, 530) if masked else None}
    roles = {"gt": su.FLOAT, "flow": su.FLOAT, "valid": su.MASK}

    def f(inp):
        return host(rows=losses.flow_metrics(cu(inp["gt"]), cu(inp["flow"]), cu(inp["valid"])))
    outs, single = points_1_and_2(name, f, sub, roles)
    want = losses.flow_metrics(torch.from_numpy(sub["gt"]), torch.from_numpy(sub["flow"]),
                               None if sub["valid"] is None else torch.from_numpy(sub["valid"])).numpy()
    err = np.abs(single["rows"] - want) / np.maximum(np.abs(want), 1e-30)
    print(f"{name}: rows {single['rows'][0].tolist()} worst rel err {float(err.max()):.3e}")
    counts = [i for i, n in enumerate(losses.METRIC_FIELDS) if n.startswith("n")]
    assert len(counts) >= 6 and np.array_equal(single["rows"][0, counts], want[0, counts])
    assert float(err.max()) <= 1e-5


# ------------------------------------------------------------------ training ops
GRAD_SHAPES = ((5, 7), (9, 13), (1, 9))


def _t64(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)


def _f32(rs, *shape):
    return rs.uniform(-1, 1, shape).astype(np.float32)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_lrelu_grad_and_channel_sums(P, shape, C, fused):
    """pwc_lrelu_grad_f32, pwc_lrelu_grad_channel_sums_f32 and pwc_channel_sums_f32.  The masked dy is per pixel: points 1 and 2
    bit for bit, point 3 exact (one float32 product).  The channel sums are ONE vector per call, not per image, and their
    partition into parts depends on the pixel count: second class -- with a zero dy for the neighbours the batch's sums and the
    single's are both compared with float64 at tests/test_gpu_grad.py:63 / :72 (`rel=1e-5` plain, `rel=2e-5` fused)."""
    from pwcnet_amd import grad_ops as G
    name = f"lrelu_grad C={C} {shape} fused={fused}"
    rs = np.random.RandomState(600)
    sub = {"y": _f32(rs, 1, *shape, C), "dy": _f32(rs, 1, *shape, C)}
    roles = {"y": su.FLOAT, "dy": su.UPSTREAM}
    sums = {}
    if not fused and C % 4:
        # the plain kernel is float4 only: it refuses another channel count (the fused form takes it)
        from pwcnet_amd._lib import PwcHipError
        y, dy = cu(sub["y"]), cu(sub["dy"])
        with pytest.raises(PwcHipError, match="not aligned"):
            G.lrelu_grad_(G.view_of(y), G.view_of(dy))
        return

    def f(inp):
        y, dy = cu(inp["y"]), cu(inp["dy"])
        out = torch.zeros(C, device="cuda")
        if fused:
            G.lrelu_grad_channel_sums_(G.view_of(y), G.view_of(dy), out, dy.device)
        else:
            G.lrelu_grad_(G.view_of(y), G.view_of(dy))
            G.channel_sums(G.view_of(dy), out, dy.device)
        res = host(dy=dy, out=out)
        sums[inp["y"].shape[0]] = res.pop("out")
        return res
    outs, single = points_1_and_2(name, f, sub, roles)
    want = sub["dy"] * np.where(sub["y"] > 0, np.float32(1.0), np.float32(0.1))
    assert np.array_equal(single["dy"], want), name
    su.check_neighbours_zero(f(su.quiet_batch(sub, roles))["dy"], name)
    ref, rel = want.astype(np.float64).reshape(-1, C).sum(0), (2e-5 if fused else 1e-5)
    print(f"{name}: channel sums batch - single {float(np.abs(sums[3] - sums[1]).max()):.3e}, against float64 "
          f"{su.rel_err(sums[3], ref):.3e} / {su.rel_err(sums[1], ref):.3e} (bound {rel:.0e})")
    su.check_close(sums[3], ref, rel, f"{name} sums of the batch")
    su.check_close(sums[1], ref, rel, f"{name} sums of the single")


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_resize_grad(P, shape, k):
    """Point 3: float64 autograd of oracle/torch_ref.py's resize_legacy, 2e-5 (tests/test_gpu_grad.py:84, `close`'s default)."""
    from oracle import torch_ref as tr
    from pwcnet_amd import grad_ops as G
    name = f"resize_grad x{k} {shape}"
    H, W = shape
    C = 2
    sub = {"dy": _f32(np.random.RandomState(610), 1, k * H, k * W, C)}

    def f(inp, base=None):
        dy = cu(inp["dy"])
        dx = torch.zeros((dy.shape[0], H, W, C), device="cuda") if base is None else cu(base)
        G.resize_grad(G.view_of(dy), G.view_of(dx), 1.0, base is not None)
        return host(dx=dx)
    outs, single = points_1_and_2(name, f, sub, {"dy": su.FLOAT})
    gradient_rules(name, f, lambda inp, bases: f(inp, bases["dx"]), sub, {"dy": su.UPSTREAM}, ("dx",))
    xt = _t64(np.zeros((1, H, W, C)))
    (tr.resize_legacy(xt, (k * H, k * W)) * torch.from_numpy(sub["dy"]).double()).sum().backward()
    print(f"{name}: rel err {su.rel_err(single['dx'], xt.grad.numpy()):.3e} (bound 2e-05)")
    su.check_close(single["dx"], xt.grad.numpy(), 2e-5, name)


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_warp_grad(P, shape, deterministic):
    """Both forms of the bilinear warp's gradient.  Deterministic (64-bit fixed point): dx and dflow; x and dy are FINITE -- one
    non-finite contribution makes the whole call's dx NaN by contract (grad_ops.warp_grad's docstring).  fp32 atomics: dflow
    alone (dx = None); that form's dx depends on the order of the atomics within ONE image, so no bits of it can be pinned.
    Point 3: tests/test_gpu_grad.py:100-101, dx 1e-5 and dflow 1e-4 of the largest reference element."""
    from oracle import torch_ref as tr
    from pwcnet_amd import grad_ops as G
    name = f"warp_grad {shape} deterministic={deterministic}"
    H, W = shape
    C = 4
    rs = np.random.RandomState(620)
    sub = {"x": _f32(rs, 1, H, W, C), "flow": su.subject_flow(H, W, 621), "dy": _f32(rs, 1, H, W, C)}
    roles = {"x": su.FINITE, "flow": su.FLOW, "dy": su.UPSTREAM}

    def f(inp, bases=None):
        x, fl, dy = cu(inp["x"]), cu(inp["flow"]), cu(inp["dy"])
        dfl = torch.zeros_like(fl) if bases is None else cu(bases["dflow"])
        dx = (torch.zeros_like(x) if bases is None else cu(bases["dx"])) if deterministic else None
        G.warp_grad(G.view_of(x), G.view_of(fl), 1.0, G.view_of(dy), None if dx is None else G.view_of(dx), G.view_of(dfl),
                    bases is not None, deterministic)
        return host(dx=dx, dflow=dfl) if deterministic else host(dflow=dfl)
    keys = ("dx", "dflow") if deterministic else ("dflow",)
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, f, sub, roles, keys)
    xt, ft = _t64(sub["x"]), _t64(sub["flow"])
    (tr.bilinear_warp(xt, ft) * torch.from_numpy(sub["dy"]).double()).sum().backward()
    for k, ref, rel in (("dx", xt.grad.numpy(), 1e-5), ("dflow", ft.grad.numpy(), 1e-4)):
        if k in keys:
            print(f"{name} {k}: rel err {su.rel_err(single[k], ref):.3e} (bound {rel:.0e})")
            su.check_close(single[k], ref, rel, f"{name} {k}")


@pytest.mark.parametrize("C", [8, 20])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_cost_volume_grad(P, shape, C):
    """Point 3: float64 autograd of oracle/torch_ref.py's cost_volume, 2e-5 (tests/test_gpu_grad.py:185-186)."""
    from oracle import torch_ref as tr
    from pwcnet_amd import grad_ops as G
    from pwcnet_amd import modules as M
    name = f"cost_volume_grad {shape} C={C}"
    H, W = shape
    rs = np.random.RandomState(630)
    sub = {"f0": _f32(rs, 1, H, W, C), "f1": _f32(rs, 1, H, W, C), "dcv": _f32(rs, 1, H, W, 81)}
    roles = {"f0": su.FLOAT, "f1": su.FLOAT, "dcv": su.UPSTREAM}
    layer = M.CostVolumeLayer(4)

    def f(inp, bases=None):
        f0, f1, dcv = cu(inp["f0"]), cu(inp["f1"]), cu(inp["dcv"])
        cv = layer(f0, f1).contiguous()
        d0 = torch.zeros_like(f0) if bases is None else cu(bases["df0"])
        d1 = torch.zeros_like(f1) if bases is None else cu(bases["df1"])
        G.cost_volume_grad(G.view_of(f0), G.view_of(f1), G.view_of(cv), G.view_of(dcv), G.view_of(d0), G.view_of(d1), bases is not None)
        return host(df0=d0, df1=d1)
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, f, sub, roles, ("df0", "df1"))
    a, b = _t64(sub["f0"]), _t64(sub["f1"])
    (tr.cost_volume(a, b) * torch.from_numpy(sub["dcv"]).double()).sum().backward()
    for k, ref in (("df0", a.grad.numpy()), ("df1", b.grad.numpy())):
        print(f"{name} {k}: rel err {su.rel_err(single[k], ref):.3e} (bound 2e-05)")
        su.check_close(single[k], ref, 2e-5, f"{name} {k}")


@pytest.mark.parametrize("Cx", [1, 3])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_dgrad_s2_narrow(P, shape, Cx):
    """pwc_conv3x3_dgrad_s2_narrow_f32: dy at h x w, dx at 2h x 2w.  Point 3: tests/test_gpu_dgrad_s2_narrow.py's `ref_dx`
    (float64 autograd) at its DGRAD_BOUND (line 17)."""
    from pwcnet_amd import grad_ops as G
    from tests.test_gpu_dgrad_s2_narrow import DGRAD_BOUND, ref_dx
    name = f"dgrad_s2_narrow {shape} Cx={Cx}"
    h, w = shape
    rs = np.random.RandomState(640)
    sub = {"dy": _f32(rs, 1, h, w, 16), "w": _f32(rs, 3, 3, Cx, 16) * np.float32(0.3)}

    def f(inp, bases=None):
        dy, wt = cu(inp["dy"]), cu(inp["w"])
        dx = torch.zeros((dy.shape[0], 2 * h, 2 * w, Cx), device="cuda") if bases is None else cu(bases["dx"])
        G.conv3x3_dgrad_s2_narrow(G.view_of(dy), wt, G.view_of(dx), bases is not None)
        return host(dx=dx)
    outs, single = points_1_and_2(name, f, sub, {"dy": su.FLOAT, "w": su.SHARED})
    gradient_rules(name, f, f, sub, {"dy": su.UPSTREAM, "w": su.SHARED}, ("dx",))
    err = su.rel_err(single["dx"], ref_dx(sub["dy"], sub["w"]))
    print(f"{name}: rel err {err:.3e} (bound {DGRAD_BOUND:.1e})")
    assert err <= DGRAD_BOUND


@pytest.mark.parametrize("cin,cout", [(16, 16), (3, 16)])
@pytest.mark.parametrize("shape", [(5, 7), (9, 13)])
def test_wgrad_is_linear_over_images(P, shape, cin, cout):
    """pwc_conv3x3_wgrad_f32 sums over the batch, so the property is linearity: the batch's dw equals the sum of the three
    singles, and with a zero dy for the neighbours (whatever finite x they hold) it equals the subject's single -- both within
    the existing wgrad bound, 3e-5 of the largest reference element (tests/test_gpu_grad.py:223), against float64."""
    from oracle import torch_ref as tr
    from pwcnet_amd import grad_ops as G
    name = f"wgrad {shape} {cin}->{cout}"
    H, W = shape
    rs = np.random.RandomState(650)
    x, dy = _f32(rs, 3, H, W, cin), _f32(rs, 3, H, W, cout)

    def run(x, dy):
        gx, gdy, dw = cu(x), cu(dy), torch.zeros((3, 3, cin, cout), device="cuda")
        G.conv3x3_wgrad(G.view_of(gx), G.view_of(gdy), dw, cin)
        return host(dw=dw)["dw"]

    def ref(x, dy):
        k = _t64(np.zeros((3, 3, cin, cout)))
        (tr.conv3x3_same(torch.from_numpy(x).double(), k, None, 1, 1) * torch.from_numpy(dy).double()).sum().backward()
        return k.grad.numpy()
    singles = [ref(x[n:n + 1], dy[n:n + 1]) for n in range(3)]
    whole = run(x, dy)
    quiet_dy = dy.copy()
    quiet_dy[[0, 2]] = 0
    quiet, alone = run(x, quiet_dy), run(x[1:2], dy[1:2])
    print(f"{name}: batch against the sum of singles {su.rel_err(whole, sum(singles)):.3e}, quiet batch {su.rel_err(quiet, singles[1]):.3e}, "
          f"single {su.rel_err(alone, singles[1]):.3e} (bound 3e-05), quiet - single {float(np.abs(quiet - alone).max()):.3e}")
    su.check_close(whole, sum(singles), 3e-5, f"{name} batch")
    su.check_close(quiet, singles[1], 3e-5, f"{name} quiet batch")
    su.check_close(alone, singles[1], 3e-5, f"{name} single")


# ------------------------------------------------------------------ convolution families
def _tile_rows(tile, W):
    """H such that H * W is the last whole number of rows inside the BM pixels of mfma tile `tile` (pwc_conv3x3_tile_shape)."""
    import ctypes
    from pwcnet_amd import _lib
    bm, bn = ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().pwc_conv3x3_tile_shape(tile, bm, bn) == 0
    return max(bm.value // W, 2), bn.value


def _conv_case(name, run, H, W, cin, cout, stride=1, dil=1, rel=1e-5):
    """Points 1 to 3 of one forward launch; point 3: oracle.conv3x3 at tests/test_gpu_ops.py's `close` (line 43: 1e-5 of the
    largest reference value, floor 1e-6)."""
    from oracle import oracle as orc
    rs = np.random.RandomState(660)
    sub = {"x": _f32(rs, 1, H, W, cin), "k": _f32(rs, 3, 3, cin, cout) * np.float32(1.0 / np.sqrt(9 * cin)), "b": _f32(rs, cout) * np.float32(0.1)}
    roles = {"x": su.FLOAT, "k": su.SHARED, "b": su.SHARED}

    def f(inp):
        return host(y=run(inp["x"], inp["k"], inp["b"]))
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = orc.conv3x3(sub["x"], sub["k"], sub["b"], stride, dil, 0.1)
    err, tol = float(np.abs(single["y"] - ref).max()), max(1e-6, rel * float(np.abs(ref).max()))
    print(f"{name}: max err {err:.3e} (bound {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("dh", [-1, 0, 1])
@pytest.mark.parametrize("tile", list(range(15)))
def test_conv_mfma_tiles(P, tile, dh):
    """pwc_conv3x3_f32 in every tile configuration (tests/test_gpu_ops.py::test_conv_mfma_every_tile_config's table).  The
    kernel tiles the N * H * W pixels jointly, BM to a workgroup: W = 7 and H = BM // 7 - 1, BM // 7, BM // 7 + 1 put the FIRST seam
    just inside, at the last whole row of, and just past the first tile's pixels; the second seam, at 14 H pixels, lands
    wherever that puts it (mid-tile in all but a few cases)."""
    from tests.test_gpu_ops import run_conv_mfma
    H, bn = _tile_rows(tile, 7)
    cout = {128: 128, 96: 192, 64: 64, 32: 32, 16: 48}[bn]
    _conv_case(f"conv mfma tile {tile} H={H + dh}", lambda x, k, b: run_conv_mfma(x, k, b, 1, 1, 0.1, tile=tile), H + dh, 7, 16, cout)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("split", [3, 9])
def test_conv_mfma_tap_split(P, split, stride):
    from tests.test_gpu_ops import run_conv_mfma
    _conv_case(f"conv mfma split {split} stride {stride}", lambda x, k, b: run_conv_mfma(x, k, b, stride, 1, 0.1, split=split),
               9, 13, 64, 32, stride)


@pytest.mark.parametrize("shape", [(5, 7), (9, 13), (3, 9)])
@pytest.mark.parametrize("family", ["wino", "wino4", "h2", "direct"])
def test_conv_families(P, family, shape):
    """One launch per further family through tests/test_gpu_ops.py's runners: Winograd F(2x2) and F(4x4) (odd H: an output
    tile of two or four rows hangs over the seam if rows are tiled across images), the F16-pipe direct kernel in its default
    variant, the fp32 direct kernel (3 -> 16, stride 2: the first extractor layer)."""
    from tests import test_gpu_ops as ops
    H, W = shape
    if family == "direct":
        return _conv_case(f"conv direct {shape}", lambda x, k, b: ops.run_conv_direct(x, k, b, 2, 1, 0.1), H, W, 3, 16, 2)
    run = {"wino": ops.run_conv_wino, "wino4": ops.run_conv_wino4, "h2": ops.run_conv_h2}[family]
    _conv_case(f"conv {family} {shape}", lambda x, k, b: run(x, k, b, 0.1), H, W, 16, 32)


# ------------------------------------------------------------------ fit, tracking, montage
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("mode", ["resize", "pad"])
@pytest.mark.parametrize("shape", [(5, 7), (9, 13), (1, 9)])
def test_fit_and_refit(P, shape, mode, dtype):
    """fit_frames to multiples of 4 and refit_flow back.  Point 3: tests/fit_ref.py in float64 at its BOUND (`ratio`: half an
    ulp of the largest corner, tests/test_gpu_fit.py's rule)."""
    from pwcnet_amd import fit
    from tests import fit_ref as fr
    name = f"fit {mode} {dtype} {shape}"
    H, W = shape
    sub, roles = su.fit_subject(H, W, dtype)

    def f(inp):
        fitted, info = fit.fit_frames(cu(inp["frames"]), mode, su.FIT_FACTOR)
        return host(fitted=fitted, refit=fit.refit_flow(cu(inp["flow"]), info))
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = su.ref_fit(mode, H, W)(sub)
    worst = max(float(fr.ratio(single[k], ref[k], ref[k + "_mag"]).max()) for k in ("fitted", "refit"))
    print(f"{name}: worst error / half ulp {worst:.4f} (bound {fr.BOUND})")
    assert worst <= fr.BOUND


@pytest.mark.parametrize("with_bw", [True, False])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_track_points(P, shape, with_bw):
    """A step across flow slice n reads slice n alone (seam_util.track_subject): the neighbouring slices of the sequence carry
    flows of +-H and +-2H px that would take a point into the subject's rows.  Point 3: tests/track_ref.py bit for bit."""
    from pwcnet_amd import track as T
    name = f"track {shape} bw={with_bw}"
    sub, roles = su.track_subject(*shape, with_bw)

    def on_gpu(fw, pts, bw, start, vf, vb):
        tracks, status = T.track_points(cu(fw), cu(pts), cu(bw), cu(start), None, cu(vf), cu(vb))
        res = host(t=tracks, s=status)
        return res["t"], res["s"]
    f = su.track_op(on_gpu)
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = su.ref_track(sub)
    print(f"{name}: states after the step {np.bincount(single['status'][0], minlength=5).tolist()} (UNSEEN VISIBLE LEFT OCCLUDED UNKNOWN)")
    assert (single["status"] == 1).any() or shape[0] == 1          # (one row: every point with a y flow has LEFT)
    for k in ref:
        su.assert_same_bits(single[k], ref[k], f"{name}: {k} against the restatement")


@pytest.mark.parametrize("shape", [(5, 7), (9, 13)])
def test_montage(P, shape):
    """pyramid_montage: the frame and two flow tiles, each coloured by its own per-image maximum (neighbours ten times larger).
    Point 3: tests/vis_ref.py's montage under its colour rule (tests/test_gpu_vis.py)."""
    from pwcnet_amd import vis
    from tests import vis_ref as vr
    name = f"montage {shape}"
    H, W = shape
    rs = np.random.RandomState(440)
    sub = {"frames": rs.randint(0, 256, (1, H, W, 3)).astype(np.uint8), "coarse": rs.normal(0, 3, (1, 3, 4, 2)).astype(np.float32),
           "fine": rs.normal(0, 3, (1, H, W, 2)).astype(np.float32)}
    roles = {"frames": su.FLOAT, "coarse": su.FLOW10, "fine": su.FLOW10}

    def f(inp):
        return host(m=vis.pyramid_montage(cu(inp["frames"]), [cu(inp["coarse"]), cu(inp["fine"])], [0.5, 1.0]))
    outs, single = points_1_and_2(name, f, sub, roles)
    want, t = vr.montage(sub["frames"], [sub["coarse"], sub["fine"]], [0.5, 1.0])
    differ, near = vr.check_color(single["m"], want, t, vr.montage_white(sub["frames"], [sub["coarse"], sub["fine"]], [0.5, 1.0]))
    print(f"{name}: {differ} values differ from the restatement's ({near} under the allowance)")


# ------------------------------------------------------------------ the remaining convolution families, at their tile heights
# Tile rows of each family, from the kernels' constants as tests/test_gpu_ops.py's docstrings state them: wino F(2x2) 2 output
# rows, wino4 F(4x4) 4, h2 8 (ragged 8 / 16-row x 32-column tiles), h2 stride-2 8 output rows, t32 and w32 8 x 32, c16pair and
# c3c16pair 16 x 32, sk's tile ids below.  H = m - 1, m, m + 1 with m = the tile rows (twice the rows below 8): in the strip of
# 3 H rows a seam then lies one row inside, on, and one row past a tile edge.
def _rows_around(rows):
    m = rows if rows >= 8 else 2 * rows
    return (m - 1, m, m + 1)


def _lib_conv(pack_name, pack_args, launch):
    """run(x, k, b) of a family whose entry points tests/test_gpu_ops.py calls through the library: pack, then launch(L, ...)."""
    import ctypes
    from pwcnet_amd import _lib

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def run(x, k, b):
        L = _lib.lib()
        N, H, W, cin = x.shape
        cout = k.shape[3]
        xg, kg, bg = cu(x), cu(k), cu(b)
        packed = torch.empty(getattr(L, pack_name + "_packed_floats")(*pack_args(cin, cout)), device="cuda")
        head = (p(kg), None, cin, cin) + ((cout,) if len(pack_args(cin, cout)) == 2 else ())
        _lib.check(getattr(L, pack_name + "_pack_f32")(*head, p(packed), None))
        y = launch(L, p, xg, packed, bg, N, H, W, cin, cout)
        torch.cuda.synchronize()
        return y
    return run


def _sk_launch(tile, stride):
    def launch(L, p, xg, packed, bg, N, H, W, cin, cout):
        from pwcnet_amd import _lib
        y = torch.full((N, -(-H // stride), -(-W // stride), cout), -7.0, device="cuda")
        args = (p(xg), cin, p(packed), p(bg), p(y), cout, N, H, W, cin, cout, stride, 1, 1, 0.1)
        _lib.check(L.pwc_conv3x3_sk_f32(*args, None) if tile == 0 else L.pwc_conv3x3_sk_variant_f32(*args, tile, None))
        return y
    return launch


@pytest.mark.parametrize("dh", [-1, 0, 1])
@pytest.mark.parametrize("family", ["wino", "wino4", "h2"])
def test_conv_families_at_tile_height(P, family, dh):
    from tests import test_gpu_ops as ops
    run, rows = {"wino": (ops.run_conv_wino, 2), "wino4": (ops.run_conv_wino4, 4), "h2": (ops.run_conv_h2, 8)}[family]
    H = _rows_around(rows)[dh + 1]
    _conv_case(f"conv {family} H={H}", lambda x, k, b: run(x, k, b, 0.1), H, 9, 16, 32)


@pytest.mark.parametrize("dh", [-1, 0, 1])
@pytest.mark.parametrize("tile", [0, 11, 21, 22, 31, 41, 42])
def test_conv_sk(P, tile, dh):
    """pwc_conv3x3_sk_f32 and every workgroup tile of pwc_conv3x3_sk_variant_f32 (the ids of
    tests/test_gpu_ops.py::test_conv_small_launch_kernel_vs_oracle), 64 -> 32."""
    H = (6, 7, 8)[dh + 1]
    _conv_case(f"conv sk tile {tile} H={H}", _lib_conv("pwc_conv3x3_sk", lambda ci, co: (ci, co), _sk_launch(tile, 1)), H, 9, 64, 32)


@pytest.mark.parametrize("H", _rows_around(8))
@pytest.mark.parametrize("family,cin,stride", [("t32", 32, 1), ("t32", 16, 2), ("w32", 32, 1), ("w32", 64, 1)])
def test_conv_t32_w32(P, family, cin, stride, H):
    """pwc_conv3x3_t32_f32 (stride 1 and 2) and pwc_conv3x3_w32_f32 (32 and 64 input channels: one and two K halves)."""
    def launch(L, p, xg, packed, bg, N, Hi, W, ci, cout):
        from pwcnet_amd import _lib
        y = torch.full((N, -(-Hi // stride), -(-W // stride), cout), -7.0, device="cuda")
        if family == "t32":
            _lib.check(L.pwc_conv3x3_t32_f32(p(xg), ci, p(packed), p(bg), p(y), cout, N, Hi, W, ci, cout, stride, 1, 0.1, None))
        else:
            _lib.check(L.pwc_conv3x3_w32_f32(p(xg), ci, p(packed), p(bg), p(y), cout, N, Hi, W, ci, 32, 1, 0.1, None))
        return y
    Hin = H * stride - (1 if stride == 2 else 0)          # stride 2: odd input heights, H output rows
    _conv_case(f"conv {family} {cin}->32 stride {stride} H={Hin}", _lib_conv(f"pwc_conv3x3_{family}", lambda ci, co: (ci,), launch),
               Hin, 13, cin, 32, stride)


@pytest.mark.parametrize("H", _rows_around(8))
def test_conv_h2_stride2(P, H):
    """pwc_conv3x3_h2_stride2_f32 (even input sizes only: 2 H x 18 in, H x 9 out), without the stream-K workspace.  The entry
    point is launched directly, as tests/test_gpu_ops.py does at small sizes: `_supported` answers the model's routing question,
    the launch's own return code says whether the kernel takes the geometry."""
    from pwcnet_amd import _lib

    def launch(L, p, xg, packed, bg, N, Hi, W, cin, cout):
        y = torch.full((N, Hi // 2, W // 2, cout), -7.0, device="cuda")
        _lib.check(L.pwc_conv3x3_h2_stride2_f32(p(xg), cin, p(packed), p(bg), p(y), cout, N, Hi, W, cin, cout, 1, 0.1, None, 0, None, None))
        return y
    _conv_case(f"conv h2 stride-2 H={2 * H}", _lib_conv("pwc_conv3x3_h2_stride2", lambda ci, co: (ci, co), launch), 2 * H, 18, 16, 32, 2)


def test_conv_halo(P):
    """The resident-weights halo-patch kernel takes 16 -> 16 at N * H * W >= 65536 pixels: 131 x 501 = 65 631, so that the
    single runs on it too (asserted), odd in both sizes."""
    from pwcnet_amd import _lib
    from tests.test_gpu_ops import run_conv_mfma
    H, W = 131, 501
    for n in (1, 3):
        assert _lib.lib().pwc_conv3x3_uses_halo_kernel(n * H * W, 16, 16, 1, 1) == 1
    _conv_case("conv halo 131x501", lambda x, k, b: run_conv_mfma(x, k, b, 1, 1, 0.1), H, W, 16, 16)


def _pair_case(name, run, refs, sub, roles):
    """The fused level-1 launches: points 1 to 3, point 3 the oracle's convolutions one after the other at `close`'s bound."""
    from oracle import oracle as orc
    outs, single = points_1_and_2(name, lambda inp: host(y=run(inp)), sub, roles)
    ref = sub["x"]
    for k, b, stride in refs:
        ref = orc.conv3x3(ref, sub[k], sub[b], stride, 1, 0.1)
    err, tol = float(np.abs(single["y"] - ref).max()), max(1e-6, 1e-5 * float(np.abs(ref).max()))
    print(f"{name}: max err {err:.3e} (bound {tol:.3e})")
    assert single["y"].shape == ref.shape and err <= tol


@pytest.mark.parametrize("H", _rows_around(16))
def test_conv_c16pair(P, H):
    """pwc_conv3x3_c16pair_f32: 16 -> 16 -> 16 in one launch, the intermediate in LDS (16 x 32-pixel tiles)."""
    import ctypes
    from pwcnet_amd import _lib
    rs = np.random.RandomState(670)
    sub = {"x": _f32(rs, 1, H, 13, 16), "k1": _f32(rs, 3, 3, 16, 16) / 12, "k2": _f32(rs, 3, 3, 16, 16) / 12, "b1": _f32(rs, 16) / 10, "b2": _f32(rs, 16) / 10}
    roles = {k: (su.FLOAT if k == "x" else su.SHARED) for k in sub}

    def run(inp):
        L, p = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
        xg, k1, k2, b1, b2 = (cu(inp[k]) for k in ("x", "k1", "k2", "b1", "b2"))
        packed = torch.empty(L.pwc_conv3x3_c16pair_packed_floats(), device="cuda")
        _lib.check(L.pwc_conv3x3_c16pair_pack_f32(p(k1), p(k2), p(packed), None))
        y = torch.full(tuple(xg.shape), -7.0, device="cuda")
        _lib.check(L.pwc_conv3x3_c16pair_f32(p(xg), 16, p(packed), p(b1), p(b2), p(y), 16, xg.shape[0], H, 13, 0.1, None))
        return y
    _pair_case(f"conv c16pair H={H}", run, (("k1", "b1", 1), ("k2", "b2", 1)), sub, roles)


@pytest.mark.parametrize("H", _rows_around(16))
def test_conv_c3c16pair(P, H):
    """pwc_conv3x3_c3c16pair_f32: all of pyramid level 1 from the raw frames, given as two tensors -- the batch of three is
    split 2 + 1, so the subject is the last image of the first tensor and one seam is the step from tensor to tensor.  Input
    2 H - 1 rows (odd: TF 'SAME' pads the top row), H output rows."""
    import ctypes
    from pwcnet_amd import _lib
    H0, W0 = 2 * H - 1, 28
    rs = np.random.RandomState(680)
    sub = {"x": rs.uniform(0, 1, (1, H0, W0, 3)).astype(np.float32), "k0": _f32(rs, 3, 3, 3, 16) / 5, "k1": _f32(rs, 3, 3, 16, 16) / 12,
           "k2": _f32(rs, 3, 3, 16, 16) / 12, "b0": _f32(rs, 16) / 10, "b1": _f32(rs, 16) / 10, "b2": _f32(rs, 16) / 10}
    roles = {k: (su.FLOAT if k == "x" else su.SHARED) for k in sub}

    def run(inp):
        L, p = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
        N = inp["x"].shape[0]
        Na = 2 if N == 3 else 1
        xa, xb = cu(inp["x"][:Na]), (cu(inp["x"][Na:]) if N > Na else None)
        k0, k1, k2, b0, b1, b2 = (cu(inp[k]) for k in ("k0", "k1", "k2", "b0", "b1", "b2"))
        packed = torch.empty(L.pwc_conv3x3_c3c16pair_packed_floats(), device="cuda")
        _lib.check(L.pwc_conv3x3_c3c16pair_pack_f32(p(k0), p(k1), p(k2), p(packed), None))
        y = torch.full((N, H, W0 // 2, 16), -7.0, device="cuda")
        _lib.check(L.pwc_conv3x3_c3c16pair_f32(p(xa), Na, None if xb is None else p(xb), N - Na, p(packed), p(b0), p(b1), p(b2), p(y), 16,
                                               H0, W0, 0.1, None))
        return y
    _pair_case(f"conv c3c16pair H0={H0}", run, (("k0", "b0", 2), ("k1", "b1", 1), ("k2", "b2", 1)), sub, roles)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (9, 13)])
def test_conv_dgrad_routed(P, shape, stride):
    """grad_ops.conv3x3_dgrad (stride 1: a forward launch on the flipped kernel; stride 2: the zero-stuffed map), 16 <- 32.
    Point 3: float64 autograd of oracle/torch_ref.py's conv3x3_same at 3e-5 (tests/test_gpu_grad_ops.py:378)."""
    from oracle import torch_ref as tr
    from pwcnet_amd import grad_ops as G
    name = f"conv dgrad stride {stride} {shape}"
    h, w = shape
    rs = np.random.RandomState(690)
    sub = {"dy": _f32(rs, 1, h, w, 32), "k": _f32(rs, 3, 3, 16, 32) * np.float32(0.2)}

    def f(inp):
        dy, k = cu(inp["dy"]), cu(inp["k"])
        dx = torch.full((dy.shape[0], stride * h, stride * w, 16), 7.0, device="cuda")
        keep = []
        G.conv3x3_dgrad(G.view_of(dy), k, G.view_of(dx), stride, 1, keep=keep, dy_tensor=dy)
        return host(dx=dx)
    outs, single = points_1_and_2(name, f, sub, {"dy": su.FLOAT, "k": su.SHARED})
    su.check_neighbours_zero(f(su.quiet_batch(sub, {"dy": su.UPSTREAM, "k": su.SHARED}))["dx"], name)
    xt = _t64(np.zeros((1, stride * h, stride * w, 16)))
    (tr.conv3x3_same(xt, torch.from_numpy(sub["k"]).double(), None, stride, 1) * torch.from_numpy(sub["dy"]).double()).sum().backward()
    print(f"{name}: rel err {su.rel_err(single['dx'], xt.grad.numpy()):.3e} (bound 3e-05)")
    su.check_close(single["dx"], xt.grad.numpy(), 3e-5, name)


# ------------------------------------------------------------------ the fused cost-volume launches
def _cv_subject(H, W, C, with_flow=True):
    rs = np.random.RandomState(700)
    sub = {"f0": _f32(rs, 1, H, W, C), "f1": _f32(rs, 1, H, W, C), "flow": su.subject_flow(H, W, 701) / np.float32(5.0) if with_flow else None}
    return sub, {"f0": su.FLOAT, "f1": su.FLOAT, "flow": su.FLOW}


def _cv_point3(name, single, sub, C, rel=4e-6, floor=4e-7):
    """tests/test_gpu_ops.py's bound for the fused launches (`close(..., rel=4e-6, floor=4e-7)`, lines 1291, 1335, 1386, 1449)
    against the oracle's warp and cost volume; the f0 copy is exact."""
    from oracle import oracle as orc
    f1w = sub["f1"] if sub["flow"] is None else orc.warp(sub["f1"], sub["flow"], "bilinear", flow_scale=5.0)
    ref = orc.cost_volume(sub["f0"], f1w, 4)
    err, tol = float(np.abs(single["cv"] - ref).max()), max(floor, rel * float(np.abs(ref).max()))
    print(f"{name}: max err {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    if "copy" in single:
        assert np.array_equal(single["copy"], sub["f0"]), name


@pytest.mark.parametrize("H", _rows_around(4))
@pytest.mark.parametrize("kind", ["concat", "concat_h2", "blk"])
def test_cost_volume_concat_kinds(P, kind, H):
    """pwc_warp_cost_volume_concat_f32, its F16-pipe form and pwc_warp_cost_volume_concat_blk_f32 through
    tests/test_gpu_ops.py's `_run_concat` (warp + cost volume + f0 copy into slices of one buffer): block rows of 4, strips of
    16 columns / 4 x 4 blocks; W = 9.  flow_scale is 5: the subject's flow is a fifth of seam_util's, the poisoned neighbours'
    +-H and +-2H become 5 H and 10 H px, through the subject's rows and out the other side of the strip."""
    from tests.test_gpu_ops import _run_concat
    C = 96 if kind == "blk" else 32
    name = f"cost_volume {kind} H={H}"
    sub, roles = _cv_subject(H, 9, C)

    def f(inp):
        E, _ = _run_concat(P, inp["f0"], inp["f1"], inp["flow"], 5.0, 84 + C + 8, True, True, f16x2=kind != "concat", blk=kind == "blk")
        return host(cv=E[..., :81].contiguous(), copy=E[..., 84:84 + C].contiguous(), pad=E[..., 81:84].contiguous())
    outs, single = points_1_and_2(name, f, sub, roles)
    _cv_point3(name, single, sub, C)


@pytest.mark.parametrize("with_flow", [True, False])
@pytest.mark.parametrize("H", _rows_around(4))
def test_cost_volume_coarse_and_fused_warp(P, H, with_flow):
    """pwc_cost_volume_coarse_f32 (warp + cost volume + f0 copy, coarse levels) and CostVolumeLayer's plain fused-warp launch."""
    from pwcnet_amd.modules import CostVolumeLayer
    C = 20
    name = f"cost_volume coarse H={H} flow={with_flow}"
    sub, roles = _cv_subject(H, 9, C, with_flow)

    def f(inp):
        f0, f1, fl = cu(inp["f0"]), cu(inp["f1"]), cu(inp["flow"])
        N = f0.shape[0]
        E = torch.full((N, H, 9, 84 + C + 4), -3.0, device="cuda")
        fused = torch.empty((N, H, 9, 81), device="cuda")
        Ev = G_view(E)
        from pwcnet_amd.modules import sub_view
        fv = None if fl is None else G_view(fl)
        CostVolumeLayer(4)._run(G_view(f0), G_view(f1), sub_view(Ev, 0, 81), flow=fv, flow_scale=5.0, f0_copy=sub_view(Ev, 84, C), coarse=True)
        CostVolumeLayer(4)._run(G_view(f0), G_view(f1), G_view(fused), flow=fv, flow_scale=5.0)
        return host(cv=E[..., :81].contiguous(), copy=E[..., 84:84 + C].contiguous(), fused=fused)
    outs, single = points_1_and_2(name, f, sub, roles)
    _cv_point3(name, single, sub, C)
    _cv_point3(name + " (plain fused warp)", {"cv": single["fused"]}, sub, C)


def G_view(t):
    from pwcnet_amd.modules import as_view
    return as_view(t)[0]


def test_cost_volume_rolling(P):
    """The rolling-window kernel takes C = 32 at 4096 pixels an image and more with out_cs % 4 == 0: 65 x 67 (a 4-row step and
    a 32-column strip both ragged), out_cs 84.  Point 3: tests/test_gpu_ops.py:1179, `close(rel=2e-6, floor=2e-7)`."""
    from pwcnet_amd import _lib
    from pwcnet_amd.modules import CostVolumeLayer, sub_view
    H, W, C = 65, 67, 32
    assert _lib.lib().pwc_cost_volume_uses_rolling_kernel(H, W, C, 4, C, C, 84) == 1
    sub, roles = _cv_subject(H, W, C, False)

    def f(inp):
        f0, f1 = cu(inp["f0"]), cu(inp["f1"])
        out = torch.full((f0.shape[0], H, W, 84), 7.0, device="cuda")
        CostVolumeLayer(4)._run(G_view(f0), G_view(f1), sub_view(G_view(out), 0, 81))
        return host(cv=out[..., :81].contiguous(), rest=out[..., 81:].contiguous())
    outs, single = points_1_and_2("cost_volume rolling", f, sub, roles)
    _cv_point3("cost_volume rolling", single, sub, C, rel=2e-6, floor=2e-7)
    assert (single["rest"] == 7.0).all()


# ------------------------------------------------------------------ warp with fused copy, resize pair, feature-norm grad
@pytest.mark.parametrize("kind", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_warp_with_fused_copy(P, shape, kind):
    """pwc_warp_copy_f32 (tests/test_gpu_ops.py::test_warp_with_fused_copy's launch): the warp as in test_warp, the copy exact."""
    from pwcnet_amd.modules import WarpingLayer, sub_view
    name = f"warp+copy {kind} {shape}"
    H, W = shape
    C = 8
    sub = {"x": su.subject_image(H, W, C, 300), "f0": su.subject_image(H, W, C, 301), "flow": su.subject_flow(H, W, 310)}
    roles = {"x": su.FLOAT, "f0": su.FLOAT, "flow": su.FLOW}

    def f(inp):
        x, f0, fl = cu(inp["x"]), cu(inp["f0"]), cu(inp["flow"])
        out, E = torch.empty_like(x), torch.full(tuple(x.shape[:3]) + (C + 12,), -4.0, device="cuda")
        WarpingLayer(kind)._run(G_view(x), G_view(fl), G_view(out), flow_scale=1.0, copy=(G_view(f0), sub_view(G_view(E), 8, C)))
        return host(y=out, E=E)
    outs, single = points_1_and_2(name, f, sub, roles)
    err = float(np.abs(single["y"] - su.warp_one(sub["x"], sub["flow"], kind == "bilinear")).max())
    print(f"{name}: max err {err:.3e}")
    assert err <= (0.0 if kind == "nearest" else 2.0 ** -20)
    assert np.array_equal(single["E"][..., 8:8 + C], sub["f0"]) and (single["E"][..., :8] == -4.0).all() and (single["E"][..., 8 + C:] == -4.0).all()


@pytest.mark.parametrize("C", [8, 20])
@pytest.mark.parametrize("shape", su.SHAPES)
def test_resize_pair(P, shape, C):
    """modules._resize_pair: flows and features of a level resized x2 in one launch.  Point 3: oracle/torch_ref.py's
    resize_legacy in float64 at tests/test_gpu_ops.py:1698's `close(rel=1e-6, floor=1e-6)`."""
    from pwcnet_amd.modules import _resize_pair, sub_view
    name = f"resize_pair {shape} C={C}"
    H, W = shape
    rs = np.random.RandomState(710)
    sub, roles = {"fl": _f32(rs, 1, H, W, 2), "ft": _f32(rs, 1, H, W, C)}, {"fl": su.FLOAT, "ft": su.FLOAT}

    def f(inp):
        fl, ft = cu(inp["fl"]), cu(inp["ft"])
        E = torch.full((fl.shape[0], 2 * H, 2 * W, 8 + C + 4), -2.0, device="cuda")
        _resize_pair(G_view(fl), sub_view(G_view(E), 4, 2), G_view(ft), sub_view(G_view(E), 8, C))
        return host(E=E)
    outs, single = points_1_and_2(name, f, sub, roles)
    for k, sl in (("fl", slice(4, 6)), ("ft", slice(8, 8 + C))):
        ref = su.ref_resize((2 * H, 2 * W))({"x": sub[k]})["y"]
        err, tol = float(np.abs(single["E"][..., sl] - ref).max()), max(1e-6, 1e-6 * float(np.abs(ref).max()))
        print(f"{name} {k}: max err {err:.3e} (bound {tol:.3e})")
        assert err <= tol


@pytest.mark.parametrize("C", [16, 19])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_feature_norm_grad(P, shape, C):
    """pwc_feature_norm_grad_f32.  Point 3: tests/featnorm_ref.py's feature_norm_grads at tests/test_gpu_featnorm.py:150's
    bound, |got - ref| <= 2^-23 A per element."""
    from pwcnet_amd import grad_ops as G
    from pwcnet_amd import modules as M
    from tests import featnorm_ref as R
    name = f"feature_norm_grad {shape} C={C}"
    H, W = shape
    rs = np.random.RandomState(720)
    sub = {"f0": rs.uniform(-1, 2, (1, H, W, C)).astype(np.float32), "f1": rs.uniform(-1, 2, (1, H, W, C)).astype(np.float32),
           "g0": _f32(rs, 1, H, W, C), "g1": _f32(rs, 1, H, W, C)}
    roles = {"f0": su.FLOAT, "f1": su.FLOAT, "g0": su.UPSTREAM, "g1": su.UPSTREAM}
    layer = M.FeatureNormLayer()

    def f(inp, bases=None):
        f0, f1, g0, g1 = (cu(inp[k]) for k in ("f0", "f1", "g0", "g1"))
        _, _, stats = layer(f0, f1, with_stats=True)
        d0 = torch.zeros_like(f0) if bases is None else cu(bases["d0"])
        d1 = torch.zeros_like(f1) if bases is None else cu(bases["d1"])
        G.feature_norm_grad(G.view_of(f0), G.view_of(f1), G.view_of(g0), G.view_of(g1), stats, G.view_of(d0), G.view_of(d1), bases is not None)
        return host(d0=d0, d1=d1)
    outs, single = points_1_and_2(name, f, sub, roles)
    gradient_rules(name, f, f, sub, roles, ("d0", "d1"))
    r0, r1, A0, A1 = R.feature_norm_grads(sub["f0"], sub["f1"], sub["g0"], sub["g1"])
    worst = max(float((np.abs(single[k] - np.asarray(r)) / (2.0 ** -23 * np.asarray(A))).max()) for k, r, A in (("d0", r0, A0), ("d1", r1, A1)))
    print(f"{name}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ augmentation
@pytest.mark.parametrize("interp", ["bilinear", "nearest"])
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape", [(5, 7), (9, 13)])
def test_augment(P, shape, dtype, interp):
    """augment_pairs with ONE record for every image (seam_util.augment_subject: zoom, rotation, shift, colour with a pow), so
    the single is comparable.  The flow is resampled and mapped, it steers nothing: NaN neighbours.  Point 3:
    tests/augment_ref.py in float64 under its `violations` (tests/test_gpu_augment.py's rule)."""
    from pwcnet_amd import augment as A
    from tests import augment_ref as ar
    name = f"augment {shape} {dtype} {interp}"
    sub, roles, crop = su.augment_subject(*shape, dtype)

    def f(inp):
        N = inp["im0"].shape[0]
        o0, o1, fl, v = A.augment_pairs(cu(inp["im0"]), cu(inp["im1"]), np.repeat(inp["record"], N, axis=0), crop, cu(inp["flow"]),
                                        cu(inp["valid"]), interp)
        return host(out0=o0, out1=o1, flow=fl, valid=v)
    outs, single = points_1_and_2(name, f, sub, roles)
    ref = su.ref_augment(crop, interp == "nearest")(sub, raw=True)
    assert ref["margin"] >= ar.MIN_MARGIN, ref["margin"]
    bad = ar.violations(single, ref)
    print(f"{name}: valid {int(single['valid'].sum())} of {single['valid'].size}, (violations, worst excess) {bad}")
    assert all(n == 0 for n, _ in bad.values()), bad
