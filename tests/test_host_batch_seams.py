"""The batch-seam checks without a GPU (tests/seam_util.py): every helper rejects a counter-example built from a reference, and
the float64 references -- the yardsticks of tests/test_gpu_batch_seams.py -- satisfy isolation and batch-equals-single themselves.
Both bit for bit, the per-image sums included."""
import numpy as np
import pytest

from tests import seam_util as su


# ------------------------------------------------------------------ the checks can fail
def _toy_op(leak=None):
    """A per-pixel op (3 x 3 box sum with zero padding, per image) and a per-image sum of it.  leak: a deliberately wrong
    variant -- "row": the box of the top row reads the previous image's last row (a halo across the seam); "credit": the last
    pixel of an image is credited to the next image's sum; "scatter": the gradient writes one element into the next image."""
    def f(inp):
        x = inp["x"].astype(np.float64)
        N, H, W = x.shape
        strip = x.reshape(N * H, W)
        out = np.zeros_like(x)
        for n in range(N):
            pad = np.zeros((H + 2, W + 2))
            pad[1:-1, 1:-1] = x[n]
            if leak == "row" and n > 0:
                pad[0, 1:-1] = strip[n * H - 1]
            for dy in range(3):
                for dx in range(3):
                    out[n] += pad[dy:dy + H, dx:dx + W]
        sums = out.reshape(N, -1).sum(axis=1)
        if leak == "credit":
            for n in range(N - 1):
                sums[n] -= out[n, -1, -1]
                sums[n + 1] += out[n, -1, -1]
        grad = inp["up"].reshape(N, 1, 1) * np.ones_like(x)
        if leak == "scatter":
            for n in range(N - 1):
                grad[n + 1, 0, 0] += inp["up"][n]
        return {"out": out, "sums": sums, "grad": grad}
    return f


def _toy_subject():
    rs = np.random.RandomState(0)
    return ({"x": rs.uniform(-1, 1, (1, 5, 7)).astype(np.float32), "up": np.array([0.75], np.float32)},
            {"x": su.FINITE, "up": su.UPSTREAM})


def test_helpers_accept_the_sound_op():
    sub, roles = _toy_subject()
    f = _toy_op()
    outs = su.check_isolation(f, sub, roles, what="toy")
    su.check_batch_equals_single(f, sub, outs["random"], what="toy")
    quiet = f(su.quiet_batch(sub, roles))
    su.check_neighbours_zero(quiet["grad"], "toy")
    su.check_close(outs["random"]["out"][1], f(sub)["out"][0], 1e-12, "toy")


def test_isolation_rejects_a_border_row_from_the_neighbour():
    sub, roles = _toy_subject()
    with pytest.raises(AssertionError, match="isolation: out"):
        su.check_isolation(_toy_op("row"), sub, roles, what="toy")


def test_batch_equals_single_rejects_a_border_row_from_the_neighbour():
    """Copies as neighbours: isolation among batches could not see a leak that is the same in all three -- the single does."""
    sub, roles = _toy_subject()
    f = _toy_op("row")
    out = f(su.batch_of(sub, roles, "copies"))
    with pytest.raises(AssertionError, match="batch against single: out"):
        su.check_batch_equals_single(f, sub, out, what="toy")


def test_both_reject_a_pixel_credited_to_the_next_image():
    sub, roles = _toy_subject()
    f = _toy_op("credit")
    with pytest.raises(AssertionError, match="isolation: sums"):
        su.check_isolation(f, sub, roles, what="toy")
    out = f(su.batch_of(sub, roles, "random"))             # (among copies what leaves an image is what comes in)
    with pytest.raises(AssertionError, match="batch against single: sums"):
        su.check_batch_equals_single(f, sub, out, what="toy")
    # second class: the key is left to the float64 rule, which rejects it too
    su.check_batch_equals_single(f, sub, out, what="toy", second_class=("sums",))
    with pytest.raises(AssertionError, match="relative error"):
        su.check_close(out["sums"][1:2], _toy_op()(sub)["sums"], 1e-5, "toy")


def test_reference_comparison_rejects_a_leaked_row():
    sub, roles = _toy_subject()
    good = _toy_op()(sub)["out"][0]
    bad = _toy_op("row")(su.batch_of(sub, roles, "random"))["out"][1]
    with pytest.raises(AssertionError, match="relative error"):
        su.check_close(bad, good, 1e-5, "toy")


def test_gradient_rules_reject_a_single_nonzero():
    sub, roles = _toy_subject()
    quiet = su.quiet_batch(sub, roles)
    g = _toy_op()(quiet)["grad"]
    su.check_neighbours_zero(g, "toy")
    g[2, 3, 4] = 1e-30
    with pytest.raises(AssertionError, match="image 2 has no upstream"):
        su.check_neighbours_zero(g, "toy")
    g[2, 3, 4] = np.nan
    with pytest.raises(AssertionError, match="image 2 has no upstream"):
        su.check_neighbours_zero(g, "toy")
    with pytest.raises(AssertionError, match="image 2 has no upstream"):       # the scatter across the seam
        su.check_neighbours_zero(_toy_op("scatter")(quiet)["grad"], "toy")
    base = np.random.RandomState(1).uniform(-1, 1, (3, 5, 7)).astype(np.float32)
    after = base.copy()
    after[1] += 1.0
    su.check_untouched(after, base, "toy")
    after[0, 4, 6] = np.nextafter(after[0, 4, 6], np.float32(2))
    with pytest.raises(AssertionError, match="accumulate onto image 0"):
        su.check_untouched(after, base, "toy")


def test_bits_tell_what_values_do_not():
    nan = np.array([np.nan], np.float32)
    assert su.same_bits(nan, nan.copy()) and not su.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not su.same_bits(np.zeros(2, np.float32), np.zeros(2, np.float64))
    with pytest.raises(AssertionError, match="first at"):
        su.assert_same_bits(np.array([1.0, 2.0], np.float32), np.array([1.0, np.nextafter(np.float32(2), np.float32(3))], np.float32), "x")


def test_poison_neighbours_are_what_the_module_says():
    sub, roles = su.pair_subject(5, 7)
    b = su.batch_of(sub, roles, "poison")
    for n in (0, 2):
        assert np.isnan(b["im0"][n]).all() and np.isnan(b["im1"][n]).all() and b["valid"][n].all() and b["dsums"][n] == 0
        assert np.isfinite(b["flow"][n]).all()
        y = b["flow"][n][..., 1]
        side = -1 if n == 0 else 1
        rows = np.arange(5)[:, None] + y            # where the neighbour's rows point, in its own frame
        target = rows + n * 5                       # ... and in the strip of 3 * 5 rows: inside the subject's rows 5 .. 9, or beyond
        assert (np.abs(y + side * 5) < 0.5).any() and (np.abs(y + side * 10) < 0.5).any()
        assert ((target > 4.5) & (target < 9.5)).any()
    assert su.same_bits(b["im0"][1], sub["im0"][0]) and su.same_bits(b["flow"][1], sub["flow"][0])


# ------------------------------------------------------------------ the references pass first
REFERENCES = {
    "photometric": (su.ref_photometric, lambda h, w: su.pair_subject(h, w), ("sums",)),
    "smoothness1": (lambda i: su.ref_smoothness(i, order=1), lambda h, w: su.pair_subject(h, w), ("sums",)),
    "smoothness2": (lambda i: su.ref_smoothness(i, order=2), lambda h, w: su.pair_subject(h, w), ("sums",)),
    "census_r1": (lambda i: su.ref_census(i, radius=1), lambda h, w: su.pair_subject(h, w), ("sums",)),
    "census_r3": (lambda i: su.ref_census(i, radius=3), lambda h, w: su.pair_subject(h, w), ("sums",)),
    "ssim": (su.ref_ssim, lambda h, w: su.pair_subject(h, w), ("sums",)),
    "fb_valid": (su.ref_fb_valid, lambda h, w: su.fb_subject(h, w), ()),
    "fb_consistency": (su.ref_fb_consistency, lambda h, w: su.fb_subject(h, w), ("sums_fw", "sums_bw")),
    "distill": (su.ref_distill, lambda h, w: su.distill_subject(h, w), ("sums",)),
    "compose": (su.ref_compose, lambda h, w: su.compose_subject(h, w), ()),
    "splat_sum": (lambda i: su.ref_splat(i, "sum"), lambda h, w: su.splat_subject(h, w), ()),
    "splat_average": (lambda i: su.ref_splat(i, "average"), lambda h, w: su.splat_subject(h, w), ()),
    "chain": (su.ref_chain, su.chain_subject, ()),
    "vis": (su.ref_vis, su.vis_subject, ()),
    "track": (su.ref_track, su.track_subject, ()),
    "track_no_bw": (su.ref_track, lambda h, w: su.track_subject(h, w, False), ()),
    "fit_resize": (None, su.fit_subject, ()),
    "fit_pad": (None, su.fit_subject, ()),
    "featnorm": (su.ref_featnorm_module, lambda h, w: _pair_of_maps(h, w, 16), ()),
    # the restatements seam_util writes itself (one image at a time by construction)
    "warp_bilinear": (su.ref_warp(True), lambda h, w: _warp_subject(h, w), ()),
    "warp_nearest": (su.ref_warp(False), lambda h, w: _warp_subject(h, w), ()),
    "cost_volume": (su.ref_cost_volume, lambda h, w: _pair_of_maps(h, w, 8), ()),
    "feature_norm": (su.ref_feature_norm, lambda h, w: _pair_of_maps(h, w, 19), ()),
    "flow_norm1": (su.ref_flow_norm(1), lambda h, w: _flow_norm_subject(h, w), ()),
    "flow_norm2": (su.ref_flow_norm(2), lambda h, w: _flow_norm_subject(h, w), ()),
    "resize": (None, lambda h, w: ({"x": su.subject_image(h, w, 2, 320)}, {"x": su.FLOAT}), ()),
}


def _pair_of_maps(h, w, C):
    rs = np.random.RandomState(340)
    return ({"f0": rs.uniform(-1, 2, (1, h, w, C)).astype(np.float32), "f1": rs.uniform(-1, 2, (1, h, w, C)).astype(np.float32)},
            {"f0": su.FLOAT, "f1": su.FLOAT})


def _warp_subject(h, w):
    return {"x": su.subject_image(h, w, 4, 300), "flow": su.subject_flow(h, w, 310)}, {"x": su.FLOAT, "flow": su.FLOW}


def _flow_norm_subject(h, w):
    rs = np.random.RandomState(500)
    return ({"pred": rs.normal(0, 0.2, (1, h, w, 2)).astype(np.float32), "gt": rs.normal(0, 4, (1, 2 * h, 2 * w, 2)).astype(np.float32),
             "valid": su.subject_mask(2 * h, 2 * w, 510)}, {"pred": su.FLOAT, "gt": su.FLOAT, "valid": su.MASK})


@pytest.mark.parametrize("shape", su.SHAPES)
@pytest.mark.parametrize("name", sorted(REFERENCES))
def test_reference_is_isolated_and_batch_equals_single(name, shape):
    f, make = REFERENCES[name][:2]
    sub, roles = make(*shape)
    if name.startswith("fit_"):
        f = su.ref_fit(name[4:], *shape)
    if name == "resize":
        f = su.ref_resize((2 * shape[0] + 1, 3 * shape[1] - 2))
    outs = su.check_isolation(f, sub, roles, what=name)
    su.check_batch_equals_single(f, sub, outs["random"], what=name)


@pytest.mark.parametrize("shape", [(4, 12), (8, 4), (12, 20)])
def test_pyramid_reference_is_isolated_and_batch_equals_single(shape):
    H, W = shape
    sub = {"frames": np.random.RandomState(400).uniform(0, 1, (1, H, W, 3)).astype(np.float32), "valid": su.subject_mask(H, W, 410, 0.8)}
    roles = {"frames": su.FLOAT, "valid": su.MASK}
    outs = su.check_isolation(su.ref_pyramids(), sub, roles, what="pyramids")
    su.check_batch_equals_single(su.ref_pyramids(), sub, outs["random"], what="pyramids")


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape", [(5, 7), (9, 13)])
def test_augment_reference_is_isolated_and_batch_equals_single(shape, dtype, nearest):
    from tests import augment_ref as ar
    sub, roles, crop = su.augment_subject(*shape, dtype)
    f = su.ref_augment(crop, nearest)
    outs = su.check_isolation(f, sub, roles, what="augment")
    single = su.check_batch_equals_single(f, sub, outs["random"], what="augment")
    assert f(sub, raw=True)["margin"] >= ar.MIN_MARGIN and single["valid"].any()
