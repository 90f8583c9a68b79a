"""Flow distillation on the GPU (pwc_distill.hip, pwcnet_amd.unsup.flow_distill_*, UnsupObjective.selfsup_term, train.py
--selfsup_weight) against the float64 restatement of tests/distill_ref.py (checked on the CPU by tests/test_host_distill.py).

Sums bound, per image: |got - ref| <= (2^-24 + (2 M + 16) 2^-53) |ref|, M = 2 h w the number of terms.
  Every term rho(d) is positive, so a sum of M of them in doubles, in any order, is within (M - 1) 2^-53 of the exact sum
  relatively: once for the kernel's order (lanes, tree, parts) and once for the restatement's, 2 M 2^-53.  A term itself -- the
  exact difference of two floats, d^2 + eps^2 and a double pow -- is within a few ulps of a double on either side: 16 2^-53 for
  both.  The kernel rounds the double sum to float32 ONCE: half an ulp, 2^-24 |ref|.  At the largest shape here (M = 514) the
  double part is 2^-43, 2^-19 of the rounding it stands beside: a kernel that summed or formed its terms in float32 (errors of
  2^-24 per term and per addition) does not pass.  The counts are exact.
Gradient bound, per element: |got - ref| <= 2^-23 A, A = |ref| the magnitude of the exact value (the splat tests' rule): the value
  dsums[n] 2 q d (d^2 + eps^2)^(q - 1) is formed in double (a few 2^-53 relative) and rounded once (2^-24 A).  A pixel that does
  not contribute has A = 0: exact zeros.
Measured figures: profiles/distill_gpu_test_figures.txt."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import distill_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w, H, W, (y0, x0)): the window at the top-left corner, flush with the bottom-right corner and inside; a single pixel; 135
# pixels (two full wavefronts and a tail of 7 lanes); 257 pixels, the smallest image of more than one part (loss_common.h cuts
# an image into ceil(h w / 256) parts of 256-pixel strides): two workgroups, the second with one pixel
SHAPES = [(5, 7, 9, 13, (0, 0)), (5, 7, 9, 13, (4, 6)), (5, 7, 9, 13, (2, 3)), (1, 1, 1, 1, (0, 0)), (9, 15, 11, 17, (1, 1)),
          (1, 257, 3, 260, (2, 3))]
MASKS = ("none", "teacher", "exclude", "both")
EPS, Q = 1e-3, 0.5


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    return pwcnet_amd


def _kw(mode, tv, ex):
    return dict(teacher_valid=tv if mode in ("teacher", "both") else None, exclude=ex if mode in ("exclude", "both") else None)


@functools.lru_cache(maxsize=None)
def _case(shape, N):
    """The seeded inputs of a shape (CPU, never written to) and the restatement's (sums, counts, gradient) per mask mode."""
    h, w, H, W, offset = shape
    student, teacher, tv, ex = R.random_case(N, h, w, H, W, seed=1000 * h + 10 * w + N + offset[0])
    dsums = torch.from_numpy((np.random.RandomState(N).uniform(0.5, 2.0, size=(N,)) * np.where(np.arange(N) % 2, -1.0, 1.0))
                             .astype(np.float32))
    ref = {}
    for mode in MASKS:
        kw = _kw(mode, tv, ex)
        sums, counts = R.distill_sums(student, teacher, offset, eps=EPS, q=Q, **kw)
        ref[mode] = (sums, counts, R.distill_grad(student, teacher, dsums, offset, eps=EPS, q=Q, **kw))
    return student, teacher, tv, ex, dsums, ref


def _sums_bound(ref, h, w):
    return (2.0 ** -24 + (4.0 * h * w + 16.0) * 2.0 ** -53) * ref.abs()


def _check_sums(tag, sums, counts, ref_sums, ref_counts, h, w):
    assert sums.dtype == torch.float32 and counts.dtype == torch.int32
    assert torch.equal(counts.cpu().long(), ref_counts), (tag, counts, ref_counts)
    err, tol = (sums.cpu().double() - ref_sums).abs(), _sums_bound(ref_sums, h, w)
    worst = float((err / tol.clamp(min=1e-300)).max())
    print(f"distill sums {tag}: counts {ref_counts.tolist()}, worst error / bound {worst:.3f}")
    assert bool((err <= tol).all()), (tag, err, tol)


def _check_grad(tag, got, ref):
    err, tol = (got.cpu().double() - ref).abs(), 2.0 ** -23 * ref.abs()
    worst = float((err / tol.clamp(min=1e-300)).max())
    print(f"distill grad {tag}: worst error / bound {worst:.3f}")
    assert bool((err <= tol).all()), (tag, float(err.max()))


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_counts_and_gradient_against_float64(P, shape, N):
    h, w, H, W, offset = shape
    student, teacher, tv, ex, dsums, ref = _case(shape, N)
    s, t, dz = student.cuda(), teacher.cuda(), dsums.cuda()
    for mode in MASKS:
        kw = _kw(mode, tv.cuda(), ex.cuda())
        ref_sums, ref_counts, ref_grad = ref[mode]
        if h * w >= 35:
            # a condition on the inputs, checked in the restatement alone: a mask bug cannot hide behind an empty or a full
            # set (a single pixel is all or nothing: the 1 x 1 shape checks the geometry, not the masks)
            share = ref_counts.double() / (h * w)
            assert 0.1 <= float(share.min()) and float(share.max()) <= 0.9, (shape, N, mode, share)
        tag = f"{h}x{w} in {H}x{W} at {offset} N {N} masks {mode}"
        sums, counts = P.flow_distill_sums(s, t, offset, eps=EPS, q=Q, **kw)
        _check_sums(tag, sums, counts, ref_sums, ref_counts, h, w)
        loss = P.flow_distill_loss(s, t, offset, eps=EPS, q=Q, **kw)
        want = ref_sums.sum() / (2.0 * ref_counts.sum().clamp(min=1))
        assert abs(float(loss) - float(want)) <= 2.0 ** -21 * float(want)          # float32 sum of N and one division
        got = P.flow_distill_grad(s, t, dz, None, offset, eps=EPS, q=Q, **kw)
        _check_grad(tag, got, ref_grad)
        # the autograd backward is that op: the same bits
        sg = s.clone().requires_grad_(True)
        tg = t.clone().requires_grad_(True)                                    # the teacher is detached inside
        (P.flow_distill_sums(sg, tg, offset, eps=EPS, q=Q, **kw)[0] * dz).sum().backward()
        assert torch.equal(sg.grad, got) and tg.grad is None


def test_bool_masks_are_the_uint8_masks(P):
    shape = SHAPES[2]
    student, teacher, tv, ex, _, _ = _case(shape, 3)
    s, t = student.cuda(), teacher.cuda()
    a = P.flow_distill_sums(s, t, shape[4], teacher_valid=tv.cuda(), exclude=ex.cuda())
    b = P.flow_distill_sums(s, t, shape[4], teacher_valid=tv.cuda().bool(), exclude=ex.cuda().bool())
    c = P.flow_distill_sums(s, t, shape[4], teacher_valid=(tv * 255).cuda(), exclude=(ex * 3).cuda())     # non-zero is set
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize("cs,off", [(5, 1), (4, 2), (3, 0)])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5]])
def test_channel_slices_are_read_and_written_in_place(P, shape, cs, off):
    """Student, teacher and dstudent as channel slices of wider buffers: odd strides and offsets take the 4-byte fetch path,
    stride 4 at offset 2 the 8-byte one -- the same bits as dense tensors either way, and nothing outside the slice is written."""
    h, w, H, W, offset = shape
    N = 3
    student, teacher, tv, ex, dsums, ref = _case(shape, N)
    s, t, dz = student.cuda(), teacher.cuda(), dsums.cuda()
    kw = _kw("both", tv.cuda(), ex.cuda())
    wide_s = torch.full((N, h, w, cs), float("nan"), device="cuda")
    wide_t = torch.full((N, H, W, cs), float("nan"), device="cuda")
    wide_s[..., off:off + 2], wide_t[..., off:off + 2] = s, t
    vs, vt = wide_s[..., off:off + 2], wide_t[..., off:off + 2]
    dense = P.flow_distill_sums(s, t, offset, eps=EPS, q=Q, **kw)
    sliced = P.flow_distill_sums(vs, vt, offset, eps=EPS, q=Q, **kw)
    _check_sums(f"slices stride {cs} offset {off}", sliced[0], sliced[1], ref["both"][0], ref["both"][1], h, w)
    assert torch.equal(dense[0], sliced[0]) and torch.equal(dense[1], sliced[1])
    g_dense = P.flow_distill_grad(s, t, dz, None, offset, eps=EPS, q=Q, **kw)
    wide_d = torch.full((N, h, w, cs), -3.0, device="cuda")
    out = P.flow_distill_grad(vs, vt, dz, wide_d[..., off:off + 2], offset, eps=EPS, q=Q, **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() == wide_d[..., off:off + 2].data_ptr()
    assert torch.equal(wide_d[..., off:off + 2], g_dense)
    rest = torch.ones(cs, dtype=torch.bool)
    rest[off:off + 2] = False
    assert bool((wide_d[..., rest.cuda()] == -3.0).all())                          # the bits beside the slice are untouched
    _check_grad(f"slices stride {cs} offset {off}", wide_d[..., off:off + 2], ref["both"][2])


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5]])
def test_accumulate_adds_what_a_plain_call_writes(P, shape):
    h, w, H, W, offset = shape
    N = 3
    student, teacher, tv, ex, dsums, ref = _case(shape, N)
    s, t, dz = student.cuda(), teacher.cuda(), dsums.cuda()
    kw = _kw("both", tv.cuda(), ex.cuda())
    plain = P.flow_distill_grad(s, t, dz, None, offset, eps=EPS, q=Q, **kw)
    base = torch.from_numpy(np.random.RandomState(5).normal(size=(N, h, w, 2)).astype(np.float32)).cuda()
    acc = P.flow_distill_grad(s, t, dz, base.clone(), offset, eps=EPS, q=Q, accumulate=True, **kw)
    assert torch.equal(acc, base + plain)                                         # one float32 addition per element
    silent = ~R.contributes(student, teacher, offset, tv, ex).cuda()
    assert bool(silent.any()) and torch.equal(acc[silent], base[silent])           # pixels that do not contribute are left alone
    # NaN in the destination of a pixel that does not contribute stays what it was; without accumulate it is overwritten by 0
    dirty = torch.full((N, h, w, 2), float("nan"), device="cuda")
    P.flow_distill_grad(s, t, dz, dirty, offset, eps=EPS, q=Q, **kw)
    assert torch.equal(dirty, plain)


def test_an_all_excluded_image_gives_zeros(P):
    h, w, H, W, offset = SHAPES[2]
    N = 3
    student, teacher, tv, ex, dsums, _ = _case(SHAPES[2], N)
    s, t, dz = student.cuda(), teacher.cuda(), dsums.cuda()
    ex1 = ex.clone()
    ex1[1] = 1
    sums, counts = P.flow_distill_sums(s, t, offset, exclude=ex1.cuda())
    assert float(sums[1]) == 0.0 and int(counts[1]) == 0 and int(counts[0]) > 0 and int(counts[2]) > 0
    g = P.flow_distill_grad(s, t, dz, None, offset, exclude=ex1.cuda())
    assert bool((g[1] == 0).all()) and bool((g[0] != 0).any())
    # nothing contributes anywhere: teacher_valid all zero; the loss is 0, not 0 / 0, and its gradient is zeros
    none = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
    sums, counts = P.flow_distill_sums(s, t, offset, teacher_valid=none)
    assert bool((sums == 0).all()) and bool((counts == 0).all())
    sg = s.clone().requires_grad_(True)
    loss = P.flow_distill_loss(sg, t, offset, teacher_valid=none)
    loss.backward()
    assert float(loss.detach()) == 0.0 and bool((sg.grad == 0).all())


def test_unknown_and_non_finite_pixels_are_left_out(P):
    h, w, H, W, offset = SHAPES[2]
    N = 3
    student, teacher, _, _, dsums, _ = _case(SHAPES[2], N)
    student, teacher = student.clone(), teacher.clone()
    y0, x0 = offset
    teacher[0, y0 + 0, x0 + 0, 0] = float("nan")
    teacher[0, y0 + 1, x0 + 2, 1] = float("inf")
    teacher[1, y0 + 4, x0 + 6, 0] = -float("inf")
    teacher[1, y0 + 2, x0 + 2, 1] = 1e10
    teacher[2, y0 + 3, x0 + 1, 0] = -1e10
    teacher[2, y0 + 3, x0 + 2, 0] = 1e9                                          # at the threshold: known
    teacher[2, 0, 0] = float("nan")                                              # outside the window: never read
    student[0, 2, 2, 0] = float("nan")
    student[1, 0, 0, 1] = float("nan")
    student[2, 4, 6, 0] = float("inf")
    ref_sums, ref_counts = R.distill_sums(student, teacher, offset, eps=EPS, q=Q)
    assert bool(torch.isfinite(ref_sums).all()) and int(ref_counts.min()) > 0
    s, t, dz = student.cuda(), teacher.cuda(), dsums.cuda()
    sums, counts = P.flow_distill_sums(s, t, offset, eps=EPS, q=Q)
    _check_sums("non-finite inputs", sums, counts, ref_sums, ref_counts, h, w)
    g = P.flow_distill_grad(s, t, dz, None, offset, eps=EPS, q=Q)
    sg = s.clone().requires_grad_(True)
    loss = P.flow_distill_loss(sg, t, offset, eps=EPS, q=Q)
    loss.backward()
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss))
    assert bool(torch.isfinite(sg.grad).all())
    _check_grad("non-finite inputs", g, R.distill_grad(student, teacher, dsums, offset, eps=EPS, q=Q))
    silent = ~R.contributes(student, teacher, offset).cuda()
    assert int(silent.sum()) >= 8 and bool((g[silent] == 0).all())                 # the eight planted here and random_case's own


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4], SHAPES[5]])
def test_two_calls_and_an_image_alone_give_the_same_bits(P, shape):
    h, w, H, W, offset = shape
    N = 3
    student, teacher, tv, ex, dsums, _ = _case(shape, N)
    s, t, dz, tvg, exg = student.cuda(), teacher.cuda(), dsums.cuda(), tv.cuda(), ex.cuda()
    a = P.flow_distill_sums(s, t, offset, teacher_valid=tvg, exclude=exg)
    b = P.flow_distill_sums(s, t, offset, teacher_valid=tvg, exclude=exg)
    ga = P.flow_distill_grad(s, t, dz, None, offset, teacher_valid=tvg, exclude=exg)
    gb = P.flow_distill_grad(s, t, dz, None, offset, teacher_valid=tvg, exclude=exg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(ga, gb)
    for n in range(N):
        one = P.flow_distill_sums(s[n:n + 1], t[n:n + 1], offset, teacher_valid=tvg[n:n + 1], exclude=exg[n:n + 1])
        assert torch.equal(one[0], a[0][n:n + 1]) and torch.equal(one[1], a[1][n:n + 1]), n
        g1 = P.flow_distill_grad(s[n:n + 1], t[n:n + 1], dz[n:n + 1], None, offset, teacher_valid=tvg[n:n + 1], exclude=exg[n:n + 1])
        assert torch.equal(g1, ga[n:n + 1]), n


@pytest.mark.parametrize("mode", ["occluded", "teacher", "all"])
def test_selfsup_term_on_stacked_flows(P, mode):
    """The 2N-stacked flows go through ONE call: per image the same bits as the two directions on their own, and the term is the
    mean the two compose."""
    shape = SHAPES[4]
    h, w, H, W, offset = shape
    N = 2
    student, teacher, tv, ex, _, _ = _case(shape, 2 * N)
    s, t = student.cuda(), teacher.cuda()
    t_masks = (tv[:N].cuda().bool(), tv[N:].cuda().bool())
    s_masks = (ex[:N].cuda().bool(), ex[N:].cuda().bool())          # True where the student's own check PASSED: those are excluded
    objective = P.UnsupObjective(occlusion="fb", selfsup_mask=mode, photo_eps=EPS, photo_q=Q)
    sg = s.clone().requires_grad_(True)
    term, counts = objective.selfsup_term(sg, t, offset, t_masks, s_masks, return_counts=True)
    assert term.dim() == 0 and torch.equal(term, objective.selfsup_term(s, t, offset, t_masks, s_masks))
    parts = []
    for lo, tm, sm in ((0, t_masks[0], s_masks[0]), (N, t_masks[1], s_masks[1])):
        kw = dict(teacher_valid=tm.to(torch.uint8) if mode != "all" else None, exclude=sm.to(torch.uint8) if mode == "occluded" else None)
        parts.append(P.flow_distill_sums(s[lo:lo + N], t[lo:lo + N], offset, eps=EPS, q=Q, **kw))
    sums = torch.cat([parts[0][0], parts[1][0]])
    cnts = torch.cat([parts[0][1], parts[1][1]])
    assert torch.equal(cnts, counts) and int(cnts.min()) > 0
    assert torch.equal(term.detach(), sums.sum() / (2 * cnts.sum().clamp(min=1)).to(torch.float32))
    # against the restatement: "occluded" excludes where the student's mask is set, "teacher" and "all" do not read it
    want = R.distill_loss(student, teacher, offset, tv if mode != "all" else None, ex if mode == "occluded" else None, eps=EPS, q=Q)
    assert abs(float(term.detach()) - float(want)) <= 2.0 ** -21 * float(want)
    if mode == "all":
        assert int(cnts.sum()) > int(R.distill_sums(student, teacher, offset, tv)[1].sum())
    term.backward()
    sd = student.double().requires_grad_(True)
    ref = torch.autograd.grad(R.distill_loss(sd, teacher, offset, tv if mode != "all" else None,
                                             ex if mode == "occluded" else None, eps=EPS, q=Q), sd)[0]
    err = (sg.grad.cpu().double() - ref).abs()
    assert bool((err <= 2.0 ** -21 * ref.abs()).all())                             # the op's 2^-23 and the float32 scale 1 / (2 count)
    with pytest.raises(ValueError, match="needs occlusion"):
        P.UnsupObjective(selfsup_mask="occluded")


# ------------------------------------------------------------------ train.py
def _train(tmp_path, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                           "128", "192", "--synthetic_pairs", "6", "--loss", "unsup", "--occlusion", "fb", *flags,
                           "--model_dir", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)


def _steps(out):
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    steps = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 2, steps                       # 6 pairs: 1 for validation, 5 to train on, batch 2, drop_last
    return steps, [ln.split("global_step")[0] for ln in out.stdout.splitlines() if ln.startswith("epoch ")]


def test_train_cli_prints_a_finite_selfsup_every_step(tmp_path):
    steps, _ = _steps(_train(tmp_path, "--selfsup_weight", "0.3", "--selfsup_crop", "32"))
    for ln in steps:
        value = float(ln.split("  selfsup ")[1].split()[0])
        share = float(ln.split("  selfsup_share ")[1].split()[0])
        assert np.isfinite(value) and value >= 0 and 0.0 <= share <= 1.0, ln
        assert np.isfinite(float(ln.split("loss/unsup")[1].split()[0])), ln


def test_train_cli_weight_zero_is_the_run_without_the_flag(tmp_path):
    off = _steps(_train(tmp_path / "a"))
    zero = _steps(_train(tmp_path / "b", "--selfsup_weight", "0", "--selfsup_crop", "32"))
    assert off == zero                                  # character for character
    assert all("selfsup" not in ln for ln in off[0])


def test_train_cli_selfsup_after_starts_the_term_late(tmp_path):
    steps, _ = _steps(_train(tmp_path, "--selfsup_weight", "0.3", "--selfsup_crop", "32", "--selfsup_after", "2"))
    assert "selfsup" not in steps[0] and "  selfsup " in steps[1], steps
