"""GPU tests of the sparse-ground-truth path: the masked loss sums and gradient (pwc_flow_loss.hip) against float64, their
identity with the unmasked kernels under an all-ones mask, the flow-metrics kernel, the Trainer with a mask against float64
autograd (bounds and machinery of tests/test_gpu_grad.py), the sharded evaluation with metrics and the two CLIs.

Bounds: 1e-5 of the largest reference value for sums (what the existing sum kernels are held to), `close`'s default 2e-5 for
the gradient, STEP_BOUNDS of tests/test_gpu_grad.py for the Trainer; counts and the all-ones / poisoned-gt identities are
exact.  Every test prints its figures before it asserts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr
from tests import util
from tests.test_gpu_grad import (LOSS_WEIGHTS, STEP_BOUNDS, _STEP_INPUTS, _check_step, _rel_err, V, close, gpu, rnd, t64)
from tests.test_gpu_grad_ops import _PYRAMID, _wide
from tests.test_host_masked import (COUNT_COLS, SUM_COLS, assert_clear_of_thresholds, assert_summary, evaluation_case,
                                    metric_inputs, metrics_ref)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def go():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import grad_ops
    return grad_ops


@pytest.fixture(scope="module")
def ls(go):
    from pwcnet_amd import losses
    return losses


def _down(a, hw):
    """tf.image.resize_nearest_neighbor of a numpy (N,H,W[,C]) array (oracle/torch_ref.py's index)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() == 3:
        return tr.resize_nearest(t.unsqueeze(3), hw)[..., 0].numpy()
    return tr.resize_nearest(t, hw).numpy()


def _poison(gt, valid, rs):
    """gt with a mix of NaN, +Inf and the .flo sentinel 1e10 at the invalid pixels."""
    bad = gt.copy()
    k = int((~valid).sum())
    bad[~valid] = rs.choice(np.array([np.nan, np.inf, 1e10], np.float32), size=(k, 2))
    return bad


def _norm_ref(pred, gtd, vd, order):
    """Per-image float64 sums of ||pred - gtd||_order over the pixels vd selects, and their numbers."""
    N = pred.shape[0]
    sums, counts = np.zeros(N), np.zeros(N, np.int64)
    for n in range(N):
        d = pred[n][vd[n]].astype(np.float64) - gtd[n][vd[n]]
        sums[n] = np.abs(d).sum() if order == 1 else np.sqrt((d * d).sum(1)).sum()
        counts[n] = int(vd[n].sum())
    return sums, counts


# ------------------------------------------------------------------ 1. masked sums vs float64
@pytest.mark.parametrize("order", [1, 2])
def test_masked_sums_vs_float64(ls, order):
    """gt 64x128 against the five pyramid sizes and against itself, strided records, ~30 % valid, NaN / Inf / 1e10 in gt and
    NaN in pred at invalid pixels; then an image without a valid pixel."""
    N, (GH, GW) = 2, (64, 128)
    rs = np.random.RandomState(40 + order)
    gt = (rs.uniform(-60, 60, (N, GH, GW, 2))).astype(np.float32)
    for case in ("random", "one image empty"):
        valid = rs.uniform(size=(N, GH, GW)) < 0.3
        if case == "one image empty":
            valid[1] = False
        wgt, _ = _wide(gpu(_poison(gt, valid, rs)), 4, 1)
        gmask = torch.from_numpy(valid).cuda()
        for h, w in _PYRAMID[(GH, GW)] + [(GH, GW)]:
            gtd = _down(gt.astype(np.float64), (h, w)) / 20.0
            vd = _down(valid, (h, w))
            pred = (gtd + rs.uniform(-0.5, 0.5, (N, h, w, 2))).astype(np.float32)
            ref, cnt = _norm_ref(pred, gtd, vd, order)
            pred[~vd & (rs.uniform(size=vd.shape) < 0.5)] = np.nan
            wp, _ = _wide(gpu(pred), 6, 2)
            sums, _, counts = ls._norm_sums(wp[..., 2:4], wgt[..., 1:3], order, gt_div=20.0, valid=gmask)
            torch.cuda.synchronize()
            print(f"ord {order} {case} {h}x{w}: sums {sums.tolist()} ref {ref.tolist()} counts {counts.tolist()}")
            assert counts.dtype == torch.int32 and counts.cpu().tolist() == cnt.tolist(), (h, w)
            assert bool(torch.isfinite(sums).all()), (h, w)
            close(sums, ref, rel=1e-5)
            u8, _, c8 = ls._norm_sums(wp[..., 2:4], wgt[..., 1:3], order, gt_div=20.0, valid=gmask.to(torch.uint8) * 7)
            assert torch.equal(u8, sums) and torch.equal(c8, counts)
            if case == "one image empty":
                assert float(sums[1]) == 0.0 and int(counts[1]) == 0


# ------------------------------------------------------------------ 2. all-ones mask == the unmasked kernels
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("gt_hw", [(64, 128), (384, 448)])
def test_all_ones_mask_is_the_unmasked_kernel(go, ls, order, gt_hw):
    N, (GH, GW) = 2, gt_hw
    gt = rnd((N, GH, GW, 2), GH + order) * 60
    wgt, vgt = _wide(gpu(gt), 4, 1)
    ones = torch.ones((N, GH, GW), dtype=torch.bool, device="cuda")
    for h, w in _PYRAMID[gt_hw] + [gt_hw]:
        pred = _down(gt, (h, w)) / 20.0 + rnd((N, h, w, 2), h + w) * 0.5
        pred[0, 0, 0] = _down(gt, (h, w))[0, 0, 0] / np.float32(20.0)          # a zero difference
        wp, vp = _wide(gpu(pred), 6, 2)
        plain, _ = ls._norm_sums(wp[..., 2:4], wgt[..., 1:3], order, gt_div=20.0)
        masked, _, counts = ls._norm_sums(wp[..., 2:4], wgt[..., 1:3], order, gt_div=20.0, valid=ones)
        assert torch.equal(masked, plain), (h, w, masked.tolist(), plain.tolist())
        assert counts.cpu().tolist() == [h * w] * N
        base = rnd((N, h, w, 2), h * w) * 0.1
        for acc in (False, True):
            a, va = _wide(gpu(base), 8, 4)
            b, vb = _wide(gpu(base), 8, 4)
            go.flow_norm_grad(vp, vgt, va, gt_div=20.0, ord=order, scale=0.16, accumulate=acc)
            go.flow_norm_grad(vp, vgt, vb, gt_div=20.0, ord=order, scale=0.16, accumulate=acc, valid=ones)
            torch.cuda.synchronize()
            assert torch.equal(a, b), (h, w, acc)


# ------------------------------------------------------------------ 3. masked gradient vs autograd
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("gt_hw", [(64, 128), (384, 448)])
def test_masked_flow_norm_grad_vs_autograd(go, order, gt_hw):
    """The construction of test_flow_norm_grad_sweep (gt multiples of 2.5; pred equal to gt / 20 in none, one or both
    components) under a random mask, NaN / 1e10 in gt at the invalid pixels."""
    N, (GH, GW) = 2, gt_hw
    rs = np.random.RandomState(GH + order + 7)
    gt = (rs.randint(-60, 61, (N, GH, GW, 2)) * 2.5).astype(np.float32)
    valid = rs.uniform(size=(N, GH, GW)) < 0.5
    bad = gt.copy()
    bad[~valid] = rs.choice(np.array([np.nan, 1e10], np.float32), size=(int((~valid).sum()), 2))
    wgt, vgt = _wide(gpu(bad), 4, 1)
    gmask = torch.from_numpy(valid).cuda()
    scale = 0.32 / N
    for h, w in _PYRAMID[gt_hw]:
        gtd = _down(gt.astype(np.float64), (h, w)) / 20.0
        vd = _down(valid, (h, w))
        pred = gtd + rs.uniform(-0.5, 0.5, (N, h, w, 2))
        sel = rs.randint(0, 4, (N, h, w))
        pred[sel == 0] = gtd[sel == 0]
        pred[sel == 1, 0] = gtd[sel == 1, 0]
        pred[sel == 2, 1] = gtd[sel == 2, 1]
        pred = pred.astype(np.float32)
        pt = t64(pred)
        (scale * torch.linalg.vector_norm(pt - torch.from_numpy(gtd), ord=order, dim=3)[torch.from_numpy(vd)].sum()).backward()
        r = pt.grad.numpy()
        assert not r[~vd].any()
        wp, vp = _wide(gpu(pred), 6, 2)
        out, vo = _wide(torch.full((N, h, w, 2), 9.0, device="cuda"), 8, 4)
        go.flow_norm_grad(vp, vgt, vo, gt_div=20.0, ord=order, scale=scale, valid=gmask)
        torch.cuda.synchronize()
        got = out[..., 4:6]
        close(got, r)
        g = got.cpu().numpy()
        assert np.all(g[~vd] == 0.0), (h, w)                                   # written as exactly 0 over the 9.0
        ok = vd
        assert np.all(g[ok & (sel == 0)] == 0.0) and np.all(g[ok & (sel == 1), 0] == 0.0) and np.all(g[ok & (sel == 2), 1] == 0.0)
        assert np.all(out[..., :4].cpu().numpy() == 0.0) and np.all(out[..., 6:].cpu().numpy() == 0.0)
        b = rnd((N, h, w, 2), h + w) * scale
        acc, va = _wide(gpu(b), 7, 3)
        acc[..., :3] = 5.0
        acc[..., 5:] = -5.0
        go.flow_norm_grad(vp, vgt, va, gt_div=20.0, ord=order, scale=scale, accumulate=True, valid=gmask)
        torch.cuda.synchronize()
        close(acc[..., 3:5], b + r)
        assert np.array_equal(acc[..., 3:5].cpu().numpy()[~vd], b[~vd])        # untouched, bit for bit
        assert bool((acc[..., :3] == 5.0).all()) and bool((acc[..., 5:] == -5.0).all())


# ------------------------------------------------------------------ 4. metrics kernel vs float64
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 15, 17), (1, 257, 1), (2, 256, 257)])
@pytest.mark.parametrize("masked", [False, True])
def test_flow_metrics_kernel_vs_float64(ls, N, H, W, masked):
    """(2,256,257): 65 792 pixels an image, past 256 parts x 256 threads, the grid-stride loop takes a second trip."""
    gt, pred, valid = metric_inputs(N, H, W, seed=H + 3 * W, frac_valid=0.6 if masked else None)
    assert_clear_of_thresholds(gt, pred, valid)
    ref = metrics_ref(gt, pred, valid)
    wg, _ = _wide(gpu(gt), 5, 3)
    wp, _ = _wide(gpu(pred), 4, 1)
    gv = None if valid is None else torch.from_numpy(valid).cuda()
    got = ls.flow_metrics(wg[..., 3:5], wp[..., 1:3], gv)
    again = ls.flow_metrics(wg[..., 3:5], wp[..., 1:3], gv)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (N, 12) and got.is_cuda
    assert torch.equal(got, again)
    g = got.cpu().numpy()
    print(f"metrics {N}x{H}x{W} masked {masked}: sums {g[:, SUM_COLS].tolist()} ref {ref[:, SUM_COLS].tolist()}")
    assert np.array_equal(g[:, COUNT_COLS], ref[:, COUNT_COLS]), (g[:, COUNT_COLS], ref[:, COUNT_COLS])
    close(g[:, SUM_COLS], ref[:, SUM_COLS], rel=1e-5)
    if not masked:
        ones = ls.flow_metrics(wg[..., 3:5], wp[..., 1:3], torch.ones((N, H, W), dtype=torch.uint8, device="cuda"))
        assert torch.equal(ones, got)
    else:
        gt2, pred2 = gt.copy(), pred.copy()
        gt2[~valid] = np.array([np.nan, 1e10], np.float32)
        pred2[~valid] = np.nan
        assert torch.equal(ls.flow_metrics(gpu(gt2), gpu(pred2), gv), got)
        # the host form computes the same twelve values
        host = ls.flow_metrics(torch.from_numpy(gt2), torch.from_numpy(pred2), torch.from_numpy(valid)).numpy()
        assert np.array_equal(host[:, COUNT_COLS], g[:, COUNT_COLS])
        close(g[:, SUM_COLS], host[:, SUM_COLS], rel=1e-5)


def test_masked_EPE_and_losses_reduce_like_the_reference(ls):
    """EPE(valid) = sum e / sum n_valid (0 when nothing is valid); L1loss / L2loss: per-image masked sums, mean over the batch."""
    gt, pred, valid = metric_inputs(2, 16, 24, seed=3, frac_valid=0.4)
    ref = metrics_ref(gt, pred, valid)
    ggt, gp, gv = gpu(_poison(gt, valid, np.random.RandomState(1))), gpu(pred), torch.from_numpy(valid).cuda()
    close(ls.EPE(ggt, gp, gv).reshape(1), np.array([ref[:, 1].sum() / ref[:, 0].sum()]), rel=1e-5)
    close(ls.L2loss(ggt, gp, gv).reshape(1), np.array([ref[:, 1].mean()]), rel=1e-5)
    l1 = np.mean([np.abs(pred[n][valid[n]].astype(np.float64) - gt[n][valid[n]]).sum() for n in range(2)])
    close(ls.L1loss(ggt, gp, gv).reshape(1), np.array([l1]), rel=1e-5)
    assert float(ls.EPE(ggt, gp, torch.zeros_like(gv))) == 0.0


# ------------------------------------------------------------------ 5. / 6. the Trainer with a mask
def _masked_ref(w, im0, im1, gt, valid, loss):
    """Float64 autograd of the masked loss, written out: per level resize_nearest of gt / 20 and of the mask, the sum over
    the valid pixels, the mean over the batch, the level weight (robust: weight * (masked L1 + 0.02)^0.4)."""
    wt = {k: t64(v) for k, v in w.items()}
    _, pyr = tr.TorchPWCDCNet(wt)(t64(im0, False), t64(im1, False))
    g, m = t64(gt, False) / 20.0, torch.from_numpy(valid)
    total = 0.0
    for wl, fs in zip(LOSS_WEIGHTS, pyr):
        gd = tr.resize_nearest(g, fs.shape[1:3])
        md = tr.resize_nearest(m.unsqueeze(3), fs.shape[1:3])[..., 0]
        nrm = torch.linalg.vector_norm(gd - fs, ord=2 if loss == "multiscale" else 1, dim=3)
        per_image = torch.where(md, nrm, torch.zeros((), dtype=torch.float64)).sum(dim=(1, 2)).mean()
        total = total + (wl * per_image if loss == "multiscale" else wl * (per_image + 0.02) ** 0.4)
    total.backward()
    return float(total.detach()), {k: v.grad for k, v in wt.items()}, [p.detach() for p in pyr]


def _step_inputs(shape=(2, 64, 128)):
    gain, s_im, s_gt, shift = _STEP_INPUTS[shape]
    N, H, W = shape
    w = util.model_weights(False, gain=gain)
    im0, im1 = util.smooth_images(N, H, W, seed=s_im, shift=shift)
    gt = util.flow_field(N, H, W, seed=s_gt, sigma=2.0, outliers=False).astype(np.float32)
    valid = np.random.RandomState(77).uniform(size=(N, H, W)) < 0.4
    return w, im0, im1, gt, valid


@pytest.mark.parametrize("loss", ["multiscale", "robust"])
def test_trainer_with_a_mask_vs_float64_autograd(go, loss):
    """64x128, batch 2, ~40 % valid: every variable's gradient, the pyramid and the loss at the bounds
    tests/test_gpu_grad.py holds the dense step to at this size (STEP_BOUNDS, _check_step)."""
    from pwcnet_amd.train import Trainer
    shape = (2, 64, 128)
    w, im0, im1, gt, valid = _step_inputs(shape)
    ref_loss, ref_g, ref_pyr = _masked_ref(w, im0, im1, gt, valid, loss)
    tn = Trainer(weights=LOSS_WEIGHTS, gamma=0.0, lr=1e-4, use_dc=False, loss=loss, epsilon=0.02, q=0.4)
    tn.load_weights(w)
    pyr = tn.forward(gpu(im0), gpu(im1))
    pyr_err = max(_rel_err(a, b) for a, b in zip(pyr, ref_pyr))
    ggt, gv = gpu(_poison(gt, valid, np.random.RandomState(5))), torch.from_numpy(valid).cuda()
    loss_err = abs(float(tn.loss_value(ggt, gv)) - ref_loss) / abs(ref_loss)
    tn.backward(ggt, gv)
    torch.cuda.synchronize()
    got = tn.gradients()
    _check_step((False, loss, shape, True), pyr_err, loss_err, {k: _rel_err(got[k], r) for k, r in ref_g.items()})


@pytest.mark.parametrize("loss", ["multiscale", "robust"])
def test_the_mask_really_masks(go, loss):
    """From one forward: clean gt + mask and gt overwritten by 1e10 / NaN at the invalid pixels + the same mask give the same
    bits (gradients and loss); an all-ones mask gives the bits of valid=None."""
    from pwcnet_amd.train import Trainer
    w, im0, im1, gt, valid = _step_inputs()
    tn = Trainer(weights=LOSS_WEIGHTS, gamma=0.0, lr=1e-4, loss=loss, epsilon=0.02, q=0.4)
    tn.load_weights(w)
    tn.forward(gpu(im0), gpu(im1))
    gv = torch.from_numpy(valid).cuda()
    runs = []
    for g in (gpu(gt), gpu(_poison(gt, valid, np.random.RandomState(6)))):
        lv = float(tn.loss_value(g, gv))
        tn.backward(g, gv)
        torch.cuda.synchronize()
        runs.append((lv, tn.grads.clone()))
    assert np.isfinite(runs[0][0]) and runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert bool(torch.isfinite(runs[1][1]).all()) and torch.equal(runs[0][1], runs[1][1])
    ggt = gpu(gt)
    l_none = float(tn.loss_value(ggt))
    tn.backward(ggt)
    dense = tn.grads.clone()
    ones = torch.ones_like(gv)
    assert float(tn.loss_value(ggt, ones)) == l_none
    tn.backward(ggt, ones)
    torch.cuda.synchronize()
    assert torch.equal(tn.grads, dense)
    assert not torch.equal(dense, runs[0][1])                     # (and the mask does change the gradients)


# ------------------------------------------------------------------ 7. sharded evaluation with metrics
def test_evaluate_pairs_with_metrics_on_the_gpu(ls):
    """A stub forward that returns stored flows: 5 pairs of two sizes, batch 2, valid fractions 0.9 / 0.05 / 0 / 0.5 / no mask;
    every number equals the numpy float64 value over all pixels of all pairs at once."""
    from pwcnet_amd import sharding
    forward, load_pair, n, exp, per_pair = evaluation_case("cuda")
    res = sharding.evaluate_pairs(forward, load_pair, n, batch=2, device="cuda", metrics=True)
    assert res["pairs"] == exp.pop("pairs")
    print("evaluate_pairs:", {k: res[k] for k in exp}, "expected", exp)
    assert_summary(res, exp, rel=1e-5)
    assert abs(np.mean(per_pair) - exp["epe"]) > 1e-3 * exp["epe"]            # a mean of per-pair means would be seen
    assert np.allclose(res["per_pair_epe"], per_pair, rtol=1e-5, atol=0) and res["per_pair_epe"][2] == 0.0


# ------------------------------------------------------------------ 8. CLIs
def test_train_cli_with_invalid_synthetic_ground_truth(tmp_path):
    """30 % of the synthetic ground truth is 1e10: a finite loss proves those pixels were masked."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2",
                          "--crop_shape", "64", "128", "--synthetic_pairs", "8", "--synthetic_invalid", "0.3",
                          "--model_dir", str(tmp_path / "model")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 1 and "Fl-all/val" in lines[0] and "EPE/val" in lines[0], out.stdout[-1500:]
    words = lines[0].split()
    loss, epe, fl = (float(words[words.index(k) + 1]) for k in ("loss/pwc", "EPE/val", "Fl-all/val"))
    assert np.isfinite(loss) and 0 < loss < 1e3, lines[0]
    assert np.isfinite(epe) and epe < 1e3 and 0.0 <= fl <= 1.0, lines[0]


def test_evaluate_cli_honours_the_sentinel_and_a_mask_column(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from PIL import Image
    from pwcnet_amd import ckpt, flow_io
    rs = np.random.RandomState(21)
    ckpt.save_weights(str(tmp_path / "m.ckpt"), util.model_weights(False))
    lines, n_valid = [], 0
    for i in range(3):
        a = rs.uniform(0, 255, size=(64, 128, 3)).astype(np.uint8)
        Image.fromarray(a).save(tmp_path / f"a{i}.png")
        Image.fromarray(np.roll(a, i + 1, axis=1)).save(tmp_path / f"b{i}.png")
        gt = np.zeros((64, 128, 2), np.float32)
        gt[..., 0] = i + 1
        valid = rs.uniform(size=(64, 128)) < (0.2, 0.7, 0.5)[i]
        gt[~valid] = 1e10                                             # the .flo sentinel
        flow_io.write_flo(str(tmp_path / f"gt{i}.flo"), gt)
        line = f"{tmp_path / f'a{i}.png'} {tmp_path / f'b{i}.png'} {tmp_path / f'gt{i}.flo'}"
        if i == 2:                                                    # an invalid/-style mask image on top of the sentinel
            inv = rs.uniform(size=(64, 128)) < 0.5
            Image.fromarray((inv * 255).astype(np.uint8)).save(tmp_path / "inv2.png")
            line += f" {tmp_path / 'inv2.png'}"
            valid &= ~inv
        n_valid += int(valid.sum())
        lines.append(line)
    (tmp_path / "pairs.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--list", str(tmp_path / "pairs.txt"),
                          "--resume", str(tmp_path / "m.ckpt"), "--batch", "2", "--mask_is_invalid"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("epe", "fl_all", "px1", "px3", "px5", "epe_s0_10", "epe_s10_40", "epe_s40", "valid_px", "per_pair_epe"):
        assert k in res, k
    assert res["valid_px"] == n_valid and res["pairs"] == 3
    assert np.isfinite(res["epe"]) and res["epe"] < 100 and 0.0 <= res["fl_all"] <= 1.0
    assert res["epe_s0_10"] is not None and res["epe_s10_40"] is None and res["epe_s40"] is None     # ||gt|| is 1, 2 or 3
    assert len(res["per_pair_epe"]) == 3 and all(np.isfinite(v) for v in res["per_pair_epe"])
