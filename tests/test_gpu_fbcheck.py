"""GPU tests of the forward-backward occlusion masks (csrc/pwc_fbcheck.hip, pwcnet_amd.unsup.fb_valid) against the float64
restatement of tests/fb_ref.py (validated on the CPU by tests/test_host_fbcheck.py) on its cases: 23 x 37 (odd sizes, tail lanes)
and 272 x 256 (more than 256 parts per image: the grid-stride loop and the capped partition), wide-stride views, flow_scale in
{1, 5}, (alpha1, alpha2) in {(0.01, 0.5), (0, 0.25)}, ~70 % input masks with NaN behind them, an image that is out of frame
everywhere, NaN and Inf at unmasked pixels.

Bounds.  The masks are decisions: they equal the reference at EVERY pixel outside the near-tie set (candidates whose margin is
within 1e-9 * max(1, bound) of 0; the kernel computes in double, a different order of a few dozen float64 operations moves the
margin by ~1e-15 of the bound) -- tests/test_host_fbcheck.py caps that set at 0.1 % of the candidates on the inputs alone, and
here its size and the disagreements inside it are printed, not asserted.  Counts: exactly the mask's sum, and the reference's up
to the number of near-ties.  Composition with the data terms: the sum bound of tests/test_gpu_unsup.py and test_gpu_census.py,
1e-5 relative.  Measured on an MI355X (profiles/fbcheck_gpu_test_figures.txt): no near-tie and no disagreement in any case, counts
equal to the reference's, losses 2.0e-8 ... 1.9e-7 off."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import census_ref as cr
from tests import fb_ref as fr
from tests import unsup_ref as ur
from tests.test_gpu_grad import gpu
from tests.test_gpu_grad_ops import _wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(fr.CASES)


@pytest.fixture(scope="module")
def us():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from pwcnet_amd import unsup
    return unsup


def _inputs(case, poisoned=True):
    """The case on the GPU: the flows as channel slices of wider buffers (`_wide`), NaN behind the masks, and the masks."""
    k = "_nan" if poisoned else ""
    fw = _wide(gpu(case["fw" + k]), 6, 3)[0][..., 3:5]
    bw = _wide(gpu(case["bw" + k]), 3, 1)[0][..., 1:3]
    vf = None if case["valid_fw"] is None else torch.from_numpy(case["valid_fw"]).cuda()
    vb = None if case["valid_bw"] is None else torch.from_numpy(case["valid_bw"]).cuda()
    return fw, bw, vf, vb


def _check_direction(what, mask, counts, d):
    """mask, counts from the GPU against Direction d of the reference."""
    N, H, W = d.mask.shape
    assert mask.dtype == torch.bool and tuple(mask.shape) == (N, H, W) and mask.is_contiguous()
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (N,)
    got = mask.cpu()
    ties = fr.near_ties(d)
    differ = got != d.mask
    per_image = ties.sum(dim=(1, 2))
    print(f"{what}: counts {counts.tolist()} ref {d.counts.tolist()}; near-ties {int(ties.sum())} of {int(d.candidate.sum())} candidates, "
          f"disagreements inside them {int((differ & ties).sum())}, outside {int((differ & ~ties).sum())}")
    assert not bool((differ & ~ties).any())
    assert not bool(got[~d.candidate].any())             # masked out, NaN, Inf, out of frame: 0
    assert counts.cpu().tolist() == got.sum(dim=(1, 2)).tolist()
    assert bool(((counts.cpu().long() - d.counts).abs() <= per_image).all())


@pytest.mark.parametrize("name", NAMES)
def test_masks_and_counts_vs_float64(us, name):
    ref = fr.reference(name)
    case = ref["case"]
    a1, a2 = case["alphas"]
    fw, bw, vf, vb = _inputs(case)
    m_fw, m_bw, c_fw, c_bw = us.fb_valid(fw, bw, case["flow_scale"], a1, a2, vf, vb, return_counts=True)
    again = us.fb_valid(fw, bw, case["flow_scale"], a1, a2, vf, vb, return_counts=True)
    plain = us.fb_valid(fw.detach().requires_grad_(True), bw, case["flow_scale"], a1, a2, vf, vb)
    torch.cuda.synchronize()
    _check_direction(name + " fw", m_fw, c_fw, ref["a"])
    _check_direction(name + " bw", m_bw, c_bw, ref["b"])
    for x, y in zip((m_fw, m_bw, c_fw, c_bw), again):
        assert torch.equal(x, y)
    assert len(plain) == 2 and torch.equal(plain[0], m_fw) and torch.equal(plain[1], m_bw) and not plain[0].requires_grad
    # the masks are bytes 0 / 1
    assert set(m_fw.view(torch.uint8).unique().tolist()) <= {0, 1} and set(m_bw.view(torch.uint8).unique().tolist()) <= {0, 1}
    if vf is not None:                          # a uint8 mask with other non-zero values is the same mask
        m8 = us.fb_valid(fw, bw, case["flow_scale"], a1, a2, vf.to(torch.uint8) * 7, vb.to(torch.uint8) * 7, return_counts=True)
        for x, y in zip((m_fw, m_bw, c_fw, c_bw), m8):
            assert torch.equal(x, y)
        assert not bool(m_fw[~vf].any()) and not bool(m_bw[~vb].any())
    if case["empty"] is not None:
        assert int(c_fw[case["empty"]]) == 0 and int(c_bw[case["empty"]]) == 0
    if case["nonfinite"]:
        for flow, mask in ((case["fw"], m_fw), (case["bw"], m_bw)):
            bad = torch.from_numpy(~np.isfinite(flow).all(axis=3)).cuda()
            assert int(bad.sum()) > 0 and not bool(mask[bad].any())


@pytest.mark.parametrize("name", ["23x37_s1_a", "272x256_s5_a"])
def test_c_entry_writes_inside_its_masks_and_one_direction_on_request(us, name):
    """Through ctypes: both directions into buffers with a guard band of 0xAB on either side (23 x 37 x 2 = 1702 bytes is no
    multiple of 4), then valid_b = NULL -- only direction a is computed."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    ref = fr.reference(name)
    case = ref["case"]
    N, H, W = case["N"], case["H"], case["W"]
    a1, a2 = case["alphas"]
    fw, bw, vf, vb = _inputs(case)
    want = us.fb_valid(fw, bw, case["flow_scale"], a1, a2, vf, vb, return_counts=True)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    G, npix = 256, N * H * W
    bufs = [torch.full((G + npix + G,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    counts = [torch.full((N + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    ws = torch.zeros((L.pwc_fb_workspace_floats(N, H, W),), dtype=torch.float32, device="cuda")
    args = (p(fw), fw.stride(2), p(bw), bw.stride(2), case["flow_scale"], p(vf), p(vb), N, H, W, a1, a2)
    rc = L.pwc_fb_valid_u8(*args, p(bufs[0][G:]), p(bufs[1][G:]), p(counts[0][1:]), p(counts[1][1:]), p(ws), ws.numel(),
                           _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    for buf, cnt, mask, c in zip(bufs, counts, want[:2], want[2:]):
        assert bool((buf[:G] == 0xAB).all()) and bool((buf[G + npix:] == 0xAB).all())
        assert torch.equal(buf[G:G + npix].view(N, H, W), mask.view(torch.uint8))
        assert cnt[0].item() == -7 and cnt[-1].item() == -7 and torch.equal(cnt[1:-1], c)
    # direction a alone, without counts and without a workspace
    only = torch.full((G + npix + G,), 0xAB, dtype=torch.uint8, device="cuda")
    rc = L.pwc_fb_valid_u8(*args, p(only[G:]), None, None, None, None, 0, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(only, bufs[0])
    # ... and with its counts
    only.fill_(0xAB)
    cnt = torch.full((N + 2,), -7, dtype=torch.int32, device="cuda")
    rc = L.pwc_fb_valid_u8(*args, p(only[G:]), None, p(cnt[1:]), None, p(ws), ws.numel(), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(only, bufs[0]) and torch.equal(cnt, counts[0])


# ------------------------------------------------------------------ composition with the data terms
@pytest.mark.parametrize("name", ["23x37_s1_a", "272x256_s5_a"])
def test_masks_go_straight_into_the_data_terms(us, name):
    """photometric_loss and census_loss take mask_fw as returned; they equal the float64 restatements run with the REFERENCE
    mask.  The case has no near-tie (a fact of its inputs, asserted first), so the two masks are the same mask."""
    ref = fr.reference(name)
    case, d = ref["case"], ref["a"]
    assert int(fr.near_ties(d).sum()) == 0
    N, H, W, C = case["N"], case["H"], case["W"], 3
    rs = np.random.RandomState(31)
    im0, im1 = (rs.uniform(0, 1, (N, H, W, C)).astype(np.float32) for _ in range(2))
    fw, bw, vf, vb = _inputs(case, poisoned=False)
    a1, a2 = case["alphas"]
    m_fw, _ = us.fb_valid(fw, bw, case["flow_scale"], a1, a2, vf, vb)
    assert torch.equal(m_fw.cpu(), d.mask)
    g0, g1 = gpu(im0), gpu(im1)
    i0, i1, fl = (torch.from_numpy(x).double() for x in (im0, im1, case["fw"]))
    s64, c64, _ = ur.photometric_ref(i0, i1, fl, case["flow_scale"], d.mask, 1e-3, 0.5)
    want = float(s64.sum()) / (C * max(int(c64.sum()), 1))
    loss = us.photometric_loss(g0, g1, fw, case["flow_scale"], valid=m_fw)
    print(f"{name}: photometric loss {float(loss):.8f} ref {want:.8f} rel err {abs(float(loss) - want) / want:.3e}, "
          f"contributing {int(c64.sum())} of {int(d.mask.sum())} valid")
    assert int(c64.sum()) > 0 and abs(float(loss) - want) <= 1e-5 * want
    s64, c64, _ = cr.census_ref(i0, i1, fl, case["flow_scale"], d.mask, radius=3, scale=255.0, **cr.CONSTS)
    want = float(s64.sum()) / max(int(c64.sum()), 1)
    loss = us.census_loss(g0, g1, fw, case["flow_scale"], valid=m_fw)
    print(f"{name}: census loss {float(loss):.8f} ref {want:.8f} rel err {abs(float(loss) - want) / want:.3e}, "
          f"contributing {int(c64.sum())}")
    assert int(c64.sum()) > 0 and abs(float(loss) - want) <= 1e-5 * want


# ------------------------------------------------------------------ trainer
@pytest.mark.parametrize("photo", [(), ("--photo", "census", "--census_radius", "1")], ids=["charbonnier", "census_r1"])
def test_train_cli_occlusion_fb(tmp_path, photo):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-d", "synthetic", "-e", "1", "-b", "2", "--crop_shape",
                          "64", "128", "--synthetic_pairs", "4", "--loss", "unsup", "--occlusion", "fb", *photo,
                          "--model_dir", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    steps = [ln for ln in out.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 1, steps                       # 4 pairs: 1 for validation, 3 to train on, batch 2, drop_last
    for ln in steps:
        m = re.search(r"loss/unsup (\S+)  (?:photometric|census) (\S+)  smoothness (\S+)  occluded (\S+)$", ln)
        assert m, ln
        assert all(np.isfinite(float(v)) for v in m.groups()[:3]), ln
        assert 0.0 <= float(m.group(4)) <= 1.0, ln
    epoch = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch ")]
    assert len(epoch) == 1 and np.isfinite(float(epoch[0].split("loss/unsup")[1].split()[0])) and "EPE/val" in epoch[0]
