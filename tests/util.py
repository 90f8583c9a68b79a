"""Shared helpers for the tests (seeded inputs, weight sets)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pwcnet_amd import weights as W  # noqa: E402  (host-side numpy only)


def images(n, h, w, seed=1234):
    rng = np.random.RandomState(seed)
    return (rng.uniform(0, 1, size=(n, h, w, 3)).astype(np.float32),
            rng.uniform(0, 1, size=(n, h, w, 3)).astype(np.float32))


def smooth_images(n, h, w, seed=7, shift=(3, -2)):
    """Second image = first one translated (plus noise): gives the net a real motion."""
    rng = np.random.RandomState(seed)
    base = rng.uniform(0, 1, size=(n, h // 8 + 2, w // 8 + 2, 3)).astype(np.float32)
    big = np.kron(base, np.ones((1, 8, 8, 1), np.float32))[:, : h + 16, : w + 16]
    im0 = big[:, 8:8 + h, 8:8 + w]
    im1 = big[:, 8 + shift[1]:8 + shift[1] + h, 8 + shift[0]:8 + shift[0] + w]
    return np.ascontiguousarray(im0), np.ascontiguousarray(im1)


def model_weights(use_dc=False, seed=0, bias_seed=1, gain=1.0):
    specs = W.conv_specs(use_dc=use_dc)
    w = W.randomize_biases(W.init_weights(specs, seed=seed), seed=bias_seed)
    if gain != 1.0:
        for k in w:
            if k.endswith("/kernel"):
                w[k] = (w[k] * gain).astype(np.float32)
    return w


def flow_field(n, h, w, seed=3, sigma=3.0, outliers=True):
    """flows ~ N(0, sigma^2) px with a few +-50 px outliers and exact integers."""
    rng = np.random.RandomState(seed)
    f = rng.normal(0, sigma, size=(n, h, w, 2)).astype(np.float32)
    if outliers:
        m = rng.uniform(size=(n, h, w)) < 0.02
        f[m] = rng.choice([-50.0, 50.0, -7.0, 3.0, 0.0], size=(int(m.sum()), 2)).astype(np.float32)
    return f


def float64_flows(w, use_dc, im0, im1):
    """(flows_final, flows_pyramid) of the float64 restatement (oracle/torch_ref.py, pinned against the C oracle in
    tests/test_oracle.py) on numpy frames: the yardstick for the fp32 forwards, whose own error the fp32 oracle shares."""
    import torch
    from oracle import torch_ref as TR
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w64 = {k: torch.from_numpy(v).to(torch.float64) for k, v in w.items()}
    with torch.no_grad():
        final, pyr = TR.TorchPWCDCNet(w64, use_dc=use_dc)(torch.from_numpy(im0).double(), torch.from_numpy(im1).double())
    return final.numpy(), [p.numpy() for p in pyr]


def check_float64(tag, got_final, got_pyr, ref, bound_px):
    """Max abs error of a forward's flows_final (px) and of every pyramid level (px / 20: bound_px / 20) against
    float64_flows' `ref`; printed, then asserted.  Returns the flows_final error."""
    def as_np(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else t
    final = as_np(got_final)
    assert final.shape == ref[0].shape, (final.shape, ref[0].shape)
    err = float(np.abs(final - ref[0]).max())
    err_p = [float(np.abs(as_np(p) - e).max()) for p, e in zip(got_pyr, ref[1])]
    assert len(err_p) == len(ref[1])
    print(f"float64 {tag}: flows_final max |flow| {float(np.abs(ref[0]).max()):.3f} px, err {err:.3e} px (bound {bound_px:.1e}); "
          f"pyramid err x20 {20.0 * max(err_p):.3e} px")
    assert err <= bound_px, (tag, err, bound_px)
    assert max(err_p) <= bound_px / 20.0, (tag, err_p, bound_px)
    return err
