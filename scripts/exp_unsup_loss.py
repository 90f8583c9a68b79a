"""The self-supervised losses (csrc/pwc_unsup.hip) against the float32 torch-op composition of the same formulas, forward plus
gradient with respect to the flow, at batch 8 x 448 x 1024 x 3 on one GPU.

Per term: the HIP forward (sums), the HIP gradient, both through torch.autograd as a user calls them, and the torch composition
(forward + autograd backward).  Each timed window is `CALLS` calls that rotate over `SETS` input sets (together above the 256 MB
last-level cache, so no call finds its inputs cached), between HIP events, after a warm-up; the median of `REPS` windows is
reported per call, with the algorithmic bytes (every input pixel read once, every output written once) and the share of 8 TB/s
they amount to.  A locally smooth flow of up to +-24 px (some pixels leave the frame), no mask.
usage: python scripts/exp_unsup_loss.py [batch [H W]]        (needs a GPU; prints one JSON line at the end)"""
import json
import sys

import torch

sys.path.insert(0, ".")
from pwcnet_amd import unsup  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (448, 1024)
C, SETS, CALLS, REPS, WARM = 3, 6, 6, 9, 2
EPS, Q, ALPHA = 1e-3, 0.5, 10.0
PEAK = 8e12
assert torch.cuda.is_available(), "exp_unsup_loss.py measures on a GPU; there is none"
dev = torch.device("cuda")


def rho(d):
    return (d * d + EPS * EPS) ** Q


def photometric_torch(im0, im1, flow):
    """tests/unsup_ref.py's restatement, float32 on the device, no mask."""
    N = im0.shape[0]
    zero = torch.zeros((), device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    px, py = xs + flow[..., 0], ys + flow[..., 1]
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    px, py = torch.where(inside, px, zero), torch.where(inside, py, zero)
    fx0, fy0 = torch.floor(px).detach(), torch.floor(py).detach()
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    wx, wy = (px - fx0).unsqueeze(3), (py - fy0).unsqueeze(3)
    n = torch.arange(N, device=dev).reshape(N, 1, 1).expand(N, H, W)
    warped = (1 - wy) * ((1 - wx) * im1[n, y0, x0] + wx * im1[n, y0, x1]) + wy * ((1 - wx) * im1[n, y1, x0] + wx * im1[n, y1, x1])
    term = torch.where(inside, rho(im0 - warped).sum(3), zero)
    return term.sum(dim=(1, 2)), inside.sum(dim=(1, 2))


def smoothness_torch(flow, image):
    dx, dy = flow[:, :, 1:] - flow[:, :, :-1], flow[:, 1:] - flow[:, :-1]
    tx = rho(dx).sum(3) * torch.exp(-ALPHA * (image[:, :, 1:] - image[:, :, :-1]).abs().mean(3))
    ty = rho(dy).sum(3) * torch.exp(-ALPHA * (image[:, 1:] - image[:, :-1]).abs().mean(3))
    return tx.sum(dim=(1, 2)) + ty.sum(dim=(1, 2))


def make_set(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    im0 = torch.rand((B, H, W, C), device=dev, generator=g)
    im1 = torch.rand((B, H, W, C), device=dev, generator=g)
    coarse = (torch.rand((B, 2, H // 32, W // 32), device=dev, generator=g) - 0.5) * 48
    flow = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear").permute(0, 2, 3, 1).contiguous()
    return im0, im1, flow, torch.empty_like(flow)


sets = [make_set(s) for s in range(SETS)]
set_bytes = sum(t.numel() * 4 for t in sets[0])
up = torch.ones((B,), device=dev)


def timed(fn):
    """Median over REPS windows of the time per call, in microseconds."""
    for _ in range(WARM):
        for s in sets:
            fn(*s)
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(CALLS):
            fn(*sets[k % SETS])
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    ts.sort()
    return ts[REPS // 2], ts[0], ts[-1]


def autograd(loss_of):
    def run(im0, im1, flow, dflow):
        fl = flow.detach().requires_grad_(True)
        loss_of(im0, im1, fl).sum().backward()
        return fl.grad
    return run


npix = B * H * W
variants = {
    # name: (callable, algorithmic bytes per pixel)
    "photometric hip forward": (lambda a, b, f, d: unsup.photometric_sums(a, b, f, eps=EPS, q=Q), 4 * (2 * C + 2)),
    "photometric hip gradient": (lambda a, b, f, d: unsup.photometric_grad(a, b, f, up, d, eps=EPS, q=Q), 4 * (2 * C + 4)),
    "photometric hip forward+gradient (autograd)": (autograd(lambda a, b, f: unsup.photometric_sums(a, b, f, eps=EPS, q=Q)[0]),
                                                    4 * (4 * C + 6)),
    "photometric torch float32 forward+gradient": (autograd(lambda a, b, f: photometric_torch(a, b, f)[0]), 4 * (4 * C + 6)),
    "smoothness hip forward": (lambda a, b, f, d: unsup.smoothness_sums(f, a, ALPHA, EPS, Q), 4 * (C + 2)),
    "smoothness hip gradient": (lambda a, b, f, d: unsup.smoothness_grad(f, up, d, a, ALPHA, EPS, Q), 4 * (C + 4)),
    "smoothness hip forward+gradient (autograd)": (autograd(lambda a, b, f: unsup.smoothness_sums(f, a, ALPHA, EPS, Q)),
                                                   4 * (2 * C + 6)),
    "smoothness torch float32 forward+gradient": (autograd(lambda a, b, f: smoothness_torch(f, a)), 4 * (2 * C + 6)),
}

# the two paths compute the same thing (float32 against float32: sums to 1e-4, gradients to 1e-3 of the largest element)
with torch.no_grad():
    hs, hc = unsup.photometric_sums(*sets[0][:3], eps=EPS, q=Q)
    ts_, tc = photometric_torch(*sets[0][:3])
    ss, st = unsup.smoothness_sums(sets[0][2], sets[0][0], ALPHA, EPS, Q), smoothness_torch(sets[0][2], sets[0][0])
gh = autograd(lambda a, b, f: unsup.photometric_sums(a, b, f, eps=EPS, q=Q)[0])(*sets[0])
gt = autograd(lambda a, b, f: photometric_torch(a, b, f)[0])(*sets[0])
agree = {"photometric_sums_rel": float(((hs - ts_).abs() / ts_.abs()).max()), "counts_equal": bool(torch.equal(hc.long(), tc)),
         "smoothness_sums_rel": float(((ss - st).abs() / st.abs()).max()),
         "photometric_grad_rel_to_max": float((gh - gt).abs().max() / gt.abs().max()),
         "share_in_frame": float(hc.sum()) / npix}
print(f"# batch {B} x {H} x {W} x {C}: {SETS} input sets of {set_bytes / 2**20:.0f} MiB, {CALLS} calls per window, median of {REPS}")
print(f"# agreement of the two paths: {agree}")
result = {"batch": B, "H": H, "W": W, "C": C, "device": torch.cuda.get_device_name(0), "agreement": agree, "us": {}}
for name, (fn, bpp) in variants.items():
    med, lo, hi = timed(fn)
    nbytes = bpp * npix
    print(f"{name:46s} {med:9.1f} us  (min {lo:9.1f}, max {hi:9.1f})   {nbytes / 1e6:7.1f} MB algorithmic   "
          f"{nbytes / (med * 1e-6) / 1e12:5.2f} TB/s = {100 * nbytes / (med * 1e-6) / PEAK:5.1f} % of 8 TB/s")
    result["us"][name] = {"median": med, "min": lo, "max": hi, "algorithmic_bytes": nbytes}
print(json.dumps(result))
