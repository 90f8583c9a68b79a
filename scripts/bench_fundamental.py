#!/usr/bin/env python
"""Time the epipolar path at 8 x 448 x 1024: fit_fundamental at iters = 4 beside fit_homography and beside the same reweighted
eight-point fit as a torch float64 loop on the same GPU in the same process (einsum for the 9 x 9 matrix, torch.linalg.eigh,
torch.linalg.svd for the rank: the route a user has without the op -- context, not a target); epipolar_residual beside
motion_residual(projective=True).  The flows are the test scene of tests/fundamental_ref.py at the bench's size with 0.05 px of
noise.  Device events around windows of calls, warm-up first, the routes alternating, several repeats; medians.  Also the largest
difference between the op's and the torch loop's matrices, up to sign.  Prints one JSON line (and writes it to --out).

    python scripts/bench_fundamental.py [--shape 8 448 1024] [--repeats 5] [--iters 5] [--out profiles/fundamental_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_eight_point(flows, iters, scale):
    """The same estimator with torch float64 ops: (N,3,3) with Frobenius norm 1 (the sign as it comes)."""
    N, H, W, _ = flows.shape
    dev = flows.device
    cx, cy, s = (W - 1) / 2.0, (H - 1) / 2.0, max(H, W) / 2.0
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    xh, yh = ((xs - cx) / s).reshape(1, -1), ((ys - cy) / s).reshape(1, -1)
    xp, yp = xh + flows[..., 0].double().reshape(N, -1) / s, yh + flows[..., 1].double().reshape(N, -1) / s
    xh, yh = xh.expand_as(xp), yh.expand_as(xp)
    one = torch.ones_like(xp)
    rows = torch.stack([xp * xh, xp * yh, xp, yp * xh, yp * yh, yp, xh, yh, one], -1)
    p, q = torch.stack([xh, yh, one], -1), torch.stack([xp, yp, one], -1)
    w = torch.ones_like(xp)
    F = None
    for it in range(iters + 1):
        A = torch.einsum("np,npi,npj->nij", w, rows, rows)
        F = torch.linalg.eigh(A)[1][:, :, 0].reshape(N, 3, 3)
        U, sv, Vt = torch.linalg.svd(F)
        sv = sv.clone()
        sv[:, 2] = 0.0
        F = U @ torch.diag_embed(sv) @ Vt
        l, lp = p @ F.transpose(1, 2), q @ F
        r = (q * l).sum(-1)
        g = l[..., 0] ** 2 + l[..., 1] ** 2 + lp[..., 0] ** 2 + lp[..., 1] ** 2
        w = torch.where(g > 0, 1.0 / (1.0 + (r * r / g) * s * s / scale ** 2) / g, torch.zeros_like(g))
    T = torch.tensor([[1 / s, 0, -cx / s], [0, 1 / s, -cy / s], [0, 0, 1]], dtype=torch.float64, device=dev)
    M = T.T @ F @ T
    return M / M.flatten(1).norm(dim=1).reshape(N, 1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window (the torch loop: one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fundamental.py needs a GPU")
    import pwcnet_amd as P
    from tests import fundamental_ref as R
    N, H, W = args.shape
    flows = torch.from_numpy(np.stack([R.scene(H, W, n, True, 0.05)[0] for n in range(N)])).cuda()
    fit_iters = 4

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    fund, ok, info = P.fit_fundamental(flows, iters=fit_iters)
    homs, hok, _ = P.fit_homography(flows, iters=fit_iters)
    runs = {
        "fit_fundamental": lambda: P.fit_fundamental(flows, iters=fit_iters),
        "fit_fundamental_iters0": lambda: P.fit_fundamental(flows, iters=0),
        "fit_fundamental_one_image": lambda: P.fit_fundamental(flows[:1], iters=fit_iters),
        "fit_homography": lambda: P.fit_homography(flows, iters=fit_iters),
        "fit_homography_one_image": lambda: P.fit_homography(flows[:1], iters=fit_iters),
        "torch_eight_point": lambda: torch_eight_point(flows, fit_iters, 1.0),
        "epipolar_residual": lambda: P.epipolar_residual(flows, fund),
        "residual_projective": lambda: P.motion_residual(flows, homs, projective=True),
    }
    calls = {key: 1 if key.startswith("torch") else args.iters for key in runs}
    for fn in runs.values():                # warm-up
        fn()
        fn()
    theirs = torch_eight_point(flows, fit_iters, 1.0)
    differ = float(torch.minimum((fund - theirs).abs().flatten(1).max(1)[0], (fund + theirs).abs().flatten(1).max(1)[0]).max())
    dist, inl = P.epipolar_residual(flows, fund)
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, calls[key]))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    must_read = 8.0 * N * H * W * (fit_iters + 1)
    res = {"what": "epipolar motion, ms per call (device events, medians of alternating windows): fit_fundamental and fit_homography "
                   "at iters 4 (and on one image of the batch, where the one-lane solve shows; and at iters 0, one pass), "
                   "torch_eight_point = the same reweighted eight-point fit as a torch float64 loop (einsum, eigh, svd), "
                   "epipolar_residual beside motion_residual(projective=True); sums_gbps_lower_bound = the flow bytes the five sums "
                   "passes must read over the WHOLE fit's time",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters, "fit_iters": fit_iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "sums_must_read_bytes": must_read,
           "sums_gbps_lower_bound": {k: must_read / (med[k] * 1e-3) / 1e9 for k in ("fit_fundamental", "fit_homography")},
           "ok": [bool(v) for v in ok.cpu().numpy()], "homography_ok": [bool(v) for v in hok.cpu().numpy()],
           "eigen": info["eigen"].cpu().numpy().tolist(),
           "inlier_share_at_1px": float(inl.float().mean()),
           "largest_entry_difference_op_vs_torch": differ, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
