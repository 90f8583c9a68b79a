#!/usr/bin/env python
"""Time the projective path at 8 x 448 x 1024: fit_homography at iters = 4 beside fit_motion(model="affine") and beside the same
reweighted direct linear transform as a torch float64 loop on the same GPU in the same process (the route a user has without the
op: context, not a target); the projective motion_residual and warp_frames beside their affine forms on the same matrices' affine
parts; the projective background_plate (median, uint8, T = 32, a 512 x 1280 canvas) beside the affine one.  Device events around
windows of calls, warm-up first, the routes alternating, several repeats; medians.  Also the largest corner distance between the
op's and the torch loop's matrices.  Prints one JSON line (and writes it to --out).

    python scripts/bench_homography.py [--shape 8 448 1024] [--repeats 7] [--iters 5] [--out profiles/homography_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_dlt(flows, iters, scale):
    """The same estimator with torch float64 ops and torch.linalg.solve on the normal equations: (N,3,3), [2][2] = 1."""
    N, H, W, _ = flows.shape
    dev = flows.device
    cx, cy, s = (W - 1) / 2.0, (H - 1) / 2.0, max(H, W) / 2.0
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    xh, yh = ((xs - cx) / s).reshape(1, -1), ((ys - cy) / s).reshape(1, -1)
    xp, yp = xh + flows[..., 0].double().reshape(N, -1) / s, yh + flows[..., 1].double().reshape(N, -1) / s
    one, zero = torch.ones_like(xp), torch.zeros_like(xp)
    xh, yh = xh.expand_as(xp), yh.expand_as(xp)
    Rx = torch.stack([xh, yh, one, zero, zero, zero, -xp * xh, -xp * yh], -1)
    Ry = torch.stack([zero, zero, zero, xh, yh, one, -yp * xh, -yp * yh], -1)
    w = torch.ones_like(xp)
    for it in range(iters + 1):
        A = torch.einsum("np,npi,npj->nij", w, Rx, Rx) + torch.einsum("np,npi,npj->nij", w, Ry, Ry)
        b = torch.einsum("np,npi->ni", w * xp, Rx) + torch.einsum("np,npi->ni", w * yp, Ry)
        g = torch.linalg.solve(A, b)
        D = g[:, 6:7] * xh + g[:, 7:8] * yh + 1.0
        rx = ((g[:, 0:1] * xh + g[:, 1:2] * yh + g[:, 2:3]) / D - xp) * s
        ry = ((g[:, 3:4] * xh + g[:, 4:5] * yh + g[:, 5:6]) / D - yp) * s
        w = torch.where(D > 0, 1.0 / (1.0 + (rx * rx + ry * ry) / scale ** 2) / (D * D), torch.zeros_like(D))
    G = torch.cat([g, torch.ones((N, 1), dtype=torch.float64, device=dev)], 1).reshape(N, 3, 3)
    T = torch.tensor([[1 / s, 0, -cx / s], [0, 1 / s, -cy / s], [0, 0, 1]], dtype=torch.float64, device=dev)
    M = torch.linalg.inv(T) @ G @ T
    return M / M[:, 2:3, 2:3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--plate_frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_homography.py needs a GPU")
    import pwcnet_amd as P
    N, H, W = args.shape
    rs = np.random.RandomState(0)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flows = np.empty((N, H, W, 2))
    for n in range(N):                      # a pan with perspective, 0.05 px of noise, a block of 15 % moving on its own
        M = np.array([[1.0 + 0.002 * n, -0.004, 2.0], [0.004, 1.0 + 0.002 * n, -1.0], [2e-5 * (n + 1), -1e-5, 1.0]])
        D = M[2, 0] * x + M[2, 1] * y + 1.0
        flows[n, ..., 0] = (M[0, 0] * x + M[0, 1] * y + M[0, 2]) / D - x
        flows[n, ..., 1] = (M[1, 0] * x + M[1, 1] * y + M[1, 2]) / D - y
    flows += rs.normal(0, 0.05, flows.shape)
    flows[:, H // 4:3 * H // 4, int(0.35 * W):int(0.65 * W)] += (9.0, 0.0)
    flows = torch.from_numpy(flows.astype(np.float32)).cuda()
    frames = torch.from_numpy(rs.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)).cuda()
    fit_iters = 4

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    homs, ok, _ = P.fit_homography(flows, iters=fit_iters)
    affs = homs.clone()
    affs[:, 2] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device="cuda")
    # the plate: T frames on a 512 x 1280 canvas, a pan of 8 px a frame, with and without perspective terms
    T, Hc, Wc = args.plate_frames, 512, 1280
    clip = torch.from_numpy(rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)).cuda()
    pm = np.tile(np.eye(3), (T, 1, 1))
    pm[:, 0, 2] = -8.0 * np.arange(T)
    pm[:, 1, 2] = -32.0
    pa = pm.copy()
    pm[:, 2, 0] = 2e-5
    pm[:, 2, 1] = -1e-5
    runs = {
        "fit_homography": lambda: P.fit_homography(flows, iters=fit_iters),
        "fit_motion_affine": lambda: P.fit_motion(flows, model="affine", iters=fit_iters),
        "torch_dlt": lambda: torch_dlt(flows, fit_iters, 1.0),
        "residual_projective": lambda: P.motion_residual(flows, homs, projective=True),
        "residual_affine": lambda: P.motion_residual(flows, affs),
        "warp_u8_projective": lambda: P.warp_frames(frames, homs, projective=True),
        "warp_u8_affine": lambda: P.warp_frames(frames, affs),
        "plate_median_u8_projective": lambda: P.background_plate(clip, pm, (Hc, Wc), projective=True),
        "plate_median_u8_affine": lambda: P.background_plate(clip, pa, (Hc, Wc)),
    }
    for fn in runs.values():                # warm-up
        fn()
        fn()
    theirs = torch_dlt(flows, fit_iters, 1.0)
    corners = torch.tensor([[0.0, 0.0, 1.0], [W - 1.0, 0.0, 1.0], [0.0, H - 1.0, 1.0], [W - 1.0, H - 1.0, 1.0]], dtype=torch.float64,
                           device="cuda").T
    qa, qb = homs @ corners, theirs @ corners
    differ = float(((qa[:, :2] / qa[:, 2:3] - qb[:, :2] / qb[:, 2:3]) ** 2).sum(1).sqrt().max())
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, args.iters))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    must_read = 8.0 * N * H * W * (fit_iters + 1)
    res = {"what": "projective motion, ms per call (device events, medians of alternating windows): fit_homography and "
                   "fit_motion(affine) at iters 4, torch_dlt = the same reweighted DLT as a torch float64 loop, the projective and "
                   "affine residual, warp (uint8, C = 3) and median plate (uint8, C = 3, T frames, a 512 x 1280 canvas); "
                   "sums_gbps_lower_bound = the flow bytes the five sums passes must read over the WHOLE fit's time",
           "shape": args.shape, "plate_frames": T, "repeats": args.repeats, "iters": args.iters, "fit_iters": fit_iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "sums_must_read_bytes": must_read,
           "sums_gbps_lower_bound": {k: must_read / (med[k] * 1e-3) / 1e9 for k in ("fit_homography", "fit_motion_affine")},
           "ok": [bool(v) for v in ok.cpu().numpy()],
           "largest_corner_distance_op_vs_torch_px": differ, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
