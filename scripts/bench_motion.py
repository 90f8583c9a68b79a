#!/usr/bin/env python
"""Time the dominant-motion ops (pwcnet_amd/motion.py) at 8 x 448 x 1024: fit_motion for each model at iters = 4 beside the same
IRLS as a torch float64 loop on the same GPU in the same process (the route a user has without the op: context, not a target),
motion_residual and warp_frames alone.  Device events around windows of calls, warm-up first, the routes alternating, several
repeats; medians.  Also reports what the sums launches achieve against the bytes they must read (8 bytes of flow per pixel and
pass; there is no mask in this run) under the assumption that the solve launches cost nothing, and the largest difference between
the two routes' matrices.  Prints one JSON line (and writes it to --out).

    python scripts/bench_motion.py [--shape 8 448 1024] [--repeats 7] [--iters 5] [--out profiles/motion_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_irls(flows, model, iters, scale):
    """The same estimator with torch float64 ops and torch.linalg.solve: (N,3,3)."""
    N, H, W, _ = flows.shape
    dev = flows.device
    cx, cy, s = (W - 1) / 2.0, (H - 1) / 2.0, max(H, W) / 2.0
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    xh, yh = ((xs - cx) / s).reshape(1, -1), ((ys - cy) / s).reshape(1, -1)
    u, v = flows[..., 0].double().reshape(N, -1), flows[..., 1].double().reshape(N, -1)
    one, zero = torch.ones_like(xh), torch.zeros_like(xh)
    if model == "translation":
        Du, Dv = torch.stack([one, zero], -1), torch.stack([zero, one], -1)
    elif model == "similarity":
        Du, Dv = torch.stack([one, zero, xh, -yh], -1), torch.stack([zero, one, yh, xh], -1)
    else:
        Du, Dv = torch.stack([one, xh, yh, zero, zero, zero], -1), torch.stack([zero, zero, zero, one, xh, yh], -1)
    w = torch.ones_like(u)
    for it in range(iters + 1):
        A = torch.einsum("np,pi,pj->nij", w, Du[0], Du[0]) + torch.einsum("np,pi,pj->nij", w, Dv[0], Dv[0])
        b = torch.einsum("np,pi->ni", w * u, Du[0]) + torch.einsum("np,pi->ni", w * v, Dv[0])
        q = torch.linalg.solve(A, b)
        mu, mv = q @ Du[0].T, q @ Dv[0].T
        w = 1.0 / (1.0 + ((u - mu) ** 2 + (v - mv) ** 2) / scale ** 2)
    if model == "translation":
        p = torch.stack([q[:, 0], 0 * q[:, 0], 0 * q[:, 0], q[:, 1], 0 * q[:, 0], 0 * q[:, 0]], -1)
    elif model == "similarity":
        p = torch.stack([q[:, 0], q[:, 2], -q[:, 3], q[:, 1], q[:, 3], q[:, 2]], -1)
    else:
        p = q
    M = torch.zeros((N, 3, 3), dtype=torch.float64, device=dev)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = 1 + p[:, 1] / s, p[:, 2] / s, p[:, 0] - (p[:, 1] * cx + p[:, 2] * cy) / s
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = p[:, 4] / s, 1 + p[:, 5] / s, p[:, 3] - (p[:, 4] * cx + p[:, 5] * cy) / s
    M[:, 2, 2] = 1.0
    return M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion.py needs a GPU")
    import pwcnet_amd as P
    N, H, W = args.shape
    rs = np.random.RandomState(0)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flows = np.empty((N, H, W, 2))
    for n in range(N):                      # a camera motion, 0.05 px of noise, a quarter of the frame moving on its own
        flows[n, ..., 0] = 2.0 + 0.01 * n * (x - W / 2) - 0.004 * (y - H / 2)
        flows[n, ..., 1] = -1.0 + 0.004 * (x - W / 2) + 0.01 * n * (y - H / 2)
    flows += rs.normal(0, 0.05, flows.shape)
    flows[:, H // 4:3 * H // 4, W // 4:3 * W // 4] += (8.0, -6.0)
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

    runs, differ = {}, {}
    for model in ("translation", "similarity", "affine"):
        runs[f"op_{model}"] = lambda model=model: P.fit_motion(flows, model=model, iters=fit_iters)
        runs[f"torch_{model}"] = lambda model=model: torch_irls(flows, model, fit_iters, 1.0)
    matrices = P.fit_motion(flows, model="affine", iters=fit_iters)[0]
    runs["residual"] = lambda: P.motion_residual(flows, matrices)
    runs["warp_u8"] = lambda: P.warp_frames(frames, matrices)
    for fn in runs.values():                # warm-up
        fn()
        fn()
    for model in ("translation", "similarity", "affine"):
        differ[model] = float((runs[f"op_{model}"]()[0] - runs[f"torch_{model}"]()).abs().max())
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, args.iters))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    must_read = 8.0 * N * H * W * (fit_iters + 1)
    res = {"what": "dominant motion, ms per call (device events, medians of alternating windows): op_* = fit_motion at iters 4, "
                   "torch_* = the same IRLS as a torch float64 loop, residual = motion_residual, warp_u8 = warp_frames on uint8 "
                   "frames; sums_gbps_lower_bound = the flow bytes the five sums passes must read over the WHOLE fit's time",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters, "fit_iters": fit_iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "sums_must_read_bytes": must_read,
           "sums_gbps_lower_bound": {m: must_read / (med[f"op_{m}"] * 1e-3) / 1e9 for m in ("translation", "similarity", "affine")},
           "largest_matrix_difference_op_vs_torch": differ, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
