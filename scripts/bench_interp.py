#!/usr/bin/env python
"""Time frame interpolation (pwcnet_amd/interp.py) beside the same result composed from the package's other public ops on the same
GPU in the same process: float32 copies of the uint8 frames, the photometric error of each direction and exp in torch, two
forward_splat(mode="average", flow_scale=t) and two range_map calls per time, the blend and the quantisation in torch.  uint8
frames with smooth flows, M = 1 and M = 3.  Device events around windows of whole passes, warm-up first, the two paths
alternating, several repeats; medians.  Also records the largest byte difference between the two routes (the composition rounds
its weights and its splats to float32).  Prints one JSON line (and writes it to --out).

    python scripts/bench_interp.py [--shape 8 448 1024] [--repeats 7] [--iters 5] [--out profiles/interp_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def match_error(own, other, flow):
    """Mean over the channels of |own - other sampled bilinearly at p + flow| and whether p + flow is in frame (float32 torch)."""
    N, H, W, _ = flow.shape
    dev = flow.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    qx, qy = xs + flow[..., 0], ys + flow[..., 1]
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    qx, qy = torch.where(inside, qx, torch.zeros_like(qx)), torch.where(inside, qy, torch.zeros_like(qy))
    fx0, fy0 = torch.floor(qx), torch.floor(qy)
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    wx, wy = (qx - fx0)[..., None], (qy - fy0)[..., None]
    img = torch.arange(N, device=dev).view(N, 1, 1) * (H * W)
    flat = other.reshape(-1, 3)
    top = (1 - wx) * flat[img + y0 * W + x0] + wx * flat[img + y0 * W + x1]
    bot = (1 - wx) * flat[img + y1 * W + x0] + wx * flat[img + y1 * W + x1]
    return (own - ((1 - wy) * top + wy * bot)).abs().mean(dim=-1), inside


def composed(P, f0, f1, fw, bw, times, alpha=20.0, min_range=0.5):
    """interpolate_frames from the other public ops; (N,M,H,W,3) uint8."""
    a, b = f0.float() / 255.0, f1.float() / 255.0
    weights = []
    for own, other, flow in ((a, b, fw), (b, a, bw)):
        e, inside = match_error(own, other, flow)
        weights.append(torch.exp(-torch.where(inside, (alpha * e).clamp(max=10.0), torch.full_like(e, 10.0))))
    outs = []
    for t in times:
        c0, d0 = P.forward_splat(a, fw, weights=weights[0], flow_scale=t, mode="average")
        c1, d1 = P.forward_splat(b, bw, weights=weights[1], flow_scale=1.0 - t, mode="average")
        cov0 = ((P.range_map(fw, flow_scale=t) >= min_range) & (d0 > 0))[..., None]
        cov1 = ((P.range_map(bw, flow_scale=1.0 - t) >= min_range) & (d1 > 0))[..., None]
        both = (1.0 - t) * torch.where(cov0, c0, a) + t * torch.where(cov1, c1, b)
        v = torch.where(cov0 & ~cov1, c0, torch.where(cov1 & ~cov0, c1, both))
        outs.append(torch.round(255.0 * v).clamp(0, 255).to(torch.uint8))
    return torch.stack(outs, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="passes per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_interp.py needs a GPU")
    import pwcnet_amd as P
    N, H, W = args.shape
    rs = np.random.RandomState(0)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fw = np.empty((N, H, W, 2))
    for n in range(N):                      # a smooth field of ~12 px plus +-0.25 px noise; the backward flow is its negative
        fw[n, ..., 0] = 12.0 * np.sin(2 * np.pi * y / H + 0.4 * n) * np.cos(np.pi * x / W)
        fw[n, ..., 1] = 12.0 * np.cos(2 * np.pi * x / W - 0.4 * n) * np.sin(np.pi * y / H)
    bw = torch.from_numpy((-fw + rs.uniform(-0.25, 0.25, fw.shape)).astype(np.float32)).cuda()
    fw = torch.from_numpy((fw + rs.uniform(-0.25, 0.25, fw.shape)).astype(np.float32)).cuda()
    tex = 0.5 + 0.25 * np.sin(0.11 * x + 0.07 * y) + 0.25 * np.cos(0.05 * x - 0.13 * y)
    f0 = torch.from_numpy(np.rint(255 * np.clip(tex[None, ..., None] + rs.uniform(-0.1, 0.1, (N, H, W, 3)), 0, 1)).astype(np.uint8)).cuda()
    f1 = torch.from_numpy(np.rint(255 * np.clip(tex[None, ..., None] + rs.uniform(-0.1, 0.1, (N, H, W, 3)), 0, 1)).astype(np.uint8)).cuda()

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    runs, differ, codes = {}, {}, {}
    for M in (1, 3):
        times = [k / (M + 1) for k in range(1, M + 1)]
        runs[f"op_m{M}"] = lambda times=times: P.interpolate_frames(f0, f1, fw, bw, times)
        runs[f"composed_m{M}"] = lambda times=times: composed(P, f0, f1, fw, bw, times)
    for fn in runs.values():                # warm-up
        fn()
        fn()
    for M in (1, 3):
        got, source = runs[f"op_m{M}"]()
        d = (got.int() - runs[f"composed_m{M}"]().int()).abs()
        differ[f"m{M}"] = {"largest": int(d.max()), "share_differing": float((d != 0).float().mean())}
        codes[f"m{M}"] = torch.bincount(source.flatten().long(), minlength=4).tolist()
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, args.iters))
    res = {"what": "frame interpolation, ms per call (device events, medians of alternating windows): op = interpolate_frames, "
                   "composed = the same result from forward_splat / range_map and torch; uint8 frames, smooth flows",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters,
           "ms": {key: float(np.median(t)) for key, t in ms.items()},
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "byte_difference_op_vs_composed": differ, "source_code_counts": codes, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
