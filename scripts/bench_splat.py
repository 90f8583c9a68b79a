#!/usr/bin/env python
"""Time forward splatting (pwcnet_amd/splat.py) beside a torch index_add_ restatement on the same GPU in the same process, at
the training frame size: forward alone and forward + backward through autograd, for C = 1 with no frame (the range map) and for
C = 3 (a frame, weighted).  Device events around windows of whole passes, warm-up first, the two paths alternating, several
repeats; medians.  The torch path is float32 index_add_ over the four corners with the same in-frame rules: one launch per
corner and more around it, float atomics (not bit reproducible).  Prints one JSON line (and writes it to --out).

    python scripts/bench_splat.py [--shape 8 384 448] [--repeats 7] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_splat(x, flow, w):
    """(out or None, coverage): the splat in float32 torch ops, index_add_ per corner."""
    N, H, W, _ = flow.shape
    dev = flow.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    px, py = xs + flow[..., 0], ys + flow[..., 1]
    ok = (px > -1) & (px < W) & (py > -1) & (py < H)
    px, py = torch.where(ok, px, torch.zeros_like(px)), torch.where(ok, py, torch.zeros_like(py))
    fx0, fy0 = torch.floor(px.detach()), torch.floor(py.detach())
    wx, wy = px - fx0, py - fy0
    x0, y0 = fx0.long(), fy0.long()
    img = torch.arange(N, device=dev).view(N, 1, 1) * (H * W)
    C = 0 if x is None else x.shape[3]
    den = torch.zeros((N * H * W,), dtype=torch.float32, device=dev)
    num = torch.zeros((N * H * W, C), dtype=torch.float32, device=dev) if C else None
    for k in range(4):
        dx, dy = k & 1, k >> 1
        cx, cy = x0 + dx, y0 + dy
        inside = ok & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        t = (img + cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).reshape(-1)
        b = (wx if dx else 1 - wx) * (wy if dy else 1 - wy)
        bw = torch.where(inside, b if w is None else b * w, torch.zeros_like(b)).reshape(-1)
        den = den.index_add(0, t, bw)
        if C:
            num = num.index_add(0, t, bw[:, None] * x.reshape(-1, C))
    return (num.view(N, H, W, C) if C else None), den.view(N, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 384, 448], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="passes per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat.py needs a GPU")
    from pwcnet_amd import splat
    N, H, W = args.shape
    rs = np.random.RandomState(0)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flow = np.empty((N, H, W, 2))
    for n in range(N):                      # a smooth field of ~12 px plus +-0.5 px noise: collisions, holes, some pixels leave the frame
        flow[n, ..., 0] = 12.0 * np.sin(2 * np.pi * y / H + 0.4 * n) * np.cos(np.pi * x / W)
        flow[n, ..., 1] = 12.0 * np.cos(2 * np.pi * x / W - 0.4 * n) * np.sin(np.pi * y / H)
    flow = torch.from_numpy((flow + rs.uniform(-0.5, 0.5, flow.shape)).astype(np.float32)).cuda()
    frame = torch.from_numpy(rs.uniform(0, 1, (N, H, W, 3)).astype(np.float32)).cuda()
    weight = torch.from_numpy(rs.uniform(0.5, 2, (N, H, W)).astype(np.float32)).cuda()
    g3 = torch.from_numpy(rs.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)).cuda()
    g1 = torch.from_numpy(rs.uniform(-1, 1, (N, H, W)).astype(np.float32)).cuda()

    def hip_c1(backward):
        def run():
            fl = flow.detach().requires_grad_(backward)
            r = splat.range_map(fl)
            if backward:
                (r * g1).sum().backward()
            return r.detach()
        return run

    def torch_c1(backward):
        def run():
            fl = flow.detach().requires_grad_(backward)
            r = torch_splat(None, fl, None)[1]
            if backward:
                (r * g1).sum().backward()
            return r.detach()
        return run

    def hip_c3(backward):
        def run():
            fl, xx, ww = (t.detach().requires_grad_(backward) for t in (flow, frame, weight))
            out, cov = splat.forward_splat(xx, fl, ww)
            if backward:
                ((out * g3).sum() + (cov * g1).sum()).backward()
            return out.detach()
        return run

    def torch_c3(backward):
        def run():
            fl, xx, ww = (t.detach().requires_grad_(backward) for t in (flow, frame, weight))
            out, cov = torch_splat(xx, fl, ww)
            if backward:
                ((out * g3).sum() + (cov * g1).sum()).backward()
            return out.detach()
        return run

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    runs = {}
    for tag, backward in (("fwd", False), ("fwd_bwd", True)):
        runs[f"hip_c1_{tag}"], runs[f"torch_c1_{tag}"] = hip_c1(backward), torch_c1(backward)
        runs[f"hip_c3_{tag}"], runs[f"torch_c3_{tag}"] = hip_c3(backward), torch_c3(backward)
    agree = {}
    for key, fn in runs.items():                       # warm-up
        fn()
        fn()
    for c in ("c1", "c3"):                             # the two paths compute the same thing (float32 torch: to its rounding)
        a, b = runs[f"hip_{c}_fwd"](), runs[f"torch_{c}_fwd"]()
        agree[c] = float((a - b).abs().max())
    torch.cuda.synchronize()
    times = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            times[key].append(window(fn, args.iters))
    res = {"what": "forward splatting, ms per pass (device events, medians of alternating windows); c1 = range map, c3 = a weighted "
                   "frame; fwd_bwd = forward + backward through autograd; torch = float32 index_add_ restatement",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters,
           "ms": {key: float(np.median(t)) for key, t in times.items()},
           "ms_min_max": {key: [min(t), max(t)] for key, t in times.items()},
           "max_abs_difference_hip_vs_torch_fwd": agree, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
