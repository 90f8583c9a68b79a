#!/usr/bin/env python
"""Time the SSIM term (ssim_sums + its gradient through autograd) beside the census term at the same radii, on the same GPU in
the same process, at the training frame size: device events around windows of whole forward + backward passes, warm-up first,
the terms alternating, several repeats; medians.  The census term is the yardstick: it was there before the SSIM term.  Prints
one JSON line (and writes it to --out).

    python scripts/bench_ssim.py [--shape 8 448 1024 3] [--radii 1 3] [--repeats 7] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=4, type=int, default=[8, 448, 1024, 3], metavar=("N", "H", "W", "C"))
    ap.add_argument("--radii", nargs="+", type=int, default=[1, 3])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="forward + backward passes per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py needs a GPU")
    from pwcnet_amd import unsup
    N, H, W, C = args.shape
    # scripts/bench_census.py's inputs: blocky content plus noise, moved by (+3, -2) px; the flow follows it to within a pixel
    rs = np.random.RandomState(0)
    base = rs.uniform(0, 1, (N, H // 8 + 3, W // 8 + 3, C)).astype(np.float32)
    big = np.kron(base, np.ones((1, 8, 8, 1), np.float32)) * 0.8 + 0.2 * rs.uniform(0, 1, (N, H + 24, W + 24, C)).astype(np.float32)
    im0 = torch.from_numpy(np.ascontiguousarray(big[:, 8:8 + H, 8:8 + W])).cuda()
    im1 = torch.from_numpy(np.ascontiguousarray(big[:, 6:6 + H, 11:11 + W])).cuda()
    blocks = rs.randint(-1, 2, size=(N, -(-H // 5), -(-W // 5), 2)).astype(np.float32)
    integer = np.kron(blocks, np.ones((1, 5, 5, 1), np.float32))[:, :H, :W] + np.array([3.0, -2.0], np.float32)
    flow = torch.from_numpy((integer + rs.uniform(0.1, 0.9, (N, H, W, 2))).astype(np.float32)).cuda()

    def passes(loss_fn, radius):
        def run():
            fl = flow.detach().requires_grad_(True)
            loss = loss_fn(im0, im1, fl, radius=radius)
            loss.backward()
            return loss.detach()
        return run

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    runs = {f"{term}_r{r}": passes(fn, r) for r in args.radii for term, fn in (("ssim", unsup.ssim_loss), ("census", unsup.census_loss))}
    losses = {}
    for key, fn in runs.items():                       # warm-up
        fn()
        losses[key] = float(fn())
    torch.cuda.synchronize()
    times = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            times[key].append(window(fn, args.iters))
    res = {"what": "loss forward + backward through autograd, ms per pass (device events, medians of alternating windows)",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters,
           "ms": {key: float(np.median(t)) for key, t in times.items()},
           "ms_min_max": {key: [min(t), max(t)] for key, t in times.items()},
           "loss": losses, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
