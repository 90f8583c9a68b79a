#!/usr/bin/env python
"""Time census_loss forward + backward on the HIP path against the float32 torch-op restatement (tests/census_ref.py) of the
same term on the same GPU, at the training frame size: device events around whole forward + backward passes, warm-up first, the
two versions alternating, several repeats; medians.  Both gradients are compared with the float64 restatement's at the
timed size (max-abs error over the largest element).  Prints one JSON line (and writes it to --out).

    python scripts/bench_census.py [--shape 8 448 1024 3] [--radius 3] [--repeats 7] [--iters 10] [--out FILE]
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
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="forward + backward passes per timed window of the HIP path")
    ap.add_argument("--ref-iters", type=int, default=2, help="... of the torch restatement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_census.py needs a GPU")
    from pwcnet_amd import unsup
    from tests import census_ref as cr
    N, H, W, C = args.shape
    rs = np.random.RandomState(0)
    base = rs.uniform(0, 1, (N, H // 8 + 3, W // 8 + 3, C)).astype(np.float32)
    big = np.kron(base, np.ones((1, 8, 8, 1), np.float32)) * 0.8 + 0.2 * rs.uniform(0, 1, (N, H + 24, W + 24, C)).astype(np.float32)
    im0 = torch.from_numpy(np.ascontiguousarray(big[:, 8:8 + H, 8:8 + W])).cuda()
    im1 = torch.from_numpy(np.ascontiguousarray(big[:, 6:6 + H, 11:11 + W])).cuda()          # content moved by (+3, -2) px
    # flow: (3, -2) px plus -1 / 0 / +1 per 5 x 5 block plus a fraction in [0.1, 0.9] -- every sample coordinate keeps 0.1 from the
    # kinks of floor, so the float32 and float64 runs sample the same corners and their gradients are comparable
    blocks = rs.randint(-1, 2, size=(N, -(-H // 5), -(-W // 5), 2)).astype(np.float32)
    integer = np.kron(blocks, np.ones((1, 5, 5, 1), np.float32))[:, :H, :W] + np.array([3.0, -2.0], np.float32)
    flow = torch.from_numpy((integer + rs.uniform(0.1, 0.9, (N, H, W, 2))).astype(np.float32)).cuda()

    def hip():
        fl = flow.detach().requires_grad_(True)
        loss = unsup.census_loss(im0, im1, fl, radius=args.radius)
        loss.backward()
        return loss.detach(), fl.grad

    def ref():
        fl = flow.detach().requires_grad_(True)
        sums, counts, _ = cr.census_ref(im0, im1, fl, radius=args.radius)
        loss = sums.sum() / counts.sum().clamp(min=1).to(torch.float32)
        loss.backward()
        return loss.detach(), fl.grad

    def ref64():
        fl = flow.double().requires_grad_(True)
        sums, counts, _ = cr.census_ref(im0.double(), im1.double(), fl, radius=args.radius)
        loss = sums.sum() / counts.sum().clamp(min=1)
        loss.backward()
        return loss.detach(), fl.grad

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    (lh, gh), (lr, gr) = hip(), ref()              # warm-up, and the two versions against each other
    hip(), ref()
    torch.cuda.synchronize()
    l64, g64 = ref64()                             # the float64 restatement at the timed size: what both are off by
    gmax = float(g64.abs().max())
    err_hip, err_ref = float((gh.double() - g64).abs().max()) / gmax, float((gr.double() - g64).abs().max()) / gmax
    del g64
    torch.cuda.empty_cache()
    t_hip, t_ref = [], []
    for _ in range(args.repeats):
        t_hip.append(window(hip, args.iters))
        t_ref.append(window(ref, args.ref_iters))
    res = {"what": "census_loss forward + backward, ms per pass (device events, medians)", "shape": args.shape,
           "radius": args.radius, "repeats": args.repeats, "iters": [args.iters, args.ref_iters],
           "hip_ms": float(np.median(t_hip)), "hip_ms_min_max": [min(t_hip), max(t_hip)],
           "torch_fp32_ms": float(np.median(t_ref)), "torch_fp32_ms_min_max": [min(t_ref), max(t_ref)],
           "speedup": float(np.median(t_ref) / np.median(t_hip)),
           "loss_hip": float(lh), "loss_torch_fp32": float(lr),
           "loss_float64": float(l64), "grad_err_hip_vs_float64": err_hip, "grad_err_torch_fp32_vs_float64": err_ref,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
